"""The recorded explicit wave stepper with a damping field, u_tt + d o u_t = c2 o (A u) - w(t) g (csrc/onchip_plan.h, DESIGN section
12.6), without a GPU.  tests/cpp/onchip_wave_sponge_plan_driver.cpp, a program of its own built with the sanitizers, (1) evaluates
the factor and the damp and runs whole steps the way the rotated kernel loop runs them -- launches, the carried acceleration, the
opening and closing damp -- with the functions the kernel calls, which is compared bit for bit with the NumPy model of
tests/wave_sponge_reference.py, and (2) restates the workspace formula for every even N from 6 to the cap.  The model's own
properties are checked here too: no damping is the stepper in a medium, a run may be split at a multiple of the cadence, the
modified energy never grows, the scheme is second order in tau.  sponge_damping is checked on the packed order, and the header,
the ctypes layer, the package and the built kernels must agree on the new entry points."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_medium_reference as M  # noqa: E402
import wave_sponge_reference as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE, STRETCHED = (1.0, 2.0, 1.0, 2.0), (0.0, 1.0, 0.0, 1.7)
LLVM = os.path.join(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")), "..", "lib", "llvm", "bin")


def grid(n):
    """N = 20 is stretched: xk != yk."""
    return S.Grid.of_domain(n, *(STRETCHED if n == 20 else SQUARE))


def medium(rng, shape):
    """A seeded medium in [0.25, 4]: wave speeds between a half and two."""
    return rng.uniform(0.25, 4.0, shape)


def damping(rng, shape, tau, top=1.0):
    """A seeded damping with (0.25 tau) d in [0, top], zero on about a third of the unknowns; tau a float or [members]."""
    e = rng.uniform(0.0, top, shape) * (rng.uniform(0.0, 1.0, shape) > 1.0 / 3.0)
    return e / (0.25 * (np.asarray(tau)[:, None] if np.ndim(tau) else tau))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("onchip_wave_sponge") / "onchip_wave_sponge_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "onchip_wave_sponge_plan_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def lines(driver):
    out = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    return [ln.split() for ln in out.stdout.splitlines()]


def run_file(driver, tmp_path, values, *mode):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in values]).tofile(src)
    out = subprocess.run([driver, src, dst, *mode], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-2000:]
    return np.fromfile(dst, dtype=np.float64)


def run_driver(driver, tmp_path, g, tau, nsteps, u, gv, v, c2, d, w, receivers, every, launch):
    got = run_file(driver, tmp_path, [[float(g.n), tau, float(nsteps), g.A0, g.xk, g.yk, float(every), float(len(receivers)), float(launch)], g.image(u), gv, v,
                                      c2, d, w, np.asarray(receivers, dtype=np.float64)])
    samples = nsteps // every
    assert got.shape == (2 * g.size + samples * len(receivers),)
    return got[:g.size], got[g.size:2 * g.size], got[2 * g.size:].reshape(samples, len(receivers))


def seeded(g, seed, nsteps, frac):
    """(tau, u, v, g, c2, d, w, receivers): states and a forcing over seven decades, a medium in [0.25, 4], tau = frac x the
    member's bound, (0.25 tau) d in [0, 1] with the largest entry at 1 exactly, amplitudes of either sign, five receivers."""
    rng = np.random.default_rng(seed)
    scale = lambda: 10.0 ** rng.integers(-3, 4, g.size)
    u, v, gv = (rng.standard_normal(g.size) * scale() for _ in range(3))
    c2 = medium(rng, g.size)
    tau = frac * M.medium_cfl(g, c2.max())
    d = damping(rng, g.size, tau)
    d[1] = 1.0 / (0.25 * tau)
    if (0.25 * tau) * d[1] > 1.0:
        d[1] = np.nextafter(d[1], 0.0)
    w = rng.standard_normal(nsteps + 1) * 10.0 ** rng.integers(-2, 3, nsteps + 1)
    receivers = [int(r) for r in rng.integers(0, g.size, 3)] + [0, g.size - 1]
    return tau, u, v, gv, c2, d, w, receivers


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the expressions and whole steps against the driver ----------------------------------------------------------------------------
def test_the_factor_and_the_damp_are_the_models(driver, tmp_path):
    rng = np.random.default_rng(21)
    tau = 10.0 ** rng.uniform(-4, 1, 600)
    d = rng.uniform(0.0, 1.0, 600) / (0.25 * tau)
    d[:4] = [0.0, 4.0 / tau[1], 2.0 / tau[2], 12.0 / tau[3]]
    v = rng.standard_normal(600) * 10.0 ** rng.integers(-3, 4, 600)
    got = run_file(driver, tmp_path, [[600.0], tau, d, v], "factor")
    s = S.sponge_factor(tau, d)
    e = (0.25 * tau) * d
    assert np.array_equal(s, (1.0 - e) / (1.0 + e))
    assert np.array_equal(got[:600], s) and np.array_equal(got[600:], s * v)
    assert s[0] == 1.0 and got[600] == v[0] and np.all(np.abs(s) <= 1.0)
    assert abs(s[1]) <= 1e-15 and abs(s[2] - 1.0 / 3.0) <= 1e-15 and abs(s[3] + 0.5) <= 1e-15       # beyond e = 1 the factor is negative


@pytest.mark.parametrize("n", [6, 10, 20])
def test_damped_steps_are_the_models_operation_by_operation(driver, tmp_path, n):
    """The driver runs the kernel's rotated loop; the model the scheme as the issue lists it.  Several launches, a cadence of 3,
    launches of one step, one launch for all."""
    g = grid(n)
    assert (g.xk != g.yk) == (n == 20)
    for frac, nsteps, every, launch in ((0.37, 1, 1, 1), (1.0, 7, 3, 3), (0.81, 0, 2, 5), (0.5, 6, 2, 1), (0.93, 23, 3, 5), (0.61, 9, 1, 100)):
        tau, u, v, gv, c2, d, w, receivers = seeded(g, 700 + n + nsteps, nsteps, frac)
        assert ((0.25 * tau) * d).max() <= 1.0 and (d == 0).sum() >= g.size // 6
        got = run_driver(driver, tmp_path, g, tau, nsteps, u, gv, v, c2, d, w, receivers, every, launch)
        want = S.verlet_sponge(g, u, v, gv, c2, d, tau, nsteps, w, receivers, every)
        assert same(got, want), (n, frac, nsteps, launch)
        assert got[2].shape == (nsteps // every, 5)
    # one step, written out once more without the model's loop
    tau, u, v, gv, c2, d, w, receivers = seeded(g, 800 + n, 1, 0.37)
    h = 0.5 * tau
    e = (0.25 * tau) * d
    s = (1.0 - e) / (1.0 + e)
    v0 = s * v
    f = w[0] * gv
    t = g.au(u)
    a = c2 * t - f
    vh = v0 + h * a
    un = u + tau * vh
    f = w[1] * gv
    t = g.au(un)
    vn = vh + h * (c2 * t - f)
    vn = s * vn
    got = run_driver(driver, tmp_path, g, tau, 1, u, gv, v, c2, d, w, receivers, 1, 1)
    assert np.array_equal(got[0], un) and np.array_equal(got[1], vn) and np.array_equal(got[2], un[receivers][None, :])
    # the acceleration a step leaves is the one the next call forms anew: three calls of one step are one call of three
    tau, u, v, gv, c2, d, w, receivers = seeded(g, 900 + n, 3, 0.37)
    one = (u, v)
    for k in range(3):
        one = run_driver(driver, tmp_path, g, tau, 1, one[0], gv, one[1], c2, d, w[k:k + 2], receivers, 1, 1)
    three = run_driver(driver, tmp_path, g, tau, 3, u, gv, v, c2, d, w, receivers, 1, 3)
    assert np.array_equal(one[0], three[0]) and np.array_equal(one[1], three[1]) and np.array_equal(one[2][0], three[2][2])


def test_the_driver_found_no_violation(lines):
    assert not [ln for ln in lines if ln and ln[0] == "FAIL"]
    assert lines[-1] == ["ok", "0"]


# ---- the model's own properties ------------------------------------------------------------------------------------------------------
def ensemble(g, seed, members, nsteps):
    rng = np.random.default_rng(seed)
    u, v = rng.standard_normal((members, g.size)), rng.standard_normal((members, g.size)) * np.sqrt(abs(g.A0))
    gv = rng.standard_normal((members, g.size)) * abs(g.A0)
    c2 = medium(rng, (members, g.size))
    tau = M.medium_cfl(g, c2.max(axis=-1)) * rng.uniform(0.1, 1.0, members)
    d = damping(rng, (members, g.size), tau)
    w = rng.standard_normal((members, nsteps + 1))
    receivers = [int(r) for r in rng.integers(0, g.size, 3)] + [0, g.size - 1]
    return u, v, gv, c2, d, tau, w, receivers


@pytest.mark.parametrize("n", [6, 10, 20])
def test_no_damping_is_the_stepper_in_a_medium(n):
    g = grid(n)
    u, v, gv, c2, _, tau, w, receivers = ensemble(g, 1000 + n, 4, 23)
    want = M.verlet_medium(g, u, v, gv, c2, tau, 23, w, receivers, 3)
    for d in (np.zeros(g.size), np.zeros((4, g.size))):
        assert same(S.verlet_sponge(g, u, v, gv, c2, d, tau, 23, w, receivers, 3), want)
    assert same(S.verlet_sponge(g, u[1], v[1], gv[1], c2[1], np.zeros(g.size), float(tau[1]), 23, w[1], receivers, 3), [x[1] for x in want])
    assert np.all(S.sponge_factor(tau[:, None], np.zeros((4, g.size))) == 1.0)


@pytest.mark.parametrize("n", [6, 10, 20])
def test_a_run_split_at_a_multiple_of_the_cadence_is_the_whole_run(n):
    g = grid(n)
    nsteps, every = 23, 3
    u, v, gv, c2, d, tau, w, receivers = ensemble(g, 1100 + n, 4, nsteps)
    whole = S.verlet_sponge(g, u, v, gv, c2, d, tau, nsteps, w, receivers, every)
    assert whole[2].shape == (4, 7, 5)
    assert not np.array_equal(whole[0], M.verlet_medium(g, u, v, gv, c2, tau, nsteps, w, receivers, every)[0])
    for cut in (3, 12, 21):
        a = S.verlet_sponge(g, u, v, gv, c2, d, tau, cut, w[:, :cut + 1], receivers, every)
        b = S.verlet_sponge(g, a[0], a[1], gv, c2, d, tau, nsteps - cut, w[:, cut:], receivers, every)
        assert same(b[:2], whole[:2]) and np.array_equal(np.concatenate([a[2], b[2]], axis=1), whole[2]), cut
    # a shared damping is that field for every member (member 0's, rescaled so that no member is above e = 1)
    d0 = d[0] * (tau[0] / tau.max())
    shared = S.verlet_sponge(g, u, v, gv, c2, d0, tau, nsteps, w, receivers, every)
    assert same(shared, S.verlet_sponge(g, u, v, gv, c2, np.stack([d0] * 4), tau, nsteps, w, receivers, every))
    assert same([x[2] for x in shared], S.verlet_sponge(g, u[2], v[2], gv[2], c2[2], d0, float(tau[2]), nsteps, w[2], receivers, every))


@pytest.mark.parametrize("n", [6, 10, 20])
@pytest.mark.parametrize("frac", [0.5, 1.0])
def test_the_modified_energy_never_grows(n, frac):
    """Without a forcing Verlet conserves E = 1/2 v^T C^-1 v - 1/2 u^T A u - (tau^2 / 8) a^T C^-1 a (section 12.5), and a factor
    |s| <= 1 on every component of v can only lower its first term: E[n + 1] - E[n] <= 1e-12 E[0] (section 12.3's margin for the
    rounding of a conserved quantity) over 2000 steps, at half the member's bound and at the bound, with (0.25 tau) d in [0, 0.8]
    and zero on a third of the unknowns; and E ends below E[0]."""
    g = grid(n)
    rng = np.random.default_rng(1200 + n)
    c2 = medium(rng, g.size)
    u, v = rng.standard_normal(g.size), rng.standard_normal(g.size) * np.sqrt(abs(g.A0))
    zero, unit = np.zeros(g.size), np.ones(2)
    tau = frac * M.medium_cfl(g, c2.max())
    d = damping(rng, g.size, tau, 0.8)
    assert (d == 0).sum() >= g.size // 4 and ((0.25 * tau) * d).max() <= 0.8
    e0 = last = M.modified_energy(g, u, v, c2, tau)
    worst = -np.inf
    for _ in range(2000):
        u, v, _ = S.verlet_sponge(g, u, v, zero, c2, d, tau, 1, unit)
        e = M.modified_energy(g, u, v, c2, tau)
        worst, last = max(worst, e - last), e
    print("N", n, "x", frac, "largest step-to-step change of the modified energy / E[0]", worst / e0, "E[end] / E[0]", last / e0)
    assert e0 > 0 and worst <= 1e-12 * e0 and last < e0


def test_the_scheme_is_second_order_in_tau():
    """A point source with the smooth pulse sin^2(pi t / T) fired into a membrane at rest in a seeded medium with a seeded damping,
    N = 6, 10 and 20 (stretched), integrated to T with tau, tau / 2 and tau / 8.  Against the model at tau / 8 the two errors are
    (1 - 1/64) C tau^2 and (1/4 - 1/64) C tau^2 up to O(tau^4): the ratio of an exact second order is 63 / 15 = 4.2, a first-order
    scheme gives (1 - 1/8) / (1/2 - 1/8) = 2.33, a third-order one 8.1.  The damping is a fixed field that the call would take at the
    member's bound, (0.25 tau_max) d in [0, 0.8], so that tau d <= 0.8 at the coarsest tau = tau_max / 4 and the expansion in tau d
    holds.  The model gives 4.19, 4.17 and 4.18 here, and 4.20, 4.19, 4.20 with twice the steps: the ratio must lie in (3.8, 4.6),
    within a tenth of 4.2 either way -- ten times the O(tau^2) relative correction seen between those two rows, and far from
    every other integer order."""
    for n in (6, 10, 20):
        g = grid(n)
        rng = np.random.default_rng(1300 + n)
        c2 = medium(rng, g.size)
        gv = np.zeros(g.size)
        gv[g.size // 2] = -abs(g.A0)
        T = 16 * M.medium_cfl(g, c2.max())
        d = damping(rng, g.size, T / 16, 0.8)

        def at(steps):
            tau = T / steps
            w = np.sin(np.pi * (np.arange(steps + 1) * tau) / T) ** 2
            return S.verlet_sponge(g, np.zeros(g.size), np.zeros(g.size), gv, c2, d, tau, steps, w)[0]

        coarse, fine, ref = at(64), at(128), at(512)
        e1, e2 = np.linalg.norm(coarse - ref), np.linalg.norm(fine - ref)
        print("N", n, "errors", e1, e2, "ratio", e1 / e2)
        assert np.linalg.norm(ref) > 0 and 3.8 < e1 / e2 < 4.6, n


# ---- sponge_damping on the packed order ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 10, 20])
def test_sponge_damping_on_the_l_shaped_packed_order(n):
    import iterative_solvers_amd as isa
    half, width, dmax = n // 2, 3, 7.5
    nodes = [(ix, iy) for iy in range(1, half + 1) for ix in range(half + 1, n)] + [(ix, iy) for iy in range(half + 1, n) for ix in range(1, n)]
    size = (half - 1) * (3 * half - 1)
    assert len(nodes) == size
    at = {node: i for i, node in enumerate(nodes)}
    dist = {"l": lambda ix, iy: ix - 1, "r": lambda ix, iy: n - 1 - ix, "b": lambda ix, iy: iy - 1, "t": lambda ix, iy: n - 1 - iy}
    for sides in ("lrbt", "l", "rt", "b", "tb"):
        d = isa.sponge_damping(n, width, dmax, sides)
        assert d.shape == (size,) and d.dtype == np.float64
        for (ix, iy), i in at.items():
            k = min(dist[s](ix, iy) for s in sides)
            assert d[i] == (dmax * ((width - k) / width) ** 2 if k < width else 0.0), (sides, ix, iy)
    d = isa.sponge_damping(n, width, dmax)
    assert d.min() == 0.0 or n < 2 * width + 2
    assert d[at[(n - 1, 1)]] == d[at[(1, n - 1)]] == d[at[(half + 2, 1)]] == dmax and d.max() == dmax       # the first interior line
    # symmetric: the mirror image about the diagonal ix = iy maps the L onto itself, left <-> bottom, right <-> top
    for (ix, iy), i in at.items():
        assert d[i] == d[at[(iy, ix)]]
    assert np.array_equal(isa.sponge_damping(n, width, dmax, "lt"), [isa.sponge_damping(n, width, dmax, "br")[at[(iy, ix)]] for ix, iy in nodes])
    one = isa.sponge_damping(n, width, dmax, "r")
    assert one[at[(n - 1, half)]] == dmax and one[at[(1, n - 1)]] == (dmax * ((width - (n - 2)) / width) ** 2 if n - 2 < width else 0.0)
    assert np.array_equal(isa.sponge_damping(n, 1, dmax), np.where(d == dmax, dmax, 0.0))
    assert not isa.sponge_damping(n, width, 0.0).any()
    for bad in ((n, 0, 1.0), (n, 2, -1.0), (n, 2, np.nan), (n, 2, 1.0, "x"), (n, 2, 1.0, ""), (n + 1, 2, 1.0)):
        with pytest.raises(ValueError):
            isa.sponge_damping(*bad)


# ---- the formula, the header, the bindings, the built kernels -----------------------------------------------------------------------
def test_workspace_formula_for_every_even_n(lines):
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    cap = [int(ln[1]) for ln in lines if ln and ln[0] == "cap"][0]
    rows = {int(ln[0][2:]): ln for ln in lines if ln and ln[0].startswith("N=")}
    assert sorted(rows) == list(range(6, cap + 1, 2))
    for n, ln in rows.items():
        unknowns = int(ln[1].split("=")[1])
        assert unknowns == (n // 2 - 1) * (3 * n // 2 - 1)
        entries = [tuple(int(v) for v in e.split(":")) for e in ln[2].split("=")[1].split(",")]
        for nsys, nsteps, nrec, every, nbytes in entries:
            want = nsys * (24 * unknowns + 456) + 8 + 16 * nsys + 8 * unknowns + 4 * 64 + 16 * nsys + 16 * nsys
            assert nbytes == want == isa.wave_medium_many_workspace(n, nsys, nsteps, nrec, every) + 16 * nsys, (n, nsys, nsteps, nrec, every)
            if n in (6, 10, 64, cap) or (nsys, nsteps) == (40, 7):
                out = C.c_longlong()
                assert lib.mi355cg_wave_sponge_many_workspace(n, nsys, nsteps, nrec, every, C.byref(out)) == _capi.OK and out.value == want
                assert isa.wave_sponge_many_workspace(n, nsys, nsteps, nrec, every) == want
    f = isa.wave_sponge_many_workspace
    assert f(10, 5, 3) < f(12, 5, 3) and f(10, 5, 3) < f(10, 6, 3) and f(10, 5, 3) == f(10, 5, 4) == f(10, 5, 4, 64, 2)
    for bad in ((cap + 2, 1, 1), (7, 1, 1), (10, 0, 1), (10, _capi.MANY_MAX + 1, 1), (10, 1, -1), (10, 1, _capi.STEPS_MANY_MAX_STEPS + 1),
                (10, 1, 1, -1), (10, 1, 1, 65), (10, 1, 1, 1, 0), (10, 1, 1, 0, -1)):
        with pytest.raises(ValueError):
            f(*bad)
    assert lib.mi355cg_wave_sponge_many_workspace(10, 1, 1, 0, 1, None) == _capi.ERR_INVALID


def test_header_ctypes_package_and_compat_agree():
    import inspect
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    text = open(os.path.join(ROOT, "include", "mi355cg.h")).read()
    lib = _capi.load()
    for name in ("mi355cg_wave_sponge_many", "mi355cg_wave_sponge_many_device", "mi355cg_wave_sponge_many_workspace"):
        assert name in _capi.EXPORTS and ("int  " + name + "(") in text
        assert hasattr(lib, name)
    doc = text[text.index("with a damping field, for absorbing"):text.index("int  mi355cg_wave_sponge_many(")]
    assert "no reference twin" in doc and "4 / tau_s" in doc
    for fn in (isa.MatrixFreeSystem.wave_record_many, isa.solver._Handle.wave_record_many):
        assert inspect.signature(fn).parameters["damping"].default is None
        assert list(inspect.signature(fn).parameters)[-2:] == ["c2", "damping"]
    assert list(inspect.signature(isa.sponge_damping).parameters) == ["n", "width", "dmax", "sides"] and inspect.signature(isa.sponge_damping).parameters["sides"].default == "lrbt"
    assert callable(isa.MatrixFreeSystem.sponge_damping)
    for name in ("wave_sponge_many_workspace", "sponge_damping"):
        assert callable(getattr(isa, name)) and name in isa.__all__
    compat = open(os.path.join(ROOT, "iterative_solvers_amd", "compat", "mi355cg_compat.hpp")).read()
    assert "waveSpongeMany(" in compat and compat.index("waveMediumMany(") < compat.index("waveSpongeMany(")
    plan = open(os.path.join(ROOT, "iterative_solvers_amd", "csrc", "onchip_plan.h")).read()
    kernels = open(os.path.join(ROOT, "iterative_solvers_amd", "csrc", "onchip_kernels.h")).read()
    assert "MI355CG_HD inline double onchip_wave_sponge_factor(double tau, double d)" in plan and "onchip_wave_sponge_factor(" in kernels
    assert "MI355CG_HD inline double onchip_wave_damp(double s, double v)" in plan and "onchip_wave_damp(" in kernels
    assert "onchip_wave_sponge_workspace_bytes(" in plan
    # the entry points refuse a null handle before they touch a GPU
    for fn in (lib.mi355cg_wave_sponge_many, lib.mi355cg_wave_sponge_many_device):
        assert fn(None, 1, 1, None, None, None, None, None, 0, None, 0, None, 0, 0, None, 1, None, 0, None, None, None) == _capi.ERR_INVALID


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")), reason="needs the ROCm LLVM tools")
def test_the_sponge_kernels_are_built_without_scratch(tmp_path):
    """All six unroll classes are built (the E = 24 class is not refused), none has scratch, none more than 256 VGPRs; the check
    launch is still the one k_oc_medium_range."""
    from iterative_solvers_amd import build as b
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", b.build(), fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={co}"])
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    found, ranges = {}, []
    for entry in notes[notes.index("amdhsa.kernels"):].split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1))
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1))
        m = re.search(r"\d+k_oc_wave_spongeILi(\d+)E", name)
        if m:
            found[int(m.group(1))] = (vgprs, scratch)
        if "k_oc_medium_range" in name:
            ranges.append(scratch)
    print("k_oc_wave_sponge<E>: (VGPRs, scratch)", found)
    assert sorted(found) == [1, 2, 4, 8, 16, 24] and not any(s for _, s in found.values())
    assert all(v <= 256 for v, _ in found.values()) and ranges == [0]
