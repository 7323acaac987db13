"""The recorded explicit wave stepper in a medium, u_tt = c2 o (A u) - w(t) g (csrc/onchip_plan.h), without a
GPU.  tests/cpp/onchip_wave_medium_plan_driver.cpp, a program of its own built with the sanitizers, (1) evaluates the new
expressions and runs whole steps -- the carried acceleration included -- with the functions the kernel calls, which is compared bit
for bit with the NumPy model of tests/wave_medium_reference.py, and (2) restates the workspace formula for every even N from 6 to
the cap.  The model's own properties are checked here too: a unit medium is the recorded stepper, c2 = 4 is a rescaled plain run,
a run may be split at a multiple of the cadence, the modified energy is conserved, the scheme is second order in tau and the
bound is sufficient.  The header, the ctypes layer, the package and the built kernels must agree on the new entry points."""
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
import wave_record_reference as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE, STRETCHED = (1.0, 2.0, 1.0, 2.0), (0.0, 1.0, 0.0, 1.7)
LLVM = os.path.join(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")), "..", "lib", "llvm", "bin")


def grid(n):
    """N = 20 is stretched: xk != yk."""
    return M.Grid.of_domain(n, *(STRETCHED if n == 20 else SQUARE))


def medium(rng, shape):
    """A seeded medium in [0.25, 4]: wave speeds between a half and two."""
    return rng.uniform(0.25, 4.0, shape)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("onchip_wave_medium") / "onchip_wave_medium_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "onchip_wave_medium_plan_driver.cpp"), "-o", exe])
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


def run_driver(driver, tmp_path, g, tau, nsteps, u, gv, v, c2, w, receivers, every):
    got = run_file(driver, tmp_path, [[float(g.n), tau, float(nsteps), g.A0, g.xk, g.yk, float(every), float(len(receivers))], g.image(u), gv, v, c2, w,
                                      np.asarray(receivers, dtype=np.float64)])
    samples = nsteps // every
    assert got.shape == (2 * g.size + samples * len(receivers),)
    return got[:g.size], got[g.size:2 * g.size], got[2 * g.size:].reshape(samples, len(receivers))


def seeded(g, seed, nsteps):
    """(u, v, g, c2, w, receivers): states and a forcing over seven decades, a medium in [0.25, 4], amplitudes of either sign, five
    receivers with both ends."""
    rng = np.random.default_rng(seed)
    scale = lambda: 10.0 ** rng.integers(-3, 4, g.size)
    u, v, gv = (rng.standard_normal(g.size) * scale() for _ in range(3))
    c2 = medium(rng, g.size)
    w = rng.standard_normal(nsteps + 1) * 10.0 ** rng.integers(-2, 3, nsteps + 1)
    receivers = [int(r) for r in rng.integers(0, g.size, 3)] + [0, g.size - 1]
    return u, v, gv, c2, w, receivers


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- the expressions and whole steps against the driver ----------------------------------------------------------------------------
def test_the_acceleration_is_two_roundings_after_the_stencil(driver, tmp_path):
    rng = np.random.default_rng(11)
    k = (-1234.5678, 300.1, 317.1839)
    cols = [medium(rng, 600)] + [rng.standard_normal(600) * 10.0 ** rng.integers(-3, 4, 600) for _ in range(6)]
    cols[0][:4] = [1.0, 4.0, 0.25, 1.0]
    got = run_file(driver, tmp_path, [[600.0, *k]] + cols, "accel")
    c2, f, uc, left, right, down, up = cols
    t = k[0] * uc + k[1] * (left + right) + k[2] * (down + up)
    assert np.array_equal(got, c2 * t - f)
    assert got[0] == t[0] - f[0] and got[3] == t[3] - f[3]                 # a unit entry: the homogeneous expression


def test_the_bound_is_the_homogeneous_one_for_a_unit_medium(driver, tmp_path):
    rng = np.random.default_rng(12)
    A0 = -np.concatenate([[grid(n).A0 * -1 for n in (6, 10, 20)], rng.uniform(1.0, 1e7, 200)])
    top = np.concatenate([[1.0, 1.0, 1.0], medium(rng, 200)])
    got = run_file(driver, tmp_path, [[float(len(A0))], A0, top], "cfl")
    assert np.array_equal(got, 2.0 / np.sqrt(2.0 * np.abs(A0) * top))
    for i, n in enumerate((6, 10, 20)):
        g = grid(n)
        assert got[i] == g.cfl() == M.medium_cfl(g, 1.0)
    g = grid(10)
    assert np.array_equal(M.medium_cfl(g, np.array([1.0, 4.0])), [g.cfl(), 0.5 * g.cfl()])     # c2max = 4: half the step, exactly


@pytest.mark.parametrize("n", [6, 10, 20])
def test_steps_in_a_medium_are_the_models_operation_by_operation(driver, tmp_path, n):
    g = grid(n)
    assert (g.xk != g.yk) == (n == 20)
    for frac, nsteps, every in ((0.37, 1, 1), (1.0, 7, 3), (0.81, 0, 2), (0.5, 6, 2)):
        u, v, gv, c2, w, receivers = seeded(g, 700 + n + nsteps, nsteps)
        tau = frac * M.medium_cfl(g, c2.max())
        got = run_driver(driver, tmp_path, g, tau, nsteps, u, gv, v, c2, w, receivers, every)
        want = M.verlet_medium(g, u, v, gv, c2, tau, nsteps, w, receivers, every)
        assert same(got, want), (n, frac, nsteps)
        assert got[2].shape == (nsteps // every, 5)
    # one step, written out once more without the model's loop
    u, v, gv, c2, w, receivers = seeded(g, 800 + n, 1)
    tau = 0.37 * M.medium_cfl(g, c2.max())
    h = 0.5 * tau
    f = w[0] * gv
    t = g.au(u)
    a = c2 * t - f
    vh = v + h * a
    un = u + tau * vh
    f = w[1] * gv
    t = g.au(un)
    vn = vh + h * (c2 * t - f)
    got = run_driver(driver, tmp_path, g, tau, 1, u, gv, v, c2, w, receivers, 1)
    assert np.array_equal(got[0], un) and np.array_equal(got[1], vn) and np.array_equal(got[2], un[receivers][None, :])
    # the acceleration a step leaves is the one the next call forms anew: three calls of one step are one call of three
    u, v, gv, c2, w, receivers = seeded(g, 900 + n, 3)
    one = (u, v)
    for k in range(3):
        one = run_driver(driver, tmp_path, g, tau, 1, one[0], gv, one[1], c2, w[k:k + 2], receivers, 1)
    three = run_driver(driver, tmp_path, g, tau, 3, u, gv, v, c2, w, receivers, 1)
    assert np.array_equal(one[0], three[0]) and np.array_equal(one[1], three[1]) and np.array_equal(one[2][0], three[2][2])


def test_the_driver_found_no_violation(lines):
    assert not [ln for ln in lines if ln and ln[0] == "FAIL"]
    assert lines[-1] == ["ok", "0"]


# ---- the model's own properties ------------------------------------------------------------------------------------------------------
def ensemble(g, seed, members, nsteps, shared=False):
    rng = np.random.default_rng(seed)
    u, v = rng.standard_normal((members, g.size)), rng.standard_normal((members, g.size)) * np.sqrt(abs(g.A0))
    gv = rng.standard_normal((members, g.size)) * abs(g.A0)
    c2 = medium(rng, g.size if shared else (members, g.size))
    tau = M.medium_cfl(g, c2.max(axis=-1)) * rng.uniform(0.1, 1.0, members)
    w = rng.standard_normal((members, nsteps + 1))
    receivers = [int(r) for r in rng.integers(0, g.size, 3)] + [0, g.size - 1]
    return u, v, gv, c2, tau, w, receivers


@pytest.mark.parametrize("n", [6, 10, 20])
def test_a_unit_medium_is_the_recorded_stepper(n):
    g = grid(n)
    u, v, gv, _, tau, w, receivers = ensemble(g, 1000 + n, 4, 23)
    want = R.verlet_record(g, u, v, gv, tau, 23, w, receivers, 3)
    for c2 in (np.ones(g.size), np.ones((4, g.size))):
        assert same(M.verlet_medium(g, u, v, gv, c2, tau, 23, w, receivers, 3), want)
    assert same(M.verlet_medium(g, u[1], v[1], gv[1], np.ones(g.size), float(tau[1]), 23, w[1], receivers, 3), [x[1] for x in want])


@pytest.mark.parametrize("n", [6, 10, 20])
def test_a_medium_of_four_is_the_plain_run_rescaled(n):
    """Every scaling by a power of two is exact: c2 = 4 with (tau, v0, g) gives the u of the plain call with (2 tau, v0 / 2, g / 4)
    and twice its v, bit for bit."""
    g = grid(n)
    u, v, gv, _, tau, w, receivers = ensemble(g, 1050 + n, 4, 40)
    tau = 0.5 * tau                                                  # c2max = 4 halves the bound
    got = M.verlet_medium(g, u, v, gv, np.full(g.size, 4.0), tau, 40, w, receivers, 3)
    plain = R.verlet_record(g, u, 0.5 * v, 0.25 * gv, 2.0 * tau, 40, w, receivers, 3)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], 2.0 * plain[1]) and np.array_equal(got[2], plain[2])
    assert not np.array_equal(got[0], u)


@pytest.mark.parametrize("n", [6, 10, 20])
def test_a_run_split_at_a_multiple_of_the_cadence_is_the_whole_run(n):
    g = grid(n)
    nsteps, every = 23, 3
    u, v, gv, c2, tau, w, receivers = ensemble(g, 1100 + n, 4, nsteps)
    whole = M.verlet_medium(g, u, v, gv, c2, tau, nsteps, w, receivers, every)
    assert whole[2].shape == (4, 7, 5)
    for cut in (3, 12, 21):
        a = M.verlet_medium(g, u, v, gv, c2, tau, cut, w[:, :cut + 1], receivers, every)
        b = M.verlet_medium(g, a[0], a[1], gv, c2, tau, nsteps - cut, w[:, cut:], receivers, every)
        assert same(b[:2], whole[:2]) and np.array_equal(np.concatenate([a[2], b[2]], axis=1), whole[2]), cut
    # a shared medium is that medium for every member
    shared = M.verlet_medium(g, u, v, gv, c2[2], tau, nsteps, w, receivers, every)
    assert same(shared, M.verlet_medium(g, u, v, gv, np.stack([c2[2]] * 4), tau, nsteps, w, receivers, every))
    assert same([x[2] for x in shared], M.verlet_medium(g, u[2], v[2], gv[2], c2[2], float(tau[2]), nsteps, w[2], receivers, every))


@pytest.mark.parametrize("n", [6, 10, 20])
def test_the_modified_energy_is_conserved(n):
    """Without a forcing the scheme conserves 1/2 v^T C^-1 v - 1/2 u^T A u - (tau^2 / 8) a^T C^-1 a, a = c2 au(u): within 1e-12
    relative over 2000 steps at half the bound (the bound DESIGN section 12.3 holds its invariants to); the plain energy moves
    by per cents."""
    g = grid(n)
    rng = np.random.default_rng(1200 + n)
    c2 = medium(rng, g.size)
    u, v = rng.standard_normal(g.size), rng.standard_normal(g.size) * np.sqrt(abs(g.A0))
    zero, unit = np.zeros(g.size), np.ones(2)
    tau = 0.5 * M.medium_cfl(g, c2.max())
    e0, p0 = M.modified_energy(g, u, v, c2, tau), M.plain_energy(g, u, v, c2)
    worst = moved = 0.0
    for _ in range(2000):
        u, v, _ = M.verlet_medium(g, u, v, zero, c2, tau, 1, unit)
        worst = max(worst, abs(M.modified_energy(g, u, v, c2, tau) - e0) / abs(e0))
        moved = max(moved, abs(M.plain_energy(g, u, v, c2) - p0) / abs(p0))
    print("N", n, "modified energy: relative deviation", worst, "plain energy", moved)
    assert worst <= 1e-12 and moved > 1e-3


def test_the_scheme_is_second_order_in_tau():
    """A point source with the smooth pulse sin^2(pi t / T) fired into a membrane at rest in a seeded medium, N = 10, integrated to
    T with tau, tau / 2 and tau / 8.  Against the model at tau / 8 the two errors are (1 - 1/64) C tau^2 and (1/4 - 1/64) C tau^2:
    the ratio of an exact second order is 4.2, and it lies in (3, 5)."""
    g = M.Grid.of_domain(10, *SQUARE)
    c2 = medium(np.random.default_rng(1300), g.size)
    gv = np.zeros(g.size)
    gv[g.size // 2] = -abs(g.A0)
    T = 16 * M.medium_cfl(g, c2.max())

    def at(steps):
        tau = T / steps
        w = np.sin(np.pi * (np.arange(steps + 1) * tau) / T) ** 2
        return M.verlet_medium(g, np.zeros(g.size), np.zeros(g.size), gv, c2, tau, steps, w)[0]

    coarse, fine, ref = at(64), at(128), at(512)
    e1, e2 = np.linalg.norm(coarse - ref), np.linalg.norm(fine - ref)
    print("errors", e1, e2, "ratio", e1 / e2)
    assert np.linalg.norm(ref) > 0 and 3.0 < e1 / e2 < 5.0


@pytest.mark.parametrize("n", [10, 20])
def test_the_bound_is_sufficient_and_not_far_from_sharp(n):
    """-C A is similar to the symmetric C^(1/2) (-A) C^(1/2) with eigenvalues in [0, 2 |A0| max c2]: at 1.0 x the bound the model
    stays bounded over 4000 steps, at 1.3 x it overflows."""
    g = grid(n)
    rng = np.random.default_rng(1400 + n)
    c2 = medium(rng, g.size)
    u0, v0 = rng.standard_normal(g.size), rng.standard_normal(g.size) * np.sqrt(abs(g.A0))
    zero, unit = np.zeros(g.size), np.ones(4001)
    bound = M.medium_cfl(g, c2.max())
    with np.errstate(over="ignore", invalid="ignore"):
        at = M.verlet_medium(g, u0, v0, zero, c2, bound, 4000, unit, range(g.size), 100)
        beyond = M.verlet_medium(g, u0, v0, zero, c2, 1.3 * bound, 4000, unit)
    print("N", n, "max |u| over the run at the bound", float(np.abs(at[2]).max()), "of", float(np.abs(u0).max()))
    assert np.all(np.isfinite(at[0])) and np.all(np.isfinite(at[1])) and np.abs(at[2]).max() <= 1e3 * np.abs(u0).max()
    assert not np.all(np.isfinite(beyond[0]))


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
            want = nsys * (24 * unknowns + 456) + 8 + 16 * nsys + 8 * unknowns + 4 * 64 + 16 * nsys
            assert nbytes == want == isa.wave_record_many_workspace(n, nsys, nsteps, nrec, every) + 16 * nsys, (n, nsys, nsteps, nrec, every)
            if n in (6, 10, 64, cap) or (nsys, nsteps) == (40, 7):
                out = C.c_longlong()
                assert lib.mi355cg_wave_medium_many_workspace(n, nsys, nsteps, nrec, every, C.byref(out)) == _capi.OK and out.value == want
                assert isa.wave_medium_many_workspace(n, nsys, nsteps, nrec, every) == want
    f = isa.wave_medium_many_workspace
    assert f(10, 5, 3) < f(12, 5, 3) and f(10, 5, 3) < f(10, 6, 3) and f(10, 5, 3) == f(10, 5, 4) == f(10, 5, 4, 64, 2)
    for bad in ((cap + 2, 1, 1), (7, 1, 1), (10, 0, 1), (10, _capi.MANY_MAX + 1, 1), (10, 1, -1), (10, 1, _capi.STEPS_MANY_MAX_STEPS + 1),
                (10, 1, 1, -1), (10, 1, 1, 65), (10, 1, 1, 1, 0), (10, 1, 1, 0, -1)):
        with pytest.raises(ValueError):
            f(*bad)
    assert lib.mi355cg_wave_medium_many_workspace(10, 1, 1, 0, 1, None) == _capi.ERR_INVALID


def test_header_ctypes_package_and_compat_agree():
    import inspect
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    text = open(os.path.join(ROOT, "include", "mi355cg.h")).read()
    lib = _capi.load()
    for name in ("mi355cg_wave_medium_many", "mi355cg_wave_medium_many_device", "mi355cg_wave_medium_many_workspace", "mi355cg_wave_medium_cfl"):
        assert name in _capi.EXPORTS and ("int  " + name + "(") in text
        assert hasattr(lib, name)
    assert "no reference twin" in text[text.index("The recorded explicit scheme in a medium"):text.index("int  mi355cg_wave_medium_many(")]
    for fn in (isa.MatrixFreeSystem.wave_record_many, isa.MatrixFreeSystem.wave_cfl):
        assert inspect.signature(fn).parameters["c2"].default is None
    assert callable(isa.wave_medium_many_workspace) and "wave_medium_many_workspace" in isa.__all__
    compat = open(os.path.join(ROOT, "iterative_solvers_amd", "compat", "mi355cg_compat.hpp")).read()
    assert "waveMediumMany(" in compat and "waveCfl(double c2max)" in compat
    plan = open(os.path.join(ROOT, "iterative_solvers_amd", "csrc", "onchip_plan.h")).read()
    kernels = open(os.path.join(ROOT, "iterative_solvers_amd", "csrc", "onchip_kernels.h")).read()
    assert "MI355CG_HD inline double onchip_wave_medium_accel(" in plan and "onchip_wave_medium_accel(" in kernels
    assert "onchip_wave_medium_cfl(" in plan and "onchip_wave_medium_workspace_bytes(" in plan
    # the entry points refuse a null handle before they touch a GPU
    for fn in (lib.mi355cg_wave_medium_many, lib.mi355cg_wave_medium_many_device):
        assert fn(None, 1, 1, None, None, None, None, None, 0, None, 0, 0, None, 1, None, 0, None, None, None) == _capi.ERR_INVALID
    out = C.c_double()
    assert lib.mi355cg_wave_medium_cfl(None, 1.0, C.byref(out)) == _capi.ERR_INVALID


# k_onchip_wave_verlet<E> and k_oc_wave_record<E> as the parent built them: the kernels of the other two calls stay the code they were
PLAIN_VGPRS = {1: 20, 2: 26, 4: 40, 8: 76, 16: 148, 24: 180}
RECORD_VGPRS = {1: 30, 2: 38, 4: 50, 8: 78, 16: 134, 24: 190}


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")), reason="needs the ROCm LLVM tools")
def test_the_medium_kernels_are_built_without_scratch_and_the_others_are_unchanged(tmp_path):
    from iterative_solvers_amd import build as b
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", b.build(), fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={co}"])
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    found = {"k_oc_wave_medium": {}, "k_oc_wave_record": {}, "k_onchip_wave_verlet": {}}
    ranges = []
    for entry in notes[notes.index("amdhsa.kernels"):].split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1))
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1))
        m = re.search(r"\d+(k_oc_wave_medium|k_oc_wave_record|k_onchip_wave_verlet)ILi(\d+)E", name)
        if m:
            found[m.group(1)][int(m.group(2))] = (vgprs, scratch)
        if "k_oc_medium_range" in name:
            ranges.append(scratch)
    print("k_oc_wave_medium<E>: (VGPRs, scratch)", found["k_oc_wave_medium"])
    for kernels in found.values():
        assert sorted(kernels) == [1, 2, 4, 8, 16, 24] and not any(s for _, s in kernels.values())
    assert all(v <= 256 for v, _ in found["k_oc_wave_medium"].values()) and ranges == [0]
    assert {e: v for e, (v, _) in found["k_onchip_wave_verlet"].items()} == PLAIN_VGPRS
    assert {e: v for e, (v, _) in found["k_oc_wave_record"].items()} == RECORD_VGPRS
