"""The host arithmetic of the on-chip wave steppers (csrc/onchip_plan.h) without a GPU.
tests/cpp/onchip_wave_plan_driver.cpp, a program of its own built with the sanitizers, (1) runs the per-node expressions the two
kernels call -- whole Verlet steps with the carried acceleration, the Newmark right-hand side and velocity -- over a seeded image,
which is compared bit for bit with the NumPy model of tests/wave_reference.py, and (2) restates the workspace formula for every even
N from 6 to the cap.  The model's own invariants are checked here too: the energies the two schemes conserve.  The header, the
ctypes layer and the package must agree on the new entry points."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_reference as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE, STRETCHED = (1.0, 2.0, 1.0, 2.0), (0.0, 1.0, 0.0, 1.7)


def grid(n):
    """N = 20 is stretched: xk != yk."""
    return W.Grid.of_domain(n, *(STRETCHED if n == 20 else SQUARE))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("onchip_wave") / "onchip_wave_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "onchip_wave_plan_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def lines(driver):
    out = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    return [ln.split() for ln in out.stdout.splitlines()]


def run_driver(driver, tmp_path, g, scheme, tau, nsteps, u, gv, v, x):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([[float(g.n), float(scheme), tau, float(nsteps), g.A0, g.xk, g.yk], g.image(u), gv, v, x]).astype(np.float64).tofile(src)
    out = subprocess.run([driver, src, dst], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-2000:]
    got = np.fromfile(dst, dtype=np.float64)
    assert got.shape == (2 * g.size,)
    return got[:g.size], got[g.size:]


def seeded(g, seed):
    rng = np.random.default_rng(seed)
    scale = lambda: 10.0 ** rng.integers(-3, 4, g.size)
    return [rng.standard_normal(g.size) * scale() for _ in range(4)]


@pytest.mark.parametrize("n", [6, 10, 20])
def test_verlet_steps_are_the_models_operation_by_operation(driver, tmp_path, n):
    g = grid(n)
    assert (g.xk != g.yk) == (n == 20) and g.size == (n // 2 - 1) * (3 * n // 2 - 1)
    u, v, gv, x = seeded(g, 300 + n)
    for frac, nsteps in ((0.37, 1), (1.0, 5), (0.81, 0)):
        tau = frac * g.cfl()
        got_u, got_v = run_driver(driver, tmp_path, g, 0, tau, nsteps, u, gv, v, x)
        want_u, want_v = W.verlet(g, u, v, gv, tau, nsteps)
        assert np.array_equal(got_u, want_u) and np.array_equal(got_v, want_v), (n, frac, nsteps)
    # one step, written out once more without the model's loop
    tau = 0.37 * g.cfl()
    h = 0.5 * tau
    a = g.au(u) - gv
    vh = v + h * a
    un = u + tau * vh
    vn = vh + h * (g.au(un) - gv)
    got_u, got_v = run_driver(driver, tmp_path, g, 0, tau, 1, u, gv, v, x)
    assert np.array_equal(got_u, un) and np.array_equal(got_v, vn)
    # k steps are k times one step, bit for bit: the carried acceleration is a function of (u, g)
    one = (u, v)
    for _ in range(3):
        one = run_driver(driver, tmp_path, g, 0, tau, 1, one[0], gv, one[1], x)
    three = run_driver(driver, tmp_path, g, 0, tau, 3, u, gv, v, x)
    assert np.array_equal(one[0], three[0]) and np.array_equal(one[1], three[1])


@pytest.mark.parametrize("n", [6, 10, 20])
def test_newmark_expressions_are_the_models_operation_by_operation(driver, tmp_path, n):
    g = grid(n)
    u, v, gv, x = seeded(g, 400 + n)
    for tau in (0.013, 3.0 * g.cfl(), 7.5):
        got_b, got_v = run_driver(driver, tmp_path, g, 1, tau, 1, u, gv, v, x)
        sigma, hv = 4.0 / (tau * tau), 2.0 / tau
        w = u + tau * v
        b = (gv + gv) - sigma * w
        img, c, p = g.image(u), g.cells, g.pitch
        au = g.A0 * img[c] + g.xk * (img[c - 1] + img[c + 1])
        au = au + g.yk * (img[c - p] + img[c + p])
        b = b - au
        assert np.array_equal(got_b, b) and np.array_equal(got_b, W.newmark_rhs(g, u, v, gv, tau))
        assert np.array_equal(got_v, hv * (x - u) - v) and np.array_equal(got_v, W.newmark_velocity(tau, x, u, v))


def test_the_driver_found_no_violation(lines):
    assert not [ln for ln in lines if ln and ln[0] == "FAIL"]
    assert lines[-1] == ["ok", "0"]


def test_workspace_formula_header_ctypes_and_package_agree(lines):
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
        assert {e[2] for e in entries} == {0, 1} and {e[3] for e in entries} == {0, 1}
        for nsys, nsteps, scheme, with_counts, nbytes in entries:
            want = nsys * (24 * unknowns + 456) + 8 + 16 * nsys + 8 * unknowns
            if scheme == _capi.WAVE_NEWMARK:
                want += 16 * nsys + (4 * nsys * nsteps if with_counts else 0)
                assert want == isa.time_steps_many_workspace(n, nsys, nsteps, bool(with_counts)) + 16 * nsys
            assert nbytes == want, (n, nsys, nsteps, scheme, with_counts)
            if n in (6, 10, 64, cap) or (nsys, nsteps) == (40, 7):
                out = C.c_longlong()
                assert lib.mi355cg_wave_steps_many_workspace(n, nsys, nsteps, scheme, with_counts, C.byref(out)) == _capi.OK and out.value == want
                assert isa.wave_steps_many_workspace(n, nsys, nsteps, scheme, bool(with_counts)) == want
    f = isa.wave_steps_many_workspace
    assert f(10, 5, 3) < f(12, 5, 3) and f(10, 5, 3) < f(10, 6, 3) and f(10, 5, 3) == f(10, 5, 4) == f(10, 5, 4, _capi.WAVE_VERLET, True)
    assert f(10, 5, 3) < f(10, 5, 3, _capi.WAVE_NEWMARK) < f(10, 5, 3, _capi.WAVE_NEWMARK, True) < f(10, 5, 4, _capi.WAVE_NEWMARK, True)
    for bad in ((cap + 2, 1, 1), (7, 1, 1), (10, 0, 1), (10, _capi.MANY_MAX + 1, 1), (10, 1, -1), (10, 1, _capi.STEPS_MANY_MAX_STEPS + 1),
                (10, 1, 1, 2), (10, 1, 1, -1), (10, 1025, 65536, _capi.WAVE_NEWMARK, True)):
        with pytest.raises(ValueError):
            f(*bad)
    assert f(10, 1024, 65536, _capi.WAVE_NEWMARK, True) > 0 and f(10, 1025, 65536, _capi.WAVE_NEWMARK) > 0
    assert lib.mi355cg_wave_steps_many_workspace(10, 1, 1, 0, 0, None) == _capi.ERR_INVALID


def test_header_ctypes_package_and_compat_agree():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    text = open(os.path.join(ROOT, "include", "mi355cg.h")).read()
    assert "#define MI355CG_WAVE_VERLET  0" in text and "#define MI355CG_WAVE_NEWMARK 1" in text
    assert (isa.WAVE_VERLET, isa.WAVE_NEWMARK) == (_capi.WAVE_VERLET, _capi.WAVE_NEWMARK) == (0, 1)
    for name in ("mi355cg_wave_steps_many", "mi355cg_wave_steps_many_device", "mi355cg_wave_steps_many_workspace", "mi355cg_wave_cfl"):
        assert name in _capi.EXPORTS and ("int  " + name + "(") in text
        assert hasattr(_capi.load(), name)
    assert callable(isa.MatrixFreeSystem.wave_steps_many) and callable(isa.MatrixFreeSystem.wave_cfl) and callable(isa.wave_steps_many_workspace)
    compat = open(os.path.join(ROOT, "iterative_solvers_amd", "compat", "mi355cg_compat.hpp")).read()
    assert "waveStepsMany(" in compat and "waveCfl(" in compat
    # the entry points refuse a null handle before they touch a GPU
    lib, out = _capi.load(), C.c_double()
    assert lib.mi355cg_wave_cfl(None, C.byref(out)) == _capi.ERR_INVALID
    assert lib.mi355cg_wave_steps_many(None, None, 1, 1, 0, None, None, None, None, 0, None, None, None, None) == _capi.ERR_INVALID


def test_the_bound_on_tau_is_gershgorins(lines):
    """onchip_wave_cfl, as the driver evaluates it for square and stretched grids, is 2 / sqrt(2 |A_diag|): every eigenvalue of -A lies
    in [0, 2 |A_diag|] (the off-diagonal row sums are at most |A_diag|), and velocity Verlet is stable while tau^2 lambda <= 4.  The
    model's bound is the same number.  (mi355cg_wave_cfl on a handle: tests/test_gpu_wave_many.py.)"""
    rows = [ln for ln in lines if ln and ln[0] == "cfl"]
    assert len(rows) == 8 and {int(ln[1]) for ln in rows} == {6, 10, 20, 64}
    for ln in rows:
        n = int(ln[1])
        width, height, diag, bound = (float.fromhex(v) for v in ln[2:])
        g = W.Grid.of_domain(n, 0.0, width, 0.0, height)
        assert diag == g.A0 == -2 * (g.xk + g.yk) and (g.xk != g.yk) == (height != 1.0)
        assert bound == 2.0 / np.sqrt(2.0 * abs(diag)) == g.cfl()
        assert bound * bound * (2.0 * abs(diag)) <= 4.0 * (1 + 4e-16)


# ---- the model's own invariants ------------------------------------------------------------------------------------------------------
# Tolerance: relative deviation <= 1e-12.  Measured with these seeds: <= 1.5e-14 for Verlet over 2000 steps, <= 5e-15 for Newmark
# over 20 steps; the margin of roughly 100 x covers other seeds.
TOL = 1e-12


@pytest.mark.parametrize("n", [6, 10, 20])
@pytest.mark.parametrize("frac", [0.5, 1.0])
def test_verlet_conserves_its_modified_energy(n, frac):
    g = grid(n)
    rng = np.random.default_rng(500 + n)
    u, v, gv = rng.standard_normal(g.size), rng.standard_normal(g.size) * np.sqrt(abs(g.A0)), rng.standard_normal(g.size) * abs(g.A0)
    tau = frac * g.cfl()
    e0 = W.verlet_energy(g, u, v, gv, tau)
    worst = 0.0
    for _ in range(20):                                   # 2000 steps, the invariant read every 100
        u, v = W.verlet(g, u, v, gv, tau, 100)
        assert np.all(np.isfinite(u)) and np.all(np.isfinite(v))
        worst = max(worst, abs(W.verlet_energy(g, u, v, gv, tau) - e0) / abs(e0))
    print("verlet N", n, "tau / bound", frac, "relative deviation of the modified energy", worst)
    assert worst <= TOL


@pytest.mark.parametrize("n", [6, 10, 20])
def test_newmark_conserves_the_energy(n):
    g = grid(n)
    rng = np.random.default_rng(600 + n)
    u, v, gv = rng.standard_normal(g.size), rng.standard_normal(g.size) * np.sqrt(abs(g.A0)), rng.standard_normal(g.size) * abs(g.A0)
    tau = 3.0 * g.cfl()                                   # beyond the explicit bound: the scheme is unconditionally stable
    e0 = W.energy(g, u, v, gv)
    worst = 0.0
    for _ in range(20):
        u, v = W.newmark(g, u, v, gv, tau, 1, tol=1e-12)
        worst = max(worst, abs(W.energy(g, u, v, gv) - e0) / abs(e0))
    print("newmark N", n, "relative deviation of the energy", worst)
    assert worst <= TOL
