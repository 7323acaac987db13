"""The block eigensolver on the GPU (mi355cg_eigs / _device, mi355cg_block_gram, mi355cg_block_combine): the
two block kernels against NumPy with the rounding bound of a sum in any order, the eigenpairs against numpy.linalg.eigvalsh of
the dense operator (built from apply() on unit vectors), the iteration counts against the NumPy restatement
(tests/eigs_reference.py) from the same start block, and the rules of the interface: locking, stop, determinism, isolation from
the handle's solves, refusals."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eigs_reference as er  # noqa: E402

pytestmark = pytest.mark.gpu

DOM = (1.0, 2.0, 1.0, 2.0)
U53 = 2.0 ** -53
GRIDS = [(16, "mg"), (34, "any"), (64, "mg")]          # one level; non-nested; two nested levels
CASES = [(1, 1), (6, 8), (16, 16)]


def system(N, kind="any", dom=DOM, precond=True):
    import iterative_solvers_amd as isa
    s = isa.MatrixFreeSystem(N, N, *dom)
    if precond:
        s.set_preconditioner(isa.PRECOND_MG if kind == "mg" else isa.PRECOND_MG_ANY)
    return s


@functools.lru_cache(maxsize=None)
def dense_spectrum(N):
    """eigvalsh of -A, A assembled column by column from apply() on unit vectors"""
    s = system(N, precond=False)
    n = s.size()
    A = np.empty((n, n))
    e = np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        A[:, j] = s.apply(e)
        e[j] = 0.0
    lam = np.linalg.eigvalsh(-0.5 * (A + A.T))
    lam.setflags(write=False)
    return lam


def start_block(m, size, seed=0):
    return np.random.default_rng(seed).standard_normal((m, size))


@functools.lru_cache(maxsize=None)
def restatement_iterations(N, nev, m):
    levels = er.levels_for(N, DOM)
    _, _, info = er.lobpcg(levels, start_block(m, int(levels[0].mask.sum())), nev, tol=1e-8)
    assert info["converged"]
    return info["iterations"]


# ---- the block kernels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 34, 258])
@pytest.mark.parametrize("na, nb", [(1, 1), (3, 5), (8, 8), (16, 48), (48, 48)])
def test_block_gram_against_numpy(N, na, nb):
    s = system(N, precond=False)
    rng = np.random.default_rng(1000 * N + 50 * na + nb)
    a, b = rng.standard_normal((na, s.size())), rng.standard_normal((nb, s.size()))
    c = s.block_gram(a, b)
    ref = a @ b.T
    bound = s.size() * U53 * (np.abs(a) @ np.abs(b).T)
    err = np.abs(c - ref)
    print("max error / bound:", (err / bound).max())
    assert c.shape == (na, nb) and np.all(err <= bound)
    assert np.array_equal(c, s.block_gram(a, b))                      # a fixed order: the same bits


@pytest.mark.parametrize("N", [16, 258])
def test_block_gram_index_lists_with_gaps_select_rows_and_columns(N):
    s = system(N, precond=False)
    rng = np.random.default_rng(N)
    a, b = rng.standard_normal((11, s.size())), rng.standard_normal((14, s.size()))
    full = s.block_gram(a, b)
    rows, cols = [0, 2, 3, 7, 10], [1, 4, 5, 6, 9, 13]
    part = s.block_gram(a, b, rows=rows, cols=cols)
    assert np.array_equal(part, full[np.ix_(rows, cols)])
    assert np.array_equal(s.block_gram(a, b, rows=[10, 0]), full[[10, 0]])
    with pytest.raises(ValueError, match="outside"):
        s.block_gram(a, b, rows=[11])


@pytest.mark.parametrize("N", [16, 34, 258])
@pytest.mark.parametrize("k, m", [(1, 1), (5, 3), (24, 8), (48, 16)])
def test_block_combine_against_numpy(N, k, m):
    s = system(N, precond=False)
    rng = np.random.default_rng(1000 * N + 50 * k + m)
    S, coef = rng.standard_normal((k, s.size())), rng.standard_normal((k, m))
    y = s.block_combine(S, coef)
    ref = coef.T @ S
    bound = k * U53 * (np.abs(coef).T @ np.abs(S))
    err = np.abs(y - ref)
    print("max error / bound:", (err / bound).max())
    assert y.shape == (m, s.size()) and np.all(err <= bound)
    assert np.array_equal(y, s.block_combine(S, coef))


# ---- eigenpairs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, kind", GRIDS)
@pytest.mark.parametrize("nev, block", CASES)
def test_eigenpairs_against_the_dense_operator(N, kind, nev, block):
    import iterative_solvers_amd as isa
    s = system(N, kind)
    ref = dense_spectrum(N)[:nev]
    x0 = start_block(block, s.size())
    lam, V, info = s.eigs(nev, block=block, tol=1e-8, x0=x0)
    cap = 2 * restatement_iterations(N, nev, block)
    print("iterations", info["iterations"], "restatement x 2", cap, "p_drops", info["p_drops"], "rel err", np.abs(lam - ref).max() / ref.max())
    assert info["converged"] and info["stop_reason"] == isa.EIG_CONVERGED
    assert lam.shape == (nev,) and V.shape == (nev, s.size())
    assert np.all(np.diff(lam) >= 0) and np.all(lam > 0)
    assert np.all(np.abs(lam - ref) <= 1e-9 * ref)
    assert info["iterations"] <= cap
    for j in range(nev):                                              # (A v + lam v), recomputed with apply()
        r = s.apply(V[j]) + lam[j] * V[j]
        assert np.linalg.norm(r) <= 2 * 1e-8 * lam[j] * np.linalg.norm(V[j])
    assert np.abs(V @ V.T - np.eye(nev)).max() <= 1e-12
    assert np.all(info["residuals"][:nev] <= 1e-8)


def test_n258_converges_within_40_iterations():
    s = system(258, "any")
    lam, V, info = s.eigs(6, block=8, tol=1e-8)
    print("iterations", info["iterations"], "lam", lam)
    assert info["converged"] and info["iterations"] <= 40
    for j in range(6):
        assert np.linalg.norm(s.apply(V[j]) + lam[j] * V[j]) <= 2e-8 * lam[j] * np.linalg.norm(V[j])


def test_first_eigenvalue_of_the_l_shaped_membrane():
    """lambda_1 = 9.6397238440219 on the L inside [-1, 1]^2; the 5-point value at N = 256 is 9.64281 (an O(h^(4/3)) corner error)"""
    s = system(256, "mg", dom=(-1.0, 1.0, -1.0, 1.0))
    lam, _, info = s.eigs(1, tol=1e-8)
    print("lambda_1 =", lam[0], "iterations", info["iterations"])
    assert info["converged"] and abs(lam[0] - 9.6397238440219) <= 5e-3


def test_shift_adds_sigma_and_is_left_alone():
    s = system(34, "any")
    x0 = start_block(8, s.size())
    lam0, _, info0 = s.eigs(6, block=8, x0=x0)
    s.set_shift(50.0)
    lam1, V1, info1 = s.eigs(6, block=8, x0=x0)
    assert info0["converged"] and info1["converged"]
    assert s.shift == 50.0
    assert np.all(np.abs(lam1 - (lam0 + 50.0)) <= 1e-9 * lam1)
    for j in range(6):                                                # apply() is the shifted operator now
        assert np.linalg.norm(s.apply(V1[j]) + lam1[j] * V1[j]) <= 2e-8 * lam1[j] * np.linalg.norm(V1[j])


# ---- locking and stop ------------------------------------------------------------------------------------------------------
def test_a_converged_start_block_takes_no_iteration():
    import iterative_solvers_amd as isa
    s = system(34, "any")
    h = s._handle
    lam, V, res, out = h.eigs(6, 8, 1e-10, 200, start_block(8, s.size()))
    assert out.converged == 1
    lam2, V2, res2, out2 = h.eigs(6, 8, 1e-8, 200, V)                  # all eight Ritz vectors of the tighter run as the start
    assert out2.iterations == 0 and out2.converged == 1 and out2.stop_reason == isa.EIG_CONVERGED
    assert np.all(np.abs(lam2[:6] - lam[:6]) <= 1e-12 * lam[:6])


def test_iteration_cap_and_stop_flag():
    import iterative_solvers_amd as isa
    s = system(64, "mg")
    lam, V, info = s.eigs(6, block=8, max_iterations=2)
    assert info["iterations"] == 2 and not info["converged"] and info["stop_reason"] == isa.EIG_ITERATIONS
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(info["residuals"])) and np.all(np.isfinite(V))
    lam, V, info = s.eigs(6, block=8, stop_flag=C.c_int(1))
    assert info["iterations"] == 0 and not info["converged"] and info["stop_reason"] == isa.EIG_INTERRUPTED
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(info["residuals"]))


# ---- determinism and isolation -----------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_on_host_and_device_vectors():
    torch = pytest.importorskip("torch")
    s = system(64, "mg")
    x0 = start_block(8, s.size(), seed=3)
    lam_a, V_a, info_a = s.eigs(6, block=8, x0=x0)
    lam_b, V_b, info_b = s.eigs(6, block=8, x0=x0)
    assert np.array_equal(lam_a, lam_b) and np.array_equal(V_a, V_b) and info_a["iterations"] == info_b["iterations"]
    assert np.array_equal(info_a["residuals"], info_b["residuals"])
    lam_d, V_d, info_d = s.eigs(6, block=8, x0=torch.from_numpy(x0).cuda())
    assert V_d.is_cuda and np.array_equal(lam_a, lam_d) and np.array_equal(V_a, V_d.cpu().numpy())
    s.eigs_release()                                                  # a fresh workspace changes nothing
    lam_c, V_c, _ = s.eigs(6, block=8, x0=x0)
    assert np.array_equal(lam_a, lam_c) and np.array_equal(V_a, V_c)


def test_an_eigen_solve_leaves_the_handles_solves_alone():
    import iterative_solvers_amd as isa
    s = system(130, "any")
    h = s._handle
    p = isa.default_params(isa.RULE_REL_2NORM)
    p.eps_rel, p.use_true_solution = 1e-8, 0
    rhs = np.random.default_rng(5).standard_normal((3, s.size()))
    r1 = h.solve(p)
    x1, b1 = h.solution(), h.rhs()
    xb1, rb1 = h.solve_batch(p, rhs)
    h.solve(p)
    s.eigs(3, tol=1e-6)
    assert np.array_equal(h.solution(), x1) and np.array_equal(h.rhs(), b1)      # the last solution and b are still there
    xb2, rb2 = h.solve_batch(p, rhs)
    r2 = h.solve(p)
    assert np.array_equal(h.solution(), x1) and r2.iterations == r1.iterations and r2.r_norm2 == r1.r_norm2
    assert np.array_equal(xb1, xb2) and [r.iterations for r in rb1] == [r.iterations for r in rb2]
    assert s.shift == 0.0


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_unchanged():
    import iterative_solvers_amd as isa
    s = system(34, precond=False)
    x0 = start_block(4, s.size())
    with pytest.raises(isa.Mi355cgError) as e:
        s.eigs(2, block=4, x0=x0)
    assert e.value.code == 3 and "preconditioner" in str(e.value)
    s.set_preconditioner(isa.PRECOND_MG_ANY, isa.CYCLE_F32)
    with pytest.raises(ValueError, match="CYCLE_F32"):
        s.eigs(2, block=4, x0=x0)
    assert s.preconditioner_info()[:2] == (isa.PRECOND_MG_ANY, isa.CYCLE_F32)
    s.set_preconditioner(isa.PRECOND_MG_ANY)
    h = s._handle
    with pytest.raises(ValueError, match="columns"):
        h.eigs(2, 17, 1e-8, 10, start_block(17, s.size()))
    with pytest.raises(ValueError, match="columns"):
        h.eigs(5, 4, 1e-8, 10, x0)
    for tol, its in ((0.0, 10), (float("nan"), 10), (float("inf"), 10), (1e-8, 0)):
        with pytest.raises(ValueError):
            h.eigs(2, 4, tol, its, x0)
    lam, V, info = s.eigs(2, block=4, x0=x0)                          # and it still works
    assert info["converged"] and np.all(np.abs(lam - dense_spectrum(34)[:2]) <= 1e-9 * lam)
    s.eigs_release()
    s.eigs_release()


def test_cpp_compat_eigs(tmp_path):
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "eigs_compat_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(root, "iterative_solvers_amd", "compat"), os.path.join(root, "tests", "cpp", "eigs_compat_driver.cpp"),
                           "-L", os.path.join(root, "iterative_solvers_amd"), "-lmi355cg",
                           "-Wl,-rpath," + os.path.join(root, "iterative_solvers_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
