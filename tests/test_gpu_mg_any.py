"""MI355CG_PRECOND_MG_ANY on the GPU: the device V-cycle against the NumPy restatement in tests/mg_model.py, the same bits
as MI355CG_PRECOND_MG where both have a hierarchy, preconditioned CG under both stop rules on grids MG refuses, determinism, the
way back to the plain path, the refusals, time to solution against the plain solve, and the C++ layer."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DOM = ref.DOM


def any_system(N, dom=DOM, kind=None):
    import iterative_solvers_amd as isa
    s = isa.MatrixFreeSystem(N, N, *dom)
    s.set_preconditioner(isa.PRECOND_MG_ANY if kind is None else kind)
    return s


def rel_solve(s, eps=1e-8, max_iterations=1000):
    import iterative_solvers_amd as isa
    solver = isa.MatrixFreeSolver(s, s.get_rhs(), eps, max_iterations)
    x = solver.solve()
    return x, solver.last_results


@pytest.mark.parametrize("N", [34, 50, 258, 1002])
def test_apply_preconditioner_matches_the_restatement(N):
    s = any_system(N)
    levels = ref.hierarchy_any(N, *ref.steps(N))
    rng = np.random.default_rng(N)
    for _ in range(2):
        r = rng.standard_normal(s.size())
        z = s._handle.apply_preconditioner(r)
        zr = ref.apply_M(levels, r)
        assert np.abs(z - zr).max() <= 1e-13 * np.abs(zr).max()


def test_apply_preconditioner_is_symmetric():
    s = any_system(258)
    rng = np.random.default_rng(3)
    r1, r2 = rng.standard_normal(s.size()), rng.standard_normal(s.size())
    m12, m21 = s._handle.apply_preconditioner(r1) @ r2, r1 @ s._handle.apply_preconditioner(r2)
    assert abs(m12 - m21) <= 1e-12 * abs(m12)


def test_same_bits_as_mg_where_both_have_a_hierarchy():
    import iterative_solvers_amd as isa
    a, m = any_system(256), any_system(256, kind=isa.PRECOND_MG)
    r = np.random.default_rng(11).standard_normal(a.size())
    assert np.array_equal(a._handle.apply_preconditioner(r), m._handle.apply_preconditioner(r))
    xa, ra = rel_solve(a)
    xm, rm = rel_solve(m)
    assert ra.iterations == rm.iterations and ra.r_norm2 == rm.r_norm2
    assert np.array_equal(xa, xm)
    m.set_preconditioner(isa.PRECOND_MG_ANY)                      # switching kinds keeps the hierarchy and the bits
    assert np.array_equal(rel_solve(m)[0], xm)


@pytest.mark.parametrize("N", [100, 258, 1000, 2002])
def test_rel_2norm_converges_in_few_iterations(N):
    from oracle.oracle import OracleGrid
    s = any_system(N)
    x, res = rel_solve(s)
    assert 1 <= res.iterations <= 12 and res.converged
    b = s.get_rhs()
    tr = OracleGrid(N, N, *DOM).apply(x) - b
    assert np.linalg.norm(tr) <= 2e-8 * np.linalg.norm(b)


def test_stretched_domain_converges():
    from oracle.oracle import OracleGrid
    for dom in ((0.0, 1.0, 0.0, 2.0), (0.0, 3.0, 0.0, 1.0)):          # xk = 4 yk, and yk = 9 xk: no exchange passes by symmetry
        s = any_system(258, dom)
        x, res = rel_solve(s)
        assert 1 <= res.iterations <= 20 and res.converged
        b = s.get_rhs()
        tr = OracleGrid(258, 258, *dom).apply(x) - b
        print(f"N=258 dom={dom}: {res.iterations} iterations, true residual {np.linalg.norm(tr) / np.linalg.norm(b):.3e}")
        assert np.linalg.norm(tr) <= 2e-8 * np.linalg.norm(b)


def test_msg_rule_stop_reason_and_callbacks():
    import iterative_solvers_amd as isa
    s = any_system(1000)
    solver = isa.MSGSolver(s, s.get_rhs(), 1e-6, 1000)
    calls = []
    solver.setIterationCallback(lambda it, p, r, e: calls.append((it, p, r, e)))
    solver.solve(s.get_true_solution_vector())
    it = solver.getIterations()
    assert solver.hasConverged() and 1 <= it <= 20
    assert solver.getStopReason() in (isa.StopCriterion.PRECISION, isa.StopCriterion.RESIDUAL, isa.StopCriterion.EXACT_ERROR)
    assert [c[0] for c in calls] == ([0, 1, it] if it > 1 else [0, it])
    assert calls[-1][1:] == (solver.getFinalPrecision(), solver.getFinalResidualNorm(), solver.getFinalErrorNorm())
    u = s.get_true_solution_vector()
    assert solver.getFinalErrorNorm() == pytest.approx(np.abs(s._handle.solution() - u).max(), rel=1e-12)


def test_stop_requested_from_the_first_callback_stops_at_iteration_one():
    import iterative_solvers_amd as isa
    s = any_system(258)
    solver = isa.MSGSolver(s, s.get_rhs(), 1e-12, 1000)
    seen = []

    def cb(it, p, r, e):
        seen.append(it)
        if it == 1:
            solver.requestStop()
    solver.setIterationCallback(cb)
    solver.solve()
    assert solver.getStopReason() == isa.StopCriterion.INTERRUPTED and not solver.hasConverged()
    assert solver.getIterations() == 1 and seen == [0, 1, 1]


def test_two_solves_are_bit_identical():
    s = any_system(1002)
    x1, r1 = rel_solve(s)
    x2, r2 = rel_solve(s)
    assert r1.iterations == r2.iterations and r1.r_norm2 == r2.r_norm2
    assert np.array_equal(x1, x2)


def test_preconditioner_none_restores_the_plain_path():
    import iterative_solvers_amd as isa
    s = any_system(258)
    rel_solve(s)
    s.set_preconditioner(isa.PRECOND_NONE)
    x1, r1 = rel_solve(s, max_iterations=100000)
    x2, r2 = rel_solve(isa.MatrixFreeSystem(258, 258, *DOM), max_iterations=100000)
    assert r1.iterations == r2.iterations > 12
    assert np.array_equal(x1, x2)
    with pytest.raises(isa.Mi355cgError):
        s._handle.apply_preconditioner(s.get_rhs())


def test_refusals_raise_value_error():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    from iterative_solvers_amd.solver import _Handle
    from oracle.oracle import OracleGrid
    with pytest.raises(ValueError, match="fp64 only"):
        isa.MatrixFreeSystem(258, 258, *DOM, dtype=isa.F32_MIXED).set_preconditioner(isa.PRECOND_MG_ANY)
    with pytest.raises(ValueError, match="CSR"):
        isa.CrsMatrix(*OracleGrid(16, 16, *DOM).csr())._handle.set_preconditioner(isa.PRECOND_MG_ANY)
    slab = _Handle.__new__(_Handle)
    slab._lib = _capi.load()
    slab._h = C.c_void_p()
    _capi.check(slab._lib.mi355cg_create_slab(64, 64, *DOM, _capi.F64, 0, 1, 31, C.byref(slab._h)))
    with pytest.raises(ValueError, match="single-GPU"):
        slab.set_preconditioner(isa.PRECOND_MG_ANY)
    slab.close()


def test_mg_on_a_grid_only_mg_any_covers_is_refused_and_keeps_mg_any():
    import iterative_solvers_amd as isa
    s = any_system(1000)
    _, before = rel_solve(s)
    with pytest.raises(ValueError, match="no multigrid hierarchy"):
        s.set_preconditioner(isa.PRECOND_MG)
    _, after = rel_solve(s)
    assert after.converged and after.iterations == before.iterations <= 12 and after.r_norm2 == before.r_norm2


def test_converged_n1000_is_at_least_five_times_faster_than_plain():
    import iterative_solvers_amd as isa
    s = isa.MatrixFreeSystem(1000, 1000, *DOM)
    _, plain = rel_solve(s, max_iterations=100000)
    assert plain.converged
    s.set_preconditioner(isa.PRECOND_MG_ANY)
    rel_solve(s)                                                   # first use of the new kernels
    _, mg = rel_solve(s)
    assert mg.converged and 1 <= mg.iterations <= 12
    assert mg.solve_seconds < 0.2 * plain.solve_seconds, (mg.solve_seconds, plain.solve_seconds)


def test_cpp_compat_mg_any(tmp_path):
    import subprocess
    from iterative_solvers_amd import build as b
    b.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "mg_any_compat_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(root, "iterative_solvers_amd", "compat"),
                           os.path.join(root, "tests", "cpp", "mg_any_compat_driver.cpp"),
                           "-L", os.path.join(root, "iterative_solvers_amd"), "-lmi355cg",
                           "-Wl,-rpath," + os.path.join(root, "iterative_solvers_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
