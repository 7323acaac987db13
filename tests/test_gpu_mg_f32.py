"""MI355CG_CYCLE_F32 on the GPU: the device's fp32 V-cycle against the fp64 NumPy restatement tests/mg_model.apply_M (which
is independent of the code under test and pinned to the fp64 device cycle at 1e-13), its symmetry, preconditioned CG under both
stop rules with the iteration counts of the fp64 cycle, one-level grids, exact scaling by powers of two, determinism, the way
back to the fp64 cycle and to the plain path, preconditioner_info, the refusals, the C++ layer, and a speed guard at N = 4096."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DOM = ref.DOM
STRETCHED = (0.0, 1.0, 0.0, 2.0)


def f32_system(N, dom=DOM, kind=None, cycle=None):
    import iterative_solvers_amd as isa
    s = isa.MatrixFreeSystem(N, N, *dom)
    s.set_preconditioner(isa.PRECOND_MG_ANY if kind is None else kind, isa.CYCLE_F32 if cycle is None else cycle)
    return s


def rel_solve(s, b=None, eps=1e-8, max_iterations=1000):
    import iterative_solvers_amd as isa
    solver = isa.MatrixFreeSolver(s, s.get_rhs() if b is None else b, eps, max_iterations)
    x = solver.solve()
    return x, solver.last_results


def true_rel(N, dom, x, b):
    from oracle.oracle import OracleGrid
    return np.linalg.norm(OracleGrid(N, N, *dom).apply(x) - b) / np.linalg.norm(b)


@pytest.mark.parametrize("N,kind", [(34, 2), (50, 2), (258, 2), (1002, 2), (256, 1)])
def test_apply_preconditioner_is_the_fp64_restatement_to_fp32_rounding(N, kind):
    s = f32_system(N, kind=kind)
    levels = ref.hierarchy_any(N, *ref.steps(N))
    rng = np.random.default_rng(N)
    for _ in range(2):
        r = rng.standard_normal(s.size())
        z = s._handle.apply_preconditioner(r)
        zr = ref.apply_M(levels, r)
        dev = np.abs(z - zr).max() / np.abs(zr).max()
        print(f"N={N} kind={kind}: max|z_dev - z_ref64| / max|z_ref64| = {dev:.3e}")
        assert dev <= 2e-6
        assert dev > 1e-9                                         # an fp64 cycle behind the flag agrees to 1e-13


def test_apply_preconditioner_is_symmetric_to_rounding():
    s = f32_system(258)
    rng = np.random.default_rng(3)
    r1, r2 = rng.standard_normal(s.size()), rng.standard_normal(s.size())
    m1, m2 = s._handle.apply_preconditioner(r1), s._handle.apply_preconditioner(r2)
    asym = abs(m1 @ r2 - r1 @ m2) / (np.linalg.norm(m1) * np.linalg.norm(r2))
    print(f"asymmetry {asym:.3e}")
    assert asym <= 1e-6


def test_zero_vector_gives_zero():
    s = f32_system(258)
    z = s._handle.apply_preconditioner(np.zeros(s.size()))
    assert not z.any()


@pytest.mark.parametrize("N,dom", [(100, DOM), (258, DOM), (1000, DOM), (2002, DOM), (4098, DOM), (258, STRETCHED)])
def test_rel_2norm_takes_the_iterations_of_the_fp64_cycle(N, dom):
    import iterative_solvers_amd as isa
    s = f32_system(N, dom)
    x, res = rel_solve(s)
    b = s.get_rhs()
    rel = true_rel(N, dom, x, b)
    s.set_preconditioner(isa.PRECOND_MG_ANY, isa.CYCLE_F64)
    _, res64 = rel_solve(s)
    print(f"N={N} dom={dom}: iterations fp32 cycle {res.iterations}, fp64 cycle {res64.iterations}; true residual {rel:.3e}; "
          f"recursive residuals {res.r_norm2:.6e} / {res64.r_norm2:.6e}")
    assert res.converged and res64.converged
    assert 1 <= res.iterations <= (20 if dom == STRETCHED else 12)
    assert res.iterations == res64.iterations
    assert rel <= 2e-8


@pytest.mark.parametrize("N", [16, 32])
def test_one_level_grids_converge_in_at_most_three_iterations(N):
    s = f32_system(N)
    assert s.preconditioner_info()[2] == 1
    x, res = rel_solve(s)
    rel = true_rel(N, DOM, x, s.get_rhs())
    print(f"N={N}: {res.iterations} iterations, true residual {rel:.3e}")
    assert res.converged and 1 <= res.iterations <= 3
    assert rel <= 2e-8


def test_msg_rule_stop_reason_and_callbacks():
    import iterative_solvers_amd as isa
    s = f32_system(1000)
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
    s = f32_system(258)
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


@pytest.mark.parametrize("k", [-140, 140])
def test_a_solve_scales_exactly_with_powers_of_two(k):
    s0, sk = f32_system(258), f32_system(258)
    b = s0.get_rhs()
    x0, r0 = rel_solve(s0, b)
    xk, rk = rel_solve(sk, np.ldexp(b, k))
    assert r0.converged and rk.converged
    assert rk.iterations == r0.iterations
    assert np.isfinite(xk).all()
    assert np.array_equal(xk, np.ldexp(x0, k))


def test_two_solves_are_bit_identical():
    s = f32_system(1002)
    x1, r1 = rel_solve(s)
    x2, r2 = rel_solve(s)
    assert r1.iterations == r2.iterations and r1.r_norm2 == r2.r_norm2
    assert np.array_equal(x1, x2)
    r = np.random.default_rng(2).standard_normal(s.size())
    assert np.array_equal(s._handle.apply_preconditioner(r), s._handle.apply_preconditioner(r))


def test_switching_to_the_fp64_cycle_gives_the_bits_of_a_fresh_fp64_handle():
    import iterative_solvers_amd as isa
    s = f32_system(258)
    x32, _ = rel_solve(s)
    s.set_preconditioner(isa.PRECOND_MG_ANY, isa.CYCLE_F64)
    assert s.preconditioner_info()[:2] == (isa.PRECOND_MG_ANY, isa.CYCLE_F64)
    x64, r64 = rel_solve(s)
    fresh = isa.MatrixFreeSystem(258, 258, *DOM)
    fresh.set_preconditioner(isa.PRECOND_MG_ANY)
    xf, rf = rel_solve(fresh)
    assert r64.iterations == rf.iterations and r64.r_norm2 == rf.r_norm2
    assert np.array_equal(x64, xf)
    assert not np.array_equal(x32, x64)                           # the fp32 cycle is another preconditioner
    r = np.random.default_rng(4).standard_normal(s.size())
    assert np.array_equal(s._handle.apply_preconditioner(r), fresh._handle.apply_preconditioner(r))
    s.set_preconditioner(isa.PRECOND_MG_ANY, isa.CYCLE_F32)       # and back: the bits of the first fp32 solve
    assert np.array_equal(rel_solve(s)[0], x32)


def test_preconditioner_none_restores_the_plain_path():
    import iterative_solvers_amd as isa
    s = f32_system(258)
    rel_solve(s)
    s.set_preconditioner(isa.PRECOND_NONE, isa.CYCLE_F32)
    assert s.preconditioner_info() == (isa.PRECOND_NONE, isa.CYCLE_F64, 0)
    x1, r1 = rel_solve(s, max_iterations=100000)
    x2, r2 = rel_solve(isa.MatrixFreeSystem(258, 258, *DOM), max_iterations=100000)
    assert r1.iterations == r2.iterations > 12
    assert np.array_equal(x1, x2)
    with pytest.raises(isa.Mi355cgError):
        s._handle.apply_preconditioner(s.get_rhs())
    s.set_preconditioner(isa.PRECOND_NONE, 77)                    # PRECOND_NONE frees everything, whatever cycle says


@pytest.mark.parametrize("n,kind", [(16, 2), (258, 2), (1000, 2), (4096, 1), (4098, 2)])
def test_preconditioner_info(n, kind):
    import iterative_solvers_amd as isa
    s = isa.MatrixFreeSystem(n, n, *DOM)
    assert s.preconditioner_info() == (isa.PRECOND_NONE, isa.CYCLE_F64, 0)
    s.set_preconditioner(kind, isa.CYCLE_F32)
    assert s.preconditioner_info() == (kind, isa.CYCLE_F32, len(isa.mg_hierarchy(n)))
    s.set_preconditioner(kind)
    assert s.preconditioner_info() == (kind, isa.CYCLE_F64, len(isa.mg_hierarchy(n)))
    k, lv = C.c_int(-1), C.c_int(-1)                              # null out-pointers are skipped
    lib = s._handle._lib
    assert lib.mi355cg_preconditioner_info(s._handle._h, C.byref(k), None, C.byref(lv)) == 0
    assert (k.value, lv.value) == (kind, len(isa.mg_hierarchy(n)))
    assert lib.mi355cg_preconditioner_info(s._handle._h, None, None, None) == 0


def test_refusals_leave_a_working_handle():
    import iterative_solvers_amd as isa
    from oracle.oracle import OracleGrid
    s = f32_system(258)
    _, before = rel_solve(s)
    with pytest.raises(ValueError, match=r"MI355CG_CYCLE_F64 = 0, MI355CG_CYCLE_F32 = 1"):
        s.set_preconditioner(isa.PRECOND_MG_ANY, 2)
    with pytest.raises(ValueError, match="no multigrid hierarchy"):
        s.set_preconditioner(isa.PRECOND_MG, isa.CYCLE_F32)
    with pytest.raises(ValueError, match="unknown preconditioner kind"):
        s.set_preconditioner(3, isa.CYCLE_F32)
    assert s.preconditioner_info() == (isa.PRECOND_MG_ANY, isa.CYCLE_F32, 4)
    _, after = rel_solve(s)
    assert after.converged and after.iterations == before.iterations and after.r_norm2 == before.r_norm2

    plain = isa.MatrixFreeSystem(258, 258, *DOM)
    with pytest.raises(ValueError, match=r"MI355CG_CYCLE_F64 = 0, MI355CG_CYCLE_F32 = 1"):
        plain.set_preconditioner(isa.PRECOND_MG_ANY, -1)
    assert plain.preconditioner_info() == (isa.PRECOND_NONE, isa.CYCLE_F64, 0)
    assert rel_solve(plain, max_iterations=100000)[1].converged

    mixed = isa.MatrixFreeSystem(258, 258, *DOM, dtype=isa.F32_MIXED)
    with pytest.raises(ValueError, match="fp64 only"):
        mixed.set_preconditioner(isa.PRECOND_MG_ANY, isa.CYCLE_F32)
    assert rel_solve(mixed, max_iterations=10 ** 6)[1].converged

    og = OracleGrid(16, 16, *DOM)
    csr = isa.CrsMatrix(*og.csr())
    with pytest.raises(ValueError, match="CSR"):
        csr._handle.set_preconditioner(isa.PRECOND_MG_ANY, isa.CYCLE_F32)
    v = np.random.default_rng(1).standard_normal(csr._handle.size)
    assert np.allclose(csr._handle.apply(v), og.apply(v), rtol=1e-13, atol=1e-9)


def test_cpp_compat_mg_f32(tmp_path):
    import subprocess
    from iterative_solvers_amd import build as b
    b.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "mg_f32_compat_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(root, "iterative_solvers_amd", "compat"),
                           os.path.join(root, "tests", "cpp", "mg_f32_compat_driver.cpp"),
                           "-L", os.path.join(root, "iterative_solvers_amd"), "-lmi355cg",
                           "-Wl,-rpath," + os.path.join(root, "iterative_solvers_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr


def test_the_fp32_cycle_is_faster_than_the_fp64_cycle_at_n4096():
    """Speed guard, margin zero: one process, one warm-up solve per setting, three timed solves of each alternating, the best
    solve_seconds of each.  The figures of record are in profiles/mg_f32_time_to_solution.txt (against the parent's build)."""
    import iterative_solvers_amd as isa
    s = isa.MatrixFreeSystem(4096, 4096, *DOM)
    best = {isa.CYCLE_F64: np.inf, isa.CYCLE_F32: np.inf}
    its = {}
    for cycle in best:                                            # warm-up: first use of each setting's kernels
        s.set_preconditioner(isa.PRECOND_MG_ANY, cycle)
        rel_solve(s)
    for _ in range(3):
        for cycle in best:
            s.set_preconditioner(isa.PRECOND_MG_ANY, cycle)
            _, res = rel_solve(s)
            assert res.converged
            its[cycle] = res.iterations
            best[cycle] = min(best[cycle], res.solve_seconds)
    print(f"N=4096 best solve_seconds: fp64 cycle {best[isa.CYCLE_F64]:.6f} ({its[isa.CYCLE_F64]} it), "
          f"fp32 cycle {best[isa.CYCLE_F32]:.6f} ({its[isa.CYCLE_F32]} it), ratio {best[isa.CYCLE_F32] / best[isa.CYCLE_F64]:.3f}")
    assert its[isa.CYCLE_F32] == its[isa.CYCLE_F64]
    assert best[isa.CYCLE_F32] < best[isa.CYCLE_F64]
