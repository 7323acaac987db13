"""Multigrid-preconditioned CG on the GPU against the high-precision restatement of tests/mg_reference.py, on
the cases of tests/mg_cases.py; tests/test_mg_reference_cpu.py shows that each of them can tell exchanged steps from the right
ones, measures the reference's own uncertainty and keeps every stop away from its threshold.
  a  the V-cycle on stretched domains (hx != hy in both directions), fp64 and fp32, and its symmetry
  b  the V-cycle where a block marches over more than one row (N = 2050; N = 4100: levels 0 and 1)
  c  the PCG iterates x_k, ||r_k|| and ||b|| after k fixed iterations
  d  the REL_2NORM diagnostics callbacks under a preconditioner, against the trace and against the returned x
  e  the MSG rule: iteration count, stop reason and the three max-norms
  f  batched solves at N = 2050: the bits of sequential solves, and system 0 against the restatement
Every tolerance is computed from the reference by the formulas of mg_reference.tol_M and tol_pcg, never from what the library
returned; every test prints the deviation it saw next to the tolerance it allowed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_cases as T  # noqa: E402
import mg_model  # noqa: E402

R = T.R
LD = np.longdouble
DBL_MAX = sys.float_info.max

pytestmark = pytest.mark.gpu


def system(c, f32=False):
    import iterative_solvers_amd as isa
    s = isa.MatrixFreeSystem(c.N, c.N, *c.dom)
    s.set_preconditioner(c.kind, isa.CYCLE_F32 if f32 else isa.CYCLE_F64)
    return s


def rel(a, b):
    return abs(a - b) / abs(b)


def show(what, dev, tol):
    print(f"  {what}: deviation {dev:.2e}, tolerance {tol:.2e}")
    return dev <= tol


# ---- a, b: the V-cycle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.CYCLES, ids=T.case_id)
def test_vcycle_matches_the_restatement(c):
    import iterative_solvers_amd as isa
    lv = T.levels(c)
    s = system(c)
    print(T.case_id(c))
    done = []
    for r in T.vectors(c):
        zr = R.apply_M(lv, r)
        tol = R.tol_M(R.cycle_floor(lv, r, zr))
        assert tol <= T.CAP
        z = s._handle.apply_preconditioner(r)
        assert show("fp64 cycle, max|z - z_ref| / max|z_ref|", np.abs(z - zr).max() / np.abs(zr).max(), tol)
        done.append((r, zr))
    if c.f32:
        s.set_preconditioner(c.kind, isa.CYCLE_F32)
        for r, zr in done:
            dev = np.abs(s._handle.apply_preconditioner(r) - zr).max() / np.abs(zr).max()
            assert show("fp32 cycle, max|z - z_ref| / max|z_ref|", dev, 2e-6)
            assert dev > 1e-9                                       # an fp64 cycle behind the flag agrees to 1e-13


def test_vcycle_is_symmetric_on_a_stretched_domain():
    c = T.SYMMETRY
    r1, r2 = T.vectors(c)
    s = system(c)
    m12, m21 = s._handle.apply_preconditioner(r1) @ r2, r1 @ s._handle.apply_preconditioner(r2)
    assert show("fp64 cycle, |(M r1, r2) - (r1, M r2)| / |(M r1, r2)|", abs(m12 - m21) / abs(m12), 1e-12)
    s = system(c, f32=True)
    m1, m2 = s._handle.apply_preconditioner(r1), s._handle.apply_preconditioner(r2)
    assert show("fp32 cycle, asymmetry over ||M r1|| ||r2||", abs(m1 @ r2 - r1 @ m2) / (np.linalg.norm(m1) * np.linalg.norm(r2)), 1e-6)


# ---- c: the PCG iterates -------------------------------------------------------------------------------------------------------
def check_iterate(ref, k, x, res):
    """x and the result fields after k fixed iterations against the trace"""
    t, i = ref.trace, k - 1
    ok = show(f"x after {k} iterations, max|x - x_ref| / max|x_ref|", np.abs(x - t.x[i]).max() / np.abs(t.x[i]).max(), ref.tol["x"][i])
    ok &= show("r_norm2", rel(res.r_norm2, t.r2[i]), ref.tol["r2"][i])
    ok &= show("initial_r_norm2", rel(res.initial_r_norm2, t.b_norm2), ref.tol["b2"][i])
    assert res.iterations == k
    assert ok


@pytest.mark.parametrize("c,k", [(c, k) for c in T.FIXED for k in (T.FIXED_K if c.k == max(T.FIXED_K) else (c.k,))],
                         ids=lambda v: T.case_id(v) if isinstance(v, tuple) else f"k{v}")
def test_fixed_iterations_give_the_iterates_of_the_trace(c, k):
    import iterative_solvers_amd as isa
    ref = T.reference(c)
    s = system(c)
    solver = isa.MatrixFreeSolver(s, ref.b, c.eps, k)
    x = solver.solve(fixed_iterations=True)
    print(T.case_id(c))
    check_iterate(ref, k, x, solver.last_results)


# ---- d: REL_2NORM diagnostics --------------------------------------------------------------------------------------------------
def norms_of(ref, x):
    """(||b - A x||_2, ||x - u||_2) in long double from a returned x"""
    L = ref.levels[0]
    g = np.zeros((L.N + 1, L.N + 1), dtype=LD)
    g[L.mask] = x.astype(LD)
    tr = ref.b.astype(LD) - R.apply_A_longdouble(ref.levels, g)[L.mask]
    e = x.astype(LD) - ref.u.astype(LD)
    return float(np.sqrt(tr @ tr)), float(np.sqrt(e @ e))


@pytest.mark.parametrize("c", T.REL + [T.REL_F32], ids=T.case_id)
def test_rel_2norm_diagnostics_under_a_preconditioner(c):
    import iterative_solvers_amd as isa
    ref = T.reference(c)
    t = ref.trace
    s = system(c, f32=c.f32)
    solver = isa.MatrixFreeSolver(s, ref.b, c.eps, 1000)
    calls = []
    solver.setIterationCallback(lambda it, dx, tr, e: calls.append((it, dx, tr, e)))
    x = solver.solve(true_solution=ref.u)
    res = solver.last_results
    print(f"{T.case_id(c)}: {res.iterations} iterations (reference {t.iterations}, margin {100 * ref.margin:.1f} %)")
    assert [q[0] for q in calls] == list(range(res.iterations))
    if c.f32:
        assert res.iterations == mg_model.pcg(ref.levels, ref.b, eps=c.eps, M=lambda r: mg_model.apply_M32(ref.levels, r))[1]
        assert res.converged
    else:
        assert res.iterations == t.iterations and bool(res.converged) == t.converged
        ok = True
        for i, (_, dx, tr, e) in enumerate(calls):
            print(f" callback {i}")
            ok &= show("||dx||_2", rel(dx, t.dx2[i]), ref.tol["dx2"][i])
            ok &= show("||b - A x||_2 over ||b||_2", abs(tr - t.true2[i]) / t.b_norm2, ref.tol["true2"][i])
            # a difference of nearly equal vectors: bounded as x is (mg_cases, the error norms)
            ok &= show("||x - u||_2 over ||x_ref||_2", abs(e - t.e2[i]) / np.linalg.norm(t.x[i]), ref.tol["x"][i])
        assert ok
    # apart from the trace: the last callback's norms are those of the returned x
    tr_x, e_x = norms_of(ref, x)
    print(" last callback against the returned x")
    ok = show("||b - A x||_2 over ||b||_2", abs(calls[-1][2] - tr_x) / t.b_norm2, ref.tol["true2"][-1])
    ok &= show("||x - u||_2", rel(calls[-1][3], e_x), 1e-13)           # the same x on both sides: only the sum's rounding is left
    assert ok


# ---- e: the MSG rule -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", T.MSG, ids=T.case_id)
def test_msg_rule_against_the_trace(c):
    import iterative_solvers_amd as isa
    ref = T.reference(c)
    t = ref.trace
    s = system(c)
    solver = isa.MSGSolver(s, ref.b, c.eps, 1000)
    if not c.exact_error:
        solver.setExactErrorEps(-1)
    calls = []
    solver.setIterationCallback(lambda it, p, r, e: calls.append((it, p, r, e)))
    x = solver.solve(ref.u)
    it = solver.getIterations()
    print(f"{T.case_id(c)}: {it} iterations, stop reason {solver.getStopReason().name} (reference {t.iterations}, "
          f"{isa.StopCriterion(t.reason).name}, margin {100 * ref.margin:.1f} %)")
    assert it == t.iterations and it > 1
    assert solver.getStopReason() == isa.StopCriterion(t.reason) and solver.hasConverged()
    if not c.exact_error:
        assert solver.getStopReason() in (isa.StopCriterion.PRECISION, isa.StopCriterion.RESIDUAL)
    assert [q[0] for q in calls] == [0, 1, it]
    assert calls[0][1] == DBL_MAX
    ok = show("callback 0, max|r|", rel(calls[0][2], t.r0_max), 1e-13)
    ok &= show("callback 0, max|x - u|", rel(calls[0][3], t.e0_max), 1e-13)
    for call, i in ((calls[1], 0), (calls[2], it - 1)):
        for name, v, q in (("max|dx|", call[1], "dx_max"), ("max|r|", call[2], "r_max")):
            ok &= show(f"callback {call[0]}, {name}", rel(v, getattr(t, q)[i]), ref.tol[q][i])
        # a difference of nearly equal vectors: bounded as x is, |e - e_ref| <= tol max|x_ref| (mg_cases, the error norms)
        ok &= show(f"callback {call[0]}, max|x - u| over max|x_ref|", abs(call[3] - t.e_max[i]) / np.abs(t.x[i]).max(), ref.tol["x"][i])
    assert ok
    assert calls[-1][1:] == (solver.getFinalPrecision(), solver.getFinalResidualNorm(), solver.getFinalErrorNorm())
    assert solver.getFinalErrorNorm() == np.abs(x - ref.u).max()    # the max of the same fp64 differences


# ---- f: batched kernels where a block takes more than one row --------------------------------------------------------------------
def test_batch_at_n2050_has_the_bits_of_sequential_solves_and_the_iterates_of_the_trace():
    import iterative_solvers_amd as isa
    from test_gpu_mg_batch import assert_same, rel_params, sequential
    c = T.BATCH
    ref = T.reference(c)
    n = ref.b.size
    rhs = np.stack([ref.b] + [np.random.default_rng(seed).standard_normal(n) for seed in T.BATCH_MORE_SEEDS])
    s = system(c)
    p = rel_params(eps=1e-8)
    xs, rs = sequential(s, p, rhs)
    xb, rb = s._handle.solve_batch(p, rhs)
    print(f"{T.case_id(c)} batch: iterations {[r.iterations for r in rs]}")
    assert all(r.converged and 1 <= r.iterations <= 12 for r in rs)
    assert_same(xb, rb, xs, rs)
    p = isa.default_params(isa.RULE_REL_2NORM)
    p.eps_rel, p.max_iterations, p.use_true_solution, p.fixed_iterations = c.eps, c.k, 0, 1
    xk, rk = s._handle.solve_batch(p, rhs)
    check_iterate(ref, c.k, xk[0], rk[0])
