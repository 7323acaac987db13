"""The line smoother of the fp64 V-cycle on the GPU (mi355cg_set_smoother) against the restatement of
tests/line_reference.py: the cycle's values in both line directions on both stretched domains, the preconditioned solves under
both rules, the direction LINE_AUTO takes, the project's bit invariants (batch = single solves, the stepper = set_rhs + solve,
repeatability, the order of set_shift and set_smoother, JACOBI after LINE = a fresh handle, one-level grids), the eigen
iteration, and the refusals.  Every tolerance is computed from the reference (mg_reference.tol_M of the line cycle's own
long-double floor, tol_pcg of the trace's own spread), never from what the library returned; tests/test_mg_line_cpu.py asserts
the caps and the stop margins of exactly these inputs."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import line_reference as LR  # noqa: E402

R = LR.R
pytestmark = pytest.mark.gpu
FIELDS = ("iterations", "converged", "stop_reason", "final_residual_norm", "final_precision", "r_norm2", "initial_r_norm2")


def isa_kind(kind):
    import iterative_solvers_amd as isa
    return isa.PRECOND_MG if kind == R.MG else isa.PRECOND_MG_ANY


def system(N, dom, kind=R.MG_ANY, smoother=None):
    import iterative_solvers_amd as isa
    s = isa.MatrixFreeSystem(N, N, *dom)
    s.set_preconditioner(isa_kind(kind))
    if smoother is not None:
        s.set_smoother(smoother)
    return s


def rel_params(eps=1e-8, max_iterations=1000):
    import iterative_solvers_amd as isa
    p = isa.default_params(isa.RULE_REL_2NORM)
    p.eps_rel, p.max_iterations, p.use_true_solution = eps, max_iterations, 0
    return p


def solve_bits(s, b=None, p=None):
    """(x, result fields) of one solve on the system's handle"""
    h = s._handle
    if b is not None:
        h.set_rhs(b)
    res = h.solve(rel_params() if p is None else p)
    return h.solution(), tuple(getattr(res, f) for f in FIELDS)


def show(what, dev, tol):
    print(f"  {what}: deviation {dev:.2e}, tolerance {tol:.2e}")
    return dev <= tol


def rel(a, b):
    return abs(a - b) / abs(b)


# ---- the cycle's values --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LR.CYCLE_CASES, ids=LR.case_id)
def test_line_cycle_matches_the_restatement(c):
    import iterative_solvers_amd as isa
    N, kind, dom, direction = c
    lv = R.levels_for(N, dom, kind)
    s = system(N, dom, kind, isa.SMOOTHER_LINE_X if direction == LR.LINE_X else isa.SMOOTHER_LINE_Y)
    assert s.smoother_info() == (direction, direction)
    ok = True
    for r, name in zip(LR.cycle_vectors(N, dom), ("standard-normal r", "smooth r")):
        zr = LR.apply_M_line(lv, r, direction)
        tol = R.tol_M(LR.cycle_floor_line(lv, r, direction, zr))        # the device's line solve is the restatement's Thomas
        z = s._handle.apply_preconditioner(r)
        ok &= show(f"{LR.case_id(c)} {name}, max|z - z_ref| / max|z_ref|", np.abs(z - zr).max() / np.abs(zr).max(), tol)
        assert np.array_equal(z, s._handle.apply_preconditioner(r))     # a fixed order: the same bits
    assert ok


# ---- preconditioned solves -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LR.PCG_CASES, ids=LR.pcg_id)
def test_solves_under_line_auto_against_the_trace(c):
    import iterative_solvers_amd as isa
    from oracle.oracle import OracleGrid
    N, kind, dom, rule, eps, _ = c
    ref = LR.pcg_reference(c)
    t, last = ref.trace, ref.trace.iterations - 1
    assert ref.margin >= LR.MARGIN
    s = system(N, dom, kind, isa.SMOOTHER_LINE_AUTO)
    assert s.smoother_info() == (isa.SMOOTHER_LINE_AUTO, LR.auto_direction(ref.levels))
    if rule == R.REL_2NORM:
        solver = isa.MatrixFreeSolver(s, ref.b, eps, 1000)
        x = solver.solve(true_solution=ref.u)
        res = solver.last_results
        print(f"{LR.pcg_id(c)}: {res.iterations} iterations (reference {t.iterations}, margin {100 * ref.margin:.1f} %)")
        assert res.iterations == t.iterations and bool(res.converged) == t.converged
        ok = show("r_norm2", rel(res.r_norm2, t.r2[last]), ref.tol["r2"][last])
        ok &= show("initial_r_norm2", rel(res.initial_r_norm2, t.b_norm2), ref.tol["b2"][last])
    else:
        solver = isa.MSGSolver(s, ref.b, eps, 1000)                     # the MSG defaults: the three tests at 1e-6
        x = solver.solve(ref.u)
        print(f"{LR.pcg_id(c)}: {solver.getIterations()} iterations, {solver.getStopReason().name} (reference {t.iterations}, "
              f"{isa.StopCriterion(t.reason).name}, margin {100 * ref.margin:.1f} %)")
        assert solver.getIterations() == t.iterations and solver.hasConverged()
        assert solver.getStopReason() == isa.StopCriterion(t.reason)
        ok = show("max|dx|", rel(solver.getFinalPrecision(), t.dx_max[last]), ref.tol["dx_max"][last])
        ok &= show("max|r|", rel(solver.getFinalResidualNorm(), t.r_max[last]), ref.tol["r_max"][last])
        # a difference of nearly equal vectors: bounded as x is (mg_cases, the error norms)
        ok &= show("max|x - u| over max|x_ref|", abs(solver.getFinalErrorNorm() - t.e_max[last]) / np.abs(t.x[last]).max(), ref.tol["x"][last])
    ok &= show("x, max|x - x_ref| / max|x_ref|", np.abs(x - t.x[last]).max() / np.abs(t.x[last]).max(), ref.tol["x"][last])
    tr = np.linalg.norm(OracleGrid(N, N, *dom).apply(x) - ref.b) / np.linalg.norm(ref.b)
    print(f"  ||A x - b|| / ||b|| = {tr:.2e}")
    assert ok and tr <= 2e-8


def test_line_auto_resolves_to_the_strongly_coupled_direction():
    import iterative_solvers_amd as isa
    for dom, direction in ((LR.STRETCH_X, LR.LINE_Y), (LR.STRETCH_Y, LR.LINE_X), (LR.SQUARE, LR.LINE_X)):
        s = isa.MatrixFreeSystem(64, 64, *dom)
        assert s.smoother_info() == (isa.SMOOTHER_JACOBI, 0)
        s.set_smoother(isa.SMOOTHER_LINE_AUTO)                           # before there is a hierarchy: remembered
        assert s.smoother_info() == (isa.SMOOTHER_LINE_AUTO, direction)
        s.set_preconditioner(isa.PRECOND_MG)
        assert s.smoother_info() == (isa.SMOOTHER_LINE_AUTO, direction) and s.preconditioner_info() == (isa.PRECOND_MG, isa.CYCLE_F64, 2)
        s.set_smoother(isa.SMOOTHER_LINE_X)
        assert s.smoother_info() == (isa.SMOOTHER_LINE_X, LR.LINE_X)
        s.set_smoother(isa.SMOOTHER_JACOBI)
        assert s.smoother_info() == (isa.SMOOTHER_JACOBI, 0)


def test_either_order_of_set_smoother_and_set_preconditioner_gives_the_same_bits():
    import iterative_solvers_amd as isa
    N, dom = 258, LR.STRETCH_X
    r = LR.cycle_vectors(N, dom)[0]
    after = system(N, dom, R.MG_ANY, isa.SMOOTHER_LINE_AUTO)
    before = isa.MatrixFreeSystem(N, N, *dom)
    before.set_smoother(isa.SMOOTHER_LINE_AUTO)
    before.set_preconditioner(isa.PRECOND_MG_ANY)
    z = after._handle.apply_preconditioner(r)
    assert np.array_equal(z, before._handle.apply_preconditioner(r))
    before.set_preconditioner(isa.PRECOND_NONE)                          # the hierarchy goes, the smoother stays for the next one
    assert before.smoother_info() == (isa.SMOOTHER_LINE_AUTO, LR.LINE_Y)
    before.set_preconditioner(isa.PRECOND_MG_ANY)
    assert np.array_equal(z, before._handle.apply_preconditioner(r))
    xa, xb = solve_bits(after), solve_bits(before)
    assert xa[1] == xb[1] and np.array_equal(xa[0], xb[0])


# ---- the project's invariants under a line smoother ----------------------------------------------------------------------------
@pytest.mark.parametrize("N,dom", [(50, LR.STRETCH_Y), (258, LR.STRETCH_X)], ids=["n50-x", "n258-y"])
def test_batch_has_the_bits_of_single_solves(N, dom):
    import iterative_solvers_amd as isa
    s = system(N, dom, R.MG_ANY, isa.SMOOTHER_LINE_AUTO)
    rhs = np.random.default_rng(N).standard_normal((4, s.size()))
    rhs[2] *= 1e-3                                                       # the systems differ in scale as well
    p = rel_params()
    singles = [solve_bits(s, b, p) for b in rhs]
    xb, rb = s._handle.solve_batch(p, rhs)
    print(f"N={N}: iterations {[f[1][0] for f in singles]}")
    for k, (x, f) in enumerate(singles):
        assert f[1] and 1 <= f[0] <= 8
        assert tuple(getattr(rb[k], q) for q in FIELDS) == f
        assert np.array_equal(xb[k], x)
    xb2, _ = s._handle.solve_batch(p, rhs)
    assert np.array_equal(xb, xb2)


def test_time_steps_have_the_bits_of_set_rhs_and_a_warm_solve():
    """theta = 1: the step's right-hand side is g - sigma u, two roundings per element that NumPy repeats exactly"""
    import iterative_solvers_amd as isa
    N, dom, tau, steps = 64, LR.STRETCH_X, 1e-4, 3
    sigma = 1.0 / tau
    rng = np.random.default_rng(N)
    n = int(R.model.interior_mask(N).sum())
    u0, g = 1e-4 * rng.standard_normal(n), rng.standard_normal(n)
    s = system(N, dom, R.MG, isa.SMOOTHER_LINE_AUTO)
    s._handle.set_rhs(g)
    un, res, done = s.time_steps(u0, tau, 1.0, steps)
    assert done == steps and all(r.converged and r.iterations >= 1 for r in res)
    o = system(N, dom, R.MG, isa.SMOOTHER_LINE_AUTO)
    h = o._handle
    h.set_shift(sigma)
    u = u0
    for k in range(steps):
        h.set_rhs(g - sigma * u)
        h.set_initial_guess(u)
        r1 = h.solve(rel_params(max_iterations=10000))
        assert tuple(getattr(r1, f) for f in FIELDS) == tuple(getattr(res[k], f) for f in FIELDS)
        u = h.solution()
    assert np.array_equal(u, un)


def test_two_identical_calls_give_identical_bits():
    import iterative_solvers_amd as isa
    for dom in (LR.STRETCH_X, LR.STRETCH_Y):
        s = system(258, dom, R.MG_ANY, isa.SMOOTHER_LINE_AUTO)
        b = np.random.default_rng(3).standard_normal(s.size())
        first, second = solve_bits(s, b), solve_bits(s, b)
        assert first[1] == second[1] and np.array_equal(first[0], second[0])
        other = solve_bits(system(258, dom, R.MG_ANY, isa.SMOOTHER_LINE_AUTO), b)
        assert first[1] == other[1] and np.array_equal(first[0], other[0])


def test_set_shift_and_set_smoother_in_either_order():
    import iterative_solvers_amd as isa
    N, kind, dom, sigma = LR.SHIFT_CASE
    lv = LR.shifted_levels(N, dom, kind, sigma)
    r = LR.cycle_vectors(N, dom)[0]
    d = LR.auto_direction(lv)
    zr = LR.apply_M_line(lv, r, d)
    tol = R.tol_M(LR.cycle_floor_line(lv, r, d, zr))
    a = system(N, dom, kind)
    a.set_shift(sigma)
    a.set_smoother(isa.SMOOTHER_LINE_AUTO)
    b = system(N, dom, kind, isa.SMOOTHER_LINE_AUTO)
    b.set_shift(sigma)
    c = isa.MatrixFreeSystem(N, N, *dom)                                 # and both before the hierarchy
    c.set_smoother(isa.SMOOTHER_LINE_AUTO)
    c.set_shift(sigma)
    c.set_preconditioner(isa_kind(kind))
    za = a._handle.apply_preconditioner(r)
    assert np.array_equal(za, b._handle.apply_preconditioner(r)) and np.array_equal(za, c._handle.apply_preconditioner(r))
    assert show("shifted line cycle, max|z - z_ref| / max|z_ref|", np.abs(za - zr).max() / np.abs(zr).max(), tol)
    b.set_shift(0.0)                                                     # back: the tables of the Laplacian again
    assert np.array_equal(b._handle.apply_preconditioner(r), system(N, dom, kind, isa.SMOOTHER_LINE_AUTO)._handle.apply_preconditioner(r))


@functools.lru_cache(maxsize=None)
def dense_spectrum(N, dom):
    """eigvalsh of -A assembled from the restatement's 5-point formula on unit vectors"""
    lv = R.levels_for(N, dom, R.MG)
    n = int(lv[0].mask.sum())
    A = np.empty((n, n))
    e = np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        A[:, j] = R.apply_A(lv, e)
        e[j] = 0.0
    return np.linalg.eigvalsh(-0.5 * (A + A.T))


def test_eigs_under_line_auto_and_under_jacobi():
    import iterative_solvers_amd as isa
    N, dom, nev, tol = 64, LR.STRETCH_X, 4, 1e-8
    truth = dense_spectrum(N, dom)
    out = {}
    for name, smoother in (("line", isa.SMOOTHER_LINE_AUTO), ("jacobi", isa.SMOOTHER_JACOBI)):
        s = system(N, dom, R.MG, smoother)
        x0 = np.random.default_rng(0).standard_normal((nev, s.size()))
        lam, V, info = s.eigs(nev, block=nev, tol=tol, max_iterations=500, x0=x0)
        assert info["converged"] and info["stop_reason"] == isa.EIG_CONVERGED
        for j in range(nev):
            v = V[j]
            res = np.linalg.norm(-s.apply(v) - lam[j] * v) / np.linalg.norm(v) / lam[j]      # relative residual of the pair
            gap = np.abs(truth - lam[j]).min() / lam[j]
            print(f"  {name} pair {j}: lambda {lam[j]:.12g}, residual {res:.1e}, distance to the spectrum {gap:.1e}")
            assert res <= 2 * tol
            assert gap <= res + 1e-12                                   # symmetric residual bound (+ the dense solver's rounding)
        out[name] = (lam, info["iterations"])
    print(f"  iterations: line {out['line'][1]}, jacobi {out['jacobi'][1]}")
    assert np.all(np.abs(out["line"][0] - out["jacobi"][0]) <= 2 * tol * out["jacobi"][0])
    assert np.all(np.abs(out["line"][0] - truth[:nev]) <= 2 * tol * truth[:nev])
    assert out["line"][1] <= out["jacobi"][1]


# ---- bits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,kind", [(64, R.MG), (258, R.MG_ANY)])
def test_jacobi_after_line_has_the_bits_of_a_fresh_handle(N, kind):
    import iterative_solvers_amd as isa
    dom = LR.STRETCH_X
    r = LR.cycle_vectors(N, dom)[0]
    fresh = system(N, dom, kind)
    z, sol = fresh._handle.apply_preconditioner(r), solve_bits(fresh, r)
    s = system(N, dom, kind, isa.SMOOTHER_LINE_Y)
    zl = s._handle.apply_preconditioner(r)
    assert np.abs(zl - z).max() > 0.1 * np.abs(z).max()                 # the line cycle is another operator
    for smoother in (isa.SMOOTHER_LINE_X, isa.SMOOTHER_JACOBI):
        s.set_smoother(smoother)
    assert np.array_equal(s._handle.apply_preconditioner(r), z)
    back = solve_bits(s, r)
    assert back[1] == sol[1] and np.array_equal(back[0], sol[0])
    xb, _ = s._handle.solve_batch(rel_params(), r[None, :])
    assert np.array_equal(xb[0], sol[0])


@pytest.mark.parametrize("n", [16, 32])
def test_one_level_grids_give_the_same_bits_under_every_smoother(n):
    import iterative_solvers_amd as isa
    dom = LR.STRETCH_X
    r = np.random.default_rng(n).standard_normal(int(R.model.interior_mask(n).sum()))
    outs = []
    for smoother in (isa.SMOOTHER_JACOBI, isa.SMOOTHER_LINE_X, isa.SMOOTHER_LINE_Y, isa.SMOOTHER_LINE_AUTO):
        s = system(n, dom, R.MG_ANY, smoother)
        assert s.preconditioner_info()[2] == 1 and s.smoother_info()[0] == smoother
        outs.append((s._handle.apply_preconditioner(r),) + solve_bits(s, r))
    for z, x, f in outs[1:]:
        assert np.array_equal(z, outs[0][0]) and np.array_equal(x, outs[0][1]) and f == outs[0][2]


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    from oracle.oracle import OracleGrid
    N, dom = 64, LR.STRETCH_X
    r = LR.cycle_vectors(N, dom)[0]
    s = system(N, dom, R.MG, isa.SMOOTHER_LINE_Y)
    z = s._handle.apply_preconditioner(r)
    state = (s.preconditioner_info(), s.smoother_info())
    for bad in (4, -1, 99):
        with pytest.raises(ValueError, match="unknown smoother"):
            s.set_smoother(bad)
        assert (s.preconditioner_info(), s.smoother_info()) == state
    with pytest.raises(ValueError, match="point Jacobi only"):         # the fp32 cycle while a line smoother is set
        s.set_preconditioner(isa.PRECOND_MG, isa.CYCLE_F32)
    assert (s.preconditioner_info(), s.smoother_info()) == state
    assert np.array_equal(s._handle.apply_preconditioner(r), z)

    f32 = isa.MatrixFreeSystem(N, N, *dom)                              # the other order: a line smoother while the cycle is fp32
    f32.set_preconditioner(isa.PRECOND_MG, isa.CYCLE_F32)
    state32 = (f32.preconditioner_info(), f32.smoother_info())
    for smoother in (isa.SMOOTHER_LINE_X, isa.SMOOTHER_LINE_Y, isa.SMOOTHER_LINE_AUTO):
        with pytest.raises(ValueError, match="MI355CG_CYCLE_F32"):
            f32.set_smoother(smoother)
        assert (f32.preconditioner_info(), f32.smoother_info()) == state32
    f32.set_smoother(isa.SMOOTHER_JACOBI)                               # what it has: accepted
    assert (f32.preconditioner_info(), f32.smoother_info()) == state32

    lone = isa.MatrixFreeSystem(N, N, *dom)                             # no hierarchy: the refusal of the fp32 cycle still holds
    lone.set_smoother(isa.SMOOTHER_LINE_AUTO)
    with pytest.raises(ValueError, match="point Jacobi only"):
        lone.set_preconditioner(isa.PRECOND_MG, isa.CYCLE_F32)
    assert lone.preconditioner_info() == (isa.PRECOND_NONE, isa.CYCLE_F64, 0) and lone.smoother_info() == (isa.SMOOTHER_LINE_AUTO, LR.LINE_Y)

    mixed = isa.MatrixFreeSystem(N, N, *dom, dtype=isa.F32_MIXED)
    with pytest.raises(ValueError, match="fp64 only"):
        mixed.set_smoother(isa.SMOOTHER_LINE_AUTO)
    assert mixed.smoother_info() == (isa.SMOOTHER_JACOBI, 0)

    csr = isa.CrsMatrix(*OracleGrid(16, 16, *dom).csr())
    with pytest.raises(ValueError, match="CSR"):
        csr._handle.set_smoother(isa.SMOOTHER_LINE_X)
    assert csr._handle.smoother_info() == (isa.SMOOTHER_JACOBI, 0)

    lib = _capi.load()
    slab = C.c_void_p()
    y_lo, y_hi = C.c_int(), C.c_int()
    _capi.check(lib.mi355cg_slab_rows(N, 2, 0, C.byref(y_lo), C.byref(y_hi)))
    _capi.check(lib.mi355cg_create_slab(N, N, *dom, _capi.F64, 0, y_lo.value, y_hi.value, C.byref(slab)))
    try:
        assert lib.mi355cg_set_smoother(slab, isa.SMOOTHER_LINE_X) == _capi.ERR_INVALID
        assert b"single-GPU only" in lib.mi355cg_last_error()
        sm, dr = C.c_int(-1), C.c_int(-1)
        assert lib.mi355cg_get_smoother(slab, C.byref(sm), C.byref(dr)) == _capi.OK and (sm.value, dr.value) == (0, 0)
    finally:
        lib.mi355cg_destroy(slab)
    assert lib.mi355cg_set_smoother(None, isa.SMOOTHER_LINE_X) == _capi.ERR_INVALID
