"""Warm starts on the GPU: a guess of zeros is the cold solve bit for bit on every path; a guess is the
shifted problem b' = b - A x0 bit for bit in everything but x; continuation after a cap or an interruption; a good guess saves
multigrid-PCG iterations; an exact guess returns at once; batches with a guess per system; the state rules and refusals; the C++
layer.  tests/test_warm_start_cpu.py restates the algorithm in NumPy and establishes the identities used here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOM = (1.0, 2.0, 1.0, 2.0)
FIELDS = ("iterations", "converged", "stop_reason", "final_residual_norm", "final_precision", "final_error_norm", "r_norm2",
          "initial_r_norm2")


def system(N, precond=None, cycle=None, env=None):
    """A MatrixFreeSystem created under `env` (the knobs are read at mi355cg_create), with a preconditioner if asked for."""
    import iterative_solvers_amd as isa
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = isa.MatrixFreeSystem(N, N, *DOM)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if precond is not None:
        s.set_preconditioner(precond, isa.CYCLE_F64 if cycle is None else cycle)
    return s


def rel_params(eps=1e-8, max_iterations=10000, fixed=False, diagnostics=0):
    import iterative_solvers_amd as isa
    p = isa.default_params(isa._capi.RULE_REL_2NORM)
    p.eps_rel, p.max_iterations, p.fixed_iterations, p.diagnostics, p.use_true_solution = eps, max_iterations, int(fixed), diagnostics, 0
    return p


def msg_params(eps_residual=1e-6, eps_precision=-1.0, eps_exact_error=-1.0, use_u=0, every=10, max_iterations=10000):
    import iterative_solvers_amd as isa
    p = isa.default_params(isa._capi.RULE_MSG_MAXNORM)
    p.eps_residual, p.eps_precision, p.eps_exact_error = eps_residual, eps_precision, eps_exact_error
    p.use_true_solution, p.callback_every, p.max_iterations = use_u, every, max_iterations
    return p


def fields(res):
    return tuple(getattr(res, f) for f in FIELDS)


def run(s, p, x0=None, cont=False, callbacks=False, stop=None, on_call=None):
    """One solve on s: (result fields, x, recursive r, callback triples)"""
    h = s._handle
    if x0 is not None:
        h.set_initial_guess(x0)
    if cont:
        h.use_solution_as_initial_guess()
    calls = []

    def cb(it, pr, rs, er):
        calls.append((it, pr, rs, er))
        if on_call:
            on_call(it)
    res = h.solve(p, cb if callbacks or on_call else None, stop)
    return fields(res), h.solution(), h.recursive_residual(), calls


def same(got, ref, what=""):
    assert got[0] == ref[0], (what, got[0], ref[0])
    assert got[3] == ref[3], what
    assert np.array_equal(got[1], ref[1]), what
    assert np.array_equal(got[2], ref[2]), what


# ---- 1. a zero guess is the cold solve --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["rel_graph", "msg_callbacks", "xfold16", "diagnostics"])
def test_zero_guess_equals_cold_on_the_plain_path(case):
    s = system(64, env={"MI355CG_XFOLD": "16"} if case == "xfold16" else None)
    if case == "xfold16":
        assert s._handle.layout()["x_fold"] == 16
    callbacks = case in ("msg_callbacks", "diagnostics")
    if case == "msg_callbacks":
        p = msg_params(eps_residual=1e-6, eps_precision=1e-9, eps_exact_error=1e-9, use_u=1, every=10)
    else:
        p = rel_params(diagnostics=1 if case == "diagnostics" else 0)      # 10000 >= 4 x 200: the chunks are graph-replayed
    cold = run(s, p, callbacks=callbacks)
    assert cold[0][0] > 32 and (not callbacks or len(cold[3]) > 3)
    warm = run(s, p, x0=np.zeros(s.size()), callbacks=callbacks)          # after a cold one with equal params: the cached graphs
    same(warm, cold, case)
    same(run(s, p, callbacks=callbacks), cold, case + ": the guess was consumed")


@pytest.mark.parametrize("N, kind, cycle", [(258, "any", 0), (258, "any", 1), (64, "mg", 0)])
def test_zero_guess_equals_cold_on_the_preconditioned_path(N, kind, cycle):
    import iterative_solvers_amd as isa
    s = system(N, isa.PRECOND_MG_ANY if kind == "any" else isa.PRECOND_MG, cycle)
    for p, callbacks in ((rel_params(), False), (msg_params(use_u=1, eps_exact_error=1e-9, every=2), True)):
        cold = run(s, p, callbacks=callbacks)
        assert 1 <= cold[0][0] <= 14
        same(run(s, p, x0=np.zeros(s.size()), callbacks=callbacks), cold, (N, kind, cycle))


def batch_problem(N=100):
    import iterative_solvers_amd as isa
    s = system(N, isa.PRECOND_MG_ANY)
    rng = np.random.default_rng(N)
    b = np.ascontiguousarray(np.stack([s.get_rhs(), rng.standard_normal(s.size()), np.ones(s.size())]))
    return s, b


def test_zero_guesses_equal_the_cold_batch():
    s, b = batch_problem()
    p = rel_params()
    xc, rc = s._handle.solve_batch(p, b)
    xw, rw = s._handle.solve_batch(p, b, x0=np.zeros_like(b))
    assert np.array_equal(xc, xw)
    assert [fields(r) for r in rc] == [fields(r) for r in rw]


# ---- 2. a guess is the shifted problem ----------------------------------------------------------------------------------------
SHIFT_CASES = [("plain", 64, None, None), ("fold", 64, None, None), ("mg_any", 258, "any", 0), ("mg_any_f32", 258, "any", 1)]


@pytest.mark.parametrize("name, N, kind, cycle", SHIFT_CASES)
def test_shift_identity(name, N, kind, cycle):
    """b with the guess x0 and b' = b - A x0 from zero: the same r0, so the same residuals, counts, reasons and residual callbacks,
    bit for bit; x_warm = x0 + x_shift up to one rounding per step on each side and the final sum."""
    import iterative_solvers_amd as isa
    s = system(N, None if kind is None else isa.PRECOND_MG_ANY, cycle, env={"MI355CG_XFOLD": "16"} if name == "fold" else None)
    b = s.get_rhs()
    x0 = 1e-2 * np.random.default_rng(7).standard_normal(s.size())
    bs = b - s.apply(x0)
    for p, callbacks in ((rel_params(max_iterations=12, fixed=True), False), (msg_params(eps_residual=1e-6, every=5), True)):
        s._handle.set_rhs(b)
        warm = run(s, p, x0=x0, callbacks=callbacks)
        s._handle.set_rhs(bs)
        shift = run(s, p, callbacks=callbacks)
        k = warm[0][0]
        assert k == shift[0][0] >= 1 and warm[0][2] == shift[0][2]                    # iterations, stop reason
        assert warm[0][6] == shift[0][6] and warm[0][3] == shift[0][3]                # ||r||_2, max |r|
        assert np.array_equal(warm[2], shift[2])
        assert [c[0] for c in warm[3]] == [c[0] for c in shift[3]] and [c[2] for c in warm[3]] == [c[2] for c in shift[3]]
        assert np.all(np.abs(warm[1] - (x0 + shift[1])) <= (k + 2) * 2.0 ** -52 * np.abs(warm[1]).max()), (name, k)
        if not callbacks:
            assert k == 12
        else:
            assert warm[0][2] == isa.StopCriterion.RESIDUAL and len(warm[3]) >= 3


# ---- 3. continuation ------------------------------------------------------------------------------------------------------------
def test_continuing_a_converged_multigrid_solve_takes_no_iteration():
    import iterative_solvers_amd as isa
    s = system(258, isa.PRECOND_MG_ANY)
    first = run(s, rel_params(1e-8))
    assert first[0][1] == 1
    again = run(s, rel_params(1e-7), cont=True)
    assert again[0][:3] == (0, 1, isa.StopCriterion.ITERATIONS)
    assert again[0][7] <= 1e-7 * first[0][7] and again[0][6] == again[0][7]      # ||r0||: the true residual of x, against ||b||
    assert np.array_equal(again[1], first[1])


@pytest.mark.parametrize("how", ["capped", "interrupted"])
def test_continuing_a_plain_solve_reaches_the_cold_target(how):
    """Plain CG at N = 64, eps 1e-8, stopped at half its cold count (ITERATIONS) or after iteration 1 (INTERRUPTED, the flag set from
    the first callback), then continued with the cap lifted.  The factor 2 on the true residual is a cap against a broken start;
    observed ratios: DESIGN section 10.4."""
    import iterative_solvers_amd as isa
    s = system(64)
    eps = 1e-8
    cold = run(s, rel_params(eps))
    assert cold[0][1] == 1
    bnorm = cold[0][7]                                                       # ||b||_2 as the library reduces it
    cold_true = np.linalg.norm(s._handle.true_residual())
    if how == "capped":
        part = run(s, rel_params(eps, max_iterations=cold[0][0] // 2))
        assert part[0][:3] == (cold[0][0] // 2, 0, isa.StopCriterion.ITERATIONS)
    else:
        flag = C.c_int(0)

        def stop_at_first(it):
            flag.value = 1
        part = run(s, rel_params(eps, diagnostics=1), stop=flag, on_call=stop_at_first)
        assert part[0][:3] == (1, 0, isa.StopCriterion.INTERRUPTED)
    rest = run(s, rel_params(eps), cont=True)
    assert rest[0][1] == 1 and rest[0][6] <= eps * bnorm
    # it starts where the first part stopped: the true residual of that x is the recursive one up to ~ k u cond(A) ||b|| =
    # 80 x 1e-16 x 4e3 ||b|| = 3e-11 ||b||, against a residual of at least 1e-8 ||b||
    assert rest[0][7] == pytest.approx(part[0][6], rel=1e-2)
    true = np.linalg.norm(s._handle.true_residual())
    print(f"{how}: cold {cold[0][0]} iterations, {part[0][0]} + {rest[0][0]}; true residual {true:.3e} against cold {cold_true:.3e}, "
          f"ratio {true / cold_true:.3f}")
    assert true <= max(eps * bnorm, 2 * cold_true)


# ---- 4. a good guess pays (multigrid) -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", [0, 1])
def test_a_good_guess_saves_multigrid_iterations(cycle):
    import iterative_solvers_amd as isa
    s = system(258, isa.PRECOND_MG_ANY, cycle)
    cold = run(s, rel_params(1e-8))
    x4 = run(s, rel_params(1e-4))[1].copy()
    warm = run(s, rel_params(1e-8), x0=x4)
    print(f"cycle {cycle}: cold {cold[0][0]}, warm from the 1e-4 solution {warm[0][0]}")
    assert warm[0][1] == 1 and 1 <= warm[0][0] < cold[0][0]
    assert warm[0][6] <= 1e-8 * cold[0][7]


def test_plain_cg_counts_with_a_guess_are_recorded():
    """A restarted plain CG has lost its Krylov space: the counts are printed, not asserted against each other."""
    s = system(64)
    cold = run(s, rel_params(1e-8))
    x4 = run(s, rel_params(1e-4))[1].copy()
    warm = run(s, rel_params(1e-8), x0=x4)
    print(f"plain N=64: cold {cold[0][0]}, warm from the 1e-4 solution {warm[0][0]}")
    assert warm[0][1] == 1 and warm[0][6] <= 1e-8 * cold[0][7]


# ---- 5. an exact guess -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, precond, tight_eps", [(100, True, 1e-12), (64, False, 1e-12), (258, True, 1e-13)])
def test_an_exact_guess_returns_at_once(N, precond, tight_eps):
    """x0 = a multigrid solution to 1e-12.  REL_2NORM 1e-8: 0 iterations, converged, x untouched.  MSG with eps_residual = 1e-6:
    RESIDUAL with 0 iterations and no NaN, on the plain (N = 64) and the preconditioned path.  The guess has to be exact for the MSG
    rule, max |b - A x0| < 1e-6: the 1e-12 solution gives 2.4e-8 at N = 64 and 2.7e-7 at N = 100, but 2.6e-6 at N = 258, where
    ||b||_2 = 1.27e7, so that grid takes the 1e-13 solution (1.3e-7; figures of the NumPy restatement in test_warm_start_cpu.py)."""
    import iterative_solvers_amd as isa
    s = system(N, isa.PRECOND_MG_ANY)
    tight = run(s, rel_params(tight_eps))
    x = tight[1].copy()
    print(f"N={N}: the {tight_eps:g} solve: {tight[0][0]} iterations, converged {tight[0][1]}, ||r||_2 {tight[0][6]:.3e}, "
          f"||b||_2 {tight[0][7]:.3e}, max |r| {np.abs(tight[2]).max():.3e}, max |b - A x| {np.abs(s._handle.true_residual()).max():.3e}")
    assert tight[0][1] == 1
    if not precond:
        s.set_preconditioner(isa.PRECOND_NONE)
    rel = run(s, rel_params(1e-8), x0=x)
    assert rel[0][:3] == (0, 1, isa.StopCriterion.ITERATIONS)
    assert np.array_equal(rel[1], x)
    msg = run(s, msg_params(eps_residual=1e-6), x0=x, callbacks=True)
    print(f"N={N}: MSG from that x: {msg[0][:3]}, callbacks {msg[3]}")
    assert msg[0][:3] == (0, 1, isa.StopCriterion.RESIDUAL)
    assert np.array_equal(msg[1], x)
    assert [c[0] for c in msg[3]] == [0, 0]                                  # the it = 0 report and the final one
    assert all(np.isfinite(v) for v in msg[0]) and np.isfinite(msg[1]).all() and np.isfinite(msg[2]).all()
    assert msg[3][0][2] == msg[0][3] < 1e-6


def test_a_stop_request_before_a_plain_warm_solve():
    """The plain path looks at the stop flag before it looks at anything else, cold or warm (the reference tests its flag at the top
    of every iteration, msg_solver.cpp:82-87, and the host has not fetched the start state yet): INTERRUPTED with 0 iterations and
    x = x0 even where the start already meets the rule, and the norms of a state that was never fetched are 0, as for a cold solve.
    The preconditioned path has the norms of the start on the host and tests the rule first (solve_mg's order, which batches follow)."""
    import iterative_solvers_amd as isa
    s = system(64, isa.PRECOND_MG_ANY)
    x = run(s, rel_params(1e-12))[1].copy()
    flag = C.c_int(1)
    mg = run(s, rel_params(1e-8), x0=x, stop=flag)
    assert mg[0][:3] == (0, 1, isa.StopCriterion.ITERATIONS) and mg[0][7] > 0
    s.set_preconditioner(isa.PRECOND_NONE)
    cold = run(s, rel_params(1e-8), stop=flag)
    assert cold[0][:3] == (0, 0, isa.StopCriterion.INTERRUPTED)
    same(run(s, rel_params(1e-8), x0=np.zeros(s.size()), stop=flag), cold, "zero guess, flag set")
    warm = run(s, rel_params(1e-8), x0=x, stop=flag)
    assert warm[0] == cold[0] and np.array_equal(warm[1], x)


# ---- 6. batches --------------------------------------------------------------------------------------------------------------------
def batch_guesses(s, b):
    """one zero, one a 1e-4 solution, one an already-converged solution"""
    h = s._handle
    x0 = np.zeros_like(b)
    h.set_rhs(b[1])
    h.solve(rel_params(1e-4))
    x0[1] = h.solution()
    h.set_rhs(b[2])
    h.solve(rel_params(1e-10))
    x0[2] = h.solution()
    return x0


def singles(s, p, b, x0, stop=None):
    out = []
    for k in range(len(b)):
        s._handle.set_rhs(b[k])
        out.append(run(s, p, x0=x0[k], stop=stop))
    return out


def test_batch_with_guesses_equals_the_single_warm_solves():
    import torch
    s, b = batch_problem()
    x0 = batch_guesses(s, b)
    p = rel_params(1e-8)
    ref = singles(s, p, b, x0)
    assert ref[2][0][0] == 0 and ref[2][0][1] == 1 and ref[1][0][0] >= 1 and ref[0][0][0] >= 2
    keep = x0.copy()
    xh, rh = s._handle.solve_batch(p, b, x0=x0)
    assert np.array_equal(x0, keep)
    xd, rd = s._handle.solve_batch(p, torch.from_numpy(b).cuda(), x0=torch.from_numpy(x0).cuda())
    for x, res in ((xh, rh), (xd.cpu().numpy(), rd)):
        for k in range(3):
            assert fields(res[k]) == ref[k][0], k
            assert np.array_equal(x[k], ref[k][1]), k
    assert rh[2].iterations == 0
    m = msg_params(eps_residual=1e-6, eps_precision=1e-9)                     # the MSG start test, per system
    refm = singles(s, m, b, x0)
    xm, rm = s._handle.solve_batch(m, b, x0=x0)
    for k in range(3):
        assert fields(rm[k]) == refm[k][0], k
        assert np.array_equal(xm[k], refm[k][1]), k
    assert (rm[2].iterations, rm[2].stop_reason) == (0, 2)


def test_batch_with_a_stop_request_before_the_call():
    """Per system the batch is the single warm solve, which tests the rule before the flag (solve_mg's order): with the three
    guesses at eps 1e-8 the converged one returns converged and the others INTERRUPTED; at eps 1e-14 every system is still
    iterating, so every system is INTERRUPTED.  x is the guess in both."""
    import iterative_solvers_amd as isa
    s, b = batch_problem()
    x0 = batch_guesses(s, b)
    flag = C.c_int(1)
    for eps, reasons in ((1e-14, [isa.StopCriterion.INTERRUPTED] * 3),
                         (1e-8, [isa.StopCriterion.INTERRUPTED, isa.StopCriterion.INTERRUPTED, isa.StopCriterion.ITERATIONS])):
        p = rel_params(eps)
        ref = singles(s, p, b, x0, stop=flag)
        x, res = s._handle.solve_batch(p, b, flag, x0=x0)
        assert [r.stop_reason for r in res] == reasons and [r.iterations for r in res] == [0, 0, 0]
        assert np.array_equal(x, x0)
        for k in range(3):
            assert fields(res[k]) == ref[k][0] and np.array_equal(x[k], ref[k][1])


# ---- 7. state and refusals ------------------------------------------------------------------------------------------------------
def test_state_rules():
    import iterative_solvers_amd as isa
    s = system(64)
    h = s._handle
    with pytest.raises(isa.Mi355cgError, match="no solve has run"):
        h.use_solution_as_initial_guess()
    p = rel_params(1e-8)
    cold = run(s, p)
    x0 = 1e-2 * np.random.default_rng(1).standard_normal(s.size())
    h.set_initial_guess(x0)
    for getter in (h.solution, h.recursive_residual, h.true_residual):
        with pytest.raises(isa.Mi355cgError, match="initial guess"):
            getter()
    h.set_rhs(s.get_rhs())                                                   # allowed between the guess and the solve
    warm = run(s, p)
    assert warm[0][1] == 1 and warm[0][7] != cold[0][7] and np.isfinite(h.true_residual()).all()
    same(run(s, p), cold, "the guess is one-shot: the second solve is cold")
    h.set_initial_guess(x0)
    h.set_initial_guess(None)                                                # withdrawn: x stays unusable until the next solve
    with pytest.raises(isa.Mi355cgError, match="initial guess"):
        h.solution()
    with pytest.raises(isa.Mi355cgError):
        h.use_solution_as_initial_guess()
    same(run(s, p), cold, "a withdrawn guess leaves a cold solve")
    h.set_initial_guess(x0)
    s.set_preconditioner(isa.PRECOND_MG)                                     # the guess belongs to the handle, not to the hierarchy
    s.set_preconditioner(isa.PRECOND_NONE)
    same(run(s, p), warm, "the guess survives the preconditioner")


def test_device_tensor_and_numpy_guess_give_the_same_bits():
    import torch
    s = system(100)
    x0 = 1e-2 * np.random.default_rng(2).standard_normal(s.size())
    p = rel_params(max_iterations=20, fixed=True)
    host = run(s, p, x0=x0)
    dev = run(s, p, x0=torch.from_numpy(x0).cuda())
    same(dev, host)
    with pytest.raises(ValueError, match="dtype"):
        s._handle.set_initial_guess(torch.from_numpy(x0).cuda().float())
    s2 = system(100)
    import iterative_solvers_amd as isa
    via_solver = isa.MatrixFreeSolver(s2, s2.get_rhs(), 1e-6, 20)
    assert np.array_equal(via_solver.solve(fixed_iterations=True, x0=x0), host[1])


def test_refusals():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    from iterative_solvers_amd.solver import _Handle
    from oracle.oracle import OracleGrid
    mixed = isa.MatrixFreeSystem(64, 64, *DOM, dtype=isa.F32_MIXED)
    csr = isa.CrsMatrix(*OracleGrid(16, 16, *DOM).csr())
    slab = _Handle.__new__(_Handle)
    slab._lib, slab._h, slab._device = _capi.load(), C.c_void_p(), 0
    _capi.check(slab._lib.mi355cg_create_slab(64, 64, *DOM, _capi.F64, 0, 1, 31, C.byref(slab._h)))
    slab.size = int(slab._lib.mi355cg_size(slab._h))
    for h, why in ((mixed._handle, "fp64 only"), (csr._handle, "CSR"), (slab, "single-GPU")):
        with pytest.raises(ValueError, match=why):
            h.set_initial_guess(np.zeros(h.size))
        with pytest.raises(ValueError, match=why):
            h.use_solution_as_initial_guess()
        with pytest.raises(ValueError, match=why):
            h.set_initial_guess(None)
    mixed_solver = isa.MatrixFreeSolver(mixed, mixed.get_rhs(), 1e-6, 10000)      # the handle is as it was
    mixed_solver.solve()
    assert mixed_solver.last_results.converged
    slab.close()


# ---- 8. C++ -------------------------------------------------------------------------------------------------------------------------
def checksum(x):
    t = 0.0
    for v in x.tolist():
        t += v
    return t


def test_cpp_compat_warm_start(tmp_path):
    """tests/cpp/warm_start_compat_driver.cpp solves, continues and warm-starts through MatrixFreeSolver and MSGSolver; it exits 0
    when its counts and checksums are the ones computed here."""
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import build as b
    b.build()
    exe = str(tmp_path / "warm_start_compat_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(ROOT, "iterative_solvers_amd", "compat"),
                           os.path.join(ROOT, "tests", "cpp", "warm_start_compat_driver.cpp"),
                           "-L", os.path.join(ROOT, "iterative_solvers_amd"), "-lmi355cg",
                           "-Wl,-rpath," + os.path.join(ROOT, "iterative_solvers_amd"), "-o", exe])
    N, cap = 64, 40
    s = system(N)
    rhs = s.get_rhs()
    cold = isa.MatrixFreeSolver(s, rhs, 1e-8, 100000)
    x_cold = cold.solve()
    capped = isa.MatrixFreeSolver(s, rhs, 1e-8, cap)
    capped.solve()
    assert capped.iterations == cap < cold.iterations
    s._handle.use_solution_as_initial_guess()
    cont = isa.MatrixFreeSolver(s, rhs, 1e-8, 100000)
    x_cont = cont.solve()
    x4 = isa.MatrixFreeSolver(s, rhs, 1e-4, 100000).solve()
    warm = isa.MatrixFreeSolver(s, rhs, 1e-8, 100000)
    x_warm = warm.solve(x0=x4)
    g = isa.GridSystem(N, N, *DOM)
    msg = isa.MSGSolver(g, g.get_rhs(), 1e-6, 100000)
    msg.setPrecisionEps(-1.0)
    msg.setExactErrorEps(-1.0)
    x_msg = msg.solve(x0=x_cold)
    expect = [str(cold.iterations), str(cont.iterations), str(warm.iterations), str(msg.iterations), str(int(msg.stop_reason)),
              checksum(x_cont).hex(), checksum(x_warm).hex(), checksum(x_msg).hex()]
    out = subprocess.run([exe, str(N), str(cap)] + expect, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
