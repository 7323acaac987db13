"""The host loop protocol of the CG solves (csrc/solve_loop.h): which iterations a callback sees, with which numbers, and what
the results report, must not depend on how the iterations are cut into chunks.  Three loops share the protocol: the plain
handle, a CSR handle and a team (here a LOCAL team of two parts on one GPU).  For each, a run with callback_every = 1
records every (it, dmax, rmax, emax); runs with other cadences and chunk lengths must deliver exactly the iterations of
msg_solver.cpp:75-77,172-183,193-195 with those bits."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

N = 64                          # the smallest grid test_gpu_csr.py trusts for the CSR MSG solve
EVERY = 7
PATHS = ["plain", "csr", "team"]
FIELDS = ("iterations", "converged", "stop_reason", "final_residual_norm", "final_precision", "final_error_norm",
          "r_norm2", "initial_r_norm2")
INTERRUPTED = 4


def _open(path):
    """(object to keep alive, solve(params, callback, stop_flag), close)"""
    import iterative_solvers_amd as isa
    from iterative_solvers_amd.distributed import Team
    from oracle.oracle import OracleGrid
    if path == "plain":
        s = isa.MatrixFreeSystem(N, N, 1.0, 2.0, 1.0, 2.0)
        return s._handle.solve, s._handle.close
    if path == "csr":
        og = OracleGrid(N, N)
        A = isa.CrsMatrix(*og.csr())
        A._handle.set_rhs(og.rhs())
        A._handle.set_true_solution(og.true_solution())
        return A._handle.solve, A._handle.close
    t = Team.local(N, 2)
    return t.solve, t.close


def _run(solve, stop_at=None, **kw):
    import iterative_solvers_amd as isa
    p = isa.default_params(0)
    p.eps_precision = p.eps_residual = 1e-9
    p.eps_exact_error = -1.0
    p.use_true_solution = 1
    for k, v in kw.items():
        setattr(p, k, v)
    cbs, stop = [], C.c_int(0)

    def cb(it, *norms):
        cbs.append((it,) + norms)
        if it == stop_at:
            stop.value = 1
    res = solve(p, cb, stop if stop_at is not None else None)
    return cbs, tuple(getattr(res, f) for f in FIELDS)


def _expected(K, every, last_in_loop=False):
    """iteration 0, iteration 1 and the cadence inside 1 .. K-1 (the iteration that stops reports only through the final
    callback; one that merely hits the iteration cap did not stop and reports in the loop as well), then the final one"""
    top = K if last_in_loop else K - 1
    return [0] + [k for k in range(1, top + 1) if k == 1 or (every > 0 and k % every == 0)] + [K]


@pytest.fixture(scope="module", params=PATHS)
def loop(request):
    solve, close = _open(request.param)
    cbs, res = _run(solve, callback_every=1)
    K = res[0]
    assert 8 * EVERY < K < 2000 and res[1] == 1 and res[2] in (1, 2)           # stopped by a criterion
    assert [c[0] for c in cbs] == _expected(K, 1)
    every_it = {c[0]: c for c in cbs[:-1]}
    every_it[K] = cbs[-1]
    yield solve, K, every_it, res
    close()


@pytest.mark.parametrize("every,sync_every", [(EVERY, 5), (EVERY, 500), (0, 0)])
def test_callbacks_and_results_do_not_depend_on_the_chunks(loop, every, sync_every):
    solve, K, every_it, res1 = loop
    cbs, res = _run(solve, callback_every=every, sync_every=sync_every)
    print(K, [c[0] for c in cbs], res)
    assert [c[0] for c in cbs] == _expected(K, every)
    assert cbs == [every_it[c[0]] for c in cbs]                                 # the same bits as with callback_every = 1
    assert res == res1


@pytest.mark.parametrize("sync_every", [5, 500])
def test_callback_at_the_iteration_cap_is_delivered_in_the_loop_and_as_the_final_one(loop, sync_every):
    solve, K, every_it, _ = loop
    cap = (K - 1) // EVERY * EVERY
    cbs, res = _run(solve, callback_every=EVERY, sync_every=sync_every, max_iterations=cap)
    print(K, cap, [c[0] for c in cbs], res)
    assert [c[0] for c in cbs] == _expected(cap, EVERY, last_in_loop=True)
    assert cbs == [every_it[c[0]] for c in cbs]
    assert res[:3] == (cap, 0, 0)                                               # ITERATIONS, not converged
    assert res[3:6] == every_it[cap][2:3] + every_it[cap][1:2] + every_it[cap][3:4]


@pytest.mark.parametrize("path", ["plain", "team"])
def test_stop_requested_from_the_callback_at_iteration_7(path):
    """The chunks land on the cadence, so the request raised in the it = 7 callback is seen before iteration 8 is queued."""
    solve, close = _open(path)
    cbs, res = _run(solve, stop_at=EVERY, callback_every=EVERY)
    print([c[0] for c in cbs], res)
    assert res[:3] == (EVERY, 0, INTERRUPTED)
    assert [c[0] for c in cbs] == [0, 1, EVERY, EVERY]
    assert cbs[-1] == cbs[-2]
    close()
