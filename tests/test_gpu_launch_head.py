"""The head of the two CG launches: item tables in place of the by-value panel list, the small loads of
the prologue issued before the rows, and instantiations without the team and queue paths for single-context launches.  None of
it may change a bit: every case here is compared with the default geometry of its size, and that with the oracle whose inner
products are evaluated exactly (oracle.exact_dots), the way tests/test_gpu_parity.py compares.

Partial counts: thread t of a consumer launch reduces the producer's partials t and t + 256 from two prefetched pairs, so the
counts 1, 2, 8, 255, 256, 257, 511 and 512 are where that can go wrong.  MI355CG_BLOCKS / MI355CG_WAVES / MI355CG_ITEM_ROWS reach
1, 2, 8, 256, 511 and 512; with XCD classes on a grid is a multiple of 8, and at N = 1026 the classes are on whenever fewer than
449 workgroups are allowed, so 255 and 257 also need MI355CG_XCD_CLASSES=0 (worked out with mi355cg_debug_plan)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("MI355CG_BLOCKS", "MI355CG_WAVES", "MI355CG_ITEM_ROWS", "MI355CG_XCD_CLASSES", "MI355CG_DYN_ROWS", "MI355CG_GRAPH", "MI355CG_DEPTH")
ITERS = 40
MSG_EPS = dict(eps_precision=1e-300, eps_residual=1e-300, eps_exact_error=1e-300)      # never met: the iteration cap ends the solve


class _Env:
    """The launch-geometry knobs are read when a context is created."""
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in KNOBS}
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(n, env, iters=ITERS):
    """Both rules for `iters` iterations on one system created under `env`: everything a caller can see."""
    import iterative_solvers_amd as isa
    with _Env(env):
        s = isa.GridSystem(n, n, 1.0, 2.0, 1.0, 2.0)
    grid = s._handle.layout()["grid_stencil"]
    b = s.get_rhs()
    sol = isa.MatrixFreeSolver(s, b, 1e-30, iters)
    x = sol.solve()
    out = {"grid": grid, "x": x, "rel2": (sol.getIterations(), sol.last_results.r_norm2, sol.last_results.initial_r_norm2)}
    m = isa.MSGSolver(s, b, 1e-300, iters)
    m.setPrecisionEps(1e-300); m.setResidualEps(1e-300); m.setExactErrorEps(1e-300)
    cbs = []
    m.setIterationCallback(lambda *a: cbs.append(tuple(a)))
    out["xm"] = m.solve(s.get_true_solution_vector(), callback_every=7)
    out["rm"] = s._handle.recursive_residual()
    out["msg"] = (m.getIterations(), int(m.getStopReason()), m.getFinalResidualNorm(), m.getFinalPrecision(), m.getFinalErrorNorm(),
                  m.last_results.r_norm2, m.last_results.initial_r_norm2)
    out["cbs"] = cbs
    s._handle.close()
    return out


def _same(a, b, what):
    assert a["rel2"] == b["rel2"], what
    assert a["msg"] == b["msg"], what
    assert a["cbs"] == b["cbs"] and len(a["cbs"]) >= 2, what
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["xm"], b["xm"]) and np.array_equal(a["rm"], b["rm"]), what


_default = {}


def default_run(n):
    if n not in _default:
        _default[n] = _run(n, {})
    return _default[n]


_oracle = {}


def oracle_run(n):
    """The oracle with exact inner products, once per size."""
    if n not in _oracle:
        from oracle import oracle
        og = oracle.OracleGrid(n, n)
        with oracle.exact_dots():
            mf = og.mf_solve(eps=1e-30, max_iterations=ITERS)
            ms = og.msg_solve(max_iterations=ITERS, **MSG_EPS)
        _oracle[n] = (mf, ms)
    return _oracle[n]


COUNTS = [
    (6, {}, 1), (6, {"MI355CG_ITEM_ROWS": "1"}, 2),
    (66, {"MI355CG_BLOCKS": "1"}, 1), (66, {"MI355CG_BLOCKS": "2"}, 2), (66, {"MI355CG_BLOCKS": "8", "MI355CG_ITEM_ROWS": "1"}, 8),
    (1026, {"MI355CG_BLOCKS": "8", "MI355CG_ITEM_ROWS": "4"}, 8),
    (1026, {"MI355CG_BLOCKS": "255", "MI355CG_ITEM_ROWS": "4", "MI355CG_XCD_CLASSES": "0"}, 255),
    (1026, {"MI355CG_BLOCKS": "256", "MI355CG_ITEM_ROWS": "4"}, 256),
    (1026, {"MI355CG_BLOCKS": "257", "MI355CG_ITEM_ROWS": "4", "MI355CG_XCD_CLASSES": "0"}, 257),
    (1026, {"MI355CG_BLOCKS": "511", "MI355CG_ITEM_ROWS": "3"}, 511),
    (1026, {"MI355CG_ITEM_ROWS": "3"}, 512),
]


@pytest.mark.parametrize("n,env,count", COUNTS)
def test_partial_count_boundaries(n, env, count):
    got = _run(n, env)
    assert got["grid"] == count, (env, got["grid"])
    _same(got, default_run(n), (n, env))


@pytest.mark.parametrize("n", [6, 66, 1026])
def test_default_geometry_equals_the_oracle_with_exact_inner_products(n):
    got = default_run(n)
    mf, ms = oracle_run(n)
    assert got["rel2"] == (mf.iterations, mf.r_norm, mf.initial_r_norm)
    assert mf.iterations == (ITERS if n > 6 else 28)          # N = 6 has 16 unknowns: CG is through (1e-30 of ||r0||) after 28 iterations, on both sides
    assert np.array_equal(got["x"], mf.x)
    assert got["msg"] == (ms.iterations, ms.stop_reason, ms.final_residual_norm, ms.final_precision, ms.final_error_norm, ms.r_norm2, ms.initial_r_norm2)
    assert np.array_equal(got["xm"], ms.x) and np.array_equal(got["rm"], ms.r)
    # the callbacks at the reference's own cadence (the runs above ask for every 7th iteration)
    import iterative_solvers_amd as isa
    s = isa.GridSystem(n, n, 1.0, 2.0, 1.0, 2.0)
    m = isa.MSGSolver(s, s.get_rhs(), 1e-300, ITERS)
    cbs = []
    m.setIterationCallback(lambda *a: cbs.append(tuple(a)))
    xm = m.solve(s.get_true_solution_vector())
    assert cbs == [tuple(c) for c in ms.callbacks] and len(cbs) >= 1
    assert np.array_equal(xm, ms.x)
    assert got["cbs"][0] == cbs[0]                                            # iteration 1 is on both cadences
    s._handle.close()


def _params(isa, rule, **kw):
    p = isa.default_params(rule)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("n", [66, 258])
@pytest.mark.parametrize("env", [{"MI355CG_BLOCKS": "2"}, {"MI355CG_BLOCKS": "8"}])
@pytest.mark.parametrize("world", [1, 2])
def test_single_context_equals_a_local_team(n, env, world):
    """The single context runs the instantiations without the team path, a LOCAL team (of one part: records gathered from a mailbox
    that holds nobody else's; of two row slabs) the ones with it."""
    import iterative_solvers_amd as isa
    from iterative_solvers_amd.distributed import Team
    for rule, kw in ((1, dict(eps_rel=1e-30, max_iterations=ITERS)), (0, dict(max_iterations=ITERS, callback_every=7, **MSG_EPS))):
        with _Env(env):
            s = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
            t = Team.local(n, world, 0)
        c1, ct = [], []
        r1 = s._handle.solve(_params(isa, rule, **kw), callback=(lambda *a: c1.append(a)) if rule == 0 else None)
        rt = t.solve(_params(isa, rule, **kw), callback=(lambda *a: ct.append(a)) if rule == 0 else None)
        assert (rt.iterations, rt.converged, rt.stop_reason) == (r1.iterations, r1.converged, r1.stop_reason) and r1.iterations == ITERS
        assert (rt.r_norm2, rt.initial_r_norm2) == (r1.r_norm2, r1.initial_r_norm2)
        assert (rt.final_residual_norm, rt.final_precision, rt.final_error_norm) == (r1.final_residual_norm, r1.final_precision, r1.final_error_norm)
        assert ct == c1 and (rule == 1 or len(c1) >= 5)
        assert np.array_equal(t.vector(0), s._handle.solution()) and np.array_equal(t.vector(1), s._handle.recursive_residual())
        t.close()
        s._handle.close()


def test_queued_items_equal_the_static_deal():
    """N = 258 with 16 workgroups has XCD classes and 162 four-row items: dealt through the run-time queues or statically."""
    n = 258
    queued = _run(n, {"MI355CG_BLOCKS": "16", "MI355CG_DYN_ROWS": "4"})
    static = _run(n, {"MI355CG_BLOCKS": "16", "MI355CG_ITEM_ROWS": "4", "MI355CG_DYN_ROWS": "0"})
    assert queued["grid"] == static["grid"] == 16
    _same(queued, static, "queued against static")
    _same(queued, default_run(n), "queued against the default geometry")


def test_a_solve_that_stops_in_mid_chunk():
    """To 1e-8 at N = 66: with sync_every = 200 the launches behind the stop have requested their rows before they learn that
    the solve is over; with sync_every = 1 there are none."""
    import iterative_solvers_amd as isa
    runs = []
    for sync in (200, 1):
        s = isa.MatrixFreeSystem(66, 66, 1.0, 2.0, 1.0, 2.0)
        sol = isa.MatrixFreeSolver(s, s.get_rhs(), 1e-8, 10 ** 5)
        x = sol.solve(sync_every=sync)
        r = sol.last_results
        assert r.converged and 0 < r.iterations < 200
        runs.append((r.iterations, r.r_norm2, r.initial_r_norm2, x, s._handle.recursive_residual()))
        s._handle.close()
    a, b = runs
    assert a[:3] == b[:3] and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


def test_graph_replay_two_solves_in_a_row():
    import iterative_solvers_amd as isa
    runs = []
    for graph in ("1", "0"):
        with _Env({"MI355CG_GRAPH": graph}):
            s = isa.MatrixFreeSystem(66, 66, 1.0, 2.0, 1.0, 2.0)
        got = []
        for _ in range(2):
            sol = isa.MatrixFreeSolver(s, s.get_rhs(), 1e-8, 10 ** 5)
            x = sol.solve()
            r = sol.last_results
            got.append((r.iterations, r.converged, r.r_norm2, r.initial_r_norm2, x))
        runs.append(got)
        s._handle.close()
    for a, b in list(zip(runs[0], runs[1])) + [(runs[0][0], runs[0][1])]:
        assert a[:4] == b[:4] and a[1] and np.array_equal(a[4], b[4])


@pytest.mark.parametrize("env", [{}, {"MI355CG_BLOCKS": "1"}])
def test_fp32_mixed_equals_the_cpu_statement(env):
    import iterative_solvers_amd as isa
    from oracle.oracle import OracleGrid
    n = 66
    og = OracleGrid(n, n)
    b = og.rhs()
    with _Env(env):
        s = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0, dtype=isa.F32_MIXED)
    sol = isa.MatrixFreeSolver(s, b, 1e-8, 10 ** 6)
    x = sol.solve()
    r = sol.last_results
    xo, its, outer, conv, rel = og.mixed_solve(b, eps=1e-8)
    assert (r.iterations, r.refine_outer, bool(r.converged)) == (its, outer, conv)
    assert np.array_equal(x, xo)
