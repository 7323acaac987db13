"""The boundary of the two CG launches: every wave starts from a ready-made start record (its item sequence and
the addressing of its first item, csrc/item_table.h) and takes its later items through the item table; the new direction is stored
nontemporal and the residual write-through.  None of it may change a bit.  No old path is kept for comparison: as in
tests/test_gpu_launch_head.py every case is compared bit for bit with the default geometry of its size -- x, r, the norms, the
iteration counts and the callbacks, for both rules -- and the default geometry with the oracle whose inner products are evaluated
exactly (oracle.exact_dots)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("MI355CG_BLOCKS", "MI355CG_WAVES", "MI355CG_ITEM_ROWS", "MI355CG_XCD_CLASSES", "MI355CG_DYN_ROWS", "MI355CG_GRAPH", "MI355CG_DEPTH", "MI355CG_XFOLD")
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
    lay = s._handle.layout()
    b = s.get_rhs()
    sol = isa.MatrixFreeSolver(s, b, 1e-30, iters)
    x = sol.solve()
    out = {"grid": lay["grid_stencil"], "x": x, "r": s._handle.recursive_residual(),
           "rel2": (sol.getIterations(), sol.last_results.r_norm2, sol.last_results.initial_r_norm2)}
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
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["r"], b["r"]), what
    assert np.array_equal(a["xm"], b["xm"]) and np.array_equal(a["rm"], b["rm"]), what


_default = {}


def default_run(n):
    """The default geometry of a size, once."""
    if n not in _default:
        _default[n] = _run(n, {})
    return _default[n]


@pytest.mark.parametrize("n", [6, 66, 258, 1026])
def test_default_geometry_equals_the_oracle_with_exact_inner_products(n):
    from oracle import oracle
    got = default_run(n)
    og = oracle.OracleGrid(n, n)
    with oracle.exact_dots():
        mf = og.mf_solve(eps=1e-30, max_iterations=ITERS)
        ms = og.msg_solve(max_iterations=ITERS, **MSG_EPS)
    assert got["rel2"] == (mf.iterations, mf.r_norm, mf.initial_r_norm)
    assert mf.iterations == (ITERS if n > 6 else 28)          # N = 6 has 16 unknowns: CG is through after 28 iterations, on both sides
    assert np.array_equal(got["x"], mf.x)
    assert got["msg"] == (ms.iterations, ms.stop_reason, ms.final_residual_norm, ms.final_precision, ms.final_error_norm, ms.r_norm2, ms.initial_r_norm2)
    assert np.array_equal(got["xm"], ms.x) and np.array_equal(got["rm"], ms.r)


def test_sixteen_unknowns_almost_every_wave_idle():
    """N = 6: two items on one workgroup, so two of its four waves start from a record that says "no item"."""
    got = default_run(6)
    assert got["grid"] == 1
    _same(_run(6, {"MI355CG_BLOCKS": "1"}), got, "N = 6, one workgroup")


@pytest.mark.parametrize("blocks", ["1", "2"])
def test_first_item_from_the_record_the_rest_from_the_table(blocks):
    """N = 66 on one and two workgroups: held at 2 rows per item every wave has several items, and only the first is in its record;
    as the plan comes (one taller item per wave) the record is all a wave reads."""
    n = 66
    for env in ({"MI355CG_BLOCKS": blocks}, {"MI355CG_BLOCKS": blocks, "MI355CG_ITEM_ROWS": "2"}):
        got = _run(n, env)
        assert got["grid"] == int(blocks), (env, got["grid"])
        _same(got, default_run(n), (n, env))


def test_xcd_classes_that_the_waves_of_a_class_do_not_divide():
    n = 258
    got = _run(n, {"MI355CG_BLOCKS": "16"})
    assert got["grid"] == 16
    _same(got, default_run(n), "N = 258 on 16 workgroups")


def test_queued_items_start_on_the_static_first_item():
    """The queued instantiations: every wave starts on the item of its record, then takes tickets."""
    n = 258
    got = _run(n, {"MI355CG_BLOCKS": "16", "MI355CG_DYN_ROWS": "4"})
    assert got["grid"] == 16
    _same(got, default_run(n), "queued against the default geometry")


def test_three_row_items_in_both_blocks_and_on_the_corner_row():
    n = 1026
    got = _run(n, {"MI355CG_ITEM_ROWS": "3"})
    assert got["grid"] == 512
    _same(got, default_run(n), "N = 1026 in 3-row items")


def _rel2_fixed(n, env, k):
    """REL_2NORM for exactly k iterations on a handle created under `env`."""
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    with _Env(env):
        s = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
    p = isa.default_params(_capi.RULE_REL_2NORM)
    p.max_iterations, p.fixed_iterations, p.use_true_solution, p.callback_every, p.sync_every = k, 1, 0, 0, 0
    res = s._handle.solve(p)
    out = (s._handle.layout()["x_fold"], res.iterations, res.r_norm2, res.initial_r_norm2, res.stop_reason, s._handle.solution(), s._handle.recursive_residual())
    s._handle.close()
    return out


@pytest.mark.parametrize("n", [66, 258])
def test_the_lean_update_feeds_the_deferred_fold(n):
    """MI355CG_XFOLD=32 against MI355CG_XFOLD=0 for 70 iterations -- two folds and a pending tail: the update without an x step
    (its residual stored with the new policy) in front of k_fold_x, the bench's own pair of kernels."""
    fold, fused = _rel2_fixed(n, {"MI355CG_XFOLD": "32"}, 70), _rel2_fixed(n, {"MI355CG_XFOLD": "0"}, 70)
    assert fold[0] == 32 and fused[0] == 0
    assert fold[1:5] == fused[1:5] and fold[1] == 70
    assert np.array_equal(fold[5], fused[5]) and np.array_equal(fold[6], fused[6])


def test_a_local_team_of_two_row_slabs():
    """The TEAM instantiations against the single context in its default geometry: parts whose storage does not start at row 0
    get records of their own."""
    import iterative_solvers_amd as isa
    from iterative_solvers_amd.distributed import Team
    n = 66
    for rule, kw in ((1, dict(eps_rel=1e-30, max_iterations=ITERS)), (0, dict(max_iterations=ITERS, callback_every=7, **MSG_EPS))):
        s = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
        t = Team.local(n, 2, 0)
        p1, pt = isa.default_params(rule), isa.default_params(rule)
        for k, v in kw.items():
            setattr(p1, k, v)
            setattr(pt, k, v)
        c1, ct = [], []
        r1 = s._handle.solve(p1, callback=(lambda *a: c1.append(a)) if rule == 0 else None)
        rt = t.solve(pt, callback=(lambda *a: ct.append(a)) if rule == 0 else None)
        assert (rt.iterations, rt.converged, rt.stop_reason) == (r1.iterations, r1.converged, r1.stop_reason) and r1.iterations == ITERS
        assert (rt.r_norm2, rt.initial_r_norm2) == (r1.r_norm2, r1.initial_r_norm2)
        assert (rt.final_residual_norm, rt.final_precision, rt.final_error_norm) == (r1.final_residual_norm, r1.final_precision, r1.final_error_norm)
        assert ct == c1 and (rule == 1 or len(c1) >= 5)
        assert np.array_equal(t.vector(0), s._handle.solution()) and np.array_equal(t.vector(1), s._handle.recursive_residual())
        t.close()
        s._handle.close()


@pytest.mark.parametrize("n", [66, 514])
def test_fp32_mixed_equals_the_cpu_statement(n):
    """The fp32 kernels: 256-column strips, records with 4-byte offsets."""
    import iterative_solvers_amd as isa
    from oracle.oracle import OracleGrid
    og = OracleGrid(n, n)
    b = og.rhs()
    s = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0, dtype=isa.F32_MIXED)
    sol = isa.MatrixFreeSolver(s, b, 1e-8, 10 ** 6)
    x = sol.solve()
    r = sol.last_results
    xo, its, outer, conv, rel = og.mixed_solve(b, eps=1e-8)
    assert (r.iterations, r.refine_outer, bool(r.converged)) == (its, outer, conv)
    assert np.array_equal(x, xo)
    s._handle.close()
