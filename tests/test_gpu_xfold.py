"""Deferred x fold: with a ring of R = 16 or 32 direction buffers no update launch touches x; one flat launch
(k_fold_x) applies the last R steps every R-th iteration and the pending it % R steps at the end of the solve.  Same roundings in
the same order as the fused update, so every comparison here is bit for bit.  The reference is always a second handle created with
MI355CG_XFOLD=0 -- the fused update, which test_gpu_parity.py / test_gpu_variants.py pin to the oracle."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _handle(n, env):
    """A MatrixFreeSystem created under `env` (the knobs are read at mi355cg_create)."""
    import iterative_solvers_amd as isa
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _params(k, sync_every=0, fixed=True, eps=None):
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    p = isa.default_params(_capi.RULE_REL_2NORM)
    p.max_iterations, p.fixed_iterations, p.use_true_solution, p.callback_every, p.sync_every = k, 1 if fixed else 0, 0, 0, sync_every
    if eps is not None:
        p.eps_rel = eps
    return p


def _run(s, p, stop=None):
    h = s._handle
    res = h.solve(p, None, stop)
    return res, h.solution(), h.recursive_residual()


def _same(got, ref, what):
    (res, x, r), (res0, x0, r0) = got, ref
    assert res.iterations == res0.iterations, what
    assert res.r_norm2 == res0.r_norm2, what
    assert res.stop_reason == res0.stop_reason, what
    assert np.array_equal(r, r0), what
    assert np.array_equal(x, x0), what


_REF = {}          # (n, K) -> result of the fused update, computed once


def _ref_fixed(n, k):
    if (n, k) not in _REF:
        s = _REF.get(("handle", n))
        if s is None:
            s = _REF[("handle", n)] = _handle(n, {"MI355CG_XFOLD": "0"})
            assert s._handle.layout()["x_fold"] == 0
        _REF[(n, k)] = _run(s, _params(k))
    return _REF[(n, k)]


@pytest.mark.parametrize("sync_every", [7, 200])
@pytest.mark.parametrize("graph", ["0", "1"])
@pytest.mark.parametrize("R", [16, 32])
@pytest.mark.parametrize("n", [66, 130, 258])
def test_fixed_counts_around_the_fold_depth(n, R, graph, sync_every):
    """K = 1, R - 1, R, R + 1, 2R, 2R + 3: flushes with 0, 1 and R - 1 pending steps, a fold on a chunk's last iteration
    (sync_every = 200: the chunk is the solve) and in mid-chunk, chunks of 7 that never end on a fold, replayed as graphs or not."""
    s = _handle(n, {"MI355CG_XFOLD": str(R), "MI355CG_GRAPH": graph})
    assert s._handle.layout()["x_fold"] == R
    for k in (1, R - 1, R, R + 1, 2 * R, 2 * R + 3):
        _same(_run(s, _params(k, sync_every)), _ref_fixed(n, k), (n, R, graph, sync_every, k))
    lay = s._handle.layout()
    assert (lay["x_fold"], lay["x_fold_buffers"]) == (R, R - 4)
    s._handle.close()


@pytest.mark.parametrize("R", [16, 32])
def test_converged_solve(R):
    n = 258
    p = _params(10000, fixed=False, eps=1e-10)
    ref = _run(_handle(n, {"MI355CG_XFOLD": "0"}), p)
    assert ref[0].converged and 300 < ref[0].iterations < 2000, ref[0].iterations
    got = _run(_handle(n, {"MI355CG_XFOLD": str(R)}), p)
    assert got[0].converged
    _same(got, ref, R)


@pytest.mark.parametrize("R", [16, 32])
def test_ring_and_step_lengths_start_clean(R):
    """Two solves in a row on one handle with different K, then another right-hand side and a third."""
    n = 130
    f, z = _handle(n, {"MI355CG_XFOLD": str(R)}), _handle(n, {"MI355CG_XFOLD": "0"})
    for k in (2 * R + 3, R - 1):
        _same(_run(f, _params(k)), _run(z, _params(k)), (R, k))
    b = np.random.default_rng(20261017).standard_normal(f._handle.size)
    f._handle.set_rhs(b)
    z._handle.set_rhs(b)
    _same(_run(f, _params(R + 5)), _run(z, _params(R + 5)), (R, "new rhs"))


@pytest.mark.parametrize("R", [16, 32])
def test_stop_request_leaves_the_pending_steps_to_the_flush(R):
    """A stop flag raised from another thread in the middle of a chunk: the launches queued behind the stop decision, folds included,
    are no-ops, and x is the fused update's x after exactly res.iterations iterations."""
    import iterative_solvers_amd as isa
    n = 514
    f = _handle(n, {"MI355CG_XFOLD": str(R)})
    _run(f, _params(50))                                                  # warm-up: the ring is allocated
    stop = C.c_int(0)
    th = threading.Timer(0.05, lambda: stop.__setattr__("value", 1))
    th.start()
    got = _run(f, _params(10 ** 7, sync_every=500), stop)
    th.join()
    assert got[0].stop_reason == isa.StopCriterion.INTERRUPTED and not got[0].converged
    k = got[0].iterations
    assert 1 <= k < 10 ** 7
    ref = _run(_handle(n, {"MI355CG_XFOLD": "0"}), _params(k))
    assert ref[0].iterations == k and ref[0].r_norm2 == got[0].r_norm2
    assert np.array_equal(got[2], ref[2])
    assert np.array_equal(got[1], ref[1]), (k, k % R)


def test_a_solve_stopped_before_its_first_iteration_applies_no_steps_of_the_one_before():
    """The flag is already up when the solve starts: no iteration runs and x = 0, whatever the previous solve on the handle left in
    the ring, the step lengths and the summary."""
    import iterative_solvers_amd as isa
    f = _handle(130, {"MI355CG_XFOLD": "16"})
    res = _run(f, _params(21))[0]
    assert res.iterations == 21
    res, x, r = _run(f, _params(50), C.c_int(1))
    assert res.iterations == 0 and res.stop_reason == isa.StopCriterion.INTERRUPTED
    assert not x.any()
    assert np.array_equal(r, f._handle.rhs())


def test_msg_and_diagnostics_solves_keep_their_launches_and_allocate_no_ring():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    n = 130
    f, z = _handle(n, {"MI355CG_XFOLD": "32"}), _handle(n, {"MI355CG_XFOLD": "0"})
    pm = isa.default_params(_capi.RULE_MSG_MAXNORM)
    pm.max_iterations, pm.eps_precision, pm.eps_residual = 6000, 1e-9, 1e-9
    pd = _params(40)
    pd.diagnostics, pd.use_true_solution = 1, 1
    for p in (pm, pd):
        got, ref = _run(f, p), _run(z, p)
        assert ref[0].iterations > 32
        _same(got, ref, p.rule)
        assert got[0].final_error_norm == ref[0].final_error_norm and got[0].final_precision == ref[0].final_precision
    lay = f._handle.layout()
    assert (lay["x_fold"], lay["x_fold_buffers"]) == (32, 0)


def test_layout_reports_the_depth_in_use():
    assert _handle(64, {})._handle.layout()["x_fold"] == 0               # default: small grids keep the fused update
    for R in (16, 32):
        assert _handle(64, {"MI355CG_XFOLD": str(R)})._handle.layout()["x_fold"] == R
    assert _handle(64, {"MI355CG_XFOLD": "32", "MI355CG_XSTEPS": "4"})._handle.layout()["x_fold"] == 0    # an explicit XSTEPS keeps its meaning


def test_the_fold_is_faster_than_the_fused_update_at_n4096():
    """One default handle (the fold, depth 32) and one MI355CG_XFOLD=0 handle; a warm-up, then three alternating pairs of 500 fixed
    iterations.  The median loop time of the fold must be below the fused one's -- no margin."""
    n = 4096
    f, z = _handle(n, {}), _handle(n, {"MI355CG_XFOLD": "0"})
    assert f._handle.layout()["x_fold"] == 32 and z._handle.layout()["x_fold"] == 0
    p = _params(500, sync_every=500)
    tf, tz = [], []
    for s in (f, z):
        s._handle.solve(p)
    for _ in range(3):
        tf.append(f._handle.solve(p).loop_seconds)
        tz.append(z._handle.solve(p).loop_seconds)
    print(f"fold {sorted(tf)} fused {sorted(tz)} ratio of medians {sorted(tz)[1] / sorted(tf)[1]:.4f}")
    assert f._handle.layout()["x_fold_buffers"] == 28
    assert sorted(tf)[1] < sorted(tz)[1], (tf, tz)
