"""On-chip ensemble time stepping: mi355cg_time_steps_many* integrates many members of one grid, one
workgroup per member with the step loop inside the launch.  Member s must get the bits of set_rhs(g_s); set_initial_guess(u0_s);
time_steps(params, tau_s, theta, nsteps) on a handle of the same grid.  The reference throughout is a SECOND handle of that grid in
the default two-launch mode running time_steps member by member: independent code from the kernel under test.  "Same" means
np.array_equal on u and == on steps_done, the iteration count of every step attempted and, for the last step attempted,
iterations, stop reason, converged, r_norm2, initial_r_norm2, final_precision and final_residual_norm.  sync_every = 7 unless said
otherwise, so that a launch holds several short steps of one member and cuts the long steps of another."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from onchip_support import DOMAIN, fields, params  # noqa: E402
from onchip_support import cap as _cap, system as _system  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [10, 12, 20, 30, 64, 100, "cap"]            # every workgroup size and unroll class of the plan (asserted below)
FACTORS = (1e6, 1e3, 10.0, 0.03)                    # sigma = |A_diag| * factor: 2 / 3 / 6 / 9 - 77 iterations per step in a NumPy model
REL = dict(eps_rel=1e-8, sync_every=7)
MSG = dict(eps_precision=1e-8, eps_residual=1e-8, eps_exact_error=0.0, sync_every=7)


_pairs = {}


def pair(n):
    """(the system the ensembles run on, the reference system in the default mode) of a grid, created once."""
    if n not in _pairs:
        _pairs[n] = (_system(n), _system(n))
        assert _pairs[n][1].solve_mode_info()["mode"] == 0
    return _pairs[n]


def rules():
    from iterative_solvers_amd import _capi
    return ((_capi.RULE_REL_2NORM, REL), (_capi.RULE_MSG_MAXNORM, MSG))


def diag_abs(sys_):
    """|A_diag| of the unshifted operator."""
    e = np.zeros(sys_.size())
    e[0] = 1.0
    return abs(float(sys_.apply(e)[0]))


def sequential(ref, p, u0, tau, theta, nsteps, g=None, stop_flag=None):
    """[(u, steps_done, [iterations of the steps attempted, then -1], fields of the last step attempted)] of time_steps member by
    member on the reference handle, which is left with the right-hand side and shift it had."""
    h = ref._handle
    old_shift, old_rhs = h.get_shift(), h.rhs()
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (len(u0),))
    out = []
    try:
        for s in range(len(u0)):
            if g is not None:
                h.set_rhs(g[s])
            h.set_initial_guess(u0[s])
            res, done = h.time_steps(p, float(tau[s]), theta, nsteps, stop_flag)
            its = [r.iterations for r in res] + [-1] * (nsteps - len(res))
            out.append((h.solution(), done, its, fields(res[-1])))
    finally:
        h.set_shift(old_shift)
        h.set_rhs(old_rhs)
    return out


def same(got, ref, what, pick=None):
    """Every member of an ensemble against the sequential results; prints the figures before it asserts."""
    u, res, done, its = got
    assert len(res) == len(u) == len(done) == len(its)
    for s in range(len(u)):
        us, ds, is_, fs = ref[s if pick is None else pick[s]]
        mine = (int(done[s]), [int(v) for v in its[s]], fields(res[s]))
        if mine != (ds, is_, fs) or not np.array_equal(u[s], us):
            print(what, "member", s, "ensemble", mine, "| sequential", (ds, is_, fs), "| max |du|", float(np.max(np.abs(u[s] - us))))
        assert mine == (ds, is_, fs), (what, s)
        assert np.array_equal(u[s], us), (what, s)
        assert res[s].final_error_norm == sys.float_info.max, (what, s)


def ensemble(sys_, seed, factors=FACTORS, theta=1.0):
    """(u0, tau, g) of one member per factor: g the system's right-hand side x (1 + 0.1 seeded noise), u0 zero for the first half
    of the members and seeded for the rest, tau_s such that 1 / (theta tau_s) = |A_diag| * factor_s up to rounding."""
    rng = np.random.default_rng(seed)
    k, size = len(factors), sys_.size()
    g = sys_.get_rhs()[None, :] * (1.0 + 0.1 * rng.standard_normal((k, size)))
    u0 = np.zeros((k, size))
    u0[(k + 1) // 2:] = rng.standard_normal((k - (k + 1) // 2, size))
    tau = 1.0 / (theta * diag_abs(sys_) * np.asarray(factors))
    return u0, tau, np.ascontiguousarray(g)


def test_the_sizes_below_cover_every_shape_of_the_plan():
    import iterative_solvers_amd as isa
    plans = [isa.onchip_plan(_cap() if n == "cap" else n) for n in SIZES]
    assert {p["threads"] for p in plans} == {64, 128, 256, 512}
    assert {p["elems_per_thread"] for p in plans} == {1, 2, 4, 8, 16, 24}
    assert _cap() == 128


@pytest.mark.parametrize("n", SIZES)
def test_parity_over_the_plan(n):
    n = _cap() if n == "cap" else n
    many, ref = pair(n)
    nsteps = 4
    for rule, kw in rules():
        for theta in (1.0, 0.5):
            p = params(rule, **kw)
            u0, tau, g = ensemble(many, seed=n, theta=theta)
            keep = (u0.copy(), g.copy())
            want = sequential(ref, p, u0, tau, theta, nsteps, g=g)
            counts = [w[2] for w in want]
            print(n, rule, theta, "iterations per step", counts)
            # from the reference's own counts: the cases this test is about occur
            assert all(w[1] == nsteps for w in want)
            assert any(c[k] + c[k + 1] + 2 <= 7 for c in counts for k in range(nsteps - 1)), counts     # two steps inside one launch
            assert any(v > 7 for c in counts for v in c), counts                                         # a step across launches
            assert len({tuple(c) for c in counts}) >= 2, counts
            got = many._handle.time_steps_many(p, u0, tau, theta, nsteps, g=g)
            same(got, want, (n, rule, theta))
            assert np.array_equal(u0, keep[0]) and np.array_equal(g, keep[1])
            assert all(r.converged == 1 for r in got[1])


@pytest.mark.parametrize("n,nsys,pool,nsteps,factors", [(10, 9000, 32, 2, None), ("cap", 300, 4, 1, (10.0,) * 4)])
def test_more_members_than_are_resident_at_once(n, nsys, pool, nsteps, factors):
    """9000 single-wave workgroups are more than 256 CUs hold at once; 300 workgroups at the cap more than 256 CUs at one per CU."""
    from iterative_solvers_amd import _capi
    n = _cap() if n == "cap" else n
    many, ref = pair(n)
    if factors is None:
        factors = tuple(FACTORS[s % 4] * (1.0 + s // 4) for s in range(pool))
    u0, tau, g = ensemble(many, seed=50 + n, factors=factors)
    p = params(_capi.RULE_REL_2NORM, **REL)
    want = sequential(ref, p, u0, tau, 1.0, nsteps, g=g)
    pick = np.arange(nsys) % pool
    got = many._handle.time_steps_many(p, np.ascontiguousarray(u0[pick]), tau[pick], 1.0, nsteps, g=np.ascontiguousarray(g[pick]))
    assert len(got[1]) == nsys
    same(got, want, (n, nsys), pick=pick)
    assert all(int(d) == nsteps for d in got[2])


def test_zero_iteration_steps_cost_a_unit_each():
    """From the steady state every step meets the residual test at its start: 50 steps of 0 iterations, 7 transitions per launch."""
    from iterative_solvers_amd import _capi
    many, ref = pair(16)
    own = many.get_rhs()
    ref._handle.set_rhs(own)
    ref._handle.solve(params(_capi.RULE_REL_2NORM, eps_rel=1e-12), None, None)
    steady = ref._handle.solution()
    u0 = np.stack([steady, steady, steady])
    tau = 1.0 / (diag_abs(many) * np.array([10.0, 0.03, 1e3]))
    p = params(_capi.RULE_MSG_MAXNORM, eps_precision=0.0, eps_residual=1e-3, eps_exact_error=0.0, sync_every=7)
    for theta in (1.0, 0.5):
        want = sequential(ref, p, u0, tau / theta, theta, 50)
        got = many._handle.time_steps_many(p, u0, tau / theta, theta, 50)
        print("zero-iteration steps", theta, got[2], [fields(r) for r in got[1]])
        assert all(w[1] == 50 and w[2] == [0] * 50 for w in want)
        same(got, want, ("zero", theta))
        assert [int(d) for d in got[2]] == [50] * 3 and not got[3].any()
        assert all(r.iterations == 0 and r.converged == 1 for r in got[1])
        assert np.array_equal(got[0], u0)


def test_one_or_two_units_per_launch():
    """sync_every = 1: every step converges exactly when its launch's budget is used up, so every transition waits for the next
    launch; sync_every = 2: some do, some do not.  Against the reference at the file's sync_every = 7: the bits of u, steps_done,
    the count of every step, iterations and converged (final_residual_norm follows the poll schedule, by contract)."""
    many, ref = pair(10)
    nsteps = 3
    for rule, kw in rules():
        for theta in (0.5, 1.0):
            u0, tau, g = ensemble(many, seed=13, factors=(1e3, 10.0, 0.03), theta=theta)
            want = sequential(ref, params(rule, **kw), u0, tau, theta, nsteps, g=g)
            assert all(w[1] == nsteps for w in want) and len({tuple(w[2]) for w in want}) == 3, [w[2] for w in want]
            for units in (1, 2):
                u, res, done, its = many._handle.time_steps_many(params(rule, **dict(kw, sync_every=units)), u0, tau, theta, nsteps, g=g)
                for s, (us, ds, is_, fs) in enumerate(want):
                    mine = (int(done[s]), [int(v) for v in its[s]], res[s].iterations, res[s].converged)
                    print("units", units, rule, theta, "member", s, "ensemble", mine, "| sequential", (ds, is_, fs[0], fs[2]))
                    assert mine == (ds, is_, fs[0], fs[2]), (units, rule, theta, s)
                    assert np.array_equal(u[s], us), (units, rule, theta, s)


def test_the_iteration_cap_ends_a_member():
    from iterative_solvers_amd import _capi
    many, ref = pair(30)
    for rule, kw in rules():
        p = params(rule, **dict(kw, max_iterations=4))
        u0, tau, g = ensemble(many, seed=4)
        want = sequential(ref, p, u0, tau, 1.0, 4, g=g)
        got = many._handle.time_steps_many(p, u0, tau, 1.0, 4, g=g)
        print("cap", rule, [(w[1], w[2]) for w in want])
        same(got, want, ("cap", rule))
        done = [int(d) for d in got[2]]
        assert 4 in done and 0 in done                             # some members finish within the cap, the others end in their first step
        for s, d in enumerate(done):
            if d < 4:
                assert (got[1][s].iterations, got[1][s].stop_reason, got[1][s].converged) == (4, _capi.STOP_ITERATIONS, 0)
                assert [int(v) for v in got[3][s][d + 1:]] == [-1] * (3 - d)


def test_fixed_iterations():
    many, ref = pair(20)
    for rule, kw in rules():
        p = params(rule, **dict(kw, fixed_iterations=1, max_iterations=3))
        u0, tau, g = ensemble(many, seed=5)
        for theta in (1.0, 0.5):
            want = sequential(ref, p, u0, tau, theta, 3, g=g)
            got = many._handle.time_steps_many(p, u0, tau, theta, 3, g=g)
            print("fixed", rule, theta, [(w[1], w[2]) for w in want])
            same(got, want, ("fixed", rule, theta))
            assert all(int(v) in (3, -1) for v in got[3].ravel())


def test_stop_flag_set_before_the_call():
    from iterative_solvers_amd import _capi
    many, ref = pair(16)
    for rule, kw in rules():
        p = params(rule, **kw)
        u0, tau, g = ensemble(many, seed=6)
        u0 = u0 + 1.0                                               # no member starts at a state that meets a rule
        got = many._handle.time_steps_many(p, u0, tau, 1.0, 3, g=g, stop_flag=C.c_int(1))
        assert [int(d) for d in got[2]] == [0] * 4
        assert [(r.iterations, r.stop_reason, r.converged) for r in got[1]] == [(0, _capi.STOP_INTERRUPTED, 0)] * 4
        assert np.array_equal(got[0], u0)
        want = sequential(ref, p, u0, tau, 1.0, 3, g=g, stop_flag=C.c_int(1))
        assert [(w[1], w[3][:3]) for w in want] == [(0, (0, _capi.STOP_INTERRUPTED, 0))] * 4
        same(got, want, ("flag up", rule))
        # a flag that stays down: the handle's watched solve (which polls after its first iteration) is the reference
        again = many._handle.time_steps_many(p, u0, tau, 1.0, 3, g=g, stop_flag=C.c_int(0))
        same(again, sequential(ref, p, u0, tau, 1.0, 3, g=g, stop_flag=C.c_int(0)), ("flag down", rule))
        assert all(int(d) == 3 for d in again[2])


def test_one_call_of_four_steps_is_four_calls_of_one():
    many, _ = pair(20)
    for rule, kw in rules():
        p = params(rule, **kw)
        u0, tau, g = ensemble(many, seed=7, theta=0.5)
        whole = many._handle.time_steps_many(p, u0, tau, 0.5, 4, g=g)
        u = u0
        for k in range(4):
            u, res, done, its = many._handle.time_steps_many(p, u, tau, 0.5, 1, g=g)
            assert [int(d) for d in done] == [1] * 4
            assert [int(v) for v in its[:, 0]] == [int(v) for v in whole[3][:, k]]
        assert np.array_equal(u, whole[0]) and [fields(r) for r in res] == [fields(r) for r in whole[1]]


def test_g_none_is_the_handles_right_hand_side_for_all():
    from iterative_solvers_amd import _capi
    many, ref = pair(12)
    p = params(_capi.RULE_REL_2NORM, **REL)
    u0, tau, _ = ensemble(many, seed=8)
    tiled = np.ascontiguousarray(np.stack([many.get_rhs()] * 4))
    a = many._handle.time_steps_many(p, u0, tau, 0.5, 3)
    b = many._handle.time_steps_many(p, u0, tau, 0.5, 3, g=tiled)
    assert np.array_equal(a[0], b[0]) and [fields(r) for r in a[1]] == [fields(r) for r in b[1]]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    same(a, sequential(ref, p, u0, tau, 0.5, 3), "g = None")
    # the convenience method: a scalar tau for all
    u, res, done, its = many.time_steps_many(u0, float(tau[2]), theta=0.5, nsteps=2, eps=1e-8)
    want = sequential(ref, params(_capi.RULE_REL_2NORM, eps_rel=1e-8, max_iterations=10000), u0, float(tau[2]), 0.5, 2)
    same((u, res, done, its), want, "scalar tau")
    assert its.shape == (4, 2) and done.shape == (4,)


def test_device_tensors():
    import torch
    many, _ = pair(20)
    u0, tau, g = ensemble(many, seed=9)
    ud, gd = torch.from_numpy(u0).cuda(), torch.from_numpy(g).cuda()
    for rule, kw in rules():
        p = params(rule, **kw)
        for host, dev in ((dict(), dict()), (dict(g=g), dict(g=gd))):
            uh, rh, dh, ih = many._handle.time_steps_many(p, u0, tau, 0.5, 3, **host)
            ut, rt, dt, it = many._handle.time_steps_many(p, ud, tau, 0.5, 3, **dev)
            assert ut.is_cuda and ut.data_ptr() != ud.data_ptr() and np.array_equal(ut.cpu().numpy(), uh)
            assert [fields(r) for r in rt] == [fields(r) for r in rh] and np.array_equal(dt, dh) and np.array_equal(it, ih)
    assert np.array_equal(ud.cpu().numpy(), u0) and np.array_equal(gd.cpu().numpy(), g)
    p = params(rules()[0][0], **REL)
    ut = many.time_steps_many(ud, torch.from_numpy(tau), theta=0.5, nsteps=3, g=gd, params=p)[0]
    assert np.array_equal(ut.cpu().numpy(), many._handle.time_steps_many(p, u0, tau, 0.5, 3, g=g)[0])


@pytest.mark.parametrize("onchip", [False, True])
def test_the_handle_is_untouched(onchip):
    from iterative_solvers_amd import _capi
    s = _system(16, onchip)
    mode = s.solve_mode_info()["mode"]
    h = s._handle
    p = params(_capi.RULE_REL_2NORM, **REL)
    for shift in (0.0, 3.0):
        h.set_shift(shift)
        first = fields(h.solve(p, None, None))
        x, r, rhs = h.solution(), h.recursive_residual(), h.rhs()
        u0, tau, g = ensemble(s, seed=10)
        um = h.time_steps_many(params(_capi.RULE_MSG_MAXNORM, **MSG), u0 + 1.0, tau, 0.5, 3, g=g)[0]
        assert not np.array_equal(um[0], x)
        h.time_steps_many(p, u0, tau, 1.0, 2)                      # g = NULL reads the handle's right-hand side
        assert np.array_equal(h.solution(), x) and np.array_equal(h.recursive_residual(), r) and np.array_equal(h.rhs(), rhs)
        assert h.get_shift() == shift and s.solve_mode_info()["mode"] == mode
        assert fields(h.solve(p, None, None)) == first              # cold: the ensemble left no pending guess behind
        assert np.array_equal(h.solution(), x) and np.array_equal(h.recursive_residual(), r)
        assert s.solve_mode_info()["onchip_launches"] > 0 if onchip else s.solve_mode_info()["onchip_launches"] == 0
        # a pending guess survives the call: the next solve is the warm solve it would have been
        guess = np.random.default_rng(18).standard_normal(s.size())
        h.set_initial_guess(guess)
        warm = fields(h.solve(p, None, None))
        xw = h.solution()
        assert warm != first
        h.set_initial_guess(guess)
        h.time_steps_many(params(_capi.RULE_MSG_MAXNORM, **MSG), u0, tau, 1.0, 2, g=g)
        assert fields(h.solve(p, None, None)) == warm and np.array_equal(h.solution(), xw)
    h.close()


def test_refusals_leave_the_handle_usable():
    import iterative_solvers_amd as isa
    import torch
    from iterative_solvers_amd import _capi
    from oracle.oracle import OracleGrid
    lib = _capi.load()
    cap = _cap()
    good = _system(16)
    size = good.size()
    p = params(_capi.RULE_REL_2NORM, **REL)
    u0, tau, g = ensemble(good, seed=11, factors=(1e3, 10.0, 0.03))
    want = good._handle.time_steps_many(p, u0, tau, 0.5, 2, g=g)
    h = good._handle._h

    def still_good():
        got = good._handle.time_steps_many(p, u0, tau, 0.5, 2, g=g)
        assert np.array_equal(got[0], want[0]) and [fields(r) for r in got[1]] == [fields(r) for r in want[1]]
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])

    def call(handle, prm, nsys, nsteps, theta, tt, gg, uu, out="res", done="done", its=None, fn=lib.mi355cg_time_steps_many):
        ptr = lambda v: (v.data_ptr() if hasattr(v, "data_ptr") else v.ctypes.data) if v is not None else None
        res = (_capi.Results * max(nsys, 1))() if out == "res" else None
        dn = np.full(max(nsys, 1), -7, dtype=np.int32) if done == "done" else None
        rc = fn(handle, C.byref(prm) if prm is not None else None, nsys, nsteps, theta, ptr(tt), ptr(gg), ptr(uu), None, res, ptr(dn), ptr(its))
        return rc, lib.mi355cg_last_error().decode(), dn

    def bad(**kw):
        q = params(_capi.RULE_REL_2NORM, **REL)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    u = u0.copy()
    both = np.zeros((6, size))
    counts = np.zeros(3 * 2, dtype=np.int32)
    t3 = lambda *v: np.array(v, dtype=np.float64)
    cases = [("null u", (h, p, 3, 2, 0.5, tau, g, None), {}, "null"), ("null params", (h, None, 3, 2, 0.5, tau, g, u), {}, "null"),
             ("null tau", (h, p, 3, 2, 0.5, None, g, u), {}, "null"), ("null out", (h, p, 3, 2, 0.5, tau, g, u), dict(out=None), "null"),
             ("null steps_done", (h, p, 3, 2, 0.5, tau, g, u), dict(done=None), "null"), ("null handle", (None, p, 3, 2, 0.5, tau, g, u), {}, "null"),
             ("no members", (h, p, 0, 2, 0.5, tau, g, u), {}, str(_capi.MANY_MAX)), ("too many", (h, p, _capi.MANY_MAX + 1, 2, 0.5, tau, g, u), {}, str(_capi.MANY_MAX)),
             ("negative nsteps", (h, p, 3, -1, 0.5, tau, g, u), {}, "nsteps"), ("too many steps", (h, p, 3, 65537, 0.5, tau, g, u), {}, "nsteps"),
             ("theta 0", (h, p, 3, 2, 0.0, tau, g, u), {}, "theta"),
             ("theta > 1", (h, p, 3, 2, 1.5, tau, g, u), {}, "theta"), ("theta nan", (h, p, 3, 2, float("nan"), tau, g, u), {}, "theta"),
             ("tau 0", (h, p, 3, 2, 0.5, t3(1.0, 0.0, 1.0), g, u), {}, "tau"), ("tau negative", (h, p, 3, 2, 0.5, t3(1.0, 1.0, -1.0), g, u), {}, "tau"),
             ("tau nan", (h, p, 3, 2, 0.5, t3(np.nan, 1.0, 1.0), g, u), {}, "tau"), ("tau inf", (h, p, 3, 2, 0.5, t3(1.0, np.inf, 1.0), g, u), {}, "tau"),
             ("1 / (theta tau) overflows", (h, p, 3, 2, 0.5, t3(1.0, 1.0, 1e-320), g, u), {}, "not finite"),
             ("u is g", (h, p, 3, 2, 0.5, tau, u, u), {}, "overlaps"), ("u overlaps g", (h, p, 3, 2, 0.5, tau, both[:3], both[1:4]), {}, "overlaps"),
             ("rule", (h, bad(rule=7), 3, 2, 0.5, tau, g, u), {}, "rule"), ("true solution", (h, bad(use_true_solution=1), 3, 2, 0.5, tau, g, u), {}, "use_true_solution"),
             ("diagnostics", (h, bad(diagnostics=1), 3, 2, 0.5, tau, g, u), {}, "diagnostics")]
    for what, args, kw, text in cases:
        rc, msg, dn = call(*args, **kw)
        assert rc == _capi.ERR_INVALID and text in msg, (what, rc, msg)
        assert dn is None or (dn == -7).all(), what                 # nothing was written
        still_good()
    assert np.array_equal(u, u0)
    # nsys * nsteps above 2^26 counts: refused with step_iterations only (the array is never touched)
    many_tau = np.full(1025, 1.0)
    rc, msg, _ = call(h, p, 1025, 65536, 0.5, many_tau, None, both, its=counts)
    assert rc == _capi.ERR_INVALID and "counts" in msg
    still_good()
    # the device entry point: the same checks
    ud, gd = torch.from_numpy(u0).cuda(), torch.from_numpy(g).cuda()
    torch.cuda.synchronize()
    dev = lib.mi355cg_time_steps_many_device
    for what, args, kw, text in [("u is g", (h, p, 3, 2, 0.5, tau, ud, ud), {}, "overlaps"), ("theta", (h, p, 3, 2, 2.0, tau, gd, ud), {}, "theta"),
                                 ("tau", (h, p, 3, 2, 0.5, t3(1.0, -2.0, 1.0), gd, ud), {}, "tau"), ("null out", (h, p, 3, 2, 0.5, tau, gd, ud), dict(out=None), "null"),
                                 ("diagnostics", (h, bad(diagnostics=1), 3, 2, 0.5, tau, gd, ud), {}, "diagnostics")]:
        rc, msg, dn = call(*args, fn=dev, **kw)
        assert rc == _capi.ERR_INVALID and text in msg, (what, rc, msg)
        still_good()
    assert np.array_equal(ud.cpu().numpy(), u0) and np.array_equal(gd.cpu().numpy(), g)
    with pytest.raises(ValueError):
        good._handle.time_steps_many(bad(diagnostics=1), u0, tau, 0.5, 2)
    with pytest.raises(ValueError):
        good._handle.time_steps_many(p, u0, tau[:2], 0.5, 2)
    with pytest.raises(ValueError):
        good._handle.time_steps_many(p, u0, tau, 0.5, 2, g=g[:2])
    still_good()
    # nsteps = 0: fine, writes only steps_done = 0
    rc, msg, dn = call(h, p, 3, 0, 0.5, tau, g, u)
    assert rc == _capi.OK and (dn == 0).all() and np.array_equal(u, u0)
    un, rn, dn, it = good._handle.time_steps_many(p, u0, tau, 0.5, 0)
    assert np.array_equal(un, u0) and not dn.any() and it.shape == (3, 0)

    # handles the on-chip mode refuses, with its message; a preconditioned handle is a matter of state
    big = _system(cap + 2)
    bb = np.ones((2, big.size()))
    rc, msg, _ = call(big._handle._h, p, 2, 1, 1.0, t3(1.0, 1.0), None, bb)
    assert rc == _capi.ERR_INVALID and str(cap) in msg and str(cap + 2) in msg
    with pytest.raises(ValueError):
        big.time_steps_many(bb, 1.0)
    big._handle.close()
    mixed = isa.MatrixFreeSystem(16, 16, *DOMAIN, dtype=isa.F32_MIXED)
    rc, msg, _ = call(mixed._handle._h, p, 3, 2, 0.5, tau, g, u)
    assert rc == _capi.ERR_INVALID and "F32_MIXED" in msg
    mixed._handle.close()
    csr = isa.CrsMatrix(*OracleGrid(8, 8).csr())
    cb = np.ones((2, csr._handle.size))
    rc, msg, _ = call(csr._handle._h, p, 2, 1, 1.0, t3(1.0, 1.0), None, cb)
    assert rc == _capi.ERR_INVALID and "CSR" in msg
    slab = C.c_void_p()
    assert lib.mi355cg_create_slab(16, 16, *DOMAIN, _capi.F64, 0, 1, 8, C.byref(slab)) == _capi.OK
    rc, msg, _ = call(slab, p, 3, 2, 0.5, tau, g, u)
    assert rc == _capi.ERR_INVALID and "part" in msg
    lib.mi355cg_destroy(slab)
    good.set_preconditioner(isa.PRECOND_MG_ANY)
    rc, msg, _ = call(h, p, 3, 2, 0.5, tau, g, u)
    assert rc == _capi.ERR_STATE and "preconditioner" in msg
    with pytest.raises(_capi.Mi355cgError):
        good._handle.time_steps_many(p, u0, tau, 0.5, 2)
    good.set_preconditioner(isa.PRECOND_NONE)
    still_good()
    good._handle.close()


def test_workspace_lifetime():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    _, ref = pair(12)
    fresh = _system(12)
    fresh.batch_release()                                            # nothing allocated: fine
    p = params(_capi.RULE_REL_2NORM, **REL)
    u0, tau, g = ensemble(fresh, seed=12, factors=tuple(FACTORS[s % 4] * (1.0 + s // 4) for s in range(40)))
    want = sequential(ref, p, u0, tau, 1.0, 3, g=g)
    same(fresh._handle.time_steps_many(p, u0[:2], tau[:2], 1.0, 3, g=g[:2]), want[:2], "two members")
    same(fresh._handle.time_steps_many(p, u0, tau, 1.0, 3, g=g), want, "forty members")           # grown
    same(fresh._handle.time_steps_many(p, u0[:2], tau[:2], 1.0, 3, g=g[:2]), want[:2], "two again")
    x, res = fresh._handle.solve_many(p, g[:5])                      # the batch solves share the workspace
    assert all(r.converged for r in res)
    same(fresh._handle.time_steps_many(p, u0[:7], tau[:7], 1.0, 3, g=g[:7]), want[:7], "after a batch")
    fresh.batch_release()
    fresh.batch_release()
    same(fresh._handle.time_steps_many(p, u0[:5], tau[:5], 1.0, 3, g=g[:5]), want[:5], "after the release")
    # the documented formula (the allocation itself is not exposed)
    size = fresh.size()
    assert isa.time_steps_many_workspace(12, 40, 3) == fresh.solve_many_info(40)["workspace_bytes"] + 16 * 40 + 8 * size + 4 * 40 * 3
    assert isa.time_steps_many_workspace(12, 40, 3, False) == 40 * (24 * size + 456) + 8 + 16 * 40 + 8 * size
    fresh._handle.close()


def test_cpp_host_steps_an_ensemble_through_the_compat_header():
    """MatrixFreeSystem::timeStepsMany of three members against time_steps on a handle here, bit for bit: the inputs are repeated
    operation by operation, the expected states go in as hex floats."""
    from iterative_solvers_amd import _capi
    from iterative_solvers_amd import build as b
    b.build()
    src = os.path.join(ROOT, "tests", "cpp", "onchip_steps_compat_driver.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "onchip_steps_compat_driver")
    headers = [os.path.join(ROOT, "iterative_solvers_amd", "compat", "mi355cg_compat.hpp"), os.path.join(ROOT, "include", "mi355cg.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src] + headers):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                               "-I", os.path.join(ROOT, "iterative_solvers_amd", "compat"), src,
                               "-L", os.path.join(ROOT, "iterative_solvers_amd"), "-lmi355cg",
                               "-Wl,-rpath," + os.path.join(ROOT, "iterative_solvers_amd"), "-o", exe])
    _, ref = pair(12)
    size, nsteps = ref.size(), 3
    i = np.arange(size)
    rhs = ref.get_rhs()
    g = np.stack([rhs * (1.0 + 0.25 * s * (((i * 37) % 101).astype(np.float64) / 101.0)) for s in range(3)])
    u0 = np.stack([0.01 * s * (((i * 11 + s) % 53).astype(np.float64) / 53.0 - 0.5) for s in range(3)])
    p = params(_capi.RULE_REL_2NORM, eps_rel=1e-9, max_iterations=10000, sync_every=7)
    want = sequential(ref, p, u0, [0.001, 0.0625, 0.5], 0.5, nsteps, g=g)
    args = []
    for us, done, its, _ in want:
        args += [str(done)] + [str(v) for v in its] + [float(v).hex() for v in us]
    env = {k: v for k, v in os.environ.items() if k != "MI355CG_ONCHIP"}
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2000:]
    members = json.loads(out.stdout)["members"]
    assert len(members) == 3
    for m, w in zip(members, want):
        assert m["same_bits"] is True and m["same_counts"] is True and m["steps_done"] == w[1] == nsteps and m["iterations"] == w[2]
    assert len({tuple(m["iterations"]) for m in members}) >= 2
