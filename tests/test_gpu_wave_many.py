"""On-chip ensemble wave-equation steps: mi355cg_wave_steps_many* integrates u_tt = A u - g for many members
of one grid, one workgroup per member.  "Same" means np.array_equal on u and v and == on counts and result fields.
Velocity Verlet is compared with the NumPy model of tests/wave_reference.py, which writes every expression operation by operation in
the kernel's order.  Newmark is compared with a SECOND handle of the grid in the default two-launch mode driven step by step: the
right-hand side built in NumPy by the documented expression, then set_shift, set_rhs, set_initial_guess, solve, get_solution, and
the velocity updated in NumPy."""
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
import wave_reference as W  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRETCHED = (0.0, 1.0, 0.0, 1.7)
SIZES = [6, 10, 12, 20, 30, 64, 100, "cap"]         # every workgroup size and unroll class of the plan (asserted below)
FRACTIONS = (1.0, 0.77, 0.5, 0.31, 0.13)            # Verlet: tau_s / bound, in (0.1, 1.0]
FACTORS = (1e3, 10.0, 0.03, 1e-3)                   # Newmark: sigma = |A_diag| * factor: 4 / 9 / 34 / 35 iterations per step at N = 10 in a NumPy model
REL = dict(eps_rel=1e-8, sync_every=7)
MSG = dict(eps_precision=1e-8, eps_residual=1e-8, eps_exact_error=0.0, sync_every=7)


def model(sys_):
    """The NumPy grid of a system, its coefficients read from the operator itself: A e_0 has the diagonal at unknown 0, xk at its
    right neighbour (unknown 1) and yk at the node above it (unknown N/2 - 1)."""
    e = np.zeros(sys_.size())
    e[0] = 1.0
    col = sys_.apply(e)
    g = W.Grid(sys_.n, col[0], col[1], col[sys_.n // 2 - 1])
    assert g.size == sys_.size() and g.A0 == -2 * (g.xk + g.yk)
    return g


_pairs = {}


def pair(n):
    """(the system the ensembles run on, the reference system in the default mode, the NumPy grid) of a grid, created once."""
    if n not in _pairs:
        _pairs[n] = (_system(n), _system(n))
        assert _pairs[n][1].solve_mode_info()["mode"] == 0
        _pairs[n] += (model(_pairs[n][0]),)
    return _pairs[n]


def rules():
    from iterative_solvers_amd import _capi
    return ((_capi.RULE_REL_2NORM, REL), (_capi.RULE_MSG_MAXNORM, MSG))


def verlet_ensemble(sys_, grid, seed, fractions=FRACTIONS):
    """(u0, v0, tau, g) of one member per fraction of the bound: g the right-hand side x (1 + 0.1 noise), u0 and v0 seeded, member 0
    at rest at zero."""
    rng = np.random.default_rng(seed)
    k, size = len(fractions), sys_.size()
    g = np.ascontiguousarray(sys_.get_rhs()[None, :] * (1.0 + 0.1 * rng.standard_normal((k, size))))
    u0, v0 = rng.standard_normal((k, size)), rng.standard_normal((k, size)) * np.sqrt(abs(grid.A0))
    u0[0] = v0[0] = 0.0
    return u0, v0, np.asarray(fractions) * grid.cfl(), g


def verlet_same(got, want, nsteps, what):
    u, v, res, done = got[:4]
    if not (np.array_equal(u, want[0]) and np.array_equal(v, want[1])):
        print(what, "max |du|", float(np.max(np.abs(u - want[0]))), "max |dv|", float(np.max(np.abs(v - want[1]))))
    assert np.array_equal(u, want[0]) and np.array_equal(v, want[1]), what
    assert [int(d) for d in done] == [nsteps] * len(u), what
    assert all((r.iterations, r.converged) == (0, 1) for r in res), what


def newmark_ensemble(sys_, grid, seed, factors=FACTORS):
    rng = np.random.default_rng(seed)
    k, size = len(factors), sys_.size()
    g = np.ascontiguousarray(sys_.get_rhs()[None, :] * (1.0 + 0.1 * rng.standard_normal((k, size))))
    u0, v0 = rng.standard_normal((k, size)), rng.standard_normal((k, size)) * np.sqrt(abs(grid.A0))
    u0[0] = v0[0] = 0.0
    tau = 2.0 / np.sqrt(abs(grid.A0) * np.asarray(factors))          # sigma = 4 / tau^2 = |A_diag| * factor up to rounding
    return u0, v0, tau, g


def newmark_sequential(ref, grid, p, u0, v0, tau, nsteps, g, stop_flag=None):
    """[(u, v, steps_done, [iterations of the steps attempted, then -1], fields of the last step attempted)] member by member on the
    reference handle, which is left with the right-hand side and shift it had."""
    h = ref._handle
    old_shift, old_rhs = h.get_shift(), h.rhs()
    tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (len(u0),))
    out = []
    try:
        for s in range(len(u0)):
            u, v, its, done, last = u0[s].copy(), v0[s].copy(), [], 0, None
            t = float(tau[s])
            for _ in range(nsteps):
                h.set_shift(4.0 / (t * t))
                h.set_rhs(W.newmark_rhs(grid, u, v, g[s], t))
                h.set_initial_guess(u)
                res = h.solve(p, None, stop_flag)
                its.append(res.iterations)
                last = fields(res)
                if not res.converged:
                    break
                x = h.solution()
                v = W.newmark_velocity(t, x, u, v)
                u = x
                done += 1
            out.append((u, v, done, its + [-1] * (nsteps - len(its)), last))
    finally:
        h.set_shift(old_shift)
        h.set_rhs(old_rhs)
    return out


def newmark_same(got, want, what):
    u, v, res, done, its = got
    for s in range(len(u)):
        us, vs, ds, is_, fs = want[s]
        mine = (int(done[s]), [int(x) for x in its[s]], fields(res[s]))
        if mine != (ds, is_, fs) or not np.array_equal(u[s], us) or not np.array_equal(v[s], vs):
            print(what, "member", s, "ensemble", mine, "| sequential", (ds, is_, fs), "| max |du|", float(np.max(np.abs(u[s] - us))),
                  "max |dv|", float(np.max(np.abs(v[s] - vs))))
        assert mine == (ds, is_, fs), (what, s)
        assert np.array_equal(u[s], us) and np.array_equal(v[s], vs), (what, s)
        assert res[s].final_error_norm == sys.float_info.max, (what, s)


def nm(many, p, u0, v0, tau, nsteps, **kw):
    from iterative_solvers_amd import _capi
    return many._handle.wave_steps_many(p, u0, v0, tau, nsteps, scheme=_capi.WAVE_NEWMARK, step_iterations=True, **kw)


def test_the_sizes_below_cover_every_shape_of_the_plan():
    import iterative_solvers_amd as isa
    plans = [isa.onchip_plan(_cap() if n == "cap" else n) for n in SIZES]
    assert {p["threads"] for p in plans} == {64, 128, 256, 512}
    assert {p["elems_per_thread"] for p in plans} == {1, 2, 4, 8, 16, 24}
    assert _cap() == 128


# ---- velocity Verlet against the NumPy model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_verlet_over_the_plan(n):
    """Five members with their own tau and g, 23 steps in launches of 7: launch cuts in mid-run and a short last launch."""
    n = _cap() if n == "cap" else n
    many, _, grid = pair(n)
    assert many.wave_cfl() == grid.cfl() == 2.0 / np.sqrt(2.0 * abs(grid.A0))
    u0, v0, tau, g = verlet_ensemble(many, grid, seed=n)
    got = many.wave_steps_many(u0, v0, tau, 23, g=g, steps_per_launch=7)
    verlet_same(got, W.verlet(grid, u0, v0, g, tau, 23), 23, ("plan", n))
    assert not np.array_equal(got[0], u0)


def test_verlet_on_a_stretched_domain():
    s = _system(20, domain=STRETCHED)
    grid = model(s)
    assert grid.xk != grid.yk
    u0, v0, tau, g = verlet_ensemble(s, grid, seed=21)
    verlet_same(s.wave_steps_many(u0, v0, tau, 23, g=g, steps_per_launch=7), W.verlet(grid, u0, v0, g, tau, 23), 23, "stretched")
    verlet_same(s.wave_steps_many(u0, v0, tau, 9, g=g), W.verlet(grid, u0, v0, g, tau, 9), 9, "stretched, one launch")
    s._handle.close()


def test_verlet_g_none_zero_steps_and_snapshots():
    many, _, grid = pair(12)
    u0, v0, tau, g = verlet_ensemble(many, grid, seed=22)
    # g = None: the handle's right-hand side for every member
    tiled = np.ascontiguousarray(np.stack([many.get_rhs()] * len(u0)))
    a = many.wave_steps_many(u0, v0, tau, 6, steps_per_launch=4)
    verlet_same(a, W.verlet(grid, u0, v0, tiled, tau, 6), 6, "g = None")
    b = many.wave_steps_many(u0, v0, tau, 6, g=tiled)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # a scalar tau for all
    verlet_same(many.wave_steps_many(u0, v0, float(tau[2]), 3, g=g), W.verlet(grid, u0, v0, g, float(tau[2]), 3), 3, "scalar tau")
    # nsteps = 0 writes only steps_done = 0
    u, v, res, done = many.wave_steps_many(u0, v0, tau, 0, g=g)
    assert np.array_equal(u, u0) and np.array_equal(v, v0) and not done.any()
    # one call of 4 steps equals 4 calls of 1
    whole = many.wave_steps_many(u0, v0, tau, 4, g=g)
    u, v = u0, v0
    for _ in range(4):
        u, v, res, done = many.wave_steps_many(u, v, tau, 1, g=g)
        assert [int(d) for d in done] == [1] * len(u0)
    assert np.array_equal(u, whole[0]) and np.array_equal(v, whole[1])


@pytest.mark.parametrize("n,nsys", [(10, 9000), ("cap", 300)])
def test_verlet_more_members_than_are_resident_at_once(n, nsys):
    n = _cap() if n == "cap" else n
    many, _, grid = pair(n)
    rng = np.random.default_rng(1000 + n)
    size = many.size()
    g = many.get_rhs()[None, :] * (1.0 + 0.1 * rng.standard_normal((nsys, 1)))
    u0, v0 = rng.standard_normal((nsys, size)), rng.standard_normal((nsys, size)) * np.sqrt(abs(grid.A0))
    tau = grid.cfl() * rng.uniform(0.1, 1.0, nsys)
    tau[-1] = grid.cfl()
    verlet_same(many.wave_steps_many(u0, v0, tau, 5, g=g, steps_per_launch=3), W.verlet(grid, u0, v0, g, tau, 5), 5, ("many", n, nsys))
    many.batch_release()


def test_verlet_device_tensors():
    import torch
    many, _, grid = pair(20)
    u0, v0, tau, g = verlet_ensemble(many, grid, seed=23)
    ud, vd, gd = (torch.from_numpy(a).cuda() for a in (u0, v0, g))
    want = W.verlet(grid, u0, v0, g, tau, 11)
    ut, vt, rt, dt = many.wave_steps_many(ud, vd, tau, 11, g=gd, steps_per_launch=4)
    assert ut.is_cuda and vt.is_cuda and ut.data_ptr() != ud.data_ptr() and vt.data_ptr() != vd.data_ptr()
    verlet_same((ut.cpu().numpy(), vt.cpu().numpy(), rt, dt), want, 11, "device")
    ut, vt, rt, dt = many.wave_steps_many(ud, vd, torch.from_numpy(tau), 11)
    tiled = np.ascontiguousarray(np.stack([many.get_rhs()] * len(u0)))
    verlet_same((ut.cpu().numpy(), vt.cpu().numpy(), rt, dt), W.verlet(grid, u0, v0, tiled, tau, 11), 11, "device, g = None")
    assert np.array_equal(ud.cpu().numpy(), u0) and np.array_equal(vd.cpu().numpy(), v0) and np.array_equal(gd.cpu().numpy(), g)


# ---- Newmark against a second handle in the default two-launch mode, driven step by step -------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_newmark_over_the_plan(n):
    n = _cap() if n == "cap" else n
    many, ref, grid = pair(n)
    for rule, kw in rules():
        p = params(rule, **kw)
        u0, v0, tau, g = newmark_ensemble(many, grid, seed=100 + n)
        want = newmark_sequential(ref, grid, p, u0, v0, tau, 4, g)
        print("newmark", n, rule, [(w[2], w[3]) for w in want])
        assert all(w[2] == 4 for w in want)
        newmark_same(nm(many, p, u0, v0, tau, 4, g=g), want, ("plan", n, rule))


def test_newmark_iteration_cap_fixed_iterations_and_snapshots():
    from iterative_solvers_amd import _capi
    many, ref, grid = pair(30)
    for rule, kw in rules():
        u0, v0, tau, g = newmark_ensemble(many, grid, seed=130)
        # an iteration cap ends a member early: its (u, v) are the reference's state after the last converged step
        p = params(rule, **dict(kw, max_iterations=6))
        want = newmark_sequential(ref, grid, p, u0, v0, tau, 4, g)
        got = nm(many, p, u0, v0, tau, 4, g=g)
        print("cap", rule, [(w[2], w[3]) for w in want])
        newmark_same(got, want, ("cap", rule))
        done = [int(d) for d in got[3]]
        assert 4 in done and min(done) < 4
        for s, d in enumerate(done):
            if d < 4:
                assert (got[2][s].iterations, got[2][s].stop_reason, got[2][s].converged) == (6, _capi.STOP_ITERATIONS, 0)
                assert [int(x) for x in got[4][s][d + 1:]] == [-1] * (3 - d)
        # fixed_iterations
        p = params(rule, **dict(kw, fixed_iterations=1, max_iterations=3))
        newmark_same(nm(many, p, u0, v0, tau, 3, g=g), newmark_sequential(ref, grid, p, u0, v0, tau, 3, g), ("fixed", rule))
        # one call of 4 steps equals 4 calls of 1; g = None
        p = params(rule, **kw)
        whole = nm(many, p, u0, v0, tau, 4)
        tiled = np.ascontiguousarray(np.stack([many.get_rhs()] * len(u0)))
        newmark_same(whole, newmark_sequential(ref, grid, p, u0, v0, tau, 4, tiled), ("g = None", rule))
        u, v = u0, v0
        for k in range(4):
            u, v, res, done, its = nm(many, p, u, v, tau, 1)
            assert [int(d) for d in done] == [1] * 4 and [int(x) for x in its[:, 0]] == [int(x) for x in whole[4][:, k]]
        assert np.array_equal(u, whole[0]) and np.array_equal(v, whole[1]) and [fields(r) for r in res] == [fields(r) for r in whole[2]]


def test_newmark_device_tensors_and_the_convenience_defaults():
    import torch
    from iterative_solvers_amd import _capi
    many, ref, grid = pair(20)
    u0, v0, tau, g = newmark_ensemble(many, grid, seed=120)
    ud, vd, gd = (torch.from_numpy(a).cuda() for a in (u0, v0, g))
    p = params(_capi.RULE_REL_2NORM, **REL)
    want = newmark_sequential(ref, grid, p, u0, v0, tau, 3, g)
    ut, vt, rt, dt, it = nm(many, p, ud, vd, tau, 3, g=gd)
    assert ut.is_cuda and vt.is_cuda and ut.data_ptr() != ud.data_ptr()
    newmark_same((ut.cpu().numpy(), vt.cpu().numpy(), rt, dt, it), want, "device")
    assert np.array_equal(ud.cpu().numpy(), u0) and np.array_equal(vd.cpu().numpy(), v0)
    # eps / rule of the convenience method, without the counts
    u, v, res, done = many.wave_steps_many(u0, v0, tau, 2, scheme=_capi.WAVE_NEWMARK, g=g, eps=1e-8)
    w2 = newmark_sequential(ref, grid, params(_capi.RULE_REL_2NORM, eps_rel=1e-8, max_iterations=10000), u0, v0, tau, 2, g)
    assert all(np.array_equal(u[s], w2[s][0]) and np.array_equal(v[s], w2[s][1]) and fields(res[s]) == w2[s][4] for s in range(4))


# ---- both schemes ------------------------------------------------------------------------------------------------------------------
def test_stop_flag():
    from iterative_solvers_amd import _capi
    many, ref, grid = pair(16)
    u0, v0, tau, g = verlet_ensemble(many, grid, seed=31)
    u, v, res, done = many.wave_steps_many(u0, v0, tau, 9, g=g, steps_per_launch=2, stop_flag=C.c_int(1))
    assert np.array_equal(u, u0) and np.array_equal(v, v0) and not done.any()
    assert [(r.iterations, r.stop_reason, r.converged) for r in res] == [(0, _capi.STOP_INTERRUPTED, 0)] * len(u0)
    verlet_same(many.wave_steps_many(u0, v0, tau, 9, g=g, steps_per_launch=2, stop_flag=C.c_int(0)), W.verlet(grid, u0, v0, g, tau, 9), 9, "flag down")
    for rule, kw in rules():
        p = params(rule, **kw)
        u0, v0, tau, g = newmark_ensemble(many, grid, seed=32)
        u0 = u0 + 1.0                                               # no member starts at a state that meets a rule
        got = nm(many, p, u0, v0, tau, 3, g=g, stop_flag=C.c_int(1))
        assert np.array_equal(got[0], u0) and np.array_equal(got[1], v0) and not got[3].any()
        assert [(r.iterations, r.stop_reason, r.converged) for r in got[2]] == [(0, _capi.STOP_INTERRUPTED, 0)] * 4
        newmark_same(got, newmark_sequential(ref, grid, p, u0, v0, tau, 3, g, stop_flag=C.c_int(1)), ("flag up", rule))
        again = nm(many, p, u0, v0, tau, 3, g=g, stop_flag=C.c_int(0))
        newmark_same(again, newmark_sequential(ref, grid, p, u0, v0, tau, 3, g, stop_flag=C.c_int(0)), ("flag down", rule))
        assert all(int(d) == 3 for d in again[3])


def test_newmark_flag_raised_in_mid_run_keeps_state_and_count_together():
    """A launch gives ONE unit (sync_every = 1), so every step converges exactly when its launch's budget is used up and its
    transition waits for the next launch.  A flag another thread raises while the call runs ends it between two launches -- inside
    a step or between two steps; wherever that is, (u, v) of every member must be the reference's state after exactly
    steps_done[s] steps, the counts of that many steps must be the reference's and the next one must be the step attempted or not
    taken.  A call that ended before the flag came satisfies the same statement with steps_done = nsteps."""
    import threading
    from iterative_solvers_amd import _capi
    many, ref, grid = pair(10)
    nsteps = 100
    p = params(_capi.RULE_REL_2NORM, eps_rel=1e-8, sync_every=1)
    u0, v0, tau, g = newmark_ensemble(many, grid, seed=71, factors=(10.0, 0.03, 1e-3))
    h = ref._handle
    old_shift, old_rhs = h.get_shift(), h.rhs()
    states, counts = [], []                                         # per member the reference's (u, v) after 0 .. nsteps steps, its iterations per step
    for s in range(len(u0)):
        u, v, t = u0[s].copy(), v0[s].copy(), float(tau[s])
        traj, cnt = [(u, v)], []
        for _ in range(nsteps):
            h.set_shift(4.0 / (t * t))
            h.set_rhs(W.newmark_rhs(grid, u, v, g[s], t))
            h.set_initial_guess(u)
            res = h.solve(p, None, None)
            assert res.converged == 1 and res.iterations >= 1
            cnt.append(res.iterations)
            x = h.solution()
            u, v = x, W.newmark_velocity(t, x, u, v)
            traj.append((u, v))
        states.append(traj)
        counts.append(cnt)
    h.set_shift(old_shift)
    h.set_rhs(old_rhs)
    seen, between = set(), 0
    for delay in (0.0005, 0.001, 0.002, 0.003, 0.005, 0.008, 0.012, 0.02):
        flag = C.c_int(0)
        timer = threading.Timer(delay, lambda: setattr(flag, "value", 1))
        timer.start()
        u, v, res, done, its = nm(many, p, u0, v0, tau, nsteps, g=g, stop_flag=flag)
        timer.cancel()
        timer.join()
        print("flag after", delay, "s: steps_done", [int(d) for d in done], "stop reasons", [r.stop_reason for r in res])
        for s in range(len(u0)):
            d = int(done[s])
            seen.add("whole" if d == nsteps else "stopped")
            assert np.array_equal(u[s], states[s][d][0]) and np.array_equal(v[s], states[s][d][1]), (delay, s, d)
            assert [int(k) for k in its[s][:d]] == counts[s][:d] and all(int(k) == -1 for k in its[s][d + 1:]), (delay, s, d)
            if d < nsteps:
                assert (res[s].stop_reason, res[s].converged) == (_capi.STOP_INTERRUPTED, 0) and -1 <= int(its[s][d]) < counts[s][d], (delay, s, d)
                between += int(its[s][d]) == -1 and d > 0                   # the next step was not begun: stopped between two steps
    print("calls ended:", sorted(seen), "| members stopped between two steps:", between)


@pytest.mark.parametrize("onchip", [False, True])
def test_the_handle_is_untouched(onchip):
    from iterative_solvers_amd import _capi
    s = _system(16, onchip)
    grid = model(s)
    mode = s.solve_mode_info()["mode"]
    h = s._handle
    p = params(_capi.RULE_REL_2NORM, **REL)
    for shift in (0.0, 3.0):
        h.set_shift(shift)
        first = fields(h.solve(p, None, None))
        x, r, rhs = h.solution(), h.recursive_residual(), h.rhs()
        u0, v0, tau, g = verlet_ensemble(s, grid, seed=41)
        verlet_same(s.wave_steps_many(u0, v0, tau, 5), W.verlet(grid, u0, v0, np.stack([rhs] * len(u0)), tau, 5), 5, "unshifted A, the handle's g")
        n0, n1, nt, ng = newmark_ensemble(s, grid, seed=42)
        nm(s, params(_capi.RULE_MSG_MAXNORM, **MSG), n0 + 1.0, n1, nt, 2, g=ng)
        nm(s, p, n0, n1, nt, 2)
        assert np.array_equal(h.solution(), x) and np.array_equal(h.recursive_residual(), r) and np.array_equal(h.rhs(), rhs)
        assert h.get_shift() == shift and s.solve_mode_info()["mode"] == mode
        assert fields(h.solve(p, None, None)) == first              # cold: the ensembles left no pending guess behind
        assert np.array_equal(h.solution(), x) and np.array_equal(h.recursive_residual(), r)
        guess = np.random.default_rng(18).standard_normal(s.size())
        h.set_initial_guess(guess)
        warm = fields(h.solve(p, None, None))
        xw = h.solution()
        h.set_initial_guess(guess)
        s.wave_steps_many(u0, v0, tau, 3, g=g)
        nm(s, p, n0, n1, nt, 1, g=ng)
        assert fields(h.solve(p, None, None)) == warm and np.array_equal(h.solution(), xw)
    h.close()


def test_refusals_leave_the_handle_usable():
    import iterative_solvers_amd as isa
    import torch
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    cap = _cap()
    good = _system(16)
    grid = model(good)
    size = good.size()
    p = params(_capi.RULE_REL_2NORM, **REL)
    V, N = _capi.WAVE_VERLET, _capi.WAVE_NEWMARK
    u0, v0, tau, g = verlet_ensemble(good, grid, seed=51, fractions=(1.0, 0.5, 0.2))
    want_v = W.verlet(grid, u0, v0, g, tau, 3)
    want_n = nm(good, p, u0, v0, 5.0 * tau, 2, g=g)
    h = good._handle._h

    def still_good():
        verlet_same(good.wave_steps_many(u0, v0, tau, 3, g=g, steps_per_launch=2), want_v, 3, "after a refusal")
        got = nm(good, p, u0, v0, 5.0 * tau, 2, g=g)
        assert np.array_equal(got[0], want_n[0]) and np.array_equal(got[1], want_n[1]) and np.array_equal(got[4], want_n[4])

    def call(handle, prm, nsys, nsteps, scheme, tt, gg, uu, vv, spl=0, out="res", done="done", its=None, fn=lib.mi355cg_wave_steps_many):
        ptr = lambda a: (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) if a is not None else None
        res = (_capi.Results * max(nsys, 1))() if out == "res" else None
        dn = np.full(max(nsys, 1), -7, dtype=np.int32) if done == "done" else None
        rc = fn(handle, C.byref(prm) if prm is not None else None, nsys, nsteps, scheme, ptr(tt), ptr(gg), ptr(uu), ptr(vv), spl, None, res, ptr(dn), ptr(its))
        return rc, lib.mi355cg_last_error().decode(), dn

    def bad(**kw):
        q = params(_capi.RULE_REL_2NORM, **REL)
        for k, val in kw.items():
            setattr(q, k, val)
        return q

    u, v = u0.copy(), v0.copy()
    both = np.zeros((6, size))
    t3 = lambda *a: np.array(a, dtype=np.float64)
    bound = good.wave_cfl()
    above = np.nextafter(bound, np.inf)
    cases = [("null u", (h, p, 3, 2, V, tau, g, None, v), {}, "null"), ("null v", (h, p, 3, 2, V, tau, g, u, None), {}, "null"),
             ("null tau", (h, p, 3, 2, V, None, g, u, v), {}, "null"), ("null out", (h, p, 3, 2, V, tau, g, u, v), dict(out=None), "null"),
             ("null steps_done", (h, p, 3, 2, V, tau, g, u, v), dict(done=None), "null"), ("null handle", (None, p, 3, 2, V, tau, g, u, v), {}, "null"),
             ("Newmark without params", (h, None, 3, 2, N, tau, g, u, v), {}, "params"),
             ("scheme 2", (h, p, 3, 2, 2, tau, g, u, v), {}, "scheme"), ("scheme -1", (h, p, 3, 2, -1, tau, g, u, v), {}, "scheme"),
             ("no members", (h, p, 0, 2, V, tau, g, u, v), {}, str(_capi.MANY_MAX)), ("too many", (h, p, _capi.MANY_MAX + 1, 2, N, tau, g, u, v), {}, str(_capi.MANY_MAX)),
             ("negative nsteps", (h, p, 3, -1, V, tau, g, u, v), {}, "nsteps"), ("too many steps", (h, p, 3, 65537, N, tau, g, u, v), {}, "nsteps"),
             ("steps_per_launch", (h, p, 3, 2, V, tau, g, u, v), dict(spl=-1), "steps_per_launch"),
             ("tau 0", (h, p, 3, 2, V, t3(bound, 0.0, bound), g, u, v), {}, "tau"), ("tau negative", (h, p, 3, 2, N, t3(1.0, 1.0, -1.0), g, u, v), {}, "tau"),
             ("tau nan", (h, p, 3, 2, V, t3(np.nan, bound, bound), g, u, v), {}, "tau"), ("tau inf", (h, p, 3, 2, N, t3(1.0, np.inf, 1.0), g, u, v), {}, "tau"),
             ("4 / tau^2 overflows", (h, p, 3, 2, N, t3(1.0, 1.0, 1e-160), g, u, v), {}, "not finite"),
             ("Verlet tau just above the bound", (h, p, 3, 2, V, t3(bound, bound, above), g, u, v), {}, "member 2"),
             ("u is v", (h, p, 3, 2, V, tau, g, u, u), {}, "overlaps"), ("u is g", (h, p, 3, 2, N, tau, u, u, v), {}, "overlaps"),
             ("v is g", (h, p, 3, 2, V, tau, v, u, v), {}, "overlaps"), ("u overlaps v", (h, p, 3, 2, V, tau, g, both[:3], both[1:4]), {}, "overlaps"),
             ("v overlaps g", (h, p, 3, 2, N, tau, both[2:5], u, both[:3]), {}, "overlaps"),
             ("rule", (h, bad(rule=7), 3, 2, N, tau, g, u, v), {}, "rule"), ("true solution", (h, bad(use_true_solution=1), 3, 2, N, tau, g, u, v), {}, "use_true_solution"),
             ("diagnostics", (h, bad(diagnostics=1), 3, 2, N, tau, g, u, v), {}, "diagnostics")]
    for what, args, kw, text in cases:
        rc, msg, dn = call(*args, **kw)
        assert rc == _capi.ERR_INVALID and text in msg, (what, rc, msg)
        assert dn is None or (dn == -7).all(), what                 # nothing was written
        if what.startswith("Verlet tau"):
            assert "%.17g" % bound in msg and "%.17g" % above in msg
        still_good()
    assert np.array_equal(u, u0) and np.array_equal(v, v0)
    # the bound itself is taken; Verlet does not read params
    rc, msg, dn = call(h, None, 3, 2, V, t3(bound, bound, bound), g, u.copy(), v.copy())
    assert rc == _capi.OK and (dn == 2).all()
    # nsys * nsteps above 2^26 counts: refused for Newmark with step_iterations only
    rc, msg, _ = call(h, p, 1025, 65536, N, np.full(1025, 1.0), None, both, both, its=np.zeros(6, dtype=np.int32))
    assert rc == _capi.ERR_INVALID and "counts" in msg
    still_good()
    # the device entry point: the same checks
    ud, vd, gd = (torch.from_numpy(a).cuda() for a in (u0, v0, g))
    torch.cuda.synchronize()
    dev = lib.mi355cg_wave_steps_many_device
    for what, args, kw, text in [("u is v", (h, p, 3, 2, V, tau, gd, ud, ud), {}, "overlaps"), ("scheme", (h, p, 3, 2, 5, tau, gd, ud, vd), {}, "scheme"),
                                 ("tau above", (h, p, 3, 2, V, t3(bound, above, bound), gd, ud, vd), {}, "member 1"),
                                 ("null out", (h, p, 3, 2, N, tau, gd, ud, vd), dict(out=None), "null"),
                                 ("diagnostics", (h, bad(diagnostics=1), 3, 2, N, tau, gd, ud, vd), {}, "diagnostics")]:
        rc, msg, dn = call(*args, fn=dev, **kw)
        assert rc == _capi.ERR_INVALID and text in msg, (what, rc, msg)
        still_good()
    assert np.array_equal(ud.cpu().numpy(), u0) and np.array_equal(vd.cpu().numpy(), v0) and np.array_equal(gd.cpu().numpy(), g)
    for kw in (dict(tau=tau[:2]), dict(g=g[:2]), dict(v0=v0[:2]), dict(scheme=3), dict(tau=t3(bound, above, bound))):
        a = dict(u0=u0, v0=v0, tau=tau, nsteps=2, g=g)
        a.update(kw)
        with pytest.raises(ValueError):
            good.wave_steps_many(**a)
        still_good()
    with pytest.raises(ValueError):
        nm(good, bad(diagnostics=1), u0, v0, tau, 2)
    still_good()
    # nsteps = 0: fine, writes only steps_done = 0
    for scheme in (V, N):
        rc, msg, dn = call(h, p, 3, 0, scheme, tau, g, u, v)
        assert rc == _capi.OK and (dn == 0).all() and np.array_equal(u, u0) and np.array_equal(v, v0)

    # handles the on-chip mode refuses, with its message; a preconditioned handle is a matter of state
    big = _system(cap + 2)
    bb, bv = np.ones((2, big.size())), np.ones((2, big.size()))
    assert big.wave_cfl() == 2.0 / np.sqrt(2.0 * abs(model(big).A0))             # the bound is host arithmetic on any grid handle
    rc, msg, _ = call(big._handle._h, p, 2, 1, V, t3(1e-6, 1e-6), None, bb, bv)
    assert rc == _capi.ERR_INVALID and str(cap) in msg and str(cap + 2) in msg
    with pytest.raises(ValueError):
        big.wave_steps_many(bb, bv, 1e-6)
    big._handle.close()
    mixed = isa.MatrixFreeSystem(16, 16, *DOMAIN, dtype=isa.F32_MIXED)
    rc, msg, _ = call(mixed._handle._h, p, 3, 2, V, tau, g, u, v)
    assert rc == _capi.ERR_INVALID and "F32_MIXED" in msg
    mixed._handle.close()
    slab = C.c_void_p()
    assert lib.mi355cg_create_slab(16, 16, *DOMAIN, _capi.F64, 0, 1, 8, C.byref(slab)) == _capi.OK
    rc, msg, _ = call(slab, p, 3, 2, N, tau, g, u, v)
    assert rc == _capi.ERR_INVALID and "part" in msg
    lib.mi355cg_destroy(slab)
    good.set_preconditioner(isa.PRECOND_MG_ANY)
    for scheme in (V, N):
        rc, msg, _ = call(h, p, 3, 2, scheme, tau, g, u, v)
        assert rc == _capi.ERR_STATE and "preconditioner" in msg
    with pytest.raises(_capi.Mi355cgError):
        good.wave_steps_many(u0, v0, tau, 2)
    good.set_preconditioner(isa.PRECOND_NONE)
    still_good()
    good._handle.close()


def test_workspace_lifetime():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    _, ref, grid = pair(12)
    fresh = _system(12)
    fresh.batch_release()                                            # nothing allocated: fine
    p = params(_capi.RULE_REL_2NORM, **REL)
    u0, v0, tau, g = verlet_ensemble(fresh, grid, seed=61, fractions=tuple(0.1 + 0.9 * (s + 1) / 40 for s in range(40)))
    want = W.verlet(grid, u0, v0, g, tau, 5)
    cut = lambda w, k: (w[0][:k], w[1][:k])
    verlet_same(fresh.wave_steps_many(u0[:2], v0[:2], tau[:2], 5, g=g[:2]), cut(want, 2), 5, "two members")
    verlet_same(fresh.wave_steps_many(u0, v0, tau, 5, g=g), want, 5, "forty members")                  # grown
    verlet_same(fresh.wave_steps_many(u0[:2], v0[:2], tau[:2], 5, g=g[:2]), cut(want, 2), 5, "two again")
    nt = 5.0 * tau[:6]
    wn = newmark_sequential(ref, grid, p, u0[:6], v0[:6], nt, 2, g[:6])
    newmark_same(nm(fresh, p, u0[:6], v0[:6], nt, 2, g=g[:6]), wn, "Newmark on the same workspace")
    x, res = fresh._handle.solve_many(p, g[:5])                      # the batch solves and the theta steppers share the workspace
    assert all(r.converged for r in res)
    assert all(int(d) == 2 for d in fresh._handle.time_steps_many(p, u0[:7], tau[:7], 1.0, 2, g=g[:7])[2])
    verlet_same(fresh.wave_steps_many(u0[:7], v0[:7], tau[:7], 5, g=g[:7]), cut(want, 7), 5, "after a batch")
    newmark_same(nm(fresh, p, u0[:6], v0[:6], nt, 2, g=g[:6]), wn, "Newmark after a batch")
    fresh.batch_release()
    fresh.batch_release()
    verlet_same(fresh.wave_steps_many(u0[:5], v0[:5], tau[:5], 5, g=g[:5]), cut(want, 5), 5, "after the release")
    newmark_same(nm(fresh, p, u0[:6], v0[:6], nt, 2, g=g[:6]), wn, "Newmark after the release")
    # the documented formula (the allocation itself is not exposed)
    size = fresh.size()
    assert isa.wave_steps_many_workspace(12, 40, 5) == fresh.solve_many_info(40)["workspace_bytes"] + 16 * 40 + 8 * size
    assert isa.wave_steps_many_workspace(12, 40, 5, _capi.WAVE_NEWMARK, True) == isa.time_steps_many_workspace(12, 40, 5) + 16 * 40
    fresh._handle.close()


def test_cpp_host_steps_an_ensemble_through_the_compat_header():
    """MatrixFreeSystem::waveStepsMany of three members, bit for bit: Verlet against the NumPy model, Newmark against the reference
    handle; the inputs are repeated operation by operation, the expected states go in as hex floats."""
    from iterative_solvers_amd import _capi
    from iterative_solvers_amd import build as b
    b.build()
    src = os.path.join(ROOT, "tests", "cpp", "onchip_wave_compat_driver.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "onchip_wave_compat_driver")
    headers = [os.path.join(ROOT, "iterative_solvers_amd", "compat", "mi355cg_compat.hpp"), os.path.join(ROOT, "include", "mi355cg.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src] + headers):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                               "-I", os.path.join(ROOT, "iterative_solvers_amd", "compat"), src,
                               "-L", os.path.join(ROOT, "iterative_solvers_amd"), "-lmi355cg",
                               "-Wl,-rpath," + os.path.join(ROOT, "iterative_solvers_amd"), "-o", exe])
    many, ref, grid = pair(12)
    size, nsteps = ref.size(), 3
    i = np.arange(size)
    rhs = ref.get_rhs()
    g = np.stack([rhs * (1.0 + 0.25 * s * (((i * 37) % 101).astype(np.float64) / 101.0)) for s in range(3)])
    u0 = np.stack([0.01 * s * (((i * 11 + s) % 53).astype(np.float64) / 53.0 - 0.5) for s in range(3)])
    v0 = np.stack([0.5 * s * (((i * 7 + s) % 31).astype(np.float64) / 31.0 - 0.5) for s in range(3)])
    bound = many.wave_cfl()
    vu, vv = W.verlet(grid, u0, v0, g, np.array([0.25 * bound, 0.5 * bound, bound]), nsteps)
    p = params(_capi.RULE_REL_2NORM, eps_rel=1e-9, max_iterations=10000, sync_every=7)
    want = newmark_sequential(ref, grid, p, u0, v0, [0.001, 0.0625, 0.5], nsteps, g)
    args = []
    for s in range(3):
        args += [float(x).hex() for x in vu[s]] + [float(x).hex() for x in vv[s]]
    for us, vs, done, its, _ in want:
        args += [str(done)] + [str(x) for x in its] + [float(x).hex() for x in us] + [float(x).hex() for x in vs]
    env = {k: val for k, val in os.environ.items() if k != "MI355CG_ONCHIP"}
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2000:]
    doc = json.loads(out.stdout)
    assert float.fromhex(doc["bound"]) == bound and len(doc["verlet"]) == len(doc["newmark"]) == 3
    for m in doc["verlet"]:
        assert m["same_u"] is True and m["same_v"] is True and (m["steps_done"], m["converged"], m["iterations"]) == (nsteps, 1, 0)
    for m, w in zip(doc["newmark"], want):
        assert m["same_u"] is True and m["same_v"] is True and m["same_counts"] is True and m["steps_done"] == w[2] == nsteps and m["iterations"] == w[3]
