"""The explicit on-chip wave stepper with a source time function and receiver traces:
mi355cg_wave_record_many* integrates u_tt = A u - w_s(t) g_s for many members of one grid, one workgroup per member, and samples u at
a few nodes inside the launch.  "Same" means np.array_equal on u, v and the traces: the NumPy model of
tests/wave_record_reference.py writes every expression operation by operation in the kernel's order."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from onchip_support import DOMAIN, fields, params  # noqa: E402
from onchip_support import cap as _cap, system as _system  # noqa: E402
import wave_record_reference as R  # noqa: E402
import wave_reference as W  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRETCHED = (0.0, 1.0, 0.0, 1.7)
SIZES = [6, 10, 12, 20, 30, 64, 100, "cap"]         # every workgroup size and unroll class of the plan (asserted below)
FRACTIONS = (1.0, 0.77, 0.5, 0.31, 0.13)            # tau_s / bound


def model(sys_):
    """The NumPy grid of a system, its coefficients read from the operator itself: A e_0 has the diagonal at unknown 0, xk at its
    right neighbour (unknown 1) and yk at the node above it (unknown N/2 - 1)."""
    e = np.zeros(sys_.size())
    e[0] = 1.0
    col = sys_.apply(e)
    g = R.Grid(sys_.n, col[0], col[1], col[sys_.n // 2 - 1])
    assert g.size == sys_.size() and g.A0 == -2 * (g.xk + g.yk)
    return g


_systems = {}


def system(n):
    """(the system the ensembles run on, the NumPy grid) of a grid, created once."""
    if n not in _systems:
        s = _system(n)
        _systems[n] = (s, model(s))
    return _systems[n]


def ensemble(sys_, grid, seed, nsteps, fractions=FRACTIONS, shared=False):
    """(u0, v0, tau, g, source, receivers) of one member per fraction of the bound: g the right-hand side x (1 + 0.1 noise), u0 and
    v0 seeded, member 0 at rest at zero, a seeded amplitude row per member (or one for all), three seeded receivers and the two
    ends of the packed order: the first slot of thread 0 and the last slot of the last owning thread."""
    rng = np.random.default_rng(seed)
    k, size = len(fractions), sys_.size()
    g = np.ascontiguousarray(sys_.get_rhs()[None, :] * (1.0 + 0.1 * rng.standard_normal((k, size))))
    u0, v0 = rng.standard_normal((k, size)), rng.standard_normal((k, size)) * np.sqrt(abs(grid.A0))
    u0[0] = v0[0] = 0.0
    source = rng.standard_normal(nsteps + 1) if shared else rng.standard_normal((k, nsteps + 1))
    receivers = [int(r) for r in rng.integers(0, size, 3)] + [0, size - 1]
    return u0, v0, np.asarray(fractions) * grid.cfl(), g, source, receivers


def same(got, want, nsteps, what):
    u, v, traces, res, done = got
    for name, a, b in (("u", u, want[0]), ("v", v, want[1]), ("traces", traces, want[2])):
        if a is None:
            assert b.size == 0, (what, name)
            continue
        if not np.array_equal(a, b):
            print(what, name, "shapes", a.shape, b.shape, "max |difference|", float(np.max(np.abs(a - b))) if a.shape == b.shape else None)
        assert np.array_equal(a, b), (what, name)
    assert [int(d) for d in done] == [nsteps] * len(u), what
    assert all((r.iterations, r.converged) == (0, 1) for r in res), what


def test_the_sizes_below_cover_every_shape_of_the_plan():
    import iterative_solvers_amd as isa
    plans = [isa.onchip_plan(_cap() if n == "cap" else n) for n in SIZES]
    assert {p["threads"] for p in plans} == {64, 128, 256, 512}
    assert {p["elems_per_thread"] for p in plans} == {1, 2, 4, 8, 16, 24}
    assert _cap() == 128


@pytest.mark.parametrize("n", SIZES)
def test_record_over_the_plan(n):
    """Five members with their own tau, g and source, 23 steps sampled every 3rd in launches of 5: neither divides the other, so an
    offset error in the amplitude block or the sample slot shows."""
    n = _cap() if n == "cap" else n
    many, grid = system(n)
    u0, v0, tau, g, source, receivers = ensemble(many, grid, seed=2000 + n, nsteps=23)
    assert receivers[3:] == [0, many.size() - 1]
    got = many.wave_record_many(u0, v0, tau, 23, source, g=g, receivers=receivers, record_every=3, steps_per_launch=5)
    assert got[2].shape == (5, 7, 5)
    same(got, R.verlet_record(grid, u0, v0, g, tau, 23, source, receivers, 3), 23, ("plan", n))
    assert not np.array_equal(got[0], u0)


@pytest.mark.parametrize("n", [10, "cap"])
def test_runs_longer_than_an_amplitude_block(n):
    """150 steps in one launch: the staging of the amplitudes wraps its two blocks; then launches of 100, cut inside a block."""
    n = _cap() if n == "cap" else n
    many, grid = system(n)
    u0, v0, tau, g, source, receivers = ensemble(many, grid, seed=2100 + n, nsteps=150)
    tau = 0.5 * tau                                                  # seeded amplitudes of either sign: keep the states moderate
    want = R.verlet_record(grid, u0, v0, g, tau, 150, source, receivers, 7)
    assert want[2].shape == (5, 21, 5) and np.all(np.isfinite(want[0]))
    same(many.wave_record_many(u0, v0, tau, 150, source, g=g, receivers=receivers, record_every=7), want, 150, ("one launch", n))
    same(many.wave_record_many(u0, v0, tau, 150, source, g=g, receivers=receivers, record_every=7, steps_per_launch=100), want, 150, ("launches of 100", n))
    same(many.wave_record_many(u0, v0, tau, 150, source, g=g, receivers=receivers, record_every=7, steps_per_launch=64), want, 150, ("launches of 64", n))


def test_a_shared_source_row_and_the_most_receivers():
    many, grid = system(30)
    u0, v0, tau, g, source, _ = ensemble(many, grid, seed=2200, nsteps=9, shared=True)
    assert source.shape == (10,)
    receivers = [int(r) for r in np.random.default_rng(5).permutation(many.size())[:64]]
    got = many.wave_record_many(u0, v0, tau, 9, source, g=g, receivers=receivers, steps_per_launch=4)
    assert got[2].shape == (5, 9, 64)
    same(got, R.verlet_record(grid, u0, v0, g, tau, 9, source, receivers, 1), 9, "shared row, 64 receivers")
    # the same row once per member: the same bits
    rows = np.ascontiguousarray(np.stack([source] * 5))
    again = many.wave_record_many(u0, v0, tau, 9, rows, g=g, receivers=receivers)
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3]))
    # g = None: the handle's right-hand side for every member
    tiled = np.ascontiguousarray(np.stack([many.get_rhs()] * 5))
    same(many.wave_record_many(u0, v0, tau, 9, source, receivers=receivers[:2], record_every=2),
         R.verlet_record(grid, u0, v0, tiled, tau, 9, source, receivers[:2], 2), 9, "g = None")


@pytest.mark.parametrize("n", [10, 64])
def test_a_unit_source_without_receivers_is_the_plain_call(n):
    many, grid = system(n)
    u0, v0, tau, g, _, _ = ensemble(many, grid, seed=2300 + n, nsteps=0)
    plain = many.wave_steps_many(u0, v0, tau, 70, g=g, steps_per_launch=33)
    for source in (np.ones(71), np.ones((5, 71))):
        u, v, traces, res, done = many.wave_record_many(u0, v0, tau, 70, source, g=g, steps_per_launch=20)
        assert traces is None and np.array_equal(u, plain[0]) and np.array_equal(v, plain[1]) and [int(d) for d in done] == [70] * 5
    assert np.array_equal(plain[0], W.verlet(grid, u0, v0, g, tau, 70)[0])


def test_chained_calls_are_one_call():
    many, grid = system(20)
    u0, v0, tau, g, source, receivers = ensemble(many, grid, seed=2400, nsteps=24)
    whole = many.wave_record_many(u0, v0, tau, 24, source, g=g, receivers=receivers, record_every=3)
    same(whole, R.verlet_record(grid, u0, v0, g, tau, 24, source, receivers, 3), 24, "whole")
    u, v, at, parts = u0, v0, 0, []
    for k in (9, 3, 12):                                            # multiples of the cadence
        u, v, traces, res, done = many.wave_record_many(u, v, tau, k, np.ascontiguousarray(source[:, at:at + k + 1]), g=g, receivers=receivers,
                                                        record_every=3, steps_per_launch=4)
        assert [int(d) for d in done] == [k] * 5
        parts.append(traces)
        at += k
    assert np.array_equal(u, whole[0]) and np.array_equal(v, whole[1]) and np.array_equal(np.concatenate(parts, axis=1), whole[2])
    # nsteps = 0 writes only steps_done = 0
    u, v, traces, res, done = many.wave_record_many(u0, v0, tau, 0, source[:, :1], g=g, receivers=receivers)
    assert np.array_equal(u, u0) and np.array_equal(v, v0) and traces.shape == (5, 0, 5) and not done.any()


def test_a_stretched_domain():
    s = _system(20, domain=STRETCHED)
    grid = model(s)
    assert grid.xk != grid.yk
    u0, v0, tau, g, source, receivers = ensemble(s, grid, seed=2500, nsteps=23)
    same(s.wave_record_many(u0, v0, tau, 23, source, g=g, receivers=receivers, record_every=3, steps_per_launch=5),
         R.verlet_record(grid, u0, v0, g, tau, 23, source, receivers, 3), 23, "stretched")
    s._handle.close()


def test_more_members_than_are_resident_at_once():
    nsys = 9000
    many, grid = system(10)
    rng = np.random.default_rng(2600)
    size = many.size()
    g = many.get_rhs()[None, :] * (1.0 + 0.1 * rng.standard_normal((nsys, 1)))
    u0, v0 = rng.standard_normal((nsys, size)), rng.standard_normal((nsys, size)) * np.sqrt(abs(grid.A0))
    tau = grid.cfl() * rng.uniform(0.1, 1.0, nsys)
    source = rng.standard_normal((nsys, 8))
    receivers = [0, 17, size - 1]
    same(many.wave_record_many(u0, v0, tau, 7, source, g=g, receivers=receivers, record_every=2, steps_per_launch=3),
         R.verlet_record(grid, u0, v0, g, tau, 7, source, receivers, 2), 7, ("many", nsys))
    many.batch_release()


def test_device_tensors():
    import torch
    many, grid = system(20)
    u0, v0, tau, g, source, receivers = ensemble(many, grid, seed=2700, nsteps=11)
    ud, vd, gd, sd = (torch.from_numpy(a).cuda() for a in (u0, v0, g, source))
    want = R.verlet_record(grid, u0, v0, g, tau, 11, source, receivers, 2)
    ut, vt, tt, rt, dt = many.wave_record_many(ud, vd, tau, 11, sd, g=gd, receivers=receivers, record_every=2, steps_per_launch=4)
    assert ut.is_cuda and vt.is_cuda and tt.is_cuda and ut.data_ptr() != ud.data_ptr() and vt.data_ptr() != vd.data_ptr() and tuple(tt.shape) == (5, 5, 5)
    same((ut.cpu().numpy(), vt.cpu().numpy(), tt.cpu().numpy(), rt, dt), want, 11, "device")
    # one row for all, no receivers, g = None
    ut, vt, tt, rt, dt = many.wave_record_many(ud, vd, torch.from_numpy(tau), 11, sd[1].contiguous())
    tiled = np.ascontiguousarray(np.stack([many.get_rhs()] * 5))
    assert tt is None
    same((ut.cpu().numpy(), vt.cpu().numpy(), None, rt, dt), R.verlet_record(grid, u0, v0, tiled, tau, 11, source[1]), 11, "device, shared row")
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in ((ud, u0), (vd, v0), (gd, g), (sd, source)))
    for bad in (dict(source=source), dict(source=sd[:, :5].contiguous()), dict(traces=np.zeros((5, 5, 5)))):
        a = dict(u0=ud, v0=vd, tau=tau, nsteps=11, source=sd, g=gd, receivers=receivers, record_every=2)
        a.update(bad)
        with pytest.raises(ValueError):
            many.wave_record_many(**a)


def test_stop_flag():
    """Raised before the call: nothing runs and nothing is written.  Raised by another thread while the call runs, it ends the call
    between two launches -- wherever that is, steps_done is a whole number of launches, (u, v) the model's state at that step, the
    samples of the steps that ran the model's and all others the caller's sentinel.  A call that ended before the flag came
    satisfies the same statement with steps_done = nsteps."""
    from iterative_solvers_amd import _capi
    many, grid = system(10)
    nsteps, every, per_launch = 6000, 7, 20
    u0, v0, tau, g, source, receivers = ensemble(many, grid, seed=2800, nsteps=nsteps)
    tau, source = 0.5 * tau, 0.1 * source
    sentinel = -12345.0
    blank = lambda: np.full((5, nsteps // every, 5), sentinel)
    traces = blank()
    u, v, tr, res, done = many.wave_record_many(u0, v0, tau, nsteps, source, g=g, receivers=receivers, record_every=every, steps_per_launch=per_launch,
                                                stop_flag=C.c_int(1), traces=traces)
    assert tr is traces and np.array_equal(u, u0) and np.array_equal(v, v0) and not done.any() and np.all(traces == sentinel)
    assert [(r.iterations, r.stop_reason, r.converged) for r in res] == [(0, _capi.STOP_INTERRUPTED, 0)] * 5
    # the model's state after every launch
    states, u, v = [(u0, v0)], u0, v0
    for lo in range(0, nsteps, per_launch):
        u, v, _ = R.verlet_record(grid, u, v, g, tau, per_launch, source[:, lo:lo + per_launch + 1])
        states.append((u, v))
    whole = R.verlet_record(grid, u0, v0, g, tau, nsteps, source, receivers, every)
    assert np.array_equal(states[-1][0], whole[0]) and np.all(np.isfinite(whole[0])) and len(states) == nsteps // per_launch + 1
    seen = set()
    for delay in (0.001, 0.003, 0.006):
        flag, traces = C.c_int(0), blank()
        timer = threading.Timer(delay, lambda: setattr(flag, "value", 1))
        timer.start()
        u, v, tr, res, done = many.wave_record_many(u0, v0, tau, nsteps, source, g=g, receivers=receivers, record_every=every,
                                                    steps_per_launch=per_launch, stop_flag=flag, traces=traces)
        timer.cancel()
        timer.join()
        d = int(done[0])
        print("flag after", delay, "s: steps_done", d)
        seen.add("whole" if d == nsteps else "stopped")
        assert [int(x) for x in done] == [d] * 5 and d % per_launch == 0 and 0 <= d <= nsteps
        assert np.array_equal(u, states[d // per_launch][0]) and np.array_equal(v, states[d // per_launch][1]), d
        assert np.array_equal(tr[:, :d // every], whole[2][:, :d // every]) and np.all(tr[:, d // every:] == sentinel), d
        assert all(r.stop_reason == _capi.STOP_INTERRUPTED and r.converged == 0 for r in res) == (d < nsteps)
    print("calls ended:", sorted(seen))


@pytest.mark.parametrize("onchip", [False, True])
def test_the_handle_is_untouched(onchip):
    from iterative_solvers_amd import _capi
    s = _system(16, onchip)
    grid = model(s)
    mode = s.solve_mode_info()["mode"]
    h = s._handle
    p = params(_capi.RULE_REL_2NORM, eps_rel=1e-8, sync_every=7)
    for shift in (0.0, 3.0):
        h.set_shift(shift)
        first = fields(h.solve(p, None, None))
        x, r, rhs = h.solution(), h.recursive_residual(), h.rhs()
        u0, v0, tau, g, source, receivers = ensemble(s, grid, seed=2900, nsteps=5)
        same(s.wave_record_many(u0, v0, tau, 5, source, receivers=receivers),
             R.verlet_record(grid, u0, v0, np.stack([rhs] * 5), tau, 5, source, receivers, 1), 5, "unshifted A, the handle's g")
        assert np.array_equal(h.solution(), x) and np.array_equal(h.recursive_residual(), r) and np.array_equal(h.rhs(), rhs)
        assert h.get_shift() == shift and s.solve_mode_info()["mode"] == mode
        assert fields(h.solve(p, None, None)) == first              # cold: the ensemble left no pending guess behind
        assert np.array_equal(h.solution(), x) and np.array_equal(h.recursive_residual(), r)
        guess = np.random.default_rng(18).standard_normal(s.size())
        h.set_initial_guess(guess)
        warm = fields(h.solve(p, None, None))
        xw = h.solution()
        h.set_initial_guess(guess)
        s.wave_record_many(u0, v0, tau, 3, source[:, :4], g=g, receivers=receivers)
        assert fields(h.solve(p, None, None)) == warm and np.array_equal(h.solution(), xw)
    h.close()


def test_workspace_lifetime():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    _, grid = system(12)
    fresh = _system(12)
    fresh.batch_release()                                            # nothing allocated: fine
    fractions = tuple(0.1 + 0.9 * (s + 1) / 40 for s in range(40))
    u0, v0, tau, g, source, receivers = ensemble(fresh, grid, seed=3000, nsteps=5, fractions=fractions)
    want = R.verlet_record(grid, u0, v0, g, tau, 5, source, receivers, 2)
    cut = lambda k: tuple(w[:k] for w in want)
    run = lambda k, **kw: fresh.wave_record_many(u0[:k], v0[:k], tau[:k], 5, source[:k], g=g[:k], receivers=receivers, record_every=2, **kw)
    same(run(2), cut(2), 5, "two members")
    same(run(40), cut(40), 5, "forty members")                      # grown
    same(run(2), cut(2), 5, "two again")
    # a longer table and more samples: the staging of the host entry point grows
    long_source = np.random.default_rng(1).standard_normal((40, 301)) * 0.1
    same(fresh.wave_record_many(u0, v0, 0.5 * tau, 300, long_source, g=g, receivers=receivers),
         R.verlet_record(grid, u0, v0, g, 0.5 * tau, 300, long_source, receivers, 1), 300, "a longer table")
    same(run(40), cut(40), 5, "forty after the longer table")
    # the plain steppers and the batch solves share the workspace
    p = params(_capi.RULE_REL_2NORM, eps_rel=1e-8, sync_every=7)
    x, res = fresh._handle.solve_many(p, g[:5])
    assert all(r.converged for r in res)
    plain = fresh.wave_steps_many(u0[:7], v0[:7], tau[:7], 5, g=g[:7])
    assert np.array_equal(plain[0], W.verlet(grid, u0[:7], v0[:7], g[:7], tau[:7], 5)[0])
    same(run(7), cut(7), 5, "after a batch")
    fresh.batch_release()
    fresh.batch_release()
    same(run(5), cut(5), 5, "after the release")
    # the documented formula (the allocation itself is not exposed)
    assert isa.wave_record_many_workspace(12, 40, 5, 5, 2) == isa.wave_steps_many_workspace(12, 40, 5) + 4 * _capi.WAVE_MAX_RECEIVERS
    assert isa.wave_record_many_workspace(12, 40, 5) == fresh.solve_many_info(40)["workspace_bytes"] + 16 * 40 + 8 * fresh.size() + 256
    fresh._handle.close()


def test_refusals_leave_the_handle_usable():
    import iterative_solvers_amd as isa
    import torch
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    cap = _cap()
    good = _system(16)
    grid = model(good)
    size = good.size()
    u0, v0, tau, g, source, receivers = ensemble(good, grid, seed=3100, nsteps=4, fractions=(1.0, 0.5, 0.2))
    want = R.verlet_record(grid, u0, v0, g, tau, 4, source, receivers, 2)
    h = good._handle._h
    nodes = np.asarray(receivers, dtype=np.int32)

    def still_good():
        same(good.wave_record_many(u0, v0, tau, 4, source, g=g, receivers=receivers, record_every=2, steps_per_launch=3), want, 4, "after a refusal")

    def call(handle, nsys, nsteps, tt, gg, uu, vv, ww, stride, nrec, nn, every, tr, spl=0, out="res", done="done", fn=lib.mi355cg_wave_record_many):
        ptr = lambda a: (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) if a is not None else None
        res = (_capi.Results * max(nsys, 1))() if out == "res" else None
        dn = np.full(max(nsys, 1), -7, dtype=np.int32) if done == "done" else None
        rc = fn(handle, nsys, nsteps, ptr(tt), ptr(gg), ptr(uu), ptr(vv), ptr(ww), stride, nrec, ptr(nn), every, ptr(tr), spl, None, res, ptr(dn))
        return rc, lib.mi355cg_last_error().decode(), dn

    u, v, w = u0.copy(), v0.copy(), source.copy()
    traces = np.full((3, 2, 5), -5.0)
    both = np.zeros((6, size))
    t3 = lambda *a: np.array(a, dtype=np.float64)
    bound = good.wave_cfl()
    above = np.nextafter(bound, np.inf)
    wbad = lambda val: np.where(np.arange(15).reshape(3, 5) == 7, val, source)
    ok = (h, 3, 4, tau, g, u, v, w, 5, 5, nodes, 2, traces)

    def but(**kw):
        names = ("handle", "nsys", "nsteps", "tt", "gg", "uu", "vv", "ww", "stride", "nrec", "nn", "every", "tr")
        a = dict(zip(names, ok))
        a.update(kw)
        return tuple(a[k] for k in names)

    cases = [("nrec -1", but(nrec=-1), {}, "64"), ("nrec 65", but(nrec=65, nn=np.zeros(65, dtype=np.int32)), {}, "64"),
             ("receiver -1", but(nn=np.array([0, 1, -1, 2, 3], dtype=np.int32)), {}, "receiver 2"),
             ("receiver size", but(nn=np.array([0, 1, 2, 3, size], dtype=np.int32)), {}, f"[0, {size})"),
             ("record_every 0", but(every=0), {}, "record_every"), ("record_every -2", but(every=-2), {}, "record_every"),
             ("null traces", but(tr=None), {}, "traces"), ("null rec_nodes", but(nn=None), {}, "rec_nodes"),
             ("null w", but(ww=None), {}, "amplitudes"), ("w_stride too short", but(stride=4), {}, "w_stride"), ("w_stride negative", but(stride=-5), {}, "w_stride"),
             ("amplitude nan", but(ww=wbad(np.nan)), {}, "member 1 at step 2"), ("amplitude inf", but(ww=wbad(np.inf)), {}, "finite"),
             ("amplitude -inf in a shared row", but(ww=np.array([0.0, 1.0, -np.inf, 0.0, 0.0]), stride=0), {}, "member 0 at step 2"),
             ("w is u", but(ww=u, stride=size), {}, "w overlaps u"), ("w in v", but(ww=v[1], stride=0), {}, "w overlaps v"),
             ("w in g", but(ww=g[2, 3:], stride=0), {}, "w overlaps g"),
             ("traces is u", but(tr=u), {}, "traces overlaps u"), ("traces in v", but(tr=v[2, 10:]), {}, "traces overlaps v"),
             ("traces in g", but(tr=g[0]), {}, "traces overlaps g"), ("traces in w", but(tr=w[1]), {}, "traces overlaps w"),
             # everything the plain Verlet call refuses
             ("null u", but(uu=None), {}, "null"), ("null v", but(vv=None), {}, "null"), ("null tau", but(tt=None), {}, "null"),
             ("null out", ok, dict(out=None), "null"), ("null steps_done", ok, dict(done=None), "null"), ("null handle", but(handle=None), {}, "null"),
             ("no members", but(nsys=0), {}, str(_capi.MANY_MAX)), ("too many", but(nsys=_capi.MANY_MAX + 1), {}, str(_capi.MANY_MAX)),
             ("negative nsteps", but(nsteps=-1), {}, "nsteps"), ("too many steps", but(nsteps=65537), {}, "nsteps"),
             ("steps_per_launch", ok, dict(spl=-1), "steps_per_launch"),
             ("tau 0", but(tt=t3(bound, 0.0, bound)), {}, "tau"), ("tau nan", but(tt=t3(np.nan, bound, bound)), {}, "tau"),
             ("tau just above the bound", but(tt=t3(bound, bound, above)), {}, "member 2"),
             ("u is v", but(vv=u), {}, "overlaps"), ("u is g", but(gg=u), {}, "overlaps"), ("v is g", but(gg=v), {}, "overlaps"),
             ("u overlaps v", but(uu=both[:3], vv=both[1:4]), {}, "overlaps")]
    for what, args, kw, text in cases:
        rc, msg, dn = call(*args, **kw)
        assert rc == _capi.ERR_INVALID and text in msg, (what, rc, msg)
        assert dn is None or (dn == -7).all(), what                 # nothing was written
        if what.startswith("tau just"):
            assert "%.17g" % bound in msg and "%.17g" % above in msg
        still_good()
    assert np.array_equal(u, u0) and np.array_equal(v, v0) and np.all(traces == -5.0) and np.array_equal(w, source)
    # the limits themselves are taken: the bound on tau, 64 receivers, no receivers with null rec_nodes and traces, a wider stride
    rc, msg, dn = call(*but(tt=t3(bound, bound, bound), uu=u.copy(), vv=v.copy(), nrec=0, nn=None, tr=None))
    assert rc == _capi.OK and (dn == 4).all()
    wide = np.zeros((3, 9))
    wide[:, :5] = source
    t64 = np.zeros((3, 2, 64))
    rc, msg, dn = call(*but(uu=u.copy(), vv=v.copy(), ww=wide, stride=9, nrec=64, nn=np.arange(64, dtype=np.int32), tr=t64))
    assert rc == _capi.OK and (dn == 4).all() and np.array_equal(t64, R.verlet_record(grid, u0, v0, g, tau, 4, source, range(64), 2)[2])
    # the device entry point: the same checks (a table in device memory is not read)
    ud, vd, gd, wd = (torch.from_numpy(a).cuda() for a in (u0, v0, g, source))
    td = torch.full((3, 2, 5), -5.0, dtype=torch.float64).cuda()
    torch.cuda.synchronize()
    dev = lib.mi355cg_wave_record_many_device
    okd = dict(gg=gd, uu=ud, vv=vd, ww=wd, tr=td)
    for what, kw, text in [("nrec", dict(nrec=70), "64"), ("receiver", dict(nn=np.array([0, 1, 2, 3, size + 5], dtype=np.int32)), "receiver 4"),
                           ("record_every", dict(every=0), "record_every"), ("null traces", dict(tr=None), "traces"), ("null w", dict(ww=None), "amplitudes"),
                           ("w is u", dict(ww=ud, stride=size), "w overlaps u"), ("traces is g", dict(tr=gd), "traces overlaps g"),
                           ("u is v", dict(vv=ud), "overlaps"), ("tau above", dict(tt=t3(bound, above, bound)), "member 1")]:
        rc, msg, dn = call(*but(**dict(okd, **kw)), fn=dev)
        assert rc == _capi.ERR_INVALID and text in msg, (what, rc, msg)
        still_good()
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in ((ud, u0), (vd, v0), (gd, g), (wd, source))) and bool((td == -5.0).all())
    # the Python layer
    for kw in (dict(tau=tau[:2]), dict(g=g[:2]), dict(v0=v0[:2]), dict(source=source[:, :4]), dict(source=source[:2]), dict(record_every=0),
               dict(receivers=[0, size]), dict(receivers=list(range(65))), dict(receivers=[[0, 1]]), dict(tau=t3(bound, above, bound)),
               dict(traces=np.zeros((3, 2, 4))), dict(source=wbad(np.nan))):
        a = dict(u0=u0, v0=v0, tau=tau, nsteps=4, source=source, g=g, receivers=receivers, record_every=2)
        a.update(kw)
        with pytest.raises(ValueError):
            good.wave_record_many(**a)
        still_good()

    # handles the on-chip mode refuses, with its message; a preconditioned handle is a matter of state
    big = _system(cap + 2)
    bb, bv = np.ones((2, big.size())), np.ones((2, big.size()))
    rc, msg, _ = call(big._handle._h, 2, 1, t3(1e-6, 1e-6), None, bb, bv, np.ones(2), 0, 0, None, 1, None)
    assert rc == _capi.ERR_INVALID and str(cap) in msg and str(cap + 2) in msg
    with pytest.raises(ValueError):
        big.wave_record_many(bb, bv, 1e-6, 1, np.ones(2))
    big._handle.close()
    mixed = isa.MatrixFreeSystem(16, 16, *DOMAIN, dtype=isa.F32_MIXED)
    rc, msg, _ = call(*but(handle=mixed._handle._h))
    assert rc == _capi.ERR_INVALID and "F32_MIXED" in msg
    mixed._handle.close()
    good.set_preconditioner(isa.PRECOND_MG_ANY)
    rc, msg, _ = call(*ok)
    assert rc == _capi.ERR_STATE and "preconditioner" in msg
    with pytest.raises(_capi.Mi355cgError):
        good.wave_record_many(u0, v0, tau, 4, source)
    good.set_preconditioner(isa.PRECOND_NONE)
    still_good()
    good._handle.close()


def test_packed_index_names_the_receivers():
    many, grid = system(12)
    n = 12
    cells, pitch = W.packed_cells(n)
    for i in (0, 5, 30, many.size() - 1):
        assert many.packed_index(int(cells[i]) % pitch, int(cells[i]) // pitch) == i
    assert many.packed_index(0, 3) == -1 and many.packed_index(3, 3) == -1 and many.packed_index(n, n) == -1
    # a point source at a node, heard at its right neighbour after one step and not before: u' = u + tau (v + h a), a = -w0 g
    src, right = many.packed_index(4, 9), many.packed_index(5, 9)
    g = np.zeros((1, many.size()))
    g[0, src] = -1.0
    zero = np.zeros((1, many.size()))
    tau = 0.5 * grid.cfl()
    u, v, traces, res, done = many.wave_record_many(zero, zero, tau, 2, np.ones(3), g=g, receivers=[src, right])
    assert traces[0, 0, 0] == tau * (0.5 * tau * 1.0) and traces[0, 0, 1] == 0.0 and traces[0, 1, 1] > 0.0
    same((u, v, traces, res, done), R.verlet_record(grid, zero, zero, g, tau, 2, np.ones(3), [src, right], 1), 2, "point source")


def test_cpp_host_records_an_ensemble_through_the_compat_header():
    """MatrixFreeSystem::waveRecordMany of three members, bit for bit against the NumPy model; the inputs are repeated operation by
    operation, the expected values go in as hex floats."""
    from iterative_solvers_amd import build as b
    b.build()
    src = os.path.join(ROOT, "tests", "cpp", "onchip_wave_record_compat_driver.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "onchip_wave_record_compat_driver")
    headers = [os.path.join(ROOT, "iterative_solvers_amd", "compat", "mi355cg_compat.hpp"), os.path.join(ROOT, "include", "mi355cg.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src] + headers):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                               "-I", os.path.join(ROOT, "iterative_solvers_amd", "compat"), src,
                               "-L", os.path.join(ROOT, "iterative_solvers_amd"), "-lmi355cg",
                               "-Wl,-rpath," + os.path.join(ROOT, "iterative_solvers_amd"), "-o", exe])
    many, grid = system(12)
    size, nsteps, every = many.size(), 7, 2
    i = np.arange(size)
    rhs = many.get_rhs()
    g = np.stack([rhs * (1.0 + 0.25 * s * (((i * 37) % 101).astype(np.float64) / 101.0)) for s in range(3)])
    u0 = np.stack([0.01 * s * (((i * 11 + s) % 53).astype(np.float64) / 53.0 - 0.5) for s in range(3)])
    v0 = np.stack([0.5 * s * (((i * 7 + s) % 31).astype(np.float64) / 31.0 - 0.5) for s in range(3)])
    source = np.stack([((np.arange(nsteps + 1) * 5 + s * 3) % 11).astype(np.float64) / 4.0 - 1.0 for s in range(3)])
    bound = many.wave_cfl()
    tau = np.array([0.25 * bound, 0.5 * bound, bound])
    receivers = [0, size // 2, size - 1]
    ru, rv, rt = R.verlet_record(grid, u0, v0, g, tau, nsteps, source, receivers, every)
    su, sv, _ = R.verlet_record(grid, u0, v0, g, tau, nsteps, source[1])
    args = []
    for s in range(3):
        args += [float(x).hex() for x in ru[s]] + [float(x).hex() for x in rv[s]] + [float(x).hex() for x in rt[s].reshape(-1)]
    for s in range(3):
        args += [float(x).hex() for x in su[s]] + [float(x).hex() for x in sv[s]]
    env = {k: val for k, val in os.environ.items() if k != "MI355CG_ONCHIP"}
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2000:]
    doc = json.loads(out.stdout)
    assert len(doc["recorded"]) == len(doc["shared"]) == 3
    for m in doc["recorded"]:
        assert m["same_u"] is True and m["same_v"] is True and m["same_traces"] is True and (m["steps_done"], m["converged"], m["iterations"]) == (nsteps, 1, 0)
    for m in doc["shared"]:
        assert m["same_u"] is True and m["same_v"] is True and m["no_traces"] is True and m["steps_done"] == nsteps
