"""The recorded explicit on-chip wave stepper in a medium: mi355cg_wave_medium_many* integrates
u_tt = c2_s o (A u) - w_s(t) g_s for many members of one grid, one workgroup per member, the squared wave speed c2 of every unknown
given per member or once for all.  "Same" means np.array_equal on u, v and the traces: the NumPy model of
tests/wave_medium_reference.py writes every expression operation by operation in the kernel's order."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from onchip_support import fields, params  # noqa: E402
from onchip_support import cap as _cap, system as _system  # noqa: E402
import wave_medium_reference as M  # noqa: E402
import wave_record_reference as R  # noqa: E402

pytestmark = pytest.mark.gpu

STRETCHED = (0.0, 1.0, 0.0, 1.7)
SIZES = [6, 10, 12, 20, 30, 64, 100, "cap"]         # every workgroup size and unroll class of the plan (asserted below)
FRACTIONS = (1.0, 0.77, 0.5, 0.31, 0.13)            # tau_s / the member's own bound


def model(sys_):
    """The NumPy grid of a system, its coefficients read from the operator itself: A e_0 has the diagonal at unknown 0, xk at its
    right neighbour (unknown 1) and yk at the node above it (unknown N/2 - 1)."""
    e = np.zeros(sys_.size())
    e[0] = 1.0
    col = sys_.apply(e)
    g = M.Grid(sys_.n, col[0], col[1], col[sys_.n // 2 - 1])
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
    """(u0, v0, tau, g, c2, source, receivers) of one member per fraction of ITS bound: g the right-hand side x (1 + 0.1 noise), u0
    and v0 seeded, member 0 at rest at zero, a seeded medium in [0.25, 4] per member (or one for all), a seeded amplitude row per
    member, three seeded receivers and the two ends of the packed order."""
    rng = np.random.default_rng(seed)
    k, size = len(fractions), sys_.size()
    g = np.ascontiguousarray(sys_.get_rhs()[None, :] * (1.0 + 0.1 * rng.standard_normal((k, size))))
    u0, v0 = rng.standard_normal((k, size)), rng.standard_normal((k, size)) * np.sqrt(abs(grid.A0))
    u0[0] = v0[0] = 0.0
    c2 = rng.uniform(0.25, 4.0, size if shared else (k, size))
    source = rng.standard_normal((k, nsteps + 1))
    receivers = [int(r) for r in rng.integers(0, size, 3)] + [0, size - 1]
    tau = np.asarray(fractions) * M.medium_cfl(grid, c2.max(axis=-1))
    return u0, v0, tau, g, c2, source, receivers


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
def test_media_over_the_plan(n):
    """Five members with their own tau, medium, g and source, 23 steps sampled every 3rd in launches of 5."""
    n = _cap() if n == "cap" else n
    many, grid = system(n)
    u0, v0, tau, g, c2, source, receivers = ensemble(many, grid, seed=4000 + n, nsteps=23)
    assert receivers[3:] == [0, many.size() - 1] and np.array_equal(many.wave_cfl(c2) * np.asarray(FRACTIONS), tau)
    got = many.wave_record_many(u0, v0, tau, 23, source, g=g, receivers=receivers, record_every=3, steps_per_launch=5, c2=c2)
    assert got[2].shape == (5, 7, 5)
    same(got, M.verlet_medium(grid, u0, v0, g, c2, tau, 23, source, receivers, 3), 23, ("plan", n))
    assert not np.array_equal(got[0], u0)


def test_the_bound_of_a_medium():
    many, grid = system(20)
    c2 = np.random.default_rng(4100).uniform(0.25, 4.0, (5, many.size()))
    assert many.wave_cfl() == many.wave_cfl(np.ones(many.size())) == grid.cfl()
    assert np.array_equal(many.wave_cfl(c2), M.medium_cfl(grid, c2.max(axis=1))) and many.wave_cfl(c2[3]) == M.medium_cfl(grid, c2[3].max())
    assert many.wave_cfl(np.full(many.size(), 4.0)) == 0.5 * grid.cfl()
    for bad in (np.zeros(many.size()), np.full(many.size(), np.nan), -c2):
        with pytest.raises(ValueError):
            many.wave_cfl(bad)


def test_a_shared_medium():
    many, grid = system(30)
    u0, v0, tau, g, c2, source, receivers = ensemble(many, grid, seed=4200, nsteps=9, shared=True)
    assert c2.shape == (many.size(),) and tau.shape == (5,)
    got = many.wave_record_many(u0, v0, tau, 9, source, g=g, receivers=receivers, steps_per_launch=4, c2=c2)
    same(got, M.verlet_medium(grid, u0, v0, g, c2, tau, 9, source, receivers, 1), 9, "shared medium")
    # the same medium once per member: the same bits
    again = many.wave_record_many(u0, v0, tau, 9, source, g=g, receivers=receivers, c2=np.ascontiguousarray(np.stack([c2] * 5)))
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3]))
    # g = None, a shared source row, no receivers
    tiled = np.ascontiguousarray(np.stack([many.get_rhs()] * 5))
    same(many.wave_record_many(u0, v0, tau, 9, source[2], c2=c2), M.verlet_medium(grid, u0, v0, tiled, c2, tau, 9, source[2]), 9, "g = None")


def test_a_two_layer_medium():
    """c2 = 1 below a row of the grid, 4 above: a point source in the slow layer, one receiver in each."""
    many, grid = system(20)
    size = many.size()
    rows = grid.cells // grid.pitch
    c2 = np.where(rows >= 14, 4.0, 1.0)
    assert 0 < (c2 == 4.0).sum() < size
    g = np.zeros((1, size))
    g[0, many.packed_index(14, 5)] = -1.0
    zero = np.zeros((1, size))
    receivers = [many.packed_index(14, 9), many.packed_index(8, 17)]
    tau = 0.9 * many.wave_cfl(c2)
    assert tau == 0.9 * 0.5 * grid.cfl()
    source = np.sin(0.5 * np.pi * np.minimum(np.arange(61) / 20, 1)) ** 2
    got = many.wave_record_many(zero, zero, tau, 60, source, g=g, receivers=receivers, c2=c2, steps_per_launch=25)
    same(got, M.verlet_medium(grid, zero, zero, g, c2, tau, 60, source, receivers, 1), 60, "two layers")
    assert np.abs(got[2]).max() > 0
    # in a homogeneous medium the traces differ
    assert not np.array_equal(got[2], many.wave_record_many(zero, zero, tau, 60, source, g=g, receivers=receivers)[2])


@pytest.mark.parametrize("n", [10, 64])
def test_a_unit_medium_is_the_call_without_one(n):
    many, grid = system(n)
    u0, v0, tau, g, _, source, receivers = ensemble(many, grid, seed=4300 + n, nsteps=70)
    plain = many.wave_record_many(u0, v0, tau, 70, source, g=g, receivers=receivers, record_every=4, steps_per_launch=33)
    for c2 in (np.ones(many.size()), np.ones((5, many.size()))):
        got = many.wave_record_many(u0, v0, tau, 70, source, g=g, receivers=receivers, record_every=4, steps_per_launch=20, c2=c2)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], plain[:3])) and [int(d) for d in got[4]] == [70] * 5
    assert np.array_equal(plain[0], R.verlet_record(grid, u0, v0, g, tau, 70, source)[0])


@pytest.mark.parametrize("n", [10, 64])
def test_a_medium_of_four_is_the_plain_call_rescaled(n):
    """Scalings by powers of two are exact: c2 = 4 with (tau, v0, g) gives the u and the traces of the plain call with (2 tau,
    v0 / 2, g / 4) and twice its v."""
    many, grid = system(n)
    u0, v0, tau, g, _, source, receivers = ensemble(many, grid, seed=4400 + n, nsteps=40)
    tau = 0.5 * tau
    got = many.wave_record_many(u0, v0, tau, 40, source, g=g, receivers=receivers, record_every=3, c2=np.full(many.size(), 4.0))
    plain = many.wave_record_many(u0, 0.5 * v0, 2.0 * tau, 40, source, g=0.25 * g, receivers=receivers, record_every=3)
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], 2.0 * plain[1]) and np.array_equal(got[2], plain[2])
    assert not np.array_equal(got[0], u0)


@pytest.mark.parametrize("n", [10, "cap"])
def test_runs_longer_than_an_amplitude_block(n):
    """150 steps in one launch: the staging of the amplitudes wraps its two blocks; then launches of 100 and 64."""
    n = _cap() if n == "cap" else n
    many, grid = system(n)
    u0, v0, tau, g, c2, source, receivers = ensemble(many, grid, seed=4500 + n, nsteps=150)
    tau = 0.5 * tau                                                  # seeded amplitudes of either sign: keep the states moderate
    want = M.verlet_medium(grid, u0, v0, g, c2, tau, 150, source, receivers, 7)
    assert want[2].shape == (5, 21, 5) and np.all(np.isfinite(want[0]))
    same(many.wave_record_many(u0, v0, tau, 150, source, g=g, receivers=receivers, record_every=7, c2=c2), want, 150, ("one launch", n))
    same(many.wave_record_many(u0, v0, tau, 150, source, g=g, receivers=receivers, record_every=7, steps_per_launch=100, c2=c2), want, 150, ("launches of 100", n))
    same(many.wave_record_many(u0, v0, tau, 150, source, g=g, receivers=receivers, record_every=7, steps_per_launch=64, c2=c2), want, 150, ("launches of 64", n))


def test_chained_calls_are_one_call():
    many, grid = system(20)
    u0, v0, tau, g, c2, source, receivers = ensemble(many, grid, seed=4600, nsteps=24)
    whole = many.wave_record_many(u0, v0, tau, 24, source, g=g, receivers=receivers, record_every=3, c2=c2)
    same(whole, M.verlet_medium(grid, u0, v0, g, c2, tau, 24, source, receivers, 3), 24, "whole")
    u, v, at, parts = u0, v0, 0, []
    for k in (9, 3, 12):                                            # multiples of the cadence
        u, v, traces, res, done = many.wave_record_many(u, v, tau, k, np.ascontiguousarray(source[:, at:at + k + 1]), g=g, receivers=receivers,
                                                        record_every=3, steps_per_launch=4, c2=c2)
        assert [int(d) for d in done] == [k] * 5
        parts.append(traces)
        at += k
    assert np.array_equal(u, whole[0]) and np.array_equal(v, whole[1]) and np.array_equal(np.concatenate(parts, axis=1), whole[2])
    # nsteps = 0 writes only steps_done = 0
    u, v, traces, res, done = many.wave_record_many(u0, v0, tau, 0, source[:, :1], g=g, receivers=receivers, c2=c2)
    assert np.array_equal(u, u0) and np.array_equal(v, v0) and traces.shape == (5, 0, 5) and not done.any()


def test_a_stretched_domain():
    s = _system(20, domain=STRETCHED)
    grid = model(s)
    assert grid.xk != grid.yk
    u0, v0, tau, g, c2, source, receivers = ensemble(s, grid, seed=4700, nsteps=23)
    same(s.wave_record_many(u0, v0, tau, 23, source, g=g, receivers=receivers, record_every=3, steps_per_launch=5, c2=c2),
         M.verlet_medium(grid, u0, v0, g, c2, tau, 23, source, receivers, 3), 23, "stretched")
    s._handle.close()


def test_more_members_than_are_resident_at_once():
    nsys = 9000
    many, grid = system(10)
    rng = np.random.default_rng(4800)
    size = many.size()
    g = many.get_rhs()[None, :] * (1.0 + 0.1 * rng.standard_normal((nsys, 1)))
    u0, v0 = rng.standard_normal((nsys, size)), rng.standard_normal((nsys, size)) * np.sqrt(abs(grid.A0))
    c2 = rng.uniform(0.25, 4.0, (nsys, size))
    tau = M.medium_cfl(grid, c2.max(axis=1)) * rng.uniform(0.1, 1.0, nsys)
    source = rng.standard_normal((nsys, 8))
    receivers = [0, 17, size - 1]
    same(many.wave_record_many(u0, v0, tau, 7, source, g=g, receivers=receivers, record_every=2, steps_per_launch=3, c2=c2),
         M.verlet_medium(grid, u0, v0, g, c2, tau, 7, source, receivers, 2), 7, ("many", nsys))
    many.batch_release()


def test_device_tensors():
    """CUDA tensors: the media are reduced by the check launch, k_oc_medium_range, not on the host."""
    import torch
    many, grid = system(20)
    u0, v0, tau, g, c2, source, receivers = ensemble(many, grid, seed=4900, nsteps=11)
    ud, vd, gd, cd, sd = (torch.from_numpy(a).cuda() for a in (u0, v0, g, c2, source))
    want = M.verlet_medium(grid, u0, v0, g, c2, tau, 11, source, receivers, 2)
    assert np.array_equal(many.wave_cfl(cd), many.wave_cfl(c2))
    ut, vt, tt, rt, dt = many.wave_record_many(ud, vd, tau, 11, sd, g=gd, receivers=receivers, record_every=2, steps_per_launch=4, c2=cd)
    assert ut.is_cuda and vt.is_cuda and tt.is_cuda and ut.data_ptr() != ud.data_ptr() and vt.data_ptr() != vd.data_ptr() and tuple(tt.shape) == (5, 5, 5)
    same((ut.cpu().numpy(), vt.cpu().numpy(), tt.cpu().numpy(), rt, dt), want, 11, "device")
    # one medium for all, no receivers, g = None; the smallest bound holds for every member
    tiled = np.ascontiguousarray(np.stack([many.get_rhs()] * 5))
    low = np.full(5, tau.min())
    ut, vt, tt, rt, dt = many.wave_record_many(ud, vd, low, 11, sd[1].contiguous(), c2=cd[3].contiguous())
    assert tt is None
    same((ut.cpu().numpy(), vt.cpu().numpy(), None, rt, dt), M.verlet_medium(grid, u0, v0, tiled, c2[3], low, 11, source[1]), 11, "device, shared medium")
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in ((ud, u0), (vd, v0), (gd, g), (cd, c2), (sd, source)))
    for bad in (dict(c2=c2), dict(c2=cd[:, :5].contiguous()), dict(c2=cd[:2].contiguous()), dict(c2=cd.float())):
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
    u0, v0, tau, g, c2, source, receivers = ensemble(many, grid, seed=5000, nsteps=nsteps)
    tau, source = 0.5 * tau, 0.1 * source
    sentinel = -12345.0
    blank = lambda: np.full((5, nsteps // every, 5), sentinel)
    traces = blank()
    u, v, tr, res, done = many.wave_record_many(u0, v0, tau, nsteps, source, g=g, receivers=receivers, record_every=every, steps_per_launch=per_launch,
                                                stop_flag=C.c_int(1), traces=traces, c2=c2)
    assert tr is traces and np.array_equal(u, u0) and np.array_equal(v, v0) and not done.any() and np.all(traces == sentinel)
    assert [(r.iterations, r.stop_reason, r.converged) for r in res] == [(0, _capi.STOP_INTERRUPTED, 0)] * 5
    # the model's state after every launch
    states, u, v = [(u0, v0)], u0, v0
    for lo in range(0, nsteps, per_launch):
        u, v, _ = M.verlet_medium(grid, u, v, g, c2, tau, per_launch, source[:, lo:lo + per_launch + 1])
        states.append((u, v))
    whole = M.verlet_medium(grid, u0, v0, g, c2, tau, nsteps, source, receivers, every)
    assert np.array_equal(states[-1][0], whole[0]) and np.all(np.isfinite(whole[0])) and len(states) == nsteps // per_launch + 1
    seen = set()
    for delay in (0.001, 0.003, 0.006):
        flag, traces = C.c_int(0), blank()
        timer = threading.Timer(delay, lambda: setattr(flag, "value", 1))
        timer.start()
        u, v, tr, res, done = many.wave_record_many(u0, v0, tau, nsteps, source, g=g, receivers=receivers, record_every=every,
                                                    steps_per_launch=per_launch, stop_flag=flag, traces=traces, c2=c2)
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
        u0, v0, tau, g, c2, source, receivers = ensemble(s, grid, seed=5100, nsteps=5)
        same(s.wave_record_many(u0, v0, tau, 5, source, receivers=receivers, c2=c2),
             M.verlet_medium(grid, u0, v0, np.stack([rhs] * 5), c2, tau, 5, source, receivers, 1), 5, "unshifted A, the handle's g")
        assert np.array_equal(h.solution(), x) and np.array_equal(h.recursive_residual(), r) and np.array_equal(h.rhs(), rhs)
        assert h.get_shift() == shift and s.solve_mode_info()["mode"] == mode
        assert fields(h.solve(p, None, None)) == first              # cold: the ensemble left no pending guess behind
        assert np.array_equal(h.solution(), x) and np.array_equal(h.recursive_residual(), r)
        guess = np.random.default_rng(18).standard_normal(s.size())
        h.set_initial_guess(guess)
        warm = fields(h.solve(p, None, None))
        xw = h.solution()
        h.set_initial_guess(guess)
        s.wave_record_many(u0, v0, tau, 3, source[:, :4], g=g, receivers=receivers, c2=c2)
        assert fields(h.solve(p, None, None)) == warm and np.array_equal(h.solution(), xw)
    h.close()


def test_workspace_lifetime():
    import iterative_solvers_amd as isa
    import torch
    _, grid = system(12)
    fresh = _system(12)
    fresh.batch_release()                                            # nothing allocated: fine
    fractions = tuple(0.1 + 0.9 * (s + 1) / 40 for s in range(40))
    u0, v0, tau, g, c2, source, receivers = ensemble(fresh, grid, seed=5200, nsteps=5, fractions=fractions)
    want = M.verlet_medium(grid, u0, v0, g, c2, tau, 5, source, receivers, 2)
    cut = lambda k: tuple(w[:k] for w in want)
    run = lambda k, **kw: fresh.wave_record_many(u0[:k], v0[:k], tau[:k], 5, source[:k], g=g[:k], receivers=receivers, record_every=2, c2=c2[:k], **kw)
    same(run(2), cut(2), 5, "two members")
    same(run(40), cut(40), 5, "forty members")                      # grown
    same(run(2), cut(2), 5, "two again")
    # the device entry point after the host's, and grown by it: the ranges of forty media
    dev = lambda k: fresh.wave_record_many(*(torch.from_numpy(np.ascontiguousarray(a[:k])).cuda() for a in (u0, v0)), tau[:k], 5, torch.from_numpy(source[:k]).cuda(),
                                           g=torch.from_numpy(g[:k]).cuda(), receivers=receivers, record_every=2, c2=torch.from_numpy(c2[:k]).cuda())
    fresh.batch_release()
    for k in (3, 40, 7):
        ut, vt, tt, rt, dt = dev(k)
        same((ut.cpu().numpy(), vt.cpu().numpy(), tt.cpu().numpy(), rt, dt), cut(k), 5, ("device", k))
    # the other ensemble calls share the workspace
    plain = fresh.wave_record_many(u0[:7], v0[:7], 0.5 * tau[:7], 5, source[:7], g=g[:7], receivers=receivers)
    same(plain, R.verlet_record(grid, u0[:7], v0[:7], g[:7], 0.5 * tau[:7], 5, source[:7], receivers, 1), 5, "the call without a medium")
    same(run(7), cut(7), 5, "after it")
    fresh.batch_release()
    fresh.batch_release()
    same(run(5), cut(5), 5, "after the release")
    # the documented formula (the allocation itself is not exposed)
    assert isa.wave_medium_many_workspace(12, 40, 5, 5, 2) == isa.wave_record_many_workspace(12, 40, 5, 5, 2) + 16 * 40
    fresh._handle.close()


def test_refusals_leave_the_handle_usable():
    import torch
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    good = _system(16)
    grid = model(good)
    size = good.size()
    u0, v0, tau, g, c2, source, receivers = ensemble(good, grid, seed=5300, nsteps=4, fractions=(1.0, 0.5, 0.2))
    want = M.verlet_medium(grid, u0, v0, g, c2, tau, 4, source, receivers, 2)
    h = good._handle._h
    nodes = np.asarray(receivers, dtype=np.int32)

    def still_good():
        same(good.wave_record_many(u0, v0, tau, 4, source, g=g, receivers=receivers, record_every=2, steps_per_launch=3, c2=c2), want, 4, "after a refusal")

    def call(handle, nsys, nsteps, tt, gg, uu, vv, cc, cstride, ww, stride, nrec, nn, every, tr, spl=0, out="res", done="done", fn=lib.mi355cg_wave_medium_many):
        ptr = lambda a: (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) if a is not None else None
        res = (_capi.Results * max(nsys, 1))() if out == "res" else None
        dn = np.full(max(nsys, 1), -7, dtype=np.int32) if done == "done" else None
        rc = fn(handle, nsys, nsteps, ptr(tt), ptr(gg), ptr(uu), ptr(vv), ptr(cc), cstride, ptr(ww), stride, nrec, ptr(nn), every, ptr(tr), spl, None, res, ptr(dn))
        return rc, lib.mi355cg_last_error().decode(), dn

    u, v, w, c = u0.copy(), v0.copy(), source.copy(), c2.copy()
    traces = np.full((3, 2, 5), -5.0)
    both = np.zeros((6, size))
    t3 = lambda *a: np.array(a, dtype=np.float64)
    bounds = good.wave_cfl(c2)
    assert np.array_equal(bounds, M.medium_cfl(grid, c2.max(axis=1))) and np.array_equal(tau, np.array([1.0, 0.5, 0.2]) * bounds)
    above = np.nextafter(bounds[2], np.inf)
    plain = good.wave_cfl()
    assert above < plain                                            # a tau the homogeneous bound allows and the member's own refuses
    cbad = lambda val: np.where(np.arange(3 * size).reshape(3, size) == size + 7, val, c2)           # one entry of member 1
    wbad = lambda val: np.where(np.arange(15).reshape(3, 5) == 7, val, source)
    ok = (h, 3, 4, tau, g, u, v, c, size, w, 5, 5, nodes, 2, traces)
    names = ("handle", "nsys", "nsteps", "tt", "gg", "uu", "vv", "cc", "cstride", "ww", "stride", "nrec", "nn", "every", "tr")

    def but(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return tuple(a[k] for k in names)

    cases = [("null c2", but(cc=None), {}, "c2"), ("c2_stride too short", but(cstride=size - 1), {}, "c2_stride"), ("c2_stride negative", but(cstride=-size), {}, "c2_stride"),
             ("c2 is u", but(cc=u), {}, "c2 overlaps u"), ("c2 in v", but(cc=v[1], cstride=0), {}, "c2 overlaps v"), ("c2 in g", but(cc=g[2], cstride=0), {}, "c2 overlaps g"),
             ("a zero in member 1", but(cc=cbad(0.0)), {}, "member 1"), ("a negative entry in member 1", but(cc=cbad(-1.0)), {}, "member 1"),
             ("a NaN in member 1", but(cc=cbad(np.nan)), {}, "member 1"), ("an infinity in member 1", but(cc=cbad(np.inf)), {}, "member 1"),
             ("a zero in the shared medium", but(cc=cbad(0.0)[1], cstride=0), {}, "one medium"),
             ("tau above the member's bound", but(tt=t3(tau[0], tau[1], above)), {}, "member 2"),
             ("tau at the homogeneous bound", but(tt=t3(plain, tau[1], tau[2])), {}, "member 0"),
             # everything the recorded call refuses
             ("nrec 65", but(nrec=65, nn=np.zeros(65, dtype=np.int32)), {}, "64"), ("receiver size", but(nn=np.array([0, 1, 2, 3, size], dtype=np.int32)), {}, f"[0, {size})"),
             ("record_every 0", but(every=0), {}, "record_every"), ("null traces", but(tr=None), {}, "traces"), ("null w", but(ww=None), {}, "amplitudes"),
             ("w_stride too short", but(stride=4), {}, "w_stride"), ("amplitude nan", but(ww=wbad(np.nan)), {}, "member 1 at step 2"),
             ("w is u", but(ww=u, stride=size), {}, "w overlaps u"), ("traces in g", but(tr=g[0]), {}, "traces overlaps g"), ("traces in w", but(tr=w[1]), {}, "traces overlaps w"),
             ("null u", but(uu=None), {}, "null"), ("null tau", but(tt=None), {}, "null"), ("null out", ok, dict(out=None), "null"),
             ("null steps_done", ok, dict(done=None), "null"), ("null handle", but(handle=None), {}, "null"),
             ("no members", but(nsys=0), {}, str(_capi.MANY_MAX)), ("negative nsteps", but(nsteps=-1), {}, "nsteps"), ("steps_per_launch", ok, dict(spl=-1), "steps_per_launch"),
             ("tau 0", but(tt=t3(tau[0], 0.0, tau[2])), {}, "tau"), ("tau nan", but(tt=t3(np.nan, tau[1], tau[2])), {}, "tau"),
             ("u is v", but(vv=u), {}, "overlaps"), ("u overlaps v", but(uu=both[:3], vv=both[1:4]), {}, "overlaps")]
    # c2 and w, c2 and the traces in one array
    cw = np.concatenate([c2.reshape(-1), source.reshape(-1)])
    cases += [("c2 meets w", but(cc=cw, ww=cw[3 * size - 2:]), {}, "c2 overlaps w"), ("c2 meets the traces", but(cc=cw, tr=cw[size:]), {}, "c2 overlaps traces")]
    for what, args, kw, text in cases:
        rc, msg, dn = call(*args, **kw)
        assert rc == _capi.ERR_INVALID and text in msg, (what, rc, msg)
        assert dn is None or (dn == -7).all(), what                 # nothing was written
        if what.startswith("tau above"):
            assert "%.17g" % bounds[2] in msg and "%.17g" % above in msg
        still_good()
    assert np.array_equal(u, u0) and np.array_equal(v, v0) and np.all(traces == -5.0) and np.array_equal(w, source) and np.array_equal(c, c2)
    # the limits themselves are taken: every member at its own bound, a wider stride, one medium for all at its bound
    rc, msg, dn = call(*but(tt=bounds.copy(), uu=u.copy(), vv=v.copy(), nrec=0, nn=None, tr=None))
    assert rc == _capi.OK and (dn == 4).all(), msg
    wide = np.ones((3, size + 3))
    wide[:, :size] = c2
    t5 = np.zeros((3, 2, 5))
    rc, msg, dn = call(*but(uu=u.copy(), vv=v.copy(), cc=wide, cstride=size + 3, tr=t5))
    assert rc == _capi.OK and (dn == 4).all() and np.array_equal(t5, want[2]), msg
    one = np.full(3, bounds[1])
    uu, vv = u.copy(), v.copy()
    rc, msg, dn = call(*but(tt=one, uu=uu, vv=vv, cc=c2[1].copy(), cstride=0, tr=t5))
    shared = M.verlet_medium(grid, u0, v0, g, c2[1], one, 4, source, receivers, 2)
    assert rc == _capi.OK and np.array_equal(uu, shared[0]) and np.array_equal(vv, shared[1]) and np.array_equal(t5, shared[2]), msg
    # the device entry point: the same checks, the media read by the check launch
    ud, vd, gd, cd, wd = (torch.from_numpy(a).cuda() for a in (u0, v0, g, c2, source))
    td = torch.full((3, 2, 5), -5.0, dtype=torch.float64).cuda()
    torch.cuda.synchronize()
    dev = lib.mi355cg_wave_medium_many_device
    okd = dict(gg=gd, uu=ud, vv=vd, cc=cd, ww=wd, tr=td)
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cwd = on(cw)
    for what, kw, text in [("null c2", dict(cc=None), "c2"), ("c2_stride", dict(cstride=5), "c2_stride"), ("c2 is u", dict(cc=ud), "c2 overlaps u"),
                           ("c2 is g", dict(cc=gd), "c2 overlaps g"), ("c2 meets w", dict(cc=cwd, ww=cwd[3 * size - 2:]), "c2 overlaps w"),
                           ("c2 meets the traces", dict(cc=cwd, tr=cwd[size:]), "c2 overlaps traces"),
                           ("a zero", dict(cc=on(cbad(0.0))), "member 1"), ("a negative entry", dict(cc=on(cbad(-2.5))), "member 1"),
                           ("a NaN", dict(cc=on(cbad(np.nan))), "member 1"), ("an infinity", dict(cc=on(cbad(-np.inf))), "member 1"),
                           ("a NaN in the shared medium", dict(cc=on(cbad(np.nan)[1]), cstride=0), "one medium"),
                           ("tau above the member's bound", dict(tt=t3(tau[0], tau[1], above)), "member 2"),
                           ("tau at the homogeneous bound", dict(tt=t3(tau[0], plain, tau[2])), "member 1"),
                           ("nrec", dict(nrec=70), "64"), ("record_every", dict(every=0), "record_every"), ("null w", dict(ww=None), "amplitudes"),
                           ("traces is g", dict(tr=gd), "traces overlaps g"), ("u is v", dict(vv=ud), "overlaps")]:
        rc, msg, dn = call(*but(**dict(okd, **kw)), fn=dev)
        assert rc == _capi.ERR_INVALID and text in msg, (what, rc, msg)
        assert (dn == -7).all(), what
        if what.startswith("tau above"):
            assert "%.17g" % bounds[2] in msg and "%.17g" % above in msg
        still_good()
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in ((ud, u0), (vd, v0), (gd, g), (cd, c2), (wd, source))) and bool((td == -5.0).all())
    rc, msg, dn = call(*but(**dict(okd, tt=bounds.copy(), uu=ud.clone(), vv=vd.clone())), fn=dev)                # every member at its own bound
    assert rc == _capi.OK and (dn == 4).all(), msg
    # the Python layer
    for kw in (dict(c2=c2[:2]), dict(c2=c2[:, :5]), dict(c2=cbad(0.0)), dict(c2=cbad(np.nan)), dict(c2=torch.from_numpy(c2)), dict(tau=t3(tau[0], tau[1], above)),
               dict(source=source[:, :4]), dict(record_every=0), dict(receivers=[0, size])):
        a = dict(u0=u0, v0=v0, tau=tau, nsteps=4, source=source, g=g, receivers=receivers, record_every=2, c2=c2)
        a.update(kw)
        with pytest.raises(ValueError):
            good.wave_record_many(**a)
        still_good()
    good._handle.close()
