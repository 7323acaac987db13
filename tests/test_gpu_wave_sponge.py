"""The recorded explicit on-chip wave stepper with a damping field: mi355cg_wave_sponge_many* integrates
u_tt + d_s o u_t = c2_s o (A u) - w_s(t) g_s for many members of one grid, one workgroup per member, the damping rate d of every
unknown given per member or once for all.  "Same" means np.array_equal on u, v and the traces: the NumPy model of
tests/wave_sponge_reference.py writes every expression operation by operation in the scheme's order, while the kernel runs the loop
rotated (both half kicks in one pass, the launch's last step cut short), so launches, chained calls and stop flags are where it
can go wrong."""
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
import wave_sponge_reference as S  # noqa: E402

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
    g = S.Grid(sys_.n, col[0], col[1], col[sys_.n // 2 - 1])
    assert g.size == sys_.size() and g.A0 == -2 * (g.xk + g.yk)
    return g


_systems = {}


def system(n):
    """(the system the ensembles run on, the NumPy grid) of a grid, created once."""
    if n not in _systems:
        s = _system(n)
        _systems[n] = (s, model(s))
    return _systems[n]


def damping_for(rng, tau, size, shared=False):
    """A seeded damping with (0.25 tau_s) d_s in [0, 1], zero on about a third of the unknowns and the bound e = 1 taken by one
    entry of every member; shared: one field, scaled by the largest tau."""
    tau = np.atleast_1d(tau)
    k = 1 if shared else len(tau)
    q = 0.25 * (np.full(1, tau.max()) if shared else tau)
    e = rng.uniform(0.0, 1.0, (k, size)) * (rng.uniform(0.0, 1.0, (k, size)) > 1.0 / 3.0)
    d = e / q[:, None]
    for s in range(k):
        d[s, 3] = 1.0 / q[s]
        while q[s] * d[s].max() > 1.0:                               # a rounding above the bound: one ulp down
            d[s] = np.where(q[s] * d[s] > 1.0, np.nextafter(d[s], 0.0), d[s])
    assert all((q[s] * d[s]).max() <= 1.0 and (q[s] * d[s]).max() > 1.0 - 1e-15 for s in range(k)) and d.min() == 0.0
    return d[0] if shared else d


def ensemble(sys_, grid, seed, nsteps, fractions=FRACTIONS, shared=False):
    """(u0, v0, tau, g, c2, d, source, receivers) of one member per fraction of ITS bound: g the right-hand side x (1 + 0.1 noise),
    u0 and v0 seeded, member 0 at rest at zero, a seeded medium in [0.25, 4] and a seeded damping per member (shared: one damping
    field for all), a seeded amplitude row per member, three seeded receivers and the two ends of the packed order."""
    rng = np.random.default_rng(seed)
    k, size = len(fractions), sys_.size()
    g = np.ascontiguousarray(sys_.get_rhs()[None, :] * (1.0 + 0.1 * rng.standard_normal((k, size))))
    u0, v0 = rng.standard_normal((k, size)), rng.standard_normal((k, size)) * np.sqrt(abs(grid.A0))
    u0[0] = v0[0] = 0.0
    c2 = rng.uniform(0.25, 4.0, (k, size))
    source = rng.standard_normal((k, nsteps + 1))
    receivers = [int(r) for r in rng.integers(0, size, 3)] + [0, size - 1]
    tau = np.asarray(fractions) * M.medium_cfl(grid, c2.max(axis=-1))
    d = damping_for(rng, tau, size, shared)
    return u0, v0, tau, g, c2, d, source, receivers


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
def test_damping_over_the_plan(n):
    """Five members with their own tau, medium, damping, g and source, 23 steps sampled every 3rd in launches of 5."""
    n = _cap() if n == "cap" else n
    many, grid = system(n)
    u0, v0, tau, g, c2, d, source, receivers = ensemble(many, grid, seed=6000 + n, nsteps=23)
    assert receivers[3:] == [0, many.size() - 1] and d.shape == c2.shape == (5, many.size())
    got = many.wave_record_many(u0, v0, tau, 23, source, g=g, receivers=receivers, record_every=3, steps_per_launch=5, c2=c2, damping=d)
    assert got[2].shape == (5, 7, 5)
    same(got, S.verlet_sponge(grid, u0, v0, g, c2, d, tau, 23, source, receivers, 3), 23, ("plan", n))
    assert not np.array_equal(got[0], u0)
    assert not np.array_equal(got[1], many.wave_record_many(u0, v0, tau, 23, source, g=g, c2=c2)[1])     # the damping was felt


@pytest.mark.parametrize("n", [6, 20, "cap"])
def test_one_step_and_launches_of_one_step(n):
    """nsteps = 1: the entry pass, one drift, the closing damp and nothing else.  Launches of one step: every step is a launch's
    last."""
    n = _cap() if n == "cap" else n
    many, grid = system(n)
    u0, v0, tau, g, c2, d, source, receivers = ensemble(many, grid, seed=6100 + n, nsteps=7)
    for spl in (0, 1, 4):
        got = many.wave_record_many(u0, v0, tau, 1, np.ascontiguousarray(source[:, :2]), g=g, receivers=receivers, steps_per_launch=spl, c2=c2, damping=d)
        same(got, S.verlet_sponge(grid, u0, v0, g, c2, d, tau, 1, source[:, :2], receivers, 1), 1, ("one step", n, spl))
    got = many.wave_record_many(u0, v0, tau, 7, source, g=g, receivers=receivers, record_every=2, steps_per_launch=1, c2=c2, damping=d)
    same(got, S.verlet_sponge(grid, u0, v0, g, c2, d, tau, 7, source, receivers, 2), 7, ("launches of one step", n))


@pytest.mark.parametrize("n", [10, "cap"])
def test_runs_longer_than_an_amplitude_block(n):
    """150 steps in one launch: the staging of the amplitudes wraps its two blocks; then launches of 100 and 64."""
    n = _cap() if n == "cap" else n
    many, grid = system(n)
    u0, v0, tau, g, c2, d, source, receivers = ensemble(many, grid, seed=6200 + n, nsteps=150)
    want = S.verlet_sponge(grid, u0, v0, g, c2, d, tau, 150, source, receivers, 7)
    assert want[2].shape == (5, 21, 5) and np.all(np.isfinite(want[0]))
    run = lambda **kw: many.wave_record_many(u0, v0, tau, 150, source, g=g, receivers=receivers, record_every=7, c2=c2, damping=d, **kw)
    same(run(), want, 150, ("one launch", n))
    same(run(steps_per_launch=100), want, 150, ("launches of 100", n))
    same(run(steps_per_launch=64), want, 150, ("launches of 64", n))


def test_chained_calls_are_one_call():
    many, grid = system(20)
    u0, v0, tau, g, c2, d, source, receivers = ensemble(many, grid, seed=6300, nsteps=24)
    whole = many.wave_record_many(u0, v0, tau, 24, source, g=g, receivers=receivers, record_every=3, c2=c2, damping=d)
    same(whole, S.verlet_sponge(grid, u0, v0, g, c2, d, tau, 24, source, receivers, 3), 24, "whole")
    u, v, at, parts = u0, v0, 0, []
    for k in (9, 3, 12):                                            # multiples of the cadence
        u, v, traces, res, done = many.wave_record_many(u, v, tau, k, np.ascontiguousarray(source[:, at:at + k + 1]), g=g, receivers=receivers,
                                                        record_every=3, steps_per_launch=4, c2=c2, damping=d)
        assert [int(x) for x in done] == [k] * 5
        parts.append(traces)
        at += k
    assert np.array_equal(u, whole[0]) and np.array_equal(v, whole[1]) and np.array_equal(np.concatenate(parts, axis=1), whole[2])
    # nsteps = 0 writes only steps_done = 0
    u, v, traces, res, done = many.wave_record_many(u0, v0, tau, 0, source[:, :1], g=g, receivers=receivers, c2=c2, damping=d)
    assert np.array_equal(u, u0) and np.array_equal(v, v0) and traces.shape == (5, 0, 5) and not done.any()


@pytest.mark.parametrize("n", [10, 64])
def test_no_damping_is_the_call_with_the_medium_only(n):
    many, grid = system(n)
    u0, v0, tau, g, c2, _, source, receivers = ensemble(many, grid, seed=6400 + n, nsteps=70)
    medium = many.wave_record_many(u0, v0, tau, 70, source, g=g, receivers=receivers, record_every=4, steps_per_launch=33, c2=c2)
    for d in (np.zeros(many.size()), np.zeros((5, many.size()))):
        got = many.wave_record_many(u0, v0, tau, 70, source, g=g, receivers=receivers, record_every=4, steps_per_launch=20, c2=c2, damping=d)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], medium[:3])) and [int(x) for x in got[4]] == [70] * 5
    assert np.array_equal(medium[0], M.verlet_medium(grid, u0, v0, g, c2, tau, 70, source)[0])


def test_damping_without_a_medium_is_a_unit_medium():
    import torch
    many, grid = system(12)
    u0, v0, tau, g, _, d, source, receivers = ensemble(many, grid, seed=6500, nsteps=19)
    tau = np.asarray(FRACTIONS) * many.wave_cfl()
    d = damping_for(np.random.default_rng(6501), tau, many.size())
    alone = many.wave_record_many(u0, v0, tau, 19, source, g=g, receivers=receivers, record_every=2, steps_per_launch=6, damping=d)
    unit = many.wave_record_many(u0, v0, tau, 19, source, g=g, receivers=receivers, record_every=2, steps_per_launch=6, c2=np.ones((5, many.size())), damping=d)
    assert all(np.array_equal(a, b) for a, b in zip(alone[:3], unit[:3]))
    same(alone, S.verlet_sponge(grid, u0, v0, g, np.ones(many.size()), d, tau, 19, source, receivers, 2), 19, "damping alone")
    ut, vt, tt, rt, dt = many.wave_record_many(*(torch.from_numpy(a).cuda() for a in (u0, v0)), tau, 19, torch.from_numpy(source).cuda(), g=torch.from_numpy(g).cuda(),
                                               receivers=receivers, record_every=2, damping=torch.from_numpy(d).cuda())
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip((ut, vt, tt), alone[:3]))


def test_a_shared_damping():
    many, grid = system(30)
    u0, v0, tau, g, c2, d, source, receivers = ensemble(many, grid, seed=6600, nsteps=9, shared=True)
    assert d.shape == (many.size(),) and c2.shape == (5, many.size())
    got = many.wave_record_many(u0, v0, tau, 9, source, g=g, receivers=receivers, steps_per_launch=4, c2=c2, damping=d)
    same(got, S.verlet_sponge(grid, u0, v0, g, c2, d, tau, 9, source, receivers, 1), 9, "shared damping")
    # the same field once per member: the same bits
    again = many.wave_record_many(u0, v0, tau, 9, source, g=g, receivers=receivers, c2=c2, damping=np.ascontiguousarray(np.stack([d] * 5)))
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3]))
    # g = None, a shared medium and source row, no receivers
    tiled = np.ascontiguousarray(np.stack([many.get_rhs()] * 5))
    low = np.full(5, tau.min())
    same(many.wave_record_many(u0, v0, low, 9, source[2], c2=c2[1], damping=d), S.verlet_sponge(grid, u0, v0, tiled, c2[1], d, low, 9, source[2]), 9, "g = None")


def test_a_sponge_layer_absorbs():
    """sponge_damping on all sides of N = 64, twelve nodes wide: a pulse from a point source leaves the grid; without the layer it
    stays.  Bit for bit the model's, and the system's helper is the module's."""
    import iterative_solvers_amd as isa
    many, grid = system(64)
    size = many.size()
    tau = 0.9 * many.wave_cfl()
    d = many.sponge_damping(12, 0.5 / tau)
    assert np.array_equal(d, isa.sponge_damping(64, 12, 0.5 / tau)) and d.shape == (size,) and d.max() == 0.5 / tau and (d == 0).sum() > size // 4
    g = np.zeros((1, size))
    g[0, many.packed_index(44, 44)] = -1.0
    zero = np.zeros((1, size))
    source = np.zeros(301)
    source[:41] = np.sin(np.pi * np.arange(41) / 40) ** 2
    receivers = [many.packed_index(44, 50), many.packed_index(20, 44)]
    got = many.wave_record_many(zero, zero, np.array([tau]), 300, source, g=g, receivers=receivers, record_every=5, damping=d)
    same(got, S.verlet_sponge(grid, zero, zero, g, np.ones(size), d, np.array([tau]), 300, source, receivers, 5), 300, "sponge layer")
    free = many.wave_record_many(zero, zero, np.array([tau]), 300, source, g=g, receivers=receivers, record_every=5)
    energy = lambda r: M.plain_energy(grid, r[0][0], r[1][0], np.ones(size))
    print("energy left with the layer / without", energy(got) / energy(free))
    assert np.abs(got[2]).max() > 0 and energy(got) < 0.5 * energy(free)


def test_a_stretched_domain():
    s = _system(20, domain=STRETCHED)
    grid = model(s)
    assert grid.xk != grid.yk
    u0, v0, tau, g, c2, d, source, receivers = ensemble(s, grid, seed=6700, nsteps=23)
    same(s.wave_record_many(u0, v0, tau, 23, source, g=g, receivers=receivers, record_every=3, steps_per_launch=5, c2=c2, damping=d),
         S.verlet_sponge(grid, u0, v0, g, c2, d, tau, 23, source, receivers, 3), 23, "stretched")
    s._handle.close()


def test_more_members_than_are_resident_at_once():
    nsys = 9000
    many, grid = system(6)
    rng = np.random.default_rng(6800)
    size = many.size()
    g = many.get_rhs()[None, :] * (1.0 + 0.1 * rng.standard_normal((nsys, 1)))
    u0, v0 = rng.standard_normal((nsys, size)), rng.standard_normal((nsys, size)) * np.sqrt(abs(grid.A0))
    c2 = rng.uniform(0.25, 4.0, (nsys, size))
    tau = M.medium_cfl(grid, c2.max(axis=1)) * rng.uniform(0.1, 1.0, nsys)
    d = rng.uniform(0.0, 1.0, (nsys, size)) * (rng.uniform(0.0, 1.0, (nsys, size)) > 1.0 / 3.0) * 0.999 / (0.25 * tau[:, None])
    source = rng.standard_normal((nsys, 8))
    receivers = [0, 3, size - 1]
    same(many.wave_record_many(u0, v0, tau, 7, source, g=g, receivers=receivers, record_every=2, steps_per_launch=3, c2=c2, damping=d),
         S.verlet_sponge(grid, u0, v0, g, c2, d, tau, 7, source, receivers, 2), 7, ("many", nsys))
    many.batch_release()


def test_device_tensors():
    """CUDA tensors: the media and the damping rows are reduced by the check launch, k_oc_medium_range, not on the host."""
    import torch
    many, grid = system(20)
    u0, v0, tau, g, c2, d, source, receivers = ensemble(many, grid, seed=6900, nsteps=11)
    ud, vd, gd, cd, dd, sd = (torch.from_numpy(a).cuda() for a in (u0, v0, g, c2, d, source))
    want = S.verlet_sponge(grid, u0, v0, g, c2, d, tau, 11, source, receivers, 2)
    ut, vt, tt, rt, dt = many.wave_record_many(ud, vd, tau, 11, sd, g=gd, receivers=receivers, record_every=2, steps_per_launch=4, c2=cd, damping=dd)
    assert ut.is_cuda and vt.is_cuda and tt.is_cuda and ut.data_ptr() != ud.data_ptr() and vt.data_ptr() != vd.data_ptr() and tuple(tt.shape) == (5, 5, 5)
    same((ut.cpu().numpy(), vt.cpu().numpy(), tt.cpu().numpy(), rt, dt), want, 11, "device")
    # one damping field and one medium for all, no receivers, g = None; the smallest tau holds for every member
    tiled = np.ascontiguousarray(np.stack([many.get_rhs()] * 5))
    low = np.full(5, tau.min())
    ut, vt, tt, rt, dt = many.wave_record_many(ud, vd, low, 11, sd[1].contiguous(), c2=cd[3].contiguous(), damping=dd[0].contiguous())
    assert tt is None
    same((ut.cpu().numpy(), vt.cpu().numpy(), None, rt, dt), S.verlet_sponge(grid, u0, v0, tiled, c2[3], d[0], low, 11, source[1]), 11, "device, shared")
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in ((ud, u0), (vd, v0), (gd, g), (cd, c2), (dd, d), (sd, source)))
    for bad in (dict(damping=d), dict(damping=dd[:, :5].contiguous()), dict(damping=dd[:2].contiguous()), dict(damping=dd.float())):
        a = dict(u0=ud, v0=vd, tau=tau, nsteps=11, source=sd, g=gd, receivers=receivers, record_every=2, c2=cd, damping=dd)
        a.update(bad)
        with pytest.raises(ValueError):
            many.wave_record_many(**a)


def test_stop_flag():
    """Raised before the call: nothing runs and nothing is written.  Raised by another thread while the call runs, it ends the call
    between two launches -- wherever that is, steps_done is a whole number of launches, (u, v) the model's state at that step (v
    behind its closing damp), the samples of the steps that ran the model's and all others the caller's sentinel.  A call that
    ended before the flag came satisfies the same statement with steps_done = nsteps."""
    from iterative_solvers_amd import _capi
    many, grid = system(10)
    nsteps, every, per_launch = 6000, 7, 20
    u0, v0, tau, g, c2, d, source, receivers = ensemble(many, grid, seed=7000, nsteps=nsteps)
    source = 0.1 * source
    sentinel = -12345.0
    blank = lambda: np.full((5, nsteps // every, 5), sentinel)
    traces = blank()
    u, v, tr, res, done = many.wave_record_many(u0, v0, tau, nsteps, source, g=g, receivers=receivers, record_every=every, steps_per_launch=per_launch,
                                                stop_flag=C.c_int(1), traces=traces, c2=c2, damping=d)
    assert tr is traces and np.array_equal(u, u0) and np.array_equal(v, v0) and not done.any() and np.all(traces == sentinel)
    assert [(r.iterations, r.stop_reason, r.converged) for r in res] == [(0, _capi.STOP_INTERRUPTED, 0)] * 5
    # the model's state after every launch
    states, u, v = [(u0, v0)], u0, v0
    for lo in range(0, nsteps, per_launch):
        u, v, _ = S.verlet_sponge(grid, u, v, g, c2, d, tau, per_launch, source[:, lo:lo + per_launch + 1])
        states.append((u, v))
    whole = S.verlet_sponge(grid, u0, v0, g, c2, d, tau, nsteps, source, receivers, every)
    assert np.array_equal(states[-1][0], whole[0]) and np.all(np.isfinite(whole[0])) and len(states) == nsteps // per_launch + 1
    seen = set()
    for delay in (0.001, 0.003, 0.006):
        flag, traces = C.c_int(0), blank()
        timer = threading.Timer(delay, lambda: setattr(flag, "value", 1))
        timer.start()
        u, v, tr, res, done = many.wave_record_many(u0, v0, tau, nsteps, source, g=g, receivers=receivers, record_every=every,
                                                    steps_per_launch=per_launch, stop_flag=flag, traces=traces, c2=c2, damping=d)
        timer.cancel()
        timer.join()
        k = int(done[0])
        print("flag after", delay, "s: steps_done", k)
        seen.add("whole" if k == nsteps else "stopped")
        assert [int(x) for x in done] == [k] * 5 and k % per_launch == 0 and 0 <= k <= nsteps
        assert np.array_equal(u, states[k // per_launch][0]) and np.array_equal(v, states[k // per_launch][1]), k
        assert np.array_equal(tr[:, :k // every], whole[2][:, :k // every]) and np.all(tr[:, k // every:] == sentinel), k
        assert all(r.stop_reason == _capi.STOP_INTERRUPTED and r.converged == 0 for r in res) == (k < nsteps)
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
        u0, v0, tau, g, c2, d, source, receivers = ensemble(s, grid, seed=7100, nsteps=5)
        same(s.wave_record_many(u0, v0, tau, 5, source, receivers=receivers, c2=c2, damping=d),
             S.verlet_sponge(grid, u0, v0, np.stack([rhs] * 5), c2, d, tau, 5, source, receivers, 1), 5, "unshifted A, the handle's g")
        assert np.array_equal(h.solution(), x) and np.array_equal(h.recursive_residual(), r) and np.array_equal(h.rhs(), rhs)
        assert h.get_shift() == shift and s.solve_mode_info()["mode"] == mode
        assert fields(h.solve(p, None, None)) == first              # cold: the ensemble left no pending guess behind
        assert np.array_equal(h.solution(), x) and np.array_equal(h.recursive_residual(), r)
        guess = np.random.default_rng(18).standard_normal(s.size())
        h.set_initial_guess(guess)
        warm = fields(h.solve(p, None, None))
        xw = h.solution()
        h.set_initial_guess(guess)
        s.wave_record_many(u0, v0, tau, 3, source[:, :4], g=g, receivers=receivers, c2=c2, damping=d)
        assert fields(h.solve(p, None, None)) == warm and np.array_equal(h.solution(), xw)
    h.close()


def test_workspace_lifetime():
    import iterative_solvers_amd as isa
    import torch
    _, grid = system(12)
    fresh = _system(12)
    fresh.batch_release()                                            # nothing allocated: fine
    fractions = tuple(0.1 + 0.9 * (s + 1) / 40 for s in range(40))
    u0, v0, tau, g, c2, d, source, receivers = ensemble(fresh, grid, seed=7200, nsteps=5, fractions=fractions)
    want = S.verlet_sponge(grid, u0, v0, g, c2, d, tau, 5, source, receivers, 2)
    cut = lambda k: tuple(w[:k] for w in want)
    run = lambda k, **kw: fresh.wave_record_many(u0[:k], v0[:k], tau[:k], 5, source[:k], g=g[:k], receivers=receivers, record_every=2, c2=c2[:k], damping=d[:k], **kw)
    same(run(2), cut(2), 5, "two members")
    same(run(40), cut(40), 5, "forty members")                      # grown
    same(run(2), cut(2), 5, "two again")
    # the device entry point after the host's, and grown by it: the ranges of forty media and damping rows
    on = lambda a, k: torch.from_numpy(np.ascontiguousarray(a[:k])).cuda()
    dev = lambda k: fresh.wave_record_many(on(u0, k), on(v0, k), tau[:k], 5, on(source, k), g=on(g, k), receivers=receivers, record_every=2, c2=on(c2, k), damping=on(d, k))
    fresh.batch_release()
    for k in (3, 40, 7):
        ut, vt, tt, rt, dt = dev(k)
        same((ut.cpu().numpy(), vt.cpu().numpy(), tt.cpu().numpy(), rt, dt), cut(k), 5, ("device", k))
    # the other ensemble calls share the workspace
    medium = fresh.wave_record_many(u0[:7], v0[:7], tau[:7], 5, source[:7], g=g[:7], receivers=receivers, c2=c2[:7])
    same(medium, M.verlet_medium(grid, u0[:7], v0[:7], g[:7], c2[:7], tau[:7], 5, source[:7], receivers, 1), 5, "the call without a damping")
    same(run(7), cut(7), 5, "after it")
    fresh.batch_release()
    fresh.batch_release()
    same(run(5), cut(5), 5, "after the release")
    # the documented formula (the allocation itself is not exposed)
    assert isa.wave_sponge_many_workspace(12, 40, 5, 5, 2) == isa.wave_medium_many_workspace(12, 40, 5, 5, 2) + 16 * 40
    fresh._handle.close()


def test_refusals_leave_the_handle_usable():
    import torch
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    good = _system(16)
    grid = model(good)
    size = good.size()
    u0, v0, tau, g, c2, d, source, receivers = ensemble(good, grid, seed=7300, nsteps=4, fractions=(1.0, 0.5, 0.2))
    want = S.verlet_sponge(grid, u0, v0, g, c2, d, tau, 4, source, receivers, 2)
    h = good._handle._h
    nodes = np.asarray(receivers, dtype=np.int32)

    def still_good():
        same(good.wave_record_many(u0, v0, tau, 4, source, g=g, receivers=receivers, record_every=2, steps_per_launch=3, c2=c2, damping=d), want, 4, "after a refusal")

    def call(handle, nsys, nsteps, tt, gg, uu, vv, cc, cstride, dd, dstride, ww, stride, nrec, nn, every, tr, spl=0, out="res", done="done", fn=lib.mi355cg_wave_sponge_many):
        ptr = lambda a: (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) if a is not None else None
        res = (_capi.Results * max(nsys, 1))() if out == "res" else None
        dn = np.full(max(nsys, 1), -7, dtype=np.int32) if done == "done" else None
        rc = fn(handle, nsys, nsteps, ptr(tt), ptr(gg), ptr(uu), ptr(vv), ptr(cc), cstride, ptr(dd), dstride, ptr(ww), stride, nrec, ptr(nn), every, ptr(tr), spl, None,
                res, ptr(dn))
        return rc, lib.mi355cg_last_error().decode(), dn

    u, v, w, c, dm = u0.copy(), v0.copy(), source.copy(), c2.copy(), d.copy()
    traces = np.full((3, 2, 5), -5.0)
    t3 = lambda *a: np.array(a, dtype=np.float64)
    bounds = good.wave_cfl(c2)
    dbad = lambda val: np.where(np.arange(3 * size).reshape(3, size) == size + 7, val, d)            # one entry of member 1
    cbad = lambda val: np.where(np.arange(3 * size).reshape(3, size) == 2 * size + 7, val, c2)       # one entry of member 2
    above = np.nextafter(4.0 / tau[1], np.inf)
    while (0.25 * tau[1]) * above <= 1.0:
        above = np.nextafter(above, np.inf)
    ok = (h, 3, 4, tau, g, u, v, c, size, dm, size, w, 5, 5, nodes, 2, traces)
    names = ("handle", "nsys", "nsteps", "tt", "gg", "uu", "vv", "cc", "cstride", "dd", "dstride", "ww", "stride", "nrec", "nn", "every", "tr")

    def but(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return tuple(a[k] for k in names)

    cases = [("null d", but(dd=None), {}, "d, the damping"), ("d_stride too short", but(dstride=size - 1), {}, "d_stride"), ("d_stride negative", but(dstride=-size), {}, "d_stride"),
             ("d is u", but(dd=u), {}, "d overlaps u"), ("d in v", but(dd=v[1], dstride=0), {}, "d overlaps v"), ("d in g", but(dd=g[2], dstride=0), {}, "d overlaps g"),
             ("d in c2", but(dd=c[0], dstride=0), {}, "d overlaps c2"),
             ("a negative entry in member 1", but(dd=dbad(-1e-300)), {}, "member 1"), ("a NaN in member 1", but(dd=dbad(np.nan)), {}, "member 1"),
             ("an infinity in member 1", but(dd=dbad(np.inf)), {}, "member 1"), ("tau d above the bound in member 1", but(dd=dbad(above)), {}, "member 1"),
             ("a negative entry in the shared field", but(dd=dbad(-1.0)[1], dstride=0), {}, "one damping field"),
             # everything the call in a medium refuses
             ("null c2", but(cc=None), {}, "c2"), ("c2_stride too short", but(cstride=size - 1), {}, "c2_stride"), ("c2 is u", but(cc=u), {}, "c2 overlaps u"),
             ("a zero in the medium of member 2", but(cc=cbad(0.0)), {}, "member 2"), ("a NaN in the medium of member 2", but(cc=cbad(np.nan)), {}, "member 2"),
             ("tau above the member's bound", but(tt=t3(tau[0], tau[1], np.nextafter(bounds[2], np.inf))), {}, "member 2"),
             ("nrec 65", but(nrec=65, nn=np.zeros(65, dtype=np.int32)), {}, "64"), ("record_every 0", but(every=0), {}, "record_every"),
             ("null traces", but(tr=None), {}, "traces"), ("null w", but(ww=None), {}, "amplitudes"), ("w_stride too short", but(stride=4), {}, "w_stride"),
             ("null u", but(uu=None), {}, "null"), ("null tau", but(tt=None), {}, "null"), ("null out", ok, dict(out=None), "null"),
             ("null steps_done", ok, dict(done=None), "null"), ("null handle", but(handle=None), {}, "null"),
             ("no members", but(nsys=0), {}, str(_capi.MANY_MAX)), ("negative nsteps", but(nsteps=-1), {}, "nsteps"), ("steps_per_launch", ok, dict(spl=-1), "steps_per_launch"),
             ("tau 0", but(tt=t3(tau[0], 0.0, tau[2])), {}, "tau"), ("u is v", but(vv=u), {}, "overlaps")]
    # d and w, d and the traces in one array
    dw = np.concatenate([d.reshape(-1), source.reshape(-1)])
    cases += [("d meets w", but(dd=dw, ww=dw[3 * size - 2:]), {}, "d overlaps w"), ("d meets the traces", but(dd=dw, tr=dw[size:]), {}, "d overlaps traces")]
    for what, args, kw, text in cases:
        rc, msg, dn = call(*args, **kw)
        assert rc == _capi.ERR_INVALID and text in msg, (what, rc, msg)
        assert dn is None or (dn == -7).all(), what                 # nothing was written
        if what.startswith("tau d above"):
            assert "%.17g" % (4.0 / tau[1]) in msg and "%.17g" % above in msg
        still_good()
    assert np.array_equal(u, u0) and np.array_equal(v, v0) and np.all(traces == -5.0) and np.array_equal(w, source) and np.array_equal(c, c2) and np.array_equal(dm, d)
    # the limits themselves are taken: e = 1 in every member (the ensemble's), a wider stride, one field for all
    assert all(((0.25 * tau[s]) * d[s]).max() > 1.0 - 1e-15 for s in range(3))
    wide = np.zeros((3, size + 3))
    wide[:, :size] = d
    t5 = np.zeros((3, 2, 5))
    rc, msg, dn = call(*but(uu=u.copy(), vv=v.copy(), dd=wide, dstride=size + 3, tr=t5))
    assert rc == _capi.OK and (dn == 4).all() and np.array_equal(t5, want[2]), msg
    uu, vv = u.copy(), v.copy()
    rc, msg, dn = call(*but(uu=uu, vv=vv, dd=d[0].copy(), dstride=0, tr=t5))                          # member 0 has the largest tau
    shared = S.verlet_sponge(grid, u0, v0, g, c2, d[0], tau, 4, source, receivers, 2)
    assert rc == _capi.OK and np.array_equal(uu, shared[0]) and np.array_equal(vv, shared[1]) and np.array_equal(t5, shared[2]), msg
    # the device entry point: the same checks, the media and the damping rows read by the check launch
    ud, vd, gd, cd, dd_, wd = (torch.from_numpy(a).cuda() for a in (u0, v0, g, c2, d, source))
    td = torch.full((3, 2, 5), -5.0, dtype=torch.float64).cuda()
    torch.cuda.synchronize()
    dev = lib.mi355cg_wave_sponge_many_device
    okd = dict(gg=gd, uu=ud, vv=vd, cc=cd, dd=dd_, ww=wd, tr=td)
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dwd = on(dw)
    for what, kw, text in [("null d", dict(dd=None), "d, the damping"), ("d_stride", dict(dstride=5), "d_stride"), ("d is u", dict(dd=ud), "d overlaps u"),
                           ("d is g", dict(dd=gd), "d overlaps g"), ("d is c2", dict(dd=cd), "d overlaps c2"), ("d meets w", dict(dd=dwd, ww=dwd[3 * size - 2:]), "d overlaps w"),
                           ("d meets the traces", dict(dd=dwd, tr=dwd[size:]), "d overlaps traces"),
                           ("a negative entry", dict(dd=on(dbad(-2.5))), "member 1"), ("a NaN", dict(dd=on(dbad(np.nan))), "member 1"),
                           ("an infinity", dict(dd=on(dbad(np.inf))), "member 1"), ("tau d above the bound", dict(dd=on(dbad(above))), "member 1"),
                           ("a NaN in the shared field", dict(dd=on(dbad(np.nan)[1]), dstride=0), "one damping field"),
                           ("a zero in the medium", dict(cc=on(cbad(0.0))), "member 2"),
                           ("tau above the member's bound", dict(tt=t3(tau[0], tau[1], np.nextafter(bounds[2], np.inf))), "member 2"),
                           ("nrec", dict(nrec=70), "64"), ("record_every", dict(every=0), "record_every"), ("null w", dict(ww=None), "amplitudes"),
                           ("u is v", dict(vv=ud), "overlaps")]:
        rc, msg, dn = call(*but(**dict(okd, **kw)), fn=dev)
        assert rc == _capi.ERR_INVALID and text in msg, (what, rc, msg)
        assert (dn == -7).all(), what
        if what.startswith("tau d above"):
            assert "%.17g" % (4.0 / tau[1]) in msg and "%.17g" % above in msg
        still_good()
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in ((ud, u0), (vd, v0), (gd, g), (cd, c2), (dd_, d), (wd, source))) and bool((td == -5.0).all())
    uc, vc = ud.clone(), vd.clone()
    rc, msg, dn = call(*but(**dict(okd, uu=uc, vv=vc)), fn=dev)                                         # e = 1 in every member
    assert rc == _capi.OK and (dn == 4).all() and np.array_equal(uc.cpu().numpy(), want[0]) and np.array_equal(vc.cpu().numpy(), want[1]), msg
    # the Python layer
    for kw in (dict(damping=d[:2]), dict(damping=d[:, :5]), dict(damping=dbad(-1.0)), dict(damping=dbad(np.nan)), dict(damping=dbad(np.inf)), dict(damping=dbad(above)),
               dict(damping=torch.from_numpy(d)), dict(c2=cbad(0.0)), dict(source=source[:, :4]), dict(record_every=0)):
        a = dict(u0=u0, v0=v0, tau=tau, nsteps=4, source=source, g=g, receivers=receivers, record_every=2, c2=c2, damping=d)
        a.update(kw)
        with pytest.raises(ValueError):
            good.wave_record_many(**a)
        still_good()
    good._handle.close()
