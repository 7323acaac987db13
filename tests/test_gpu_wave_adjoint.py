"""The adjoint of the recorded explicit on-chip wave stepper in a medium: mi355cg_wave_history_many* is
the forward run of mi355cg_wave_medium_many* that also writes H[n] = au(u_n), mi355cg_wave_adjoint_many* the exact transpose of
its steps, wave_gradient_many the least-squares gradient made of the two.  "Same" means np.array_equal: the NumPy model of
tests/wave_adjoint_reference.py writes every expression operation by operation in the kernels' order."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from onchip_support import fields, params  # noqa: E402
from onchip_support import cap as _cap, system as _system  # noqa: E402
import wave_adjoint_reference as A  # noqa: E402
import wave_medium_reference as M  # noqa: E402

pytestmark = pytest.mark.gpu

STRETCHED = (0.0, 1.0, 0.0, 1.7)
SIZES = [6, 10, 12, 20, 30, 64, 100, "cap"]         # test_gpu_wave_medium.py's: every workgroup size and unroll class (asserted below)
FRACTIONS = (1.0, 0.77, 0.5, 0.31, 0.13)            # tau_s / the member's own bound


def model(sys_):
    """The NumPy grid of a system, its coefficients read from the operator itself (as tests/test_gpu_wave_medium.py does)."""
    e = np.zeros(sys_.size())
    e[0] = 1.0
    col = sys_.apply(e)
    g = A.Grid(sys_.n, col[0], col[1], col[sys_.n // 2 - 1])
    assert g.size == sys_.size() and g.A0 == -2 * (g.xk + g.yk)
    return g


_systems = {}


def system(n):
    if n not in _systems:
        s = _system(n)
        _systems[n] = (s, model(s))
    return _systems[n]


def ensemble(sys_, grid, seed, nsteps, every, fractions=FRACTIONS, shared=False):
    """(u0, v0, tau, g, c2, source, receivers, adj): test_gpu_wave_medium.py's ensemble -- one member per fraction of ITS bound, a
    seeded medium in [0.25, 4] per member (or one for all), three seeded receivers and the two ends of the packed order -- and a
    seeded adjoint source per member."""
    rng = np.random.default_rng(seed)
    k, size = len(fractions), sys_.size()
    g = np.ascontiguousarray(sys_.get_rhs()[None, :] * (1.0 + 0.1 * rng.standard_normal((k, size))))
    u0, v0 = rng.standard_normal((k, size)), rng.standard_normal((k, size)) * np.sqrt(abs(grid.A0))
    u0[0] = v0[0] = 0.0
    c2 = rng.uniform(0.25, 4.0, size if shared else (k, size))
    source = rng.standard_normal((k, nsteps + 1))
    receivers = [int(r) for r in rng.integers(0, size, 3)] + [0, size - 1]
    tau = np.asarray(fractions) * M.medium_cfl(grid, c2.max(axis=-1))
    adj = rng.standard_normal((k, nsteps // every, len(receivers)))
    return u0, v0, tau, g, c2, source, receivers, adj


def same(got, want, what):
    for name, a, b in zip(("lam", "q", "S"), got, want):
        if not np.array_equal(a, b):
            print(what, name, "max |difference|", float(np.max(np.abs(a - b))), "of", float(np.max(np.abs(b))))
        assert np.array_equal(a, b), (what, name)


def test_the_sizes_below_cover_every_shape_of_the_plan():
    import iterative_solvers_amd as isa
    plans = [isa.onchip_plan(_cap() if n == "cap" else n) for n in SIZES]
    assert {p["threads"] for p in plans} == {64, 128, 256, 512}
    assert {p["elems_per_thread"] for p in plans} == {1, 2, 4, 8, 16, 24}
    assert _cap() == 128


@pytest.mark.parametrize("n", SIZES)
def test_history_and_adjoint_over_the_plan(n):
    """Five members with their own tau, medium and adjoint source, 23 steps sampled every 3rd (3 does not divide 23) in launches
    of 5: the history call has the bits of wave_record_many(c2=) and the model's H, the adjoint call the model's lam, q, S."""
    n = _cap() if n == "cap" else n
    many, grid = system(n)
    u0, v0, tau, g, c2, source, receivers, adj = ensemble(many, grid, seed=6000 + n, nsteps=23, every=3)
    assert receivers[3:] == [0, many.size() - 1] and adj.shape == (5, 7, 5)
    plain = many.wave_record_many(u0, v0, tau, 23, source, g=g, receivers=receivers, record_every=3, steps_per_launch=5, c2=c2)
    u, v, traces, hist, res, done = many.wave_history_many(u0, v0, tau, 23, source, g=g, receivers=receivers, record_every=3, steps_per_launch=5, c2=c2)
    assert np.array_equal(u, plain[0]) and np.array_equal(v, plain[1]) and np.array_equal(traces, plain[2]) and [int(d) for d in done] == [23] * 5
    want = A.verlet_history(grid, u0, v0, g, c2, tau, 23, source, receivers, 3)
    assert np.array_equal(u, want[0]) and np.array_equal(v, want[1]) and np.array_equal(traces, want[2])
    assert hist.shape == (5, 24, many.size()) and np.array_equal(hist, want[3])
    lam, q, S, res, done = many.wave_adjoint_many(hist, tau, c2, adj, receivers=receivers, record_every=3, steps_per_launch=5, return_info=True)
    same((lam, q, S), A.adjoint(grid, want[3], c2, tau, adj, receivers, 3), ("plan", n))
    assert [int(d) for d in done] == [23] * 5 and all((r.iterations, r.converged) == (0, 1) for r in res)
    assert np.abs(S).max() > 0 and np.abs(lam).max() > 0


def test_chained_calls_and_launches_are_invisible():
    many, grid = system(20)
    u0, v0, tau, g, c2, source, receivers, adj = ensemble(many, grid, seed=6100, nsteps=24, every=3)
    hist = many.wave_history_many(u0, v0, tau, 24, source, g=g, receivers=receivers, record_every=3, c2=c2)[3]
    rng = np.random.default_rng(6101)
    start = tuple(rng.standard_normal((5, many.size())) for _ in range(3))          # a state that is not zero
    for lam0, q0, S0 in ((None, None, None), start):
        want = A.adjoint(grid, hist, c2, tau, adj, receivers, 3, lam0, q0, S0)
        whole = many.wave_adjoint_many(hist, tau, c2, adj, receivers=receivers, record_every=3, lam=lam0, q=q0, sens=S0)
        same(whole, want, "one call")
        for per_launch in (1, 4, 24):
            same(many.wave_adjoint_many(hist, tau, c2, adj, receivers=receivers, record_every=3, lam=lam0, q=q0, sens=S0, steps_per_launch=per_launch), want,
                 ("launches of", per_launch))
        # backwards, the last 9 steps first: states 15 .. 24 and the samples of steps 18, 21, 24; then states 0 .. 15
        first = many.wave_adjoint_many(np.ascontiguousarray(hist[:, 15:]), tau, c2, np.ascontiguousarray(adj[:, 5:]), receivers=receivers, record_every=3,
                                       lam=lam0, q=q0, sens=S0, steps_per_launch=4)
        second = many.wave_adjoint_many(np.ascontiguousarray(hist[:, :16]), tau, c2, np.ascontiguousarray(adj[:, :5]), receivers=receivers, record_every=3,
                                        lam=first[0], q=first[1], sens=first[2], steps_per_launch=4)
        same(second, want, "9 + 15")
    again = np.random.default_rng(6101)
    assert all(np.array_equal(a, again.standard_normal((5, many.size()))) for a in start)         # nothing passed in was modified


def test_strides_and_counts():
    many, grid = system(30)
    u0, v0, tau, g, c2, source, receivers, adj = ensemble(many, grid, seed=6200, nsteps=11, every=2, shared=True)
    assert c2.shape == (many.size(),)
    hist = many.wave_history_many(u0, v0, tau, 11, source, g=g, receivers=receivers, record_every=2, c2=c2)[3]
    assert np.array_equal(hist, A.verlet_history(grid, u0, v0, g, c2, tau, 11, source)[3])
    # one shared medium is that medium once per member
    shared = many.wave_adjoint_many(hist, tau, c2, adj, receivers=receivers, record_every=2, steps_per_launch=4)
    same(shared, A.adjoint(grid, hist, c2, tau, adj, receivers, 2), "shared medium")
    same(many.wave_adjoint_many(hist, tau, np.ascontiguousarray(np.stack([c2] * 5)), adj, receivers=receivers, record_every=2), shared, "the medium repeated")
    # one table of sources for all members
    same(many.wave_adjoint_many(hist, tau, c2, np.ascontiguousarray(adj[2]), receivers=receivers, record_every=2),
         A.adjoint(grid, hist, c2, tau, adj[2], receivers, 2), "a shared table")
    # no receivers, a state that is not zero: the homogeneous transpose
    rng = np.random.default_rng(6201)
    lam0, q0, S0 = (rng.standard_normal((5, many.size())) for _ in range(3))
    got = many.wave_adjoint_many(hist, tau, c2, None, lam=lam0, q=q0, sens=S0, steps_per_launch=3)
    same(got, A.adjoint(grid, hist, c2, tau, np.zeros((5, 5, 0)), (), 2, lam0, q0, S0), "nrec = 0")
    assert not np.array_equal(got[0], lam0)
    # nothing in, nothing out
    zero = many.wave_adjoint_many(hist, tau, c2, np.zeros_like(adj), receivers=receivers, record_every=2)
    assert not any(np.any(a) for a in zero)
    # a duplicated receiver adds twice, in the order of the list; every sampled step, every step sampled
    twice = [receivers[1], 7, receivers[1], 7, 7]
    for every in (1, 11):
        a2 = rng.standard_normal((5, 11 // every, 5))
        same(many.wave_adjoint_many(hist, tau, c2, a2, receivers=twice, record_every=every, steps_per_launch=5),
             A.adjoint(grid, hist, c2, tau, a2, twice, every), ("a duplicated receiver", every))
    # sixty-four receivers, a cadence longer than the run
    all64 = [int(r) for r in rng.integers(0, many.size(), 64)]
    a64 = rng.standard_normal((5, 3, 64))
    same(many.wave_adjoint_many(hist, tau, c2, a64, receivers=all64, record_every=3), A.adjoint(grid, hist, c2, tau, a64, all64, 3), "64 receivers")
    same(many.wave_adjoint_many(hist, tau, c2, np.zeros((5, 0, 5)), receivers=receivers, record_every=12, lam=lam0, q=q0, sens=S0),
         A.adjoint(grid, hist, c2, tau, np.zeros((5, 0, 5)), receivers, 12, lam0, q0, S0), "no sampled step")


def test_a_stretched_domain_and_device_tensors():
    import torch
    s = _system(20, domain=STRETCHED)
    grid = model(s)
    assert grid.xk != grid.yk
    u0, v0, tau, g, c2, source, receivers, adj = ensemble(s, grid, seed=6300, nsteps=23, every=3)
    want = A.verlet_history(grid, u0, v0, g, c2, tau, 23, source, receivers, 3)
    back = A.adjoint(grid, want[3], c2, tau, adj, receivers, 3)
    ud, vd, gd, cd, sd, ad = (torch.from_numpy(a).cuda() for a in (u0, v0, g, c2, source, adj))
    ut, vt, tt, ht, _, dt = s.wave_history_many(ud, vd, tau, 23, sd, g=gd, receivers=receivers, record_every=3, steps_per_launch=5, c2=cd)
    assert ht.is_cuda and tuple(ht.shape) == (5, 24, s.size()) and [int(d) for d in dt] == [23] * 5
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip((ut, vt, tt, ht), want))
    got = s.wave_adjoint_many(ht, tau, cd, ad, receivers=receivers, record_every=3, steps_per_launch=5)
    assert all(a.is_cuda for a in got)
    same(tuple(a.cpu().numpy() for a in got), back, "device, stretched")
    assert all(np.array_equal(a.cpu().numpy(), b) for a, b in ((ud, u0), (vd, v0), (cd, c2), (ad, adj)))
    for bad in (dict(c2=c2), dict(adjoint_source=adj), dict(lam=u0), dict(c2=cd[:, :5].contiguous()), dict(adjoint_source=ad[:, :3].contiguous())):
        a = dict(hist=ht, tau=tau, c2=cd, adjoint_source=ad, receivers=receivers, record_every=3)
        a.update(bad)
        with pytest.raises(ValueError):
            s.wave_adjoint_many(**a)
    s._handle.close()


def misfit_of(many, u0, v0, tau, nsteps, source, observed, g, receivers, every, c2):
    traces = many.wave_record_many(u0, v0, tau, nsteps, source, g=g, receivers=receivers, record_every=every, c2=c2)[2]
    r = traces - observed
    return 0.5 * np.sum((r * r).reshape(len(u0), -1), axis=-1)


@pytest.mark.parametrize("n", [10, 30])
def test_the_gradient_call(n):
    """wave_gradient_many equals the model bit for bit, segment=6 equals segment=None bit for bit, and grad_c2 agrees with central
    differences of the device's own wave_record_many: relative step 1e-5 along one seeded direction, tolerance 1e-6 relative (the
    worst value of the CPU model's own check is 6.6e-9)."""
    import torch
    many, grid = system(n)
    u0, v0, tau, g, c2, source, receivers, _ = ensemble(many, grid, seed=6400 + n, nsteps=23, every=3, fractions=(0.77, 0.5, 0.31))
    observed = np.random.default_rng(6401 + n).standard_normal((3, 7, 5))
    want = A.gradient(grid, u0, v0, g, c2, tau, 23, source, observed, receivers, 3)
    whole = many.wave_gradient_many(u0, v0, tau, 23, source, observed, g=g, receivers=receivers, record_every=3, c2=c2)
    cut = many.wave_gradient_many(u0, v0, tau, 23, source, observed, g=g, receivers=receivers, record_every=3, c2=c2, segment=6)
    for name, a, b, w in zip(("misfit", "grad_c2", "grad_u0", "grad_v0", "traces"), whole, cut, want):
        assert isinstance(a, np.ndarray) and np.array_equal(a, w), (name, "model")
        assert np.array_equal(a, b), (name, "segment=6")
    assert whole[0].shape == (3,) and np.array_equal(whole[0], misfit_of(many, u0, v0, tau, 23, source, observed, g, receivers, 3, c2))
    # tensors in, tensors out, the same bits; a unit medium when c2 is None
    dev = many.wave_gradient_many(*(torch.from_numpy(a).cuda() for a in (u0, v0)), tau, 23, torch.from_numpy(source).cuda(), torch.from_numpy(observed).cuda(),
                                  g=torch.from_numpy(g).cuda(), receivers=receivers, record_every=3, c2=torch.from_numpy(c2).cuda(), segment=9)
    assert all(a.is_cuda and np.array_equal(a.cpu().numpy(), b) for a, b in zip(dev, whole))
    low = 0.5 * many.wave_cfl() * np.ones(3)
    unit = many.wave_gradient_many(u0, v0, low, 23, source, observed, g=g, receivers=receivers, record_every=3)
    assert all(np.array_equal(a, b) for a, b in zip(unit, A.gradient(grid, u0, v0, g, np.ones(many.size()), low, 23, source, observed, receivers, 3)))
    # central differences of the device's own forward call
    rng = np.random.default_rng(6402 + n)
    d = rng.standard_normal(c2.shape)
    worst = 0.0
    for s in range(3):
        e = 1e-5 * np.linalg.norm(c2[s]) / np.linalg.norm(d[s])
        up, down = c2.copy(), c2.copy()
        up[s] += e * d[s]
        down[s] -= e * d[s]
        fd = (misfit_of(many, u0, v0, tau, 23, source, observed, g, receivers, 3, up)[s] - misfit_of(many, u0, v0, tau, 23, source, observed, g, receivers, 3, down)[s]) / (2 * e)
        err = abs(fd - whole[1][s] @ d[s]) / abs(fd)
        print("N", n, "member", s, "directional derivative", fd, "adjoint", whole[1][s] @ d[s], "relative difference", err)
        worst = max(worst, err)
    assert worst <= 1e-6
    for bad in (dict(segment=4), dict(segment=0), dict(damping=np.zeros(many.size())), dict(receivers=None), dict(observed=observed[:, :3])):
        a = dict(u0=u0, v0=v0, tau=tau, nsteps=23, source=source, observed=observed, g=g, receivers=receivers, record_every=3, c2=c2)
        a.update(bad)
        with pytest.raises(ValueError):
            many.wave_gradient_many(**a)
    with pytest.raises(TypeError):                                   # a misspelt keyword is Python's own error, not the damping's
        many.wave_gradient_many(u0, v0, tau, 23, source, observed, g=g, recievers=receivers, record_every=3, c2=c2)


def test_stop_flag():
    from iterative_solvers_amd import _capi
    many, grid = system(10)
    u0, v0, tau, g, c2, source, receivers, adj = ensemble(many, grid, seed=6500, nsteps=12, every=2)
    hist = many.wave_history_many(u0, v0, tau, 12, source, g=g, receivers=receivers, record_every=2, c2=c2)[3]
    rng = np.random.default_rng(6501)
    lam0, q0, S0 = (rng.standard_normal((5, many.size())) for _ in range(3))
    lam, q, S, res, done = many.wave_adjoint_many(hist, tau, c2, adj, receivers=receivers, record_every=2, lam=lam0, q=q0, sens=S0, steps_per_launch=5,
                                                  stop_flag=C.c_int(1), return_info=True)
    assert np.array_equal(lam, lam0) and np.array_equal(q, q0) and np.array_equal(S, S0) and not done.any()
    assert [(r.iterations, r.stop_reason, r.converged) for r in res] == [(0, _capi.STOP_INTERRUPTED, 0)] * 5
    lam, q, S, res, done = many.wave_adjoint_many(hist, tau, c2, adj, receivers=receivers, record_every=2, lam=lam0, q=q0, sens=S0, steps_per_launch=5,
                                                  stop_flag=C.c_int(0), return_info=True)
    same((lam, q, S), A.adjoint(grid, hist, c2, tau, adj, receivers, 2, lam0, q0, S0), "flag down")
    assert [int(d) for d in done] == [12] * 5 and all(r.converged == 1 for r in res)
    # the history under a raised flag: nothing runs, nothing is written
    u, v, tr, h2, res, done = many.wave_history_many(u0, v0, tau, 12, source, g=g, receivers=receivers, record_every=2, c2=c2, stop_flag=C.c_int(1))
    assert np.array_equal(u, u0) and np.array_equal(v, v0) and not done.any() and not h2.any()


def test_refusals_leave_the_handle_usable():
    import torch
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    good = _system(16, True)
    grid = model(good)
    size = good.size()
    mode = good.solve_mode_info()["mode"]
    hd = good._handle
    hd.set_shift(3.0)
    rhs = hd.rhs()
    u0, v0, tau, g, c2, source, receivers, adj = ensemble(good, grid, seed=6600, nsteps=4, every=2, fractions=(1.0, 0.5, 0.2))
    fwd = A.verlet_history(grid, u0, v0, g, c2, tau, 4, source, receivers, 2)
    hist = fwd[3].copy()
    want = A.adjoint(grid, hist, c2, tau, adj, receivers, 2)
    h = hd._h
    nodes = np.asarray(receivers, dtype=np.int32)

    def still_good():
        assert hd.get_shift() == 3.0 and good.solve_mode_info()["mode"] == mode and np.array_equal(hd.rhs(), rhs)
        got = good.wave_history_many(u0, v0, tau, 4, source, g=g, receivers=receivers, record_every=2, steps_per_launch=3, c2=c2)
        assert all(np.array_equal(a, b) for a, b in zip(got[:4], fwd)), "the forward call after a refusal"
        same(good.wave_adjoint_many(hist, tau, c2, adj, receivers=receivers, record_every=2, steps_per_launch=3), want, "after a refusal")

    def call(handle, nsys, nsteps, tt, cc, cstride, hh, hstride, nrec, nn, every, aa, astride, ll, qq, ss, spl=0, out="res", done="done", fn=lib.mi355cg_wave_adjoint_many):
        ptr = lambda a: (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data) if a is not None else None
        res = (_capi.Results * max(nsys, 1))() if out == "res" else None
        dn = np.full(max(nsys, 1), -7, dtype=np.int32) if done == "done" else None
        rc = fn(handle, nsys, nsteps, ptr(tt), ptr(cc), cstride, ptr(hh), hstride, nrec, ptr(nn), every, ptr(aa), astride, ptr(ll), ptr(qq), ptr(ss), spl, None, res, ptr(dn))
        return rc, lib.mi355cg_last_error().decode(), dn

    lam, q, S = (np.full((3, size), 0.5) for _ in range(3))
    t3 = lambda *a: np.array(a, dtype=np.float64)
    bounds = good.wave_cfl(c2)
    above = np.nextafter(bounds[2], np.inf)
    cbad = lambda val: np.where(np.arange(3 * size).reshape(3, size) == size + 7, val, c2)           # one entry of member 1
    abad = lambda val: np.where(np.arange(30).reshape(3, 2, 5) == 17, val, adj)                      # member 1, sample 1, receiver 2
    ok = (h, 3, 4, tau, c2, size, hist, 5 * size, 5, nodes, 2, adj, 10, lam, q, S)
    names = ("handle", "nsys", "nsteps", "tt", "cc", "cstride", "hh", "hstride", "nrec", "nn", "every", "aa", "astride", "ll", "qq", "ss")

    def but(**kw):
        a = dict(zip(names, ok))
        a.update(kw)
        return tuple(a[k] for k in names)

    big = np.zeros(2 * 15 * size)
    cases = [("null c2", but(cc=None), {}, "c2"), ("c2_stride too short", but(cstride=size - 1), {}, "c2_stride"),
             ("a zero in member 1", but(cc=cbad(0.0)), {}, "member 1"), ("a NaN in member 1", but(cc=cbad(np.nan)), {}, "member 1"),
             ("tau above the member's bound", but(tt=t3(tau[0], tau[1], above)), {}, "member 2"), ("tau 0", but(tt=t3(tau[0], 0.0, tau[2])), {}, "tau"),
             ("tau nan", but(tt=t3(np.nan, tau[1], tau[2])), {}, "tau"), ("null tau", but(tt=None), {}, "null"),
             ("nrec 65", but(nrec=65, nn=np.zeros(65, dtype=np.int32)), {}, "64"), ("receiver size", but(nn=np.array([0, 1, 2, 3, size], dtype=np.int32)), {}, f"[0, {size})"),
             ("record_every 0", but(every=0), {}, "record_every"), ("null rec_nodes", but(nn=None), {}, "rec_nodes"),
             ("null hist", but(hh=None), {}, "hist"), ("hist_stride too short", but(hstride=5 * size - 1), {}, "hist_stride"),
             ("null adj", but(aa=None), {}, "adj"), ("adj_stride too short", but(astride=9), {}, "adj_stride"), ("adj_stride negative", but(astride=-10), {}, "adj_stride"),
             ("a NaN source", but(aa=abad(np.nan)), {}, "member 1 at sample 1, receiver 2"), ("an infinite source", but(aa=abad(np.inf)), {}, "member 1"),
             ("null lam", but(ll=None), {}, "null"), ("null q", but(qq=None), {}, "null"), ("null S", but(ss=None), {}, "null"),
             ("lam is q", but(qq=lam), {}, "lam overlaps q"), ("lam is S", but(ss=lam), {}, "lam overlaps S"), ("q is S", but(ss=q), {}, "q overlaps S"),
             ("c2 is lam", but(cc=lam), {}, "c2 overlaps lam"), ("c2 in q", but(cc=q[1], cstride=0), {}, "c2 overlaps q"), ("c2 in S", but(cc=S[2], cstride=0), {}, "c2 overlaps S"),
             ("hist meets lam", but(hh=big, ll=big[15 * size - 3:]), {}, "hist overlaps lam"), ("hist meets q", but(hh=big, qq=big[:3 * size]), {}, "hist overlaps q"),
             ("hist meets S", but(hh=big, ss=big[size:]), {}, "hist overlaps S"), ("hist meets c2", but(hh=big, cc=big[7:]), {}, "hist overlaps c2"),
             ("adj meets hist", but(hh=big, aa=big[5:]), {}, "adj overlaps hist"), ("adj in lam", but(aa=lam), {}, "adj overlaps lam"),
             ("adj in q", but(aa=q), {}, "adj overlaps q"), ("adj in S", but(aa=S), {}, "adj overlaps S"), ("adj in c2", but(aa=c2), {}, "adj overlaps c2"),
             ("null out", ok, dict(out=None), "null"), ("null steps_done", ok, dict(done=None), "null"), ("null handle", but(handle=None), {}, "null"),
             ("no members", but(nsys=0), {}, str(_capi.MANY_MAX)), ("negative nsteps", but(nsteps=-1), {}, "nsteps"), ("steps_per_launch", ok, dict(spl=-1), "steps_per_launch")]
    for what, args, kw, text in cases:
        rc, msg, dn = call(*args, **kw)
        assert rc == _capi.ERR_INVALID and text in msg, (what, rc, msg)
        assert dn is None or (dn == -7).all(), what                 # nothing was written
        still_good()
    assert all(np.all(a == 0.5) for a in (lam, q, S))
    # the limits themselves are taken: every member at its own bound, wider strides
    wide_h, wide_a = np.zeros((3, 5 * size + 3)), np.zeros((3, 13))
    wide_h[:, :5 * size], wide_a[:, :10] = hist.reshape(3, -1), adj.reshape(3, -1)
    lz, qz, sz = (np.zeros((3, size)) for _ in range(3))
    rc, msg, dn = call(*but(hh=wide_h, hstride=5 * size + 3, aa=wide_a, astride=13, ll=lz, qq=qz, ss=sz))
    assert rc == _capi.OK and (dn == 4).all(), msg
    same((lz, qz, sz), want, "wider strides")
    rc, msg, dn = call(*but(tt=bounds.copy(), ll=lz, qq=qz, ss=sz))
    assert rc == _capi.OK and (dn == 4).all(), msg
    # the history call: what it refuses on top of the medium call
    def hcall(**kw):
        a = dict(tt=tau, gg=g, uu=u0.copy(), vv=v0.copy(), cc=c2, cstride=size, hh=np.zeros((3, 5 * size)), hstride=5 * size, ww=source, wstride=5, nrec=5, nn=nodes, every=2,
                 tr=np.zeros((3, 2, 5)))
        a.update(kw)
        ptr = lambda x: x.ctypes.data if x is not None else None
        res, dn = (_capi.Results * 3)(), np.full(3, -7, dtype=np.int32)
        rc = lib.mi355cg_wave_history_many(h, 3, 4, ptr(a["tt"]), ptr(a["gg"]), ptr(a["uu"]), ptr(a["vv"]), ptr(a["cc"]), a["cstride"], ptr(a["hh"]), a["hstride"], ptr(a["ww"]),
                                           a["wstride"], a["nrec"], ptr(a["nn"]), a["every"], ptr(a["tr"]), 0, None, res, dn.ctypes.data)
        return rc, lib.mi355cg_last_error().decode(), dn, a
    cw = np.concatenate([c2.reshape(-1), np.zeros(15 * size)])
    own = np.zeros((3, 5 * size))                                    # large enough to be a history, and the state of the same call
    for what, kw, text in [("null hist", dict(hh=None), "hist"), ("hist_stride", dict(hstride=5 * size - 1), "hist_stride"), ("hist is u", dict(hh=own, uu=own), "hist overlaps u"),
                           ("hist meets c2", dict(cc=cw, hh=cw[2 * size:]), "hist overlaps c2"), ("hist is v", dict(hh=own, vv=own), "hist overlaps v"),
                           ("a zero in member 1", dict(cc=cbad(0.0)), "member 1"), ("tau above the bound", dict(tt=t3(tau[0], tau[1], above)), "member 2"),
                           ("null c2", dict(cc=None), "c2")]:
        rc, msg, dn, _ = hcall(**kw)
        assert rc == _capi.ERR_INVALID and text in msg and (dn == -7).all(), (what, rc, msg)
        still_good()
    rc, msg, dn, a = hcall()
    assert rc == _capi.OK and (dn == 4).all() and np.array_equal(a["hh"].reshape(3, 5, size), hist) and np.array_equal(a["uu"], fwd[0]), msg
    # the device entry point: the same checks, the media read by the check launch
    cd, hdv, ad = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (c2, hist, adj))
    ld, qd, sd = (torch.full((3, size), 0.5, dtype=torch.float64).cuda() for _ in range(3))
    torch.cuda.synchronize()
    dev = lib.mi355cg_wave_adjoint_many_device
    okd = dict(cc=cd, hh=hdv, aa=ad, ll=ld, qq=qd, ss=sd)
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for what, kw, text in [("null c2", dict(cc=None), "c2"), ("c2_stride", dict(cstride=5), "c2_stride"), ("a zero", dict(cc=on(cbad(0.0))), "member 1"),
                           ("a NaN", dict(cc=on(cbad(np.nan))), "member 1"), ("tau above the member's bound", dict(tt=t3(tau[0], tau[1], above)), "member 2"),
                           ("hist_stride", dict(hstride=4 * size), "hist_stride"), ("adj_stride", dict(astride=3), "adj_stride"), ("lam is q", dict(qq=ld), "lam overlaps q"),
                           ("c2 is S", dict(cc=sd), "c2 overlaps S"), ("adj is lam", dict(aa=ld), "adj overlaps lam"), ("nrec", dict(nrec=70), "64")]:
        rc, msg, dn = call(*but(**dict(okd, **kw)), fn=dev)
        assert rc == _capi.ERR_INVALID and text in msg and (dn == -7).all(), (what, rc, msg)
        still_good()
    assert all(bool((a == 0.5).all()) for a in (ld, qd, sd))
    # the Python layer
    for kw in (dict(c2=c2[:2]), dict(c2=cbad(0.0)), dict(adjoint_source=adj[:, :1]), dict(adjoint_source=None), dict(tau=t3(tau[0], tau[1], above)), dict(record_every=0),
               dict(receivers=[0, size, 1, 2, 3]), dict(lam=lam[:2]), dict(hist=hist[:, :, :5]), dict(hist=hist.astype(np.float32)), dict(c2=torch.from_numpy(c2))):
        a = dict(hist=hist, tau=tau, c2=c2, adjoint_source=adj, receivers=receivers, record_every=2)
        a.update(kw)
        with pytest.raises(ValueError):
            good.wave_adjoint_many(**a)
        still_good()
    # a plain solve on the handle still gives what it gave
    p = params(_capi.RULE_REL_2NORM, eps_rel=1e-8, sync_every=7)
    first = fields(hd.solve(p, None, None))
    good.wave_adjoint_many(hist, tau, c2, adj, receivers=receivers, record_every=2)
    assert fields(hd.solve(p, None, None)) == first
    hd.close()
