"""Batched on-chip solves: mi355cg_solve_many* runs many small systems of one grid, one workgroup each.
System s must get the bits of set_shift(sigma_s); set_rhs(b_s); [set_initial_guess(x0_s);] solve; solution() on a handle of the
same grid.  The reference throughout is a SECOND handle of that grid in the default two-launch mode, solved one system after
another: independent code from the kernel under test.  "Same" means np.array_equal on x and == on iterations, stop reason,
converged, r_norm2, initial_r_norm2, final_precision and final_residual_norm.  sync_every = 7 unless said otherwise, so that solves
span many chunks and the systems of a batch finish in different chunks."""
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
SIZES = [10, 12, 20, 30, 64, 100, "cap"]            # a subset of test_gpu_onchip.SIZES that still covers every shape of the plan
REL = dict(eps_rel=1e-10, sync_every=7)
MSG = dict(eps_precision=1e-9, eps_residual=1e-9, eps_exact_error=0.0, sync_every=7)


_pairs = {}


def pair(n):
    """(the system the batches run on, the reference system in the default mode) of a grid, created once."""
    if n not in _pairs:
        _pairs[n] = (_system(n), _system(n))
        assert _pairs[n][1].solve_mode_info()["mode"] == 0
    return _pairs[n]


def rules():
    from iterative_solvers_amd import _capi
    return ((_capi.RULE_REL_2NORM, REL), (_capi.RULE_MSG_MAXNORM, MSG))


def sequential(ref, p, b, x0=None, sigma=None, stop_flag=None):
    """[(x, fields)] of one solve after another on the reference handle, which is left with the shift it had."""
    h = ref._handle
    old = h.get_shift()
    out = []
    try:
        for s in range(len(b)):
            if sigma is not None:
                h.set_shift(float(sigma[s]))
            h.set_rhs(b[s])
            if x0 is not None:
                h.set_initial_guess(x0[s])
            res = h.solve(p, None, stop_flag)
            out.append((h.solution(), fields(res)))
    finally:
        h.set_shift(old)
    return out


def same(x, res, ref, what):
    """Every row of a batch against the sequential results; prints the figures before it asserts."""
    assert len(res) == len(ref) == len(x)
    for s, (xs, fs) in enumerate(ref):
        got = fields(res[s])
        if got != fs or not np.array_equal(x[s], xs):
            print(what, "system", s, "batch", got, "| sequential", fs, "| max |dx|", float(np.max(np.abs(x[s] - xs))))
        assert got == fs, (what, s)
        assert np.array_equal(x[s], xs), (what, s)
        assert res[s].final_error_norm == sys.float_info.max, (what, s)


def rhs_set(sys_, seed=0):
    """Five right-hand sides with different iteration counts: the system's own, two seeded random ones, one scaled by 1e-6, a smooth one."""
    u = sys_.size()
    rng = np.random.default_rng(seed)
    smooth = np.sin(np.linspace(0.0, 3.0, u)) + 2.0
    return np.stack([sys_.get_rhs(), rng.standard_normal(u), rng.standard_normal(u), 1e-6 * rng.standard_normal(u), smooth])


def test_the_sizes_below_cover_every_shape_of_the_plan():
    import iterative_solvers_amd as isa
    plans = [isa.onchip_plan(_cap() if n == "cap" else n) for n in SIZES]
    assert {p["threads"] for p in plans} == {64, 128, 256, 512}
    assert {p["elems_per_thread"] for p in plans} == {1, 2, 4, 8, 16, 24}
    assert _cap() == 128


@pytest.mark.parametrize("n", SIZES)
def test_converged_batches_both_rules(n):
    n = _cap() if n == "cap" else n
    many, ref = pair(n)
    b = rhs_set(many)
    for rule, kw in rules():
        p = params(rule, **kw)
        x, res = many._handle.solve_many(p, b)
        same(x, res, sequential(ref, p, b), (n, rule))
        its = [r.iterations for r in res]
        print(n, rule, "iterations", its)
        assert len(set(its)) >= 2, its
        assert all(r.converged == 1 for r in res)
        assert max(its) > 7                                       # more than one chunk


@pytest.mark.parametrize("n,nsys,pool,cap_it", [(10, 9000, 7, None), ("cap", 300, 3, 40)])
def test_more_systems_than_fit_at_once(n, nsys, pool, cap_it):
    """9000 single-wave workgroups are more than 256 CUs x 32 waves hold; 300 workgroups at the cap more than 256 CUs at one per CU."""
    from iterative_solvers_amd import _capi
    n = _cap() if n == "cap" else n
    many, ref = pair(n)
    rng = np.random.default_rng(5)
    vecs = np.concatenate([rhs_set(many, seed=1), rng.standard_normal((2, many.size()))])[:pool]
    pick = rng.permutation(np.arange(nsys) % pool)
    b = np.ascontiguousarray(vecs[pick])
    kw = dict(REL) if cap_it is None else dict(REL, max_iterations=cap_it)
    p = params(_capi.RULE_REL_2NORM, **kw)
    want = sequential(ref, p, vecs)
    x, res = many._handle.solve_many(p, b)
    assert len(res) == nsys
    for s in range(nsys):
        xs, fs = want[pick[s]]
        assert fields(res[s]) == fs, (s, pick[s], fields(res[s]), fs)
        assert np.array_equal(x[s], xs), (s, pick[s])
    assert len({r.iterations for r in res}) >= (2 if cap_it is None else 1)


def test_warm_starts():
    """A guess that already meets the rule (0 iterations, x = x0), a 1e-4-accurate one, zeros (= the cold batch) and a random one."""
    from iterative_solvers_amd import _capi
    n = 16
    many, ref = pair(n)
    own = many.get_rhs()
    ref._handle.set_rhs(own)
    ref._handle.solve(params(_capi.RULE_REL_2NORM, eps_rel=1e-13), None, None)
    xstar = ref._handle.solution()
    rng = np.random.default_rng(2)
    x0 = np.stack([xstar, xstar * (1.0 + 1e-4 * rng.standard_normal(xstar.size)), np.zeros_like(xstar), rng.standard_normal(xstar.size)])
    b = np.stack([own] * 4)
    keep = x0.copy()
    for rule, kw in rules():
        p = params(rule, **kw)
        x, res = many._handle.solve_many(p, b, x0=x0)
        assert np.array_equal(x0, keep)
        same(x, res, sequential(ref, p, b, x0=x0), ("warm", rule))
        print("warm", rule, [fields(r) for r in res])
        assert res[0].iterations == 0 and res[0].converged == 1 and np.array_equal(x[0], x0[0])
        assert res[1].iterations > 0 and res[3].iterations > 0
        xc, rc = many._handle.solve_many(p, b[:1])
        assert np.array_equal(x[2], xc[0]) and fields(res[2]) == fields(rc[0])


def test_per_system_shift():
    from iterative_solvers_amd import _capi
    n = 16
    many, ref = _system(n), _system(n)
    sigma = np.array([0.0, 1.0, 50.0, 1e4])
    rhs = rhs_set(many, seed=3)
    for b in (np.stack([rhs[0]] * 4), rhs[:4]):
        for rule, kw in rules():
            p = params(rule, **kw)
            x, res = many._handle.solve_many(p, b, sigma=sigma)
            same(x, res, sequential(ref, p, b, sigma=sigma), ("shift", rule))
            assert len({r.iterations for r in res}) >= 2
            assert many.shift == 0.0
    many.set_shift(3.0)
    p = params(_capi.RULE_REL_2NORM, **REL)
    x, res = many._handle.solve_many(p, rhs[:3])
    assert many.shift == 3.0
    x3, res3 = many._handle.solve_many(p, rhs[:3], sigma=[3.0] * 3)
    assert many.shift == 3.0
    assert np.array_equal(x, x3) and [fields(r) for r in res] == [fields(r) for r in res3]
    same(x, res, sequential(ref, p, rhs[:3], sigma=[3.0] * 3), "the handle's own shift")
    for s in (many, ref):
        s._handle.close()


def test_fixed_iterations_and_caps():
    from iterative_solvers_amd import _capi
    many, ref = pair(30)
    b = rhs_set(many, seed=4)
    for rule, kw in rules():
        p = params(rule, **dict(kw, fixed_iterations=1, max_iterations=3))
        x, res = many._handle.solve_many(p, b)
        same(x, res, sequential(ref, p, b), ("fixed", rule))
        assert [r.iterations for r in res] == [3] * len(b)
    for rule, kw in ((_capi.RULE_REL_2NORM, dict(eps_rel=1e-30, sync_every=7)),
                     (_capi.RULE_MSG_MAXNORM, dict(eps_precision=1e-30, eps_residual=1e-30, eps_exact_error=0.0, sync_every=7))):
        p = params(rule, **dict(kw, max_iterations=10))              # the cap cuts the second chunk of 7
        x, res = many._handle.solve_many(p, b)
        same(x, res, sequential(ref, p, b), ("cap", rule))
        assert [(r.iterations, r.stop_reason, r.converged) for r in res] == [(10, _capi.STOP_ITERATIONS, 0)] * len(b)


def test_stop_flag_set_before_the_call():
    from iterative_solvers_amd import _capi
    many, ref = pair(16)
    b = rhs_set(many, seed=6)
    x0 = np.random.default_rng(6).standard_normal(b.shape)
    for rule, kw in rules():
        p = params(rule, **kw)
        for guess in (None, x0):
            flag = C.c_int(1)
            x, res = many._handle.solve_many(p, b, stop_flag=flag, x0=guess)
            assert [(r.iterations, r.stop_reason, r.converged) for r in res] == [(0, _capi.STOP_INTERRUPTED, 0)] * len(b)
            assert np.array_equal(x, np.zeros_like(b) if guess is None else guess)
            same(x, res, sequential(ref, p, b, x0=guess, stop_flag=C.c_int(1)), ("stopped", rule, guess is not None))


def test_device_tensors():
    import torch
    from iterative_solvers_amd import _capi
    many, _ = pair(20)
    b = rhs_set(many, seed=7)
    x0 = np.random.default_rng(7).standard_normal(b.shape)
    sigma = np.array([0.0, 2.0, 0.5, 10.0, 1.0])
    bd, xd, sd = (torch.from_numpy(v).cuda() for v in (b, x0, sigma))
    for rule, kw in rules():
        p = params(rule, **kw)
        for host, dev in ((dict(), dict()), (dict(x0=x0, sigma=sigma), dict(x0=xd, sigma=sd))):
            xh, rh = many._handle.solve_many(p, b, **host)
            xt, rt = many._handle.solve_many(p, bd, **dev)
            assert xt.is_cuda and np.array_equal(xt.cpu().numpy(), xh)
            assert [fields(r) for r in rt] == [fields(r) for r in rh]
    assert np.array_equal(bd.cpu().numpy(), b) and np.array_equal(xd.cpu().numpy(), x0) and np.array_equal(sd.cpu().numpy(), sigma)


@pytest.mark.parametrize("onchip", [False, True])
def test_the_handle_is_untouched(onchip):
    from iterative_solvers_amd import _capi
    s = _system(16, onchip)
    mode = s.solve_mode_info()["mode"]
    h = s._handle
    p = params(_capi.RULE_REL_2NORM, **REL)
    first = fields(h.solve(p, None, None))
    x, r, rhs = h.solution(), h.recursive_residual(), h.rhs()
    b = rhs_set(s, seed=8)
    xm, _ = h.solve_many(params(_capi.RULE_MSG_MAXNORM, **MSG), b, x0=np.ones_like(b), sigma=[1.0, 2.0, 3.0, 4.0, 5.0])
    assert not np.array_equal(xm[0], x)
    assert np.array_equal(h.solution(), x) and np.array_equal(h.recursive_residual(), r) and np.array_equal(h.rhs(), rhs)
    assert h.get_shift() == 0.0 and s.solve_mode_info()["mode"] == mode
    assert fields(h.solve(p, None, None)) == first                  # cold: the batch left no pending guess behind
    assert np.array_equal(h.solution(), x) and np.array_equal(h.recursive_residual(), r)
    assert s.solve_mode_info()["onchip_launches"] > 0 if onchip else s.solve_mode_info()["onchip_launches"] == 0
    # a pending guess survives a batch: the next solve is the warm solve it would have been
    guess = np.random.default_rng(18).standard_normal(s.size())
    h.set_initial_guess(guess)
    warm = fields(h.solve(p, None, None))
    xw = h.solution()
    assert warm != first
    h.set_initial_guess(guess)
    h.solve_many(params(_capi.RULE_MSG_MAXNORM, **MSG), b, x0=np.ones_like(b))
    assert fields(h.solve(p, None, None)) == warm and np.array_equal(h.solution(), xw)
    h.close()


def test_refusals_leave_the_handle_usable():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    from oracle.oracle import OracleGrid
    lib = _capi.load()
    cap = _cap()
    good = _system(16)
    u = good.size()
    b = rhs_set(good, seed=9)[:3]
    p = params(_capi.RULE_REL_2NORM, **REL)
    want_x, want_res = good._handle.solve_many(p, b)
    want = [fields(r) for r in want_res]

    def call(handle, prm, nsys, bb, xx, sg=None, fn=lib.mi355cg_solve_many):
        res = (_capi.Results * max(nsys, 1))()
        rc = fn(handle, C.byref(prm) if prm is not None else None, nsys, bb.ctypes.data if bb is not None else None,
                xx.ctypes.data if xx is not None else None, sg.ctypes.data if sg is not None else None, None, res)
        return rc, lib.mi355cg_last_error().decode()

    def still_good():
        x, res = good._handle.solve_many(p, b)
        assert np.array_equal(x, want_x) and [fields(r) for r in res] == want

    h = good._handle._h
    x = np.empty_like(b)
    def bad(**kw):
        q = params(_capi.RULE_REL_2NORM, **REL)
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    both = np.empty((6, u))
    cases = [("null b", (h, p, 3, None, x), "null"), ("null x", (h, p, 3, b, None), "null"), ("null params", (h, None, 3, b, x), "null"),
             ("no systems", (h, p, 0, b, x), str(_capi.MANY_MAX)), ("too many", (h, p, _capi.MANY_MAX + 1, b, x), str(_capi.MANY_MAX)),
             ("x is b", (h, p, 3, b, b), "overlaps"), ("x overlaps b", (h, p, 3, both[:3], both[1:4]), "overlaps"),
             ("rule", (h, bad(rule=7), 3, b, x), "rule"), ("true solution", (h, bad(use_true_solution=1), 3, b, x), "use_true_solution"),
             ("diagnostics", (h, bad(diagnostics=1), 3, b, x), "diagnostics"),
             ("negative sigma", (h, p, 3, b, x, np.array([0.0, -1.0, 0.0])), "sigma"), ("nan sigma", (h, p, 3, b, x, np.array([0.0, 1.0, np.nan])), "sigma"),
             ("inf sigma", (h, p, 3, b, x, np.array([np.inf, 1.0, 0.0])), "sigma")]
    for what, args, text in cases:
        for fn in (lib.mi355cg_solve_many, lib.mi355cg_solve_many_from):
            rc, msg = call(*args, fn=fn)
            assert rc == _capi.ERR_INVALID and text in msg, (what, rc, msg)
        still_good()
    # a null results array, a null handle
    for fn in (lib.mi355cg_solve_many, lib.mi355cg_solve_many_from):
        assert fn(h, C.byref(p), 3, b.ctypes.data, x.ctypes.data, None, None, None) == _capi.ERR_INVALID
        assert "null" in lib.mi355cg_last_error().decode()
        assert fn(None, C.byref(p), 3, b.ctypes.data, x.ctypes.data, None, None, (_capi.Results * 3)()) == _capi.ERR_INVALID
        assert "null" in lib.mi355cg_last_error().decode()
    assert lib.mi355cg_solve_many_info(None, 3, None, None, None) == _capi.ERR_INVALID
    still_good()
    # the device entry points: the same checks, sigma after its copy to the host
    import torch
    bd = torch.from_numpy(b).cuda()
    xd = torch.zeros_like(bd)
    ok_sigma = torch.zeros(3, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dev_cases = [("negative sigma", (3, bd, xd, torch.tensor([0.0, -1.0, 0.0], dtype=torch.float64, device="cuda"), p), "sigma"),
                 ("nan sigma", (3, bd, xd, torch.tensor([0.0, float("nan"), 0.0], dtype=torch.float64, device="cuda"), p), "sigma"),
                 ("x is b", (3, bd, bd, ok_sigma, p), "overlaps"), ("too many", (_capi.MANY_MAX + 1, bd, xd, ok_sigma, p), str(_capi.MANY_MAX)),
                 ("diagnostics", (3, bd, xd, ok_sigma, bad(diagnostics=1)), "diagnostics"), ("null out", (3, bd, xd, ok_sigma, p), "null")]
    for what, (nsys, bt, xt, st, prm), text in dev_cases:
        for fn in (lib.mi355cg_solve_many_device, lib.mi355cg_solve_many_device_from):
            out = None if what == "null out" else (_capi.Results * 3)()
            rc = fn(h, C.byref(prm), nsys, bt.data_ptr(), xt.data_ptr(), st.data_ptr(), None, out)
            assert rc == _capi.ERR_INVALID and text in lib.mi355cg_last_error().decode(), (what, rc, lib.mi355cg_last_error())
        still_good()
    assert np.array_equal(bd.cpu().numpy(), b) and not xd.any()     # nothing was written
    xt, rt = good._handle.solve_many(p, bd, sigma=ok_sigma)
    assert np.array_equal(xt.cpu().numpy(), want_x) and [fields(r) for r in rt] == want
    with pytest.raises(ValueError):
        good._handle.solve_many(bad(diagnostics=1), b)
    with pytest.raises(ValueError):
        good._handle.solve_many(p, b, sigma=[0.0, 1.0])
    still_good()

    # handles the on-chip mode refuses, with its message; a preconditioned handle is a matter of state
    big = _system(cap + 2)
    bb = np.ones((2, big.size()))
    rc, msg = call(big._handle._h, p, 2, bb, np.empty_like(bb))
    assert rc == _capi.ERR_INVALID and str(cap) in msg and str(cap + 2) in msg
    with pytest.raises(ValueError):
        big.solve_many(bb)
    with pytest.raises(ValueError):
        big.solve_many_info(2)
    big._handle.close()
    csr = isa.CrsMatrix(*OracleGrid(8, 8).csr())
    cb = np.ones((2, csr._handle.size))
    rc, msg = call(csr._handle._h, p, 2, cb, np.empty_like(cb))
    assert rc == _capi.ERR_INVALID and "CSR" in msg
    mixed = isa.MatrixFreeSystem(16, 16, *DOMAIN, dtype=isa.F32_MIXED)
    rc, msg = call(mixed._handle._h, p, 3, b, x)
    assert rc == _capi.ERR_INVALID and "F32_MIXED" in msg
    mixed._handle.close()
    slab = C.c_void_p()
    assert lib.mi355cg_create_slab(16, 16, *DOMAIN, _capi.F64, 0, 1, 8, C.byref(slab)) == _capi.OK
    rc, msg = call(slab, p, 3, b, x)
    assert rc == _capi.ERR_INVALID and "part" in msg
    lib.mi355cg_destroy(slab)
    good.set_preconditioner(isa.PRECOND_MG_ANY)
    rc, msg = call(h, p, 3, b, x)
    assert rc == _capi.ERR_STATE and "preconditioner" in msg
    with pytest.raises(_capi.Mi355cgError):
        good._handle.solve_many(p, b)
    good.set_preconditioner(isa.PRECOND_NONE)
    still_good()
    good._handle.close()


def test_workspace_lifetime():
    from iterative_solvers_amd import _capi
    many, ref = pair(12)
    fresh = _system(12)
    fresh.batch_release()                                            # nothing allocated: fine
    rng = np.random.default_rng(10)
    b = rng.standard_normal((40, fresh.size()))
    p = params(_capi.RULE_REL_2NORM, **REL)
    want = sequential(ref, p, b)
    x, res = fresh._handle.solve_many(p, b[:2])
    same(x, res, want[:2], "two systems")
    x, res = fresh._handle.solve_many(p, b)                          # grown
    same(x, res, want, "forty systems")
    x, res = fresh._handle.solve_many(p, b[:2])                      # the larger workspace is kept
    same(x, res, want[:2], "two again")
    fresh.batch_release()
    fresh.batch_release()
    x, res = fresh._handle.solve_many(p, b[:5], x0=np.zeros((5, fresh.size())))
    same(x, res, want[:5], "after the release")
    fresh._handle.close()


def test_solve_many_info():
    import iterative_solvers_amd as isa
    small = pair(10)[0].solve_many_info(4096)
    print("N = 10:", small)
    assert small["workgroups_per_cu"] >= 4                           # a statically declared image of the largest grid gives 1
    for n in range(6, _cap() + 1, 2):                                # every accepted N
        s = pair(n)[0] if n in _pairs else _system(n)
        info = s.solve_many_info(7)
        plan = isa.onchip_plan(n)
        assert plan["lds_bytes"] == (n + 1) ** 2 * 8 + 8 * (4 + 10) * 8 + 256          # the image plus the side data
        assert plan["lds_bytes"] <= info["lds_bytes_per_workgroup"] <= 160 * 1024, (n, info)
        assert info["workgroups_per_cu"] >= 1, (n, info)
        assert info["workspace_bytes"] == 7 * (24 * s.size() + 456) + 8, (n, info)
        if n not in _pairs:
            s._handle.close()
    assert pair(_cap())[0].solve_many_info(1)["workgroups_per_cu"] == 1
    with pytest.raises(ValueError):
        pair(10)[0].solve_many_info(0)


def test_cpp_host_solves_many_through_the_compat_header():
    """MatrixFreeSystem::solveMany of three systems with a shift and a guess each against three MSGSolver solves, bit for bit."""
    from iterative_solvers_amd import build as b
    b.build()
    src = os.path.join(ROOT, "tests", "cpp", "onchip_many_compat_driver.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "onchip_many_compat_driver")
    headers = [os.path.join(ROOT, "iterative_solvers_amd", "compat", "mi355cg_compat.hpp"), os.path.join(ROOT, "include", "mi355cg.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src] + headers):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                               "-I", os.path.join(ROOT, "iterative_solvers_amd", "compat"), src,
                               "-L", os.path.join(ROOT, "iterative_solvers_amd"), "-lmi355cg",
                               "-Wl,-rpath," + os.path.join(ROOT, "iterative_solvers_amd"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if k != "MI355CG_ONCHIP"}
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-500:] + out.stderr[-2000:]
    systems = json.loads(out.stdout)["systems"]
    assert [s["sigma"] for s in systems] == [0.0, 2.5, 40.0]
    for s in systems:
        assert s["same_bits"] is True and s["many"] == s["single"]
        assert s["iterations_many"] == s["iterations_single"] > 1 and s["converged_many"] == 1
    assert len({s["iterations_many"] for s in systems}) >= 2
