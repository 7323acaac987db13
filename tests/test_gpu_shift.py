"""The diagonal shift A - sigma I on the GPU (mi355cg_set_shift) against the shifted restatement of
tests/shift_reference.py: the operator, the refusals, no stale state across a change of sigma, plain CG, the V-cycle in both
precisions, multigrid-PCG solves, the order of set_preconditioner and set_shift, batches, warm starts and the deferred x fold.
Every tolerance is computed from the reference (mg_reference.tol_M, tol_pcg) or from the number formats, never from what the
library returned; tests/test_shift_cpu.py asserts the stop margins of the cases whose iteration counts are compared here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model  # noqa: E402
import shift_reference as S  # noqa: E402

R = S.R
pytestmark = pytest.mark.gpu

CYCLE_GRIDS = S.GRIDS                  # (34, ANY, ISO), (64, MG, ISO), (258, ANY, WIDE_Y)
_CACHE = {}


def system(N, dom=R.ISO, kind=None, cycle=None, sigma=None, env=None):
    """A MatrixFreeSystem created under `env` (the knobs are read at mi355cg_create), the shift set BEFORE the preconditioner"""
    import iterative_solvers_amd as isa
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        s = isa.MatrixFreeSystem(N, N, *dom)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if sigma is not None:
        s.set_shift(sigma)
    if kind is not None:
        s.set_preconditioner(kind, isa.CYCLE_F64 if cycle is None else cycle)
    return s


def rel_params(eps=S.EPS, max_iterations=10000, fixed=False):
    import iterative_solvers_amd as isa
    p = isa.default_params(isa.RULE_REL_2NORM)
    p.eps_rel, p.max_iterations, p.fixed_iterations, p.use_true_solution = eps, max_iterations, int(fixed), 0
    return p


def msg_params():
    import iterative_solvers_amd as isa
    p = isa.default_params(isa.RULE_MSG_MAXNORM)
    p.eps_precision = p.eps_residual = 1e-9
    p.use_true_solution = 0
    return p


def solve(s, p, b=None, x0=None):
    h = s._handle
    if b is not None:
        h.set_rhs(b)
    if x0 is not None:
        h.set_initial_guess(x0)
    res = h.solve(p)
    return h.solution(), res


def levels(N, dom, kind, sigma):
    key = ("levels", N, dom, kind, sigma)
    if key not in _CACHE:
        _CACHE[key] = S.shifted_levels(N, dom, kind, sigma)
    return _CACHE[key]


def show(what, dev, tol):
    print(f"  {what}: deviation {dev:.2e}, tolerance {tol:.2e}")
    return dev <= tol


def rel(a, b):
    return abs(a - b) / abs(b)


# ---- the operator -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dom", [R.ISO, R.WIDE_X], ids=["iso", "wide_x"])
@pytest.mark.parametrize("N", [6, 34, 64])
def test_apply_is_the_shifted_stencil(N, dom):
    """|y - y_ref| <= 8 2^-53 (|diag_sigma| + 2 x_k + 2 y_k) max|x|: five products and four additions to first order"""
    s, fresh = system(N, dom), system(N, dom)
    x = np.random.default_rng(N).standard_normal(s.size())
    y0 = fresh.apply(x)
    for sigma in (0.0, 1.0, 1e4):
        s.set_shift(sigma)
        assert s.shift == sigma
        L = S.shifted_levels(N, dom, R.MG_ANY, sigma)
        y = s.apply(x)
        bound = 8 * 2.0 ** -53 * (abs(L[0].diag) + 2 * L[0].xk + 2 * L[0].yk) * np.abs(x).max()
        assert show(f"N={N} sigma={sigma:g} max|y - y_ref|", np.abs(y - R.apply_A(L, x)).max(), bound)
        if sigma == 0.0:
            assert np.array_equal(y, y0)                            # A - 0.0 == A: the handle that never had a shift
        else:
            # y and y0 each within their bound (<= this one), and three roundings of size sigma max|x| <= bound / 8 in the expression
            assert np.abs(y - y0 + sigma * x).max() <= 3 * bound and not np.array_equal(y, y0)
    s.set_shift(0.0)
    assert np.array_equal(s.apply(x), y0)
    import torch
    xd = torch.from_numpy(x).cuda()
    yd = torch.empty_like(xd)
    s.set_shift(1e4)
    torch.cuda.synchronize()
    from iterative_solvers_amd import _capi
    _capi.check(s._handle._lib.mi355cg_apply_device(s._handle._h, xd.data_ptr(), yd.data_ptr()))
    assert np.array_equal(yd.cpu().numpy(), s.apply(x))


def test_refusals_leave_the_handle_as_it_was():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    from iterative_solvers_amd.solver import _Handle
    from oracle.oracle import OracleGrid
    s = system(34, sigma=2.5)
    x = np.random.default_rng(1).standard_normal(s.size())
    y = s.apply(x)
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError, match="finite and >= 0"):
            s.set_shift(bad)
        assert s.shift == 2.5
    assert np.array_equal(s.apply(x), y)
    mixed = isa.MatrixFreeSystem(64, 64, *R.ISO, dtype=isa.F32_MIXED)
    csr = isa.CrsMatrix(*OracleGrid(16, 16, *R.ISO).csr())
    slab = _Handle.__new__(_Handle)
    slab._lib, slab._h, slab._device = _capi.load(), C.c_void_p(), 0
    _capi.check(slab._lib.mi355cg_create_slab(64, 64, *R.ISO, _capi.F64, 0, 1, 31, C.byref(slab._h)))
    slab.size = int(slab._lib.mi355cg_size(slab._h))
    for h, why in ((mixed._handle, "fp64 only"), (csr._handle, "CSR"), (slab, "single-GPU")):
        for sigma in (1.0, 0.0):
            with pytest.raises(ValueError, match=why):
                h.set_shift(sigma)
        assert h.get_shift() == 0.0
    v = np.random.default_rng(2).standard_normal(csr._handle.size)
    assert np.allclose(csr._handle.apply(v), OracleGrid(16, 16, *R.ISO).apply(v), rtol=1e-13, atol=1e-9)
    slab.close()


# ---- no stale state across a change of sigma (N = 64: the chunks of a solve are replayed as graphs) -----------------------------------
@pytest.mark.parametrize("rule", ["rel", "msg"])
def test_a_change_of_sigma_leaves_no_stale_state(rule):
    p = rel_params() if rule == "rel" else msg_params()
    s = system(64)
    x_first, r_first = solve(s, p)
    s.set_shift(1e4)
    x_mid, r_mid = solve(s, p)
    true_res = s._handle.true_residual()                           # (A - sigma I) x - b follows the shift
    s.set_shift(0.0)
    x_last, r_last = solve(s, p)
    fresh = system(64, sigma=1e4)
    x_fresh, r_fresh = solve(fresh, p)
    print(f"{rule}: iterations sigma=0 {r_first.iterations}, sigma=1e4 {r_mid.iterations}")
    assert r_first.converged and r_mid.converged and r_mid.iterations < r_first.iterations
    assert r_mid.iterations == r_fresh.iterations and r_mid.r_norm2 == r_fresh.r_norm2
    assert np.array_equal(x_mid, x_fresh)
    assert r_last.iterations == r_first.iterations and r_last.r_norm2 == r_first.r_norm2
    assert np.array_equal(x_last, x_first)
    if rule == "rel":                                               # ||r||_2 <= 1e-8 ||b||_2 recursively; the true one is not far
        assert np.linalg.norm(true_res) <= 1e-7 * np.linalg.norm(s.get_rhs())
    assert np.array_equal(true_res, fresh._handle.true_residual())


# ---- plain CG ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dom", [R.ISO, R.WIDE_Y], ids=["iso", "wide_y"])
def test_plain_cg_gives_the_iterates_of_the_identity_trace(dom):
    N, sigma, k = 34, 1e3, 20
    L = S.shifted_levels(N, dom, R.MG_ANY, sigma)
    b = S.rhs_vector(N)
    ident = lambda r: r
    t = R.pcg_trace(L, b, iterations=k, M=ident)
    tol = {q: R.tol_pcg(v) for q, v in R.spread(L, b, k, M=ident, exact=t).items()}
    s = system(N, dom, sigma=sigma)
    x, res = solve(s, rel_params(max_iterations=k, fixed=True), b=b)
    assert res.iterations == k
    ok = show(f"x after {k} iterations, max|x - x_ref| / max|x_ref|", np.abs(x - t.x[-1]).max() / np.abs(t.x[-1]).max(), tol["x"][-1])
    ok &= show("r_norm2", rel(res.r_norm2, t.r2[-1]), tol["r2"][-1])
    ok &= show("initial_r_norm2", rel(res.initial_r_norm2, t.b_norm2), tol["b2"][-1])
    assert ok


# ---- the V-cycle -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [1e3, 1e5])
@pytest.mark.parametrize("N,kind,dom", CYCLE_GRIDS, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_vcycle_matches_the_shifted_restatement(N, kind, dom, sigma):
    import iterative_solvers_amd as isa
    L = levels(N, dom, kind, sigma)
    s = system(N, dom, kind, sigma=sigma)
    r = np.random.default_rng(N + 1).standard_normal(s.size())
    zr = R.apply_M(L, r)
    tol = R.tol_M(R.cycle_floor(L, r, zr))
    z = s._handle.apply_preconditioner(r)
    ok = show(f"N={N} sigma={sigma:g} fp64 cycle, max|z - z_ref| / max|z_ref|", np.abs(z - zr).max() / np.abs(zr).max(), tol)
    s.set_preconditioner(kind, isa.CYCLE_F32)
    z32 = s._handle.apply_preconditioner(r)
    dev = np.abs(z32 - zr).max() / np.abs(zr).max()
    ok &= show("fp32 cycle against the fp64 restatement", dev, 2e-6)
    zr32 = mg_model.apply_M32(L, r)
    ok &= show("fp32 cycle against the fp32 restatement", np.abs(z32 - zr32).max() / np.abs(zr32).max(), 2e-6)
    assert ok
    assert dev > 1e-9                                               # an fp64 cycle behind the flag agrees to 1e-13
    unshifted = R.apply_M(levels(N, dom, kind, 0.0), r)             # the test can tell a cycle that ignored the shift
    assert np.abs(unshifted - zr).max() / np.abs(zr).max() > 1e-3


# ---- multigrid-PCG solves ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", S.SIGMAS)
@pytest.mark.parametrize("N,kind,dom", CYCLE_GRIDS, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_mg_pcg_solves_match_the_trace(N, kind, dom, sigma):
    import iterative_solvers_amd as isa
    L = levels(N, dom, kind, sigma)
    b = S.rhs_vector(N)
    t = R.pcg_trace(L, b, eps=S.EPS)
    assert R.stop_margin(t, R.REL_2NORM, S.EPS) >= S.MARGIN         # tests/test_shift_cpu.py: it holds for every case
    tol = {q: R.tol_pcg(v) for q, v in R.spread(L, b, t.iterations, exact=t).items()}
    s = system(N, dom, kind, sigma=sigma)
    x, res = solve(s, rel_params(max_iterations=1000), b=b)
    print(f"N={N} sigma={sigma:g}: {res.iterations} iterations (reference {t.iterations})")
    assert res.iterations == t.iterations and bool(res.converged) == t.converged
    ok = show("x, max|x - x_ref| / max|x_ref|", np.abs(x - t.x[-1]).max() / np.abs(t.x[-1]).max(), tol["x"][-1])
    ok &= show("r_norm2", rel(res.r_norm2, t.r2[-1]), tol["r2"][-1])
    ok &= show("initial_r_norm2", rel(res.initial_r_norm2, t.b_norm2), tol["b2"][-1])
    assert ok
    s.set_preconditioner(kind, isa.CYCLE_F32)
    x32, res32 = solve(s, rel_params(max_iterations=1000))
    assert res32.converged and res32.iterations == res.iterations
    true = b - R.apply_A(L, x32)
    assert np.linalg.norm(true) <= 2e-8 * np.linalg.norm(b)


# ---- the two call orders ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cycle", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("N,kind", [(34, R.MG_ANY), (64, R.MG)])
def test_preconditioner_then_shift_is_shift_then_preconditioner(N, kind, cycle):
    sigma = 1e3
    a = system(N, kind=kind, cycle=cycle)
    info = a.preconditioner_info()
    a.set_shift(sigma)
    b = system(N, kind=kind, cycle=cycle, sigma=sigma)
    assert a.preconditioner_info() == info == b.preconditioner_info()
    r = np.random.default_rng(N).standard_normal(a.size())
    za, zb = a._handle.apply_preconditioner(r), b._handle.apply_preconditioner(r)
    assert np.array_equal(za, zb)
    plain = system(N, kind=kind, cycle=cycle)
    assert not np.array_equal(za, plain._handle.apply_preconditioner(r))
    xa, ra = solve(a, rel_params())
    xb, rb = solve(b, rel_params())
    assert ra.iterations == rb.iterations and ra.r_norm2 == rb.r_norm2 and np.array_equal(xa, xb)
    a.set_shift(0.0)                                                # and back: the handle that never had a shift
    assert np.array_equal(a._handle.apply_preconditioner(r), plain._handle.apply_preconditioner(r))
    assert a.preconditioner_info() == info


# ---- batches ---------------------------------------------------------------------------------------------------------------------------
def test_a_batch_has_the_bits_of_its_single_solves():
    from test_gpu_mg_batch import assert_same, sequential
    N, sigma = 34, 1e3
    s = system(N, kind=R.MG_ANY, sigma=sigma)
    rhs = np.stack([S.rhs_vector(N, seed) for seed in (1, 2, 3)])
    p = rel_params(max_iterations=1000)
    xs, rs = sequential(s, p, rhs)
    xb, rb = s._handle.solve_batch(p, rhs)
    assert all(r.converged for r in rs)
    assert_same(xb, rb, xs, rs)
    xw, rw = s._handle.solve_batch(p, rhs, x0=0.5 * xs)             # the warm entry points follow the shift too
    for k in range(3):
        xk, rk = solve(s, p, b=rhs[k], x0=0.5 * xs[k])
        assert rw[k].iterations == rk.iterations and np.array_equal(xw[k], xk)
    L = S.shifted_levels(N, R.ISO, R.MG_ANY, sigma)
    for k in range(3):
        assert np.linalg.norm(rhs[k] - R.apply_A(L, xb[k])) <= 2e-8 * np.linalg.norm(rhs[k])
    s.set_shift(0.0)                                                # the workspace stays across a change of sigma
    x0b, r0b = s._handle.solve_batch(p, rhs)
    x0s, r0s = sequential(s, p, rhs)
    assert_same(x0b, r0b, x0s, r0s)


# ---- warm starts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [None, R.MG_ANY], ids=["plain", "mg"])
def test_a_converged_shifted_solution_is_a_finished_warm_start(kind):
    N, sigma = 34, 1e3
    s = system(N, kind=kind, sigma=sigma)
    b = S.rhs_vector(N)
    x, res = solve(s, rel_params(eps=1e-11), b=b)
    assert res.converged and res.iterations > 0
    xw, rw = solve(s, rel_params(), x0=x)
    assert rw.iterations == 0 and rw.converged
    assert np.array_equal(xw, x)
    s.set_shift(0.0)                                                # the same guess does not solve the Laplacian
    _, r0 = solve(s, rel_params(), x0=x)
    assert r0.iterations > 0


# ---- the deferred x fold -------------------------------------------------------------------------------------------------------------------
def test_the_deferred_fold_follows_the_shift():
    N, sigma, k = 2400, 1e5, 70
    f, z = system(N, sigma=sigma), system(N, sigma=sigma, env={"MI355CG_XFOLD": "0"})
    assert f._handle.layout()["x_fold"] > 0 and z._handle.layout()["x_fold"] == 0
    p = rel_params(max_iterations=k, fixed=True)
    xf, rf = solve(f, p)
    xz, rz = solve(z, p)
    assert rf.iterations == rz.iterations == k and rf.r_norm2 == rz.r_norm2
    assert np.array_equal(xf, xz)
    plain = system(N, env={"MI355CG_XFOLD": "0"})
    assert not np.array_equal(solve(plain, p)[0], xz)
