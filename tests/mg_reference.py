"""The high-precision restatement the preconditioned-CG GPU tests compare against: the hierarchies and the
V-cycle of tests/mg_model.py on any domain, the PCG loop of solve_mg with exactly rounded inner products and every quantity the
library reports recorded per iteration, the loop's own sensitivity to the order of its sums, and the V-cycle in long double, its
smoother an argument.  A plain module: no test in here, nothing that needs a GPU or the oracle binaries.

Packed vectors are in the library's order (row-major over the interior nodes), as in mg_model."""
import math
import os
import sys
import threading
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model as model  # noqa: E402

ISO = (1.0, 2.0, 1.0, 2.0)
WIDE_Y = (0.0, 1.0, 0.0, 2.0)          # hy = 2 hx: xk = 4 yk
WIDE_X = (0.0, 3.0, 0.0, 1.0)          # hx = 3 hy: yk = 9 xk
MG, MG_ANY = 1, 2                      # MI355CG_PRECOND_MG, MI355CG_PRECOND_MG_ANY
REL_2NORM, MSG = "REL_2NORM", "MSG"
# stop reasons of a trace; the MSG ones carry the values of iterative_solvers_amd.StopCriterion
ITERATIONS, PRECISION, RESIDUAL, EXACT_ERROR = 0, 1, 2, 3
LD = np.longdouble


def levels_for(N, dom, kind, exchanged=False, sigma=0.0):
    """the restatement hierarchy of an N x N grid on the domain (a, b, c, d), of A - sigma I; exchanged=True builds the wrong one,
    with hx and hy exchanged (what the tests must be able to tell from the right one)"""
    a, b, c, d = dom
    hx, hy = (b - a) / N, (d - c) / N
    if exchanged:
        hx, hy = hy, hx
    return model.hierarchy(N, hx, hy, sigma) if kind == MG else model.hierarchy_any(N, hx, hy, sigma)


def apply_M(levels, r):
    """z = M r, one V-cycle"""
    return model.apply_M(levels, r)


def apply_A(levels, v):
    """A v for a packed v on level 0"""
    L = levels[0]
    return model.packed(L, model.apply_A(L, model.grid(L, v)))


# ---- sums -----------------------------------------------------------------------------------------------------------------------
def _fsum(v):
    return math.fsum(v.tolist())                                   # exactly rounded


def _reversed_sum(v):
    return float(np.cumsum(v[::-1])[-1]) if v.size else 0.0        # cumsum adds serially: the naive sum, last element first


# ---- the PCG of solve_mg ---------------------------------------------------------------------------------------------------------
def pcg_trace(levels, b, u=None, x0=None, iterations=None, rule=REL_2NORM, eps=1e-8, eps_exact_error=None, max_iterations=100,
              M=None, total=_fsum):
    """Hestenes-Stiefel PCG as solve_mg states it: z = M r, beta = rz / rho, p = z + beta p, q = A p, alpha = rho / (p, q),
    x += alpha p, r -= alpha q, dx = x_new - x_old.  Every inner product and squared norm is total() of the elementwise products
    (default: math.fsum).  iterations = k runs exactly k iterations without stop tests (fixed_iterations); otherwise rule decides:
      REL_2NORM  before every iteration, stop when not ||r|| > eps ||r0|| (||b|| with a guess x0); converged = ||r|| <= eps ||r0||
      MSG        after every iteration, in this order, each strict: max|dx| < eps -> PRECISION, max|r| < eps -> RESIDUAL,
                 max|x - u| < eps_exact_error (default eps) -> EXACT_ERROR; an eps <= 0, or no u, switches that test off
    M: another preconditioner, a function of the packed r (the fp32 cycle's restatement).
    Returns a namespace: iterations, converged, reason, b_norm2, r0_norm2, r0_max, e0_max, and one entry per iteration in x and in
    dx2, r2 (recursive), true2 (||b - A x||), e2, dx_max, r_max, e_max (the error norms only with u)."""
    sq = lambda v: math.sqrt(total(v * v))
    amax = lambda v: float(np.abs(v).max())
    M = (lambda r: apply_M(levels, r)) if M is None else M
    if eps_exact_error is None:
        eps_exact_error = eps
    x = np.zeros_like(b) if x0 is None else x0.copy()
    r = b.copy() if x0 is None else b - apply_A(levels, x)
    t = SimpleNamespace(x=[], dx2=[], r2=[], true2=[], e2=[], dx_max=[], r_max=[], e_max=[], converged=False, reason=ITERATIONS)
    t.b_norm2, t.r0_norm2, t.r0_max = sq(b), sq(r), amax(r)
    t.e0_max = amax(x - u) if u is not None else None
    refnorm = t.r0_norm2 if x0 is None else t.b_norm2
    rnorm, rho, p, it = t.r0_norm2, 0.0, None, 0
    cap = max_iterations if iterations is None else iterations
    while it < cap:
        if iterations is None and rule == REL_2NORM and not rnorm > eps * refnorm:
            break
        z = M(r)
        rz = total(r * z)
        p = z if it == 0 else z + (rz / rho) * p
        rho = rz
        q = apply_A(levels, p)
        alpha = rho / total(p * q)
        xn = x + alpha * p
        r = r - alpha * q
        dx = xn - x
        x = xn
        it += 1
        rnorm = sq(r)
        t.x.append(x)
        t.dx2.append(sq(dx)); t.r2.append(rnorm); t.true2.append(sq(b - apply_A(levels, x)))
        t.dx_max.append(amax(dx)); t.r_max.append(amax(r))
        if u is not None:
            t.e2.append(sq(x - u)); t.e_max.append(amax(x - u))
        if iterations is None and rule == MSG:
            if eps > 0 and t.dx_max[-1] < eps: t.converged, t.reason = True, PRECISION; break
            if eps > 0 and t.r_max[-1] < eps: t.converged, t.reason = True, RESIDUAL; break
            if eps_exact_error > 0 and u is not None and t.e_max[-1] < eps_exact_error: t.converged, t.reason = True, EXACT_ERROR; break
    if rule == REL_2NORM:
        t.converged = rnorm <= eps * refnorm
    t.iterations = it
    return t


SCALARS = ("dx2", "r2", "e2", "dx_max", "r_max", "e_max")


def spread(levels, b, iterations, u=None, M=None, exact=None):
    """The reference's own sensitivity to the order of its sums: the trace run again with naive sums in reversed element order.
    Returns a dict of arrays, one entry per iteration: 'x' = max|x_fsum - x_rev| / max|x_fsum|, every scalar of SCALARS its
    relative difference, 'b2' that of ||b||_2, 'true2' its difference over ||b||_2 (the true residual is a difference of large
    terms; the tests bound it that way), and 'all' the largest of them.  exact: the fsum trace if the caller has it."""
    a = pcg_trace(levels, b, u=u, iterations=iterations, M=M) if exact is None else exact
    v = pcg_trace(levels, b, u=u, iterations=iterations, M=M, total=_reversed_sum)
    out = {"x": np.array([np.abs(xa - xv).max() / np.abs(xa).max() for xa, xv in zip(a.x[:iterations], v.x)])}
    for name in SCALARS:
        sa, sv = np.array(getattr(a, name)[:iterations]), np.array(getattr(v, name))
        if sa.size:
            out[name] = np.abs(sa - sv) / np.abs(sa)
    out["true2"] = np.abs(np.array(a.true2[:iterations]) - np.array(v.true2)) / a.b_norm2
    out["b2"] = np.full(iterations, abs(a.b_norm2 - v.b_norm2) / a.b_norm2)
    out["all"] = np.max(np.stack(list(out.values())), axis=0)
    return out


def tol_pcg(spread_all):
    """the bound on a PCG quantity, per iteration"""
    return np.maximum(1e-13, 64.0 * np.asarray(spread_all))


def tol_M(floor):
    """the bound on the fp64 device cycle against the restatement"""
    return max(1e-13, 16.0 * floor)


# ---- stop margins ----------------------------------------------------------------------------------------------------------------
def stop_margin(t, rule, eps, eps_exact_error=None):
    """How far the numbers that decide a rule-driven trace stay from their thresholds: the smallest |value / threshold - 1| over
    every test the loop made -- those that did not fire (every iteration before the last, and on the last the tests in front of
    the one that fired) and the one that did.  A trace that ran into its iteration cap has no deciding test: 0."""
    if eps_exact_error is None:
        eps_exact_error = eps
    if not t.converged:
        return 0.0
    m = []
    if rule == REL_2NORM:
        thr = eps * t.r0_norm2
        for i, v in enumerate([t.r0_norm2] + t.r2):
            ratio = v / thr
            assert (ratio <= 1.0) == (i == t.iterations)
            m.append(abs(ratio - 1.0))
        return min(m)
    for i in range(t.iterations):
        tests = [(PRECISION, t.dx_max[i], eps), (RESIDUAL, t.r_max[i], eps)]
        if t.e_max:
            tests.append((EXACT_ERROR, t.e_max[i], eps_exact_error))
        for reason, v, e in tests:
            if not e > 0:
                continue
            ratio = v / e
            fires = i == t.iterations - 1 and reason == t.reason
            assert (ratio < 1.0) == fires
            m.append(abs(ratio - 1.0))
            if fires:
                break
    return min(m)


# The plain formulas of mg_model in long double would do; the row blocks, the threads and the tap-based transfers below are
# there only for the time a cycle takes at N = 4100 (long double has no SIMD and no BLAS).  test_mg_reference_cpu pins the
# result to apply_M at 1e-14.
# ---- the V-cycle in long double ----------------------------------------------------------------------------------------------------
_POOL = ThreadPoolExecutor(max_workers=8)
_SCRATCH = threading.local()
_BLOCK = 64                                                        # rows per block of a sweep


def _sweep_ld(L, u, r, smooth):
    """smooth: t = u + omega ((r - A u) / diag), else s = r - A u; at the interior nodes, 0 elsewhere.  Long double has no SIMD, and
    NumPy releases the GIL inside an array operation: blocks of rows go to a few threads, each with two scratch blocks of its own,
    so that no operation allocates."""
    N = L.N
    out = np.zeros_like(u)
    d, xk, yk, om = LD(L.diag), LD(L.xk), LD(L.yk), LD(model.OMEGA)

    def rows(lo):
        hi = min(lo + _BLOCK, N)
        if getattr(_SCRATCH, "n", 0) < N:
            _SCRATCH.a, _SCRATCH.b, _SCRATCH.n = np.empty((_BLOCK, N - 1), dtype=LD), np.empty((_BLOCK, N - 1), dtype=LD), N
        a, b = _SCRATCH.a[:hi - lo, :N - 1], _SCRATCH.b[:hi - lo, :N - 1]
        c = u[lo:hi, 1:-1]
        np.add(u[lo:hi, :-2], u[lo:hi, 2:], out=a)
        a *= xk
        np.add(u[lo - 1:hi - 1, 1:-1], u[lo + 1:hi + 1, 1:-1], out=b)
        b *= yk
        a += b
        np.multiply(c, d, out=b)
        a += b                                                      # a = A u
        np.subtract(r[lo:hi, 1:-1], a, out=a)
        if smooth:
            a /= d
            a *= om
            a += c
        a *= L.mask[lo:hi, 1:-1]
        out[lo:hi, 1:-1] = a
    list(_POOL.map(rows, range(1, N, _BLOCK)))
    return out


def apply_A_longdouble(levels, g):
    """A g on level 0 for a long double grid g (zero off the interior), coefficients promoted"""
    return -_sweep_ld(levels[0], g, np.zeros_like(g), False)


def _smooth_ld(L, u, r):
    return _sweep_ld(L, u, r, True)


def _taps(Nf, Nc):
    """the 1-D transfer of mg_model.weights(Nf, Nc) without the dense matrix: per coarse node X the <= 5 fine nodes of its support
    (clipped to the grid; a node off the support has weight 0) and their long double weights"""
    X = np.arange(Nc + 1, dtype=np.int64)
    lo = (X - 1) * Nf // Nc + 1
    idx = np.clip(lo[:, None] + np.arange(5)[None, :], 0, Nf)
    d = np.abs(idx * Nc - X[:, None] * Nf)
    return idx, np.where(d < Nf, (Nf - d) / Nf, 0.0).astype(LD)                # the fp64 weights, promoted


def _col_blocks(fn, n):
    """fn(lo, hi) over the columns 0 .. n - 1 in blocks, on the threads of _sweep_ld where the grid is large"""
    if n < 512:
        return fn(0, n)
    step = -(-n // 32)
    list(_POOL.map(lambda lo: fn(lo, min(lo + step, n)), range(0, n, step)))


def _restrict_rows_ld(s, idx, w):
    """W s along the first axis: out[X, :] = sum_k w[X, k] s[idx[X, k], :]"""
    out = np.empty((idx.shape[0], s.shape[1]), dtype=LD)

    def cols(lo, hi):
        acc = w[:, 0, None] * s[idx[:, 0], lo:hi]
        for k in range(1, idx.shape[1]):
            acc += w[:, k, None] * s[idx[:, k], lo:hi]
        out[:, lo:hi] = acc
    _col_blocks(cols, s.shape[1])
    return out


def _prolong_rows_ld(e, Nf, idx, w):
    """W^T e along the first axis, by the two coarse neighbours of every fine node"""
    Nc = e.shape[0] - 1
    x = np.arange(Nf + 1, dtype=np.int64)
    X0 = np.minimum(x * Nc // Nf, Nc - 1)
    wt = lambda X: np.where(np.abs(x * Nc - X * Nf) < Nf, (Nf - np.abs(x * Nc - X * Nf)) / Nf, 0.0).astype(LD)
    w0, w1 = wt(X0)[:, None], wt(X0 + 1)[:, None]
    out = np.empty((Nf + 1, e.shape[1]), dtype=LD)

    def cols(lo, hi):
        out[:, lo:hi] = w0 * e[X0, lo:hi] + w1 * e[X0 + 1, lo:hi]
    _col_blocks(cols, e.shape[1])
    return out


def _vcycle_ld(levels, l, r, smooth=_smooth_ld):
    L = levels[l]
    if l == len(levels) - 1:
        g = np.zeros_like(r)
        g[L.mask] = L.inv.astype(LD) @ r[L.mask]
        return g
    Cl = levels[l + 1]
    u = smooth(L, np.zeros_like(r), r)
    u = smooth(L, u, r)
    s = _sweep_ld(L, u, r, False)
    idx, w = _taps(L.N, Cl.N)                                       # nested or not: R = (N_c / N_f)^2 W s W^T, P = W^T e W
    rc = LD(Cl.N * Cl.N / (L.N * L.N)) * _restrict_rows_ld(_restrict_rows_ld(s, idx, w).T, idx, w).T
    rc[~Cl.mask] = 0
    e = _vcycle_ld(levels, l + 1, rc, smooth)
    pe = _prolong_rows_ld(_prolong_rows_ld(e, L.N, idx, w).T, L.N, idx, w).T
    pe[~L.mask] = 0
    u = u + pe
    u = smooth(L, u, r)
    return smooth(L, u, r)


def apply_M_longdouble(levels, r, smooth=_smooth_ld):
    """z = M r with every array and every coefficient of the fp64 restatement (diagonal, x_k, y_k, omega, the transfer weights,
    the coarse inverse) promoted to long double: the same operator, its rounding errors some 2^-11 of the fp64 cycle's."""
    L = levels[0]
    g = np.zeros((L.N + 1, L.N + 1), dtype=LD)
    g[L.mask] = r.astype(LD)
    return _vcycle_ld(levels, 0, g, smooth)[L.mask]


def cycle_floor(levels, r, z=None):
    """max|apply_M - apply_M_longdouble| / max|apply_M_longdouble|: the fp64 rounding floor of the cycle on r"""
    z = apply_M(levels, r) if z is None else z
    zl = apply_M_longdouble(levels, r)
    return float(np.abs(z.astype(LD) - zl).max() / np.abs(zl).max())
