"""The NumPy restatement of the multigrid preconditioner (include/mi355cg.h), written once: the hierarchy rules
of mi355cg_mg_levels and mi355cg_mg_hierarchy, the level operators, the V-cycle with the smoother as an argument, its float32 run
(MI355CG_CYCLE_F32) and the plain PCG loop.  Every multigrid, shift, line-smoother, eigen, warm-start and
time-stepping test is judged against these functions.  A plain module: no test in here, nothing that needs a GPU or the oracle
binaries.

Grids are (N+1) x (N+1) arrays indexed [y, x]; every node off the L-shaped interior holds 0.  The packed order of the library is
the row-major order of the interior nodes, i.e. v2d[interior_mask(N)].

Ladder: N_{l+1} = 2 floor(N_l / 4) while N_l > 32.  A level with N_f = 2 N_c is nested: full weighting and bilinear prolongation.
Any other (N_f % 4 == 2) keeps the domain (h_c = h_f N_f / N_c) and transfers by the 1-D bilinear weights
w(x, X) = max(0, 1 - |x N_c - X N_f| / N_f): P e = W^T e W masked to the fine interior, R s = (N_c / N_f)^2 W s W^T masked to
the coarse interior, so R = (N_c / N_f)^2 P^T.

The level operators work in the dtype of the array they are given, with every level constant (diagonal, x_k, y_k, omega,
(N_c / N_f)^2, the non-nested weights, the coarse inverse) the fp64 value rounded to that dtype: the float32 cycle is the same
code run on a float32 grid over the same levels."""
import numpy as np

OMEGA = 0.8
DOM = (1.0, 2.0, 1.0, 2.0)


def steps(N):
    a, b, c, d = DOM
    return (b - a) / N, (d - c) / N


def interior_mask(N):
    y, x = np.mgrid[0:N + 1, 0:N + 1]
    h = N // 2
    return (y >= 1) & (y <= N - 1) & (x <= N - 1) & (x >= np.where(y <= h, h + 1, 1))


class Level:
    def __init__(self, N, hx, hy):
        self.N, self.mask, self.hx, self.hy = N, interior_mask(N), hx, hy
        self.xk, self.yk = 1 / (hx * hx), 1 / (hy * hy)
        self.diag = -2 * (self.xk + self.yk)
        self.inv = None


def grid(L, v):
    g = np.zeros((L.N + 1, L.N + 1), dtype=v.dtype)
    g[L.mask] = v
    return g


def packed(L, g):
    return g[L.mask]


def ladder(N):
    ns = [N]
    while ns[-1] > 32:
        ns.append(2 * (ns[-1] // 4))
    return ns


def weights(Nf, Nc):
    """W[X, x] = w(x, X); the numerator |x N_c - X N_f| is an exact integer"""
    d = np.abs(np.arange(Nf + 1, dtype=np.int64)[None, :] * Nc - np.arange(Nc + 1, dtype=np.int64)[:, None] * Nf)
    return np.where(d < Nf, (Nf - d) / Nf, 0.0)


# ---- hierarchies ----------------------------------------------------------------------------------------------------------------
def coarse_inverse(C):
    """the dense A_L^-1 of level C, with the diagonal C has now, from the Cholesky factor of -A_L"""
    n = int(C.mask.sum())
    S = np.empty((n, n))
    for j in range(n):
        e = np.zeros(n)
        e[j] = 1.0
        S[:, j] = -packed(C, apply_A(C, grid(C, e)))
    T = np.linalg.inv(np.linalg.cholesky(S))
    return -(T.T @ T)


def _finish(levels, sigma):
    """A - sigma I on every level (the same sigma, no scaling), then the coarsest level's inverse"""
    for L in levels:
        L.diag = L.diag - sigma
    levels[-1].inv = coarse_inverse(levels[-1])
    return levels


def hierarchy(N, hx, hy, sigma=0.0):
    """MI355CG_PRECOND_MG: levels N, N/2, ... while N_l % 4 == 0 and N_l > 32"""
    levels = [Level(N, hx, hy)]
    while levels[-1].N % 4 == 0 and levels[-1].N > 32:
        L = levels[-1]
        levels.append(Level(L.N // 2, 2 * L.hx, 2 * L.hy))
    if levels[-1].N > 32:
        raise ValueError(f"grid {N} has no hierarchy")
    return _finish(levels, sigma)


def hierarchy_any(N, hx, hy, sigma=0.0):
    """MI355CG_PRECOND_MG_ANY: the levels of ladder(N); a non-nested level carries its weights W"""
    levels = [Level(N, hx, hy)]
    for Nc in ladder(N)[1:]:
        F = levels[-1]
        if F.N == 2 * Nc:
            levels.append(Level(Nc, 2 * F.hx, 2 * F.hy))
        else:
            levels.append(Level(Nc, F.hx * F.N / Nc, F.hy * F.N / Nc))
            F.W = weights(F.N, Nc)
    return _finish(levels, sigma)


# ---- level operators, in the dtype of their argument ------------------------------------------------------------------------------
def _rounded(L, name, dt):
    """L.W or L.inv rounded to dt; the copy is kept on the level for as long as the fp64 array is the same object"""
    a = getattr(L, name)
    if a.dtype == dt:
        return a
    kept = L.__dict__.setdefault("_rounded", {})
    if (name, dt) not in kept or kept[name, dt][0] is not a:
        kept[name, dt] = (a, a.astype(dt))
    return kept[name, dt][1]


def apply_A(L, u):
    dt = u.dtype.type
    out = np.zeros_like(u)
    out[1:-1, 1:-1] = dt(L.diag) * u[1:-1, 1:-1] + dt(L.xk) * (u[1:-1, :-2] + u[1:-1, 2:]) + dt(L.yk) * (u[:-2, 1:-1] + u[2:, 1:-1])
    out[~L.mask] = 0
    return out


def smooth(L, u, r):
    """one damped point-Jacobi sweep t = u + omega (r - A u) / diag"""
    dt = u.dtype.type
    t = u + dt(OMEGA) * ((r - apply_A(L, u)) / dt(L.diag))
    t[~L.mask] = 0
    return t


def restrict(F, C, s, nested=None):
    """nested (by default: whether the pair is): full weighting 1/16 [1 2 1; 2 4 2; 1 2 1] at fine node (2X, 2Y) for every coarse
    interior node; else by the weights"""
    dt = s.dtype.type
    if not (F.N == 2 * C.N if nested is None else nested):
        W = _rounded(F, "W", dt)
        out = dt(C.N * C.N / (F.N * F.N)) * (W @ s @ W.T)
    else:
        c = s[2:-1:2, 2:-1:2]
        l, r = s[2:-1:2, 1:-2:2], s[2:-1:2, 3::2]
        d, u = s[1:-2:2, 2:-1:2], s[3::2, 2:-1:2]
        ld, rd = s[1:-2:2, 1:-2:2], s[1:-2:2, 3::2]
        lu, ru = s[3::2, 1:-2:2], s[3::2, 3::2]
        out = np.zeros((C.N + 1, C.N + 1), dtype=dt)
        out[1:-1, 1:-1] = dt(0.0625) * (dt(4) * c + dt(2) * (l + r + d + u) + (ld + rd + lu + ru))
    out[~C.mask] = 0
    return out


def prolong(F, C, e, nested=None):
    """nested: bilinear interpolation of the coarse correction, else by the weights; masked to the fine interior"""
    dt = e.dtype.type
    if not (F.N == 2 * C.N if nested is None else nested):
        W = _rounded(F, "W", dt)
        f = W.T @ e @ W
    else:
        f = np.zeros((F.N + 1, F.N + 1), dtype=dt)
        f[0::2, 0::2] = e
        f[0::2, 1::2] = dt(0.5) * (e[:, :-1] + e[:, 1:])
        f[1::2, 0::2] = dt(0.5) * (e[:-1, :] + e[1:, :])
        f[1::2, 1::2] = dt(0.25) * (e[:-1, :-1] + e[:-1, 1:] + e[1:, :-1] + e[1:, 1:])
    f[~F.mask] = 0
    return f


# ---- the cycle ----------------------------------------------------------------------------------------------------------------------
def vcycle(levels, l, r, smoother=smooth):
    L = levels[l]
    if l == len(levels) - 1:
        return grid(L, _rounded(L, "inv", r.dtype.type) @ packed(L, r))
    C = levels[l + 1]
    u = smoother(L, np.zeros_like(r), r)
    u = smoother(L, u, r)
    s = r - apply_A(L, u)
    s[~L.mask] = 0
    e = vcycle(levels, l + 1, restrict(L, C, s), smoother)
    assert e.dtype == r.dtype
    u = u + prolong(L, C, e)
    u = smoother(L, u, r)
    return smoother(L, u, r)


def apply_M(levels, r_packed, smoother=smooth):
    return packed(levels[0], vcycle(levels, 0, grid(levels[0], r_packed), smoother))


def apply_M32(levels, r_packed, scaled=True):
    """z = M32 r for a float64 packed r:  s = 2^e with max|r| = m 2^e, 0.5 <= m < 1;  r32 = fl32(r / s);  the V-cycle on the float32
    grid;  z = s * float64(z32).  scaled=False leaves out the power-of-two scale (what the scale is there to prevent)"""
    L = levels[0]
    assert r_packed.dtype == np.float64
    rmax = np.abs(r_packed).max()
    if rmax == 0:
        return np.zeros_like(r_packed)
    e = int(np.frexp(rmax)[1]) if scaled else 0
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        z32 = vcycle(levels, 0, grid(L, np.ldexp(r_packed, -e).astype(np.float32)))
    assert z32.dtype == np.float32
    return np.ldexp(z32[L.mask].astype(np.float64), e)


def pcg(levels, b, eps=1e-8, max_iterations=100, M=None):
    """Hestenes-Stiefel PCG from x = 0, REL_2NORM stop on the recursive residual; returns (x, iterations).  M: another
    preconditioner, a function of the packed r (default: apply_M on levels)."""
    L = levels[0]
    M = (lambda r: apply_M(levels, r)) if M is None else M
    x = np.zeros_like(b)
    r = b.copy()
    r0 = np.linalg.norm(r)
    it, rho, p = 0, 0.0, None
    while it < max_iterations and np.linalg.norm(r) > eps * r0:
        z = M(r)
        rz = r @ z
        p = z if it == 0 else z + (rz / rho) * p
        rho = rz
        q = packed(L, apply_A(L, grid(L, p)))
        alpha = rho / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        it += 1
    return x, it
