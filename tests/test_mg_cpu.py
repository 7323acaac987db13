"""The multigrid preconditioner without a GPU: the hierarchy rule of mi355cg_mg_levels, and a NumPy restatement of the algorithm
(include/mi355cg.h) that tests/test_gpu_mg.py compares the device against.

Grids are (N+1) x (N+1) arrays indexed [y, x]; every node off the L-shaped interior holds 0.  The packed order of the library is
the row-major order of the interior nodes, i.e. v2d[interior_mask(N)]."""
import numpy as np
import pytest

OMEGA = 0.8


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


def hierarchy(N, hx, hy):
    """Levels N, N/2, ... while N_l % 4 == 0 and N_l > 32; the coarsest gets A_L^-1 from the Cholesky factor of -A_L."""
    levels = [Level(N, hx, hy)]
    while levels[-1].N % 4 == 0 and levels[-1].N > 32:
        L = levels[-1]
        levels.append(Level(L.N // 2, 2 * L.hx, 2 * L.hy))
    C = levels[-1]
    if C.N > 32:
        raise ValueError(f"grid {N} has no hierarchy")
    n = int(C.mask.sum())
    S = np.empty((n, n))
    for j in range(n):
        e = np.zeros(n)
        e[j] = 1.0
        S[:, j] = -packed(C, apply_A(C, grid(C, e)))
    Lc = np.linalg.cholesky(S)
    T = np.linalg.inv(Lc)
    C.inv = -(T.T @ T)
    return levels


def grid(L, v):
    g = np.zeros((L.N + 1, L.N + 1))
    g[L.mask] = v
    return g


def packed(L, g):
    return g[L.mask]


def apply_A(L, u):
    out = np.zeros_like(u)
    out[1:-1, 1:-1] = L.diag * u[1:-1, 1:-1] + L.xk * (u[1:-1, :-2] + u[1:-1, 2:]) + L.yk * (u[:-2, 1:-1] + u[2:, 1:-1])
    out[~L.mask] = 0.0
    return out


def smooth(L, u, r):
    t = u + OMEGA * ((r - apply_A(L, u)) / L.diag)
    t[~L.mask] = 0.0
    return t


def restrict(F, C, s):
    """full weighting 1/16 [1 2 1; 2 4 2; 1 2 1] at fine node (2X, 2Y) for every coarse interior node"""
    c = s[2:-1:2, 2:-1:2]
    l, r = s[2:-1:2, 1:-2:2], s[2:-1:2, 3::2]
    d, u = s[1:-2:2, 2:-1:2], s[3::2, 2:-1:2]
    ld, rd = s[1:-2:2, 1:-2:2], s[1:-2:2, 3::2]
    lu, ru = s[3::2, 1:-2:2], s[3::2, 3::2]
    out = np.zeros((C.N + 1, C.N + 1))
    out[1:-1, 1:-1] = 0.0625 * (4.0 * c + 2.0 * (l + r + d + u) + (ld + rd + lu + ru))
    out[~C.mask] = 0.0
    return out


def prolong(F, e):
    """bilinear interpolation of the coarse correction, masked to the fine interior"""
    f = np.zeros((F.N + 1, F.N + 1))
    f[0::2, 0::2] = e
    f[0::2, 1::2] = 0.5 * (e[:, :-1] + e[:, 1:])
    f[1::2, 0::2] = 0.5 * (e[:-1, :] + e[1:, :])
    f[1::2, 1::2] = 0.25 * (e[:-1, :-1] + e[:-1, 1:] + e[1:, :-1] + e[1:, 1:])
    f[~F.mask] = 0.0
    return f


def vcycle(levels, l, r):
    L = levels[l]
    if l == len(levels) - 1:
        return grid(L, L.inv @ packed(L, r))
    u = smooth(L, np.zeros_like(r), r)
    u = smooth(L, u, r)
    s = r - apply_A(L, u)
    s[~L.mask] = 0.0
    e = vcycle(levels, l + 1, restrict(L, levels[l + 1], s))
    u = u + prolong(L, e)
    u = smooth(L, u, r)
    return smooth(L, u, r)


def apply_M(levels, r_packed):
    return packed(levels[0], vcycle(levels, 0, grid(levels[0], r_packed)))


def pcg(levels, b, eps=1e-8, max_iterations=100):
    """Hestenes-Stiefel PCG from x = 0, REL_2NORM stop on the recursive residual; returns (x, iterations)."""
    L = levels[0]
    x = np.zeros_like(b)
    r = b.copy()
    r0 = np.linalg.norm(r)
    it, rho, p = 0, 0.0, None
    while it < max_iterations and np.linalg.norm(r) > eps * r0:
        z = apply_M(levels, r)
        rz = r @ z
        p = z if it == 0 else z + (rz / rho) * p
        rho = rz
        q = packed(L, apply_A(L, grid(L, p)))
        alpha = rho / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        it += 1
    return x, it


# ---- the library's hierarchy rule (host arithmetic: no GPU) -------------------------------------------------------------
@pytest.mark.parametrize("n,expected", [(6, (1, 6)), (10, (1, 10)), (16, (1, 16)), (32, (1, 32)), (64, (2, 32)),
                                        (256, (4, 32)), (4096, (8, 32)), (32768, (11, 32))])
def test_mg_levels(n, expected):
    import iterative_solvers_amd as isa
    assert isa.mg_levels(n) == expected


@pytest.mark.parametrize("n", [258, 1000])
def test_mg_levels_refuses_grids_without_a_hierarchy(n):
    import iterative_solvers_amd as isa
    with pytest.raises(ValueError, match="no multigrid hierarchy"):
        isa.mg_levels(n)


def test_mg_levels_through_the_c_abi():
    import ctypes as C
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    L, nc = C.c_int(), C.c_int()
    assert lib.mi355cg_mg_levels(4096, C.byref(L), C.byref(nc)) == _capi.OK and (L.value, nc.value) == (8, 32)
    assert lib.mi355cg_mg_levels(258, C.byref(L), C.byref(nc)) == _capi.ERR_INVALID
    assert b"no multigrid hierarchy" in lib.mi355cg_last_error()


def test_restatement_hierarchy_matches_the_rule():
    assert [L.N for L in hierarchy(256, 1 / 256, 1 / 256)] == [256, 128, 64, 32]
    with pytest.raises(ValueError):
        hierarchy(1000, 1e-3, 1e-3)


# ---- the restatement itself --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 64, 256])
def test_restatement_is_symmetric_and_negative_definite(N):
    levels = hierarchy(N, 1 / N, 1 / N)
    rng = np.random.default_rng(N)
    n = int(levels[0].mask.sum())
    for _ in range(3):
        u, v = rng.standard_normal(n), rng.standard_normal(n)
        Mu, Mv = apply_M(levels, u), apply_M(levels, v)
        assert abs(Mu @ v - u @ Mv) <= 1e-12 * abs(Mu @ v)
        assert Mu @ u < 0 and Mv @ v < 0


def test_restatement_single_level_is_the_exact_inverse():
    levels = hierarchy(16, 1 / 16, 1 / 16)
    L = levels[0]
    b = np.random.default_rng(1).standard_normal(int(L.mask.sum()))
    z = apply_M(levels, b)
    assert np.abs(packed(L, apply_A(L, grid(L, z))) - b).max() <= 1e-12 * np.abs(b).max()


def test_restatement_pcg_converges_in_at_most_10_iterations_at_n256():
    N = 256
    levels = hierarchy(N, 1 / N, 1 / N)
    L = levels[0]
    b = np.random.default_rng(7).standard_normal(int(L.mask.sum()))
    x, it = pcg(levels, b)
    assert it <= 10, it
    true_r = b - packed(L, apply_A(L, grid(L, x)))
    assert np.linalg.norm(true_r) <= 2e-8 * np.linalg.norm(b)
