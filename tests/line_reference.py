"""The restatement of the line smoother of the fp64 V-cycle (mi355cg_set_smoother) on top of
tests/mg_model.py and tests/mg_reference.py, imported, not copied: the line solve (Thomas with the reciprocal pivots the device
keeps in its tables, vectorised across the lines of one length), the sweep t = u + omega T^-1 (r - A u) as the smoother of
their V-cycles, in fp64 and in long double for the rounding floor.  A plain module: no test in here, nothing that needs a GPU.

Directions carry the values mi355cg_get_smoother reports: 0 = damped point Jacobi, 1 = lines along x (rows), 2 = lines along y
(columns).  Grids are [y, x] arrays as in mg_model; the L-shaped interior is symmetric under x <-> y, so a solve along
columns is the solve along rows of the transposed grid with y_k in the place of x_k."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model as ref  # noqa: E402
import mg_reference as R  # noqa: E402

JACOBI, LINE_X, LINE_Y = 0, 1, 2
LD = np.longdouble
# the domains of the record in DESIGN section 10.8
SQUARE = (0.0, 1.0, 0.0, 1.0)
STRETCH_X = (0.0, 10.0, 0.0, 1.0)      # hx = 10 hy: y_k = 100 x_k, the lines run along y
STRETCH_Y = (0.0, 1.0, 0.0, 10.0)      # x_k = 100 y_k, the lines run along x
DOMAINS = (SQUARE, (0.0, 3.0, 0.0, 1.0), STRETCH_X, STRETCH_Y, (0.0, 32.0, 0.0, 1.0), (0.0, 1.0, 0.0, 100.0), (0.0, 1.0, 0.0, 32.0))


def auto_direction(levels):
    """MI355CG_SMOOTHER_LINE_AUTO: y-lines if level 0 has y_k > x_k, else x-lines; one decision for all levels"""
    return LINE_Y if levels[0].yk > levels[0].xk else LINE_X


def thomas_table(diag, k, n, dtype=np.float64):
    """inv_i = 1 / (diag - k cp_{i-1}), cp_i = k inv_i for i = 1 .. n (index 0 unused, cp_0 = 0): a line of length m <= n uses
    the first m entries"""
    inv, cp = np.zeros(n + 1, dtype=dtype), np.zeros(n + 1, dtype=dtype)
    diag, k, one = dtype(diag), dtype(k), dtype(1)
    for i in range(1, n + 1):
        inv[i] = one / (diag - k * cp[i - 1])
        cp[i] = k * inv[i]
    return inv, cp


def _solve_rows(s, k, inv, cp):
    """T e = s for every row of s (rows x n): d_i = (s_i - k d_{i-1}) inv_i, e_i = d_i - cp_i e_{i+1}"""
    n = s.shape[1]
    d = np.empty_like(s)
    carry = np.zeros(s.shape[0], dtype=s.dtype)
    for i in range(n):
        carry = (s[:, i] - k * carry) * inv[i + 1]
        d[:, i] = carry
    carry = np.zeros(s.shape[0], dtype=s.dtype)
    for i in range(n - 1, -1, -1):
        carry = d[:, i] - cp[i + 1] * carry
        d[:, i] = carry
    return d


def line_solve(L, s, direction):
    """e = T^-1 s on the interior of level L (s is 0 off it), T = diag and the two neighbours along the lines of `direction`"""
    dtype = s.dtype.type
    N, h = L.N, L.N // 2
    k = dtype(L.xk if direction == LINE_X else L.yk)
    inv, cp = thomas_table(L.diag, k, N - 1, dtype)
    g = s if direction == LINE_X else s.T
    e = np.zeros_like(g)
    e[1:h + 1, h + 1:N] = _solve_rows(g[1:h + 1, h + 1:N], k, inv, cp)       # the short lines, N/2 - 1 nodes
    e[h + 1:N, 1:N] = _solve_rows(g[h + 1:N, 1:N], k, inv, cp)               # the long ones, N - 1
    return e if direction == LINE_X else e.T


def smooth_line(L, u, r, direction):
    """one damped line-Jacobi sweep t = u + omega T^-1 (r - A u)"""
    s = r - ref.apply_A(L, u)
    s[~L.mask] = 0.0
    t = u + ref.OMEGA * line_solve(L, s, direction)
    t[~L.mask] = 0.0
    return t


def smoother_of(direction):
    """the smoother of `direction` as mg_model.vcycle takes it"""
    return functools.partial(smooth_line, direction=direction) if direction else ref.smooth


def apply_M_line(levels, r_packed, direction):
    """z = M r with the smoother of `direction` (0: the point cycle, bit for bit mg_reference.apply_M)"""
    return ref.apply_M(levels, r_packed, smoother_of(direction))


def M_of(levels, direction):
    """the preconditioner as mg_reference.pcg_trace, spread and stop_margin take it"""
    return lambda r: apply_M_line(levels, r, direction)


# ---- the same in long double ------------------------------------------------------------------------------------------------------
def _smooth_ld(L, u, r, direction):
    if not direction:
        return R._smooth_ld(L, u, r)
    s = R._sweep_ld(L, u, r, False)                                  # r - A u at the interior nodes, 0 elsewhere
    t = u + LD(ref.OMEGA) * line_solve(L, s, direction)
    t[~L.mask] = 0
    return t


def apply_M_line_longdouble(levels, r, direction):
    """z = M r with every array and coefficient of the fp64 restatement, the Thomas factors included, in long double"""
    return R.apply_M_longdouble(levels, r, functools.partial(_smooth_ld, direction=direction))


def cycle_floor_line(levels, r, direction, z=None):
    """max|apply_M_line - apply_M_line_longdouble| / max|apply_M_line_longdouble|: the fp64 rounding floor of the line cycle on r"""
    z = apply_M_line(levels, r, direction) if z is None else z
    zl = apply_M_line_longdouble(levels, r, direction)
    return float(np.abs(z.astype(LD) - zl).max() / np.abs(zl).max())


# ---- the inputs the CPU and the GPU tests share ------------------------------------------------------------------------------------
CYCLE_GRIDS = ((50, R.MG_ANY), (64, R.MG), (258, R.MG_ANY), (2050, R.MG_ANY))
CYCLE_CASES = [(N, kind, dom, direction) for N, kind in CYCLE_GRIDS for dom in (STRETCH_X, STRETCH_Y) for direction in (LINE_X, LINE_Y)]


def cycle_vectors(N, dom):
    """a standard-normal r and a smooth one (a product of sines over the bounding square), packed"""
    mask = ref.interior_mask(N)
    rng = np.random.default_rng(7 * N + int(dom[1]))
    y, x = np.mgrid[0:N + 1, 0:N + 1]
    smooth_r = (np.sin(np.pi * x / N) * np.sin(2 * np.pi * y / N) + 0.25)[mask]
    return rng.standard_normal(int(mask.sum())), smooth_r


def case_id(c):
    N, kind, dom, direction = c
    return f"n{N}-{'mg' if kind == R.MG else 'any'}-{int(dom[1])}x{int(dom[3])}-{'xy'[direction - 1]}"


# PCG cases under LINE_AUTO: (N, kind, domain, rule, eps, seed); b = A u for a seeded standard-normal u.  Every stop test of every
# trace misses its threshold by >= 1 % with these seeds (test_mg_line_cpu asserts it).
MARGIN = 0.01
PCG_CASES = [(N, kind, dom, rule, eps, seed) for (N, kind, dom), seeds in (
    ((50, R.MG_ANY, STRETCH_X), (50001, 50002)), ((64, R.MG, STRETCH_Y), (64001, 64002)),
    ((258, R.MG_ANY, STRETCH_X), (258001, 258002))) for (rule, eps), seed in zip(((R.REL_2NORM, 1e-8), (R.MSG, 1e-6)), seeds)]


def pcg_id(c):
    return f"n{c[0]}-{int(c[2][1])}x{int(c[2][3])}-{c[3]}"


@functools.lru_cache(maxsize=None)
def pcg_reference(c):
    """the fsum trace of a case under the line cycle of LINE_AUTO, tol[quantity][iteration] = tol_pcg of the quantity's spread,
    and the stop margin"""
    N, kind, dom, rule, eps, seed = c
    lv = R.levels_for(N, dom, kind)
    u = np.random.default_rng(seed).standard_normal(int(lv[0].mask.sum()))
    b = R.apply_A(lv, u)
    M = M_of(lv, auto_direction(lv))
    t = R.pcg_trace(lv, b, u=u, rule=rule, eps=eps, M=M)
    sp = R.spread(lv, b, t.iterations, u=u, M=M, exact=t)
    return SimpleNamespace(levels=lv, b=b, u=u, trace=t, tol={q: R.tol_pcg(v) for q, v in sp.items()}, margin=R.stop_margin(t, rule, eps))


# the shifted operator A - sigma I under the line cycle: (N, kind, domain, sigma); tables on three levels, sigma of the diagonal's size
SHIFT_CASE = (258, R.MG_ANY, STRETCH_X, 1e5)


def shifted_levels(N, dom, kind, sigma):
    """shift_reference.shifted_levels: every level's diagonal, and with it the lines' Thomas factors, shifted by sigma"""
    import shift_reference
    return shift_reference.shifted_levels(N, dom, kind, sigma)
