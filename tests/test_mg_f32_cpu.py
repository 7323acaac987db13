"""MI355CG_CYCLE_F32 without a GPU: a float32 NumPy restatement of the fp32 V-cycle inside the fp64 PCG (include/mi355cg.h,
DESIGN section 10.2), built on the helpers of tests/test_mg_cpu.py and tests/test_mg_any_cpu.py, and the new entry points.

z = M32 r:  s = 2^e with max|r| = m 2^e, 0.5 <= m < 1;  r32 = fl32(r / s);  the V-cycle of the two fp64 restatements with every
array float32 and every level constant (diagonal, x_k, y_k, omega, (N_c / N_f)^2, the non-nested weights, the coarse inverse) the
fp64 value rounded to float32;  z = s * float64(z32).  The PCG around it is the fp64 one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_mg_any_cpu as ref_any  # noqa: E402
import test_mg_cpu as ref  # noqa: E402

F = np.float32
DOM = ref_any.DOM
STRETCHED = (0.0, 1.0, 0.0, 2.0)


class Level32:
    """the fp64 Level with its constants rounded to float32"""

    def __init__(self, L, coarser_n):
        self.N, self.mask = L.N, L.mask
        self.diag, self.xk, self.yk, self.omega = F(L.diag), F(L.xk), F(L.yk), F(ref.OMEGA)
        self.W = None if getattr(L, "W", None) is None else L.W.astype(F)
        self.scale = None if coarser_n is None else F(coarser_n * coarser_n / (L.N * L.N))
        self.inv = None if L.inv is None else L.inv.astype(F)


def hierarchy32(levels):
    return [Level32(L, levels[i + 1].N if i + 1 < len(levels) else None) for i, L in enumerate(levels)]


def apply_A(L, u):
    out = np.zeros_like(u)
    out[1:-1, 1:-1] = L.diag * u[1:-1, 1:-1] + L.xk * (u[1:-1, :-2] + u[1:-1, 2:]) + L.yk * (u[:-2, 1:-1] + u[2:, 1:-1])
    out[~L.mask] = 0
    return out


def smooth(L, u, r):
    t = u + L.omega * ((r - apply_A(L, u)) / L.diag)
    t[~L.mask] = 0
    return t


def restrict(Cl, s):
    c = s[2:-1:2, 2:-1:2]
    l, r = s[2:-1:2, 1:-2:2], s[2:-1:2, 3::2]
    d, u = s[1:-2:2, 2:-1:2], s[3::2, 2:-1:2]
    ld, rd = s[1:-2:2, 1:-2:2], s[1:-2:2, 3::2]
    lu, ru = s[3::2, 1:-2:2], s[3::2, 3::2]
    out = np.zeros((Cl.N + 1, Cl.N + 1), dtype=F)
    out[1:-1, 1:-1] = F(0.0625) * (F(4) * c + F(2) * (l + r + d + u) + (ld + rd + lu + ru))
    out[~Cl.mask] = 0
    return out


def prolong(Fl, e):
    f = np.zeros((Fl.N + 1, Fl.N + 1), dtype=F)
    f[0::2, 0::2] = e
    f[0::2, 1::2] = F(0.5) * (e[:, :-1] + e[:, 1:])
    f[1::2, 0::2] = F(0.5) * (e[:-1, :] + e[1:, :])
    f[1::2, 1::2] = F(0.25) * (e[:-1, :-1] + e[:-1, 1:] + e[1:, :-1] + e[1:, 1:])
    f[~Fl.mask] = 0
    return f


def restrict_nn(Fl, Cl, s):
    out = Fl.scale * (Fl.W @ s @ Fl.W.T)
    out[~Cl.mask] = 0
    return out


def prolong_nn(Fl, e):
    out = Fl.W.T @ e @ Fl.W
    out[~Fl.mask] = 0
    return out


def vcycle(levels, l, r):
    L = levels[l]
    assert r.dtype == F
    if l == len(levels) - 1:
        g = np.zeros((L.N + 1, L.N + 1), dtype=F)
        g[L.mask] = L.inv @ r[L.mask]
        return g
    Cl = levels[l + 1]
    nested = L.N == 2 * Cl.N
    u = smooth(L, np.zeros_like(r), r)
    u = smooth(L, u, r)
    s = r - apply_A(L, u)
    s[~L.mask] = 0
    e = vcycle(levels, l + 1, restrict(Cl, s) if nested else restrict_nn(L, Cl, s))
    assert e.dtype == F
    u = u + (prolong(L, e) if nested else prolong_nn(L, e))
    u = smooth(L, u, r)
    return smooth(L, u, r)


def apply_M32(levels32, r_packed, scaled=True):
    """z = M32 r for a float64 packed r; scaled=False leaves out the power-of-two scale (what the scale is there to prevent)"""
    L = levels32[0]
    assert r_packed.dtype == np.float64
    rmax = np.abs(r_packed).max()
    if rmax == 0:
        return np.zeros_like(r_packed)
    e = int(np.frexp(rmax)[1]) if scaled else 0
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        g = np.zeros((L.N + 1, L.N + 1), dtype=F)
        g[L.mask] = np.ldexp(r_packed, -e).astype(F)
        z32 = vcycle(levels32, 0, g)
    assert z32.dtype == F
    return np.ldexp(z32[L.mask].astype(np.float64), e)


def pcg(apply_M, L, b, eps=1e-8, max_iterations=100):
    """test_mg_any_cpu.pcg with the preconditioner passed in: fp64 Hestenes-Stiefel PCG from x = 0, REL_2NORM stop"""
    x = np.zeros_like(b)
    r = b.copy()
    r0 = np.linalg.norm(r)
    it, rho, p = 0, 0.0, None
    while it < max_iterations and np.linalg.norm(r) > eps * r0:
        z = apply_M(r)
        rz = r @ z
        p = z if it == 0 else z + (rz / rho) * p
        rho = rz
        q = ref.packed(L, ref.apply_A(L, ref.grid(L, p)))
        alpha = rho / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        it += 1
    return x, it


def both_hierarchies(N, dom=DOM):
    a, b, c, d = dom
    levels = ref_any.hierarchy_any(N, (b - a) / N, (d - c) / N)
    return levels, hierarchy32(levels)


def oracle_rhs(N, dom=DOM):
    from oracle.oracle import OracleGrid
    return np.asarray(OracleGrid(N, N, *dom).rhs(), dtype=np.float64)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 34, 50, 256, 258])
def test_fp32_cycle_is_float32_throughout_and_close_to_the_fp64_cycle(N):
    levels, levels32 = both_hierarchies(N)
    rng = np.random.default_rng(N)
    for _ in range(2):
        r = rng.standard_normal(int(levels[0].mask.sum()))
        z32, z64 = apply_M32(levels32, r), ref_any.apply_M(levels, r)
        assert z32.dtype == np.float64                       # what the PCG sees; the cycle asserts float32 on every level
        dev = np.abs(z32 - z64).max() / np.abs(z64).max()
        assert 1e-9 < dev <= 2e-6, dev                       # fp32 rounding: not the fp64 cycle, and nothing worse than rounding


def test_zero_residual_gives_zero():
    levels, levels32 = both_hierarchies(34)
    z = apply_M32(levels32, np.zeros(int(levels[0].mask.sum())))
    assert z.dtype == np.float64 and not z.any()


@pytest.mark.parametrize("N,dom", [(34, DOM), (100, DOM), (258, DOM), (1000, DOM), (258, STRETCHED)])
def test_pcg_with_the_fp32_cycle_takes_the_iterations_of_the_fp64_cycle(N, dom):
    levels, levels32 = both_hierarchies(N, dom)
    L = levels[0]
    b = oracle_rhs(N, dom)
    x64, it64 = ref_any.pcg(levels, b)
    x32, it32 = pcg(lambda r: apply_M32(levels32, r), L, b)
    print(f"N={N} dom={dom}: iterations fp64 cycle {it64}, fp32 cycle {it32}")
    assert it32 == it64
    true_r = b - ref.packed(L, ref.apply_A(L, ref.grid(L, x32)))
    rel = np.linalg.norm(true_r) / np.linalg.norm(b)
    print(f"  true residual {rel:.3e}")
    assert rel <= 2e-8


@pytest.mark.parametrize("k", [-140, 140])
def test_the_cycle_commutes_with_powers_of_two(k):
    levels, levels32 = both_hierarchies(258)
    r = oracle_rhs(258)
    z0 = apply_M32(levels32, r)
    zk = apply_M32(levels32, np.ldexp(r, k))
    assert np.isfinite(zk).all() and zk.any()
    assert np.array_equal(zk, np.ldexp(z0, k))
    # without the scale the float32 copy of r overflows (k > 0) or falls among the subnormals and loses its digits (k < 0)
    naive = apply_M32(levels32, np.ldexp(r, k), scaled=False)
    assert not np.isfinite(naive).all() or np.abs(naive - zk).max() > 1e-3 * np.abs(zk).max()


@pytest.mark.parametrize("k", [-140, 140])
def test_a_whole_solve_scales_exactly(k):
    levels, levels32 = both_hierarchies(258)
    L = levels[0]
    b = oracle_rhs(258)
    x0, it0 = pcg(lambda r: apply_M32(levels32, r), L, b)
    xk, itk = pcg(lambda r: apply_M32(levels32, r), L, np.ldexp(b, k))
    assert itk == it0
    assert np.array_equal(xk, np.ldexp(x0, k))


@pytest.mark.parametrize("N", [6, 10, 16, 32])
def test_one_level_grids_take_a_second_iteration(N):
    levels, levels32 = both_hierarchies(N)
    assert len(levels) == 1
    L = levels[0]
    b = oracle_rhs(N)
    assert ref_any.pcg(levels, b)[1] == 1
    x, it = pcg(lambda r: apply_M32(levels32, r), L, b)
    assert it == 2
    true_r = b - ref.packed(L, ref.apply_A(L, ref.grid(L, x)))
    assert np.linalg.norm(true_r) <= 2e-8 * np.linalg.norm(b)


# ---- the entry points (no GPU needed) ----------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_listed():
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    for name in ("mi355cg_set_preconditioner_ex", "mi355cg_preconditioner_info"):
        assert hasattr(lib, name), name
        assert name in _capi.EXPORTS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355cg.h")).read()
    assert "#define MI355CG_CYCLE_F64 0" in header and "#define MI355CG_CYCLE_F32 1" in header


def test_cycle_constants_in_python():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    assert (isa.CYCLE_F64, isa.CYCLE_F32) == (0, 1)
    assert (_capi.CYCLE_F64, _capi.CYCLE_F32) == (0, 1)


def test_null_handles_are_refused_before_touching_the_gpu():
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    k = C.c_int(-1)
    assert lib.mi355cg_preconditioner_info(None, C.byref(k), None, None) == _capi.ERR_INVALID
    assert lib.mi355cg_set_preconditioner_ex(None, _capi.PRECOND_MG_ANY, _capi.CYCLE_F32) == _capi.ERR_INVALID
    assert k.value == -1
