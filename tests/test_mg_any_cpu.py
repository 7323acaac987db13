"""MI355CG_PRECOND_MG_ANY without a GPU: the ladder of mi355cg_mg_hierarchy, and a NumPy restatement of the non-nested levels
(include/mi355cg.h) on top of the one in tests/test_mg_cpu.py, which tests/test_gpu_mg_any.py compares the
device against.

Ladder: N_{l+1} = 2 floor(N_l / 4) while N_l > 32.  A level with N_f = 2 N_c is nested and uses test_mg_cpu's full weighting and
bilinear prolongation; any other (N_f % 4 == 2) keeps the domain (h_c = h_f N_f / N_c) and transfers by the 1-D bilinear weights
w(x, X) = max(0, 1 - |x N_c - X N_f| / N_f): P e = W^T e W masked to the fine interior, R s = (N_c / N_f)^2 W s W^T masked to
the coarse interior, so R = (N_c / N_f)^2 P^T."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_mg_cpu as ref  # noqa: E402

DOM = (1.0, 2.0, 1.0, 2.0)


def ladder(N):
    ns = [N]
    while ns[-1] > 32:
        ns.append(2 * (ns[-1] // 4))
    return ns


def weights(Nf, Nc):
    """W[X, x] = w(x, X); the numerator |x N_c - X N_f| is an exact integer"""
    d = np.abs(np.arange(Nf + 1, dtype=np.int64)[None, :] * Nc - np.arange(Nc + 1, dtype=np.int64)[:, None] * Nf)
    return np.where(d < Nf, (Nf - d) / Nf, 0.0)


def hierarchy_any(N, hx, hy):
    levels = [ref.Level(N, hx, hy)]
    for Nc in ladder(N)[1:]:
        F = levels[-1]
        if F.N == 2 * Nc:
            levels.append(ref.Level(Nc, 2 * F.hx, 2 * F.hy))
        else:
            levels.append(ref.Level(Nc, F.hx * F.N / Nc, F.hy * F.N / Nc))
            F.W = weights(F.N, Nc)
    Lc = levels[-1]
    Lc.inv = ref.hierarchy(Lc.N, Lc.hx, Lc.hy)[0].inv          # N_L <= 32: one level, its dense inverse
    return levels


def restrict_nn(F, Cl, s):
    out = (Cl.N * Cl.N / (F.N * F.N)) * (F.W @ s @ F.W.T)
    out[~Cl.mask] = 0.0
    return out


def prolong_nn(F, e):
    out = F.W.T @ e @ F.W
    out[~F.mask] = 0.0
    return out


def vcycle(levels, l, r):
    L = levels[l]
    if l == len(levels) - 1:
        return ref.grid(L, L.inv @ ref.packed(L, r))
    Cl = levels[l + 1]
    nested = L.N == 2 * Cl.N
    u = ref.smooth(L, np.zeros_like(r), r)
    u = ref.smooth(L, u, r)
    s = r - ref.apply_A(L, u)
    s[~L.mask] = 0.0
    e = vcycle(levels, l + 1, ref.restrict(L, Cl, s) if nested else restrict_nn(L, Cl, s))
    u = u + (ref.prolong(L, e) if nested else prolong_nn(L, e))
    u = ref.smooth(L, u, r)
    return ref.smooth(L, u, r)


def apply_M(levels, r_packed):
    return ref.packed(levels[0], vcycle(levels, 0, ref.grid(levels[0], r_packed)))


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
        q = ref.packed(L, ref.apply_A(L, ref.grid(L, p)))
        alpha = rho / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        it += 1
    return x, it


def steps(N):
    a, b, c, d = DOM
    return (b - a) / N, (d - c) / N


# ---- the library's ladder (host arithmetic: no GPU) --------------------------------------------------------------------
LADDERS = [(6, (6,)), (32, (32,)), (34, (34, 16)), (258, (258, 128, 64, 32)), (1000, (1000, 500, 250, 124, 62, 30)),
           (4098, (4098, 2048, 1024, 512, 256, 128, 64, 32)),
           (10000, (10000, 5000, 2500, 1250, 624, 312, 156, 78, 38, 18))]


@pytest.mark.parametrize("n,expected", LADDERS)
def test_mg_hierarchy_in_python(n, expected):
    import iterative_solvers_amd as isa
    assert isa.mg_hierarchy(n) == expected
    assert isa.mg_hierarchy(n, kind=isa.PRECOND_MG_ANY) == expected
    assert tuple(ladder(n)) == expected


@pytest.mark.parametrize("n,expected", LADDERS)
def test_mg_hierarchy_through_the_c_abi(n, expected):
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    L, buf = C.c_int(), (C.c_int * 16)(*([-1] * 16))
    assert lib.mi355cg_mg_hierarchy(_capi.PRECOND_MG_ANY, n, 16, C.byref(L), buf) == _capi.OK
    assert L.value == len(expected) and tuple(buf[:L.value]) == expected and buf[L.value] == -1


def test_mg_hierarchy_writes_at_most_max_levels():
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    L, buf = C.c_int(), (C.c_int * 4)(-1, -1, -1, -1)
    assert lib.mi355cg_mg_hierarchy(_capi.PRECOND_MG_ANY, 1000, 2, C.byref(L), buf) == _capi.OK
    assert L.value == 6 and list(buf) == [1000, 500, -1, -1]
    assert lib.mi355cg_mg_hierarchy(_capi.PRECOND_MG_ANY, 1000, 0, C.byref(L), None) == _capi.OK and L.value == 6
    assert lib.mi355cg_mg_hierarchy(_capi.PRECOND_MG_ANY, 1000, 3, C.byref(L), None) == _capi.ERR_INVALID


def test_n32768_has_the_levels_of_mg_levels():
    import iterative_solvers_amd as isa
    levels, coarsest = isa.mg_levels(32768)
    assert isa.mg_hierarchy(32768) == tuple(32768 >> l for l in range(11))
    assert (levels, coarsest) == (11, 32)


@pytest.mark.parametrize("n", [6, 10, 16, 32, 64, 256, 4096, 32768])
def test_kind_mg_is_mg_levels(n):
    import iterative_solvers_amd as isa
    ns = isa.mg_hierarchy(n, kind=isa.PRECOND_MG)
    assert (len(ns), ns[-1]) == isa.mg_levels(n)
    assert ns == isa.mg_hierarchy(n)


@pytest.mark.parametrize("n", [258, 1000, 4098])
def test_kind_mg_still_refuses_grids_without_a_nested_hierarchy(n):
    import iterative_solvers_amd as isa
    with pytest.raises(ValueError, match="no multigrid hierarchy"):
        isa.mg_hierarchy(n, kind=isa.PRECOND_MG)
    assert len(isa.mg_hierarchy(n)) >= 2


@pytest.mark.parametrize("n", [7, 1001, 4, 2, 0, -6])
def test_odd_and_small_grids_are_refused(n):
    import iterative_solvers_amd as isa
    with pytest.raises(ValueError, match="rejected"):
        isa.mg_hierarchy(n)


@pytest.mark.parametrize("kind", [0, 3, 7, -1])
def test_unknown_kinds_are_refused(kind):
    import iterative_solvers_amd as isa
    with pytest.raises(ValueError, match="no multigrid hierarchy"):
        isa.mg_hierarchy(256, kind=kind)


def test_every_even_grid_up_to_10000_has_a_ladder_and_agrees_with_mg():
    import iterative_solvers_amd as isa
    with_mg = 0
    for n in range(6, 10001, 2):
        ns = isa.mg_hierarchy(n)
        assert list(ns) == ladder(n)
        assert (16 <= ns[-1] <= 32) if n > 32 else ns == (n,)
        try:
            mg = isa.mg_hierarchy(n, kind=isa.PRECOND_MG)
        except ValueError:
            continue
        with_mg += 1
        assert mg == ns
    assert with_mg == 79


# ---- the restatement of the non-nested transfers -------------------------------------------------------------------------
@pytest.mark.parametrize("Nc", [16, 32, 64])
def test_weights_of_a_nested_pair_are_full_weighting_and_bilinear(Nc):
    Nf = 2 * Nc
    W = weights(Nf, Nc)
    expect = np.zeros((Nc + 1, Nf + 1))
    for X in range(Nc + 1):
        expect[X, 2 * X] = 1.0
        if X > 0:
            expect[X, 2 * X - 1] = 0.5
        if X < Nc:
            expect[X, 2 * X + 1] = 0.5
    assert np.array_equal(W, expect)
    F, Cl = ref.Level(Nf, 1 / Nf, 1 / Nf), ref.Level(Nc, 2 / Nf, 2 / Nf)
    F.W = W
    rng = np.random.default_rng(Nc)
    # small integers: every sum is exact in fp64, so equal operators give equal bits whatever the order of the sums
    s = ref.grid(F, rng.integers(-8, 9, int(F.mask.sum())).astype(np.float64))
    e = ref.grid(Cl, rng.integers(-8, 9, int(Cl.mask.sum())).astype(np.float64))
    assert np.array_equal(restrict_nn(F, Cl, s), ref.restrict(F, Cl, s))
    assert np.array_equal(prolong_nn(F, e), ref.prolong(F, e))


@pytest.mark.parametrize("Nf", [34, 50, 258])
def test_restriction_is_a_multiple_of_the_transposed_prolongation(Nf):
    Nc = ladder(Nf)[1]
    assert Nf != 2 * Nc
    F, Cl = ref.Level(Nf, 1 / Nf, 1 / Nf), ref.Level(Nc, 1 / Nc, 1 / Nc)
    F.W = weights(Nf, Nc)
    rng = np.random.default_rng(Nf)
    for _ in range(3):
        s = ref.grid(F, rng.standard_normal(int(F.mask.sum())))
        e = ref.grid(Cl, rng.standard_normal(int(Cl.mask.sum())))
        lhs = ref.packed(Cl, restrict_nn(F, Cl, s)) @ ref.packed(Cl, e)          # (R s, e)
        rhs = (Nc * Nc / (Nf * Nf)) * (ref.packed(F, s) @ ref.packed(F, prolong_nn(F, e)))   # (N_c/N_f)^2 (s, P e)
        assert abs(lhs - rhs) <= 1e-13 * abs(lhs)
    # each fine node is covered by weights summing to 1 in each direction: P reproduces constants away from the boundary
    assert np.allclose(F.W.sum(axis=0), 1.0, rtol=0, atol=1e-15)


def test_restatement_ladder_and_steps():
    levels = hierarchy_any(1000, *steps(1000))
    assert [L.N for L in levels] == [1000, 500, 250, 124, 62, 30]
    for L in levels:                                    # every level spans the same domain (to rounding on non-nested levels)
        assert L.hx * L.N == pytest.approx(1.0, rel=1e-15) and L.hy * L.N == pytest.approx(1.0, rel=1e-15)
    assert levels[1].hx == 2 * levels[0].hx and levels[2].hx == 2 * levels[1].hx     # nested: exactly doubled


@pytest.mark.parametrize("N", [34, 50, 258])
def test_restatement_is_symmetric_and_negative_definite(N):
    levels = hierarchy_any(N, *steps(N))
    rng = np.random.default_rng(N)
    n = int(levels[0].mask.sum())
    for _ in range(3):
        u, v = rng.standard_normal(n), rng.standard_normal(n)
        Mu, Mv = apply_M(levels, u), apply_M(levels, v)
        assert abs(Mu @ v - u @ Mv) <= 1e-12 * abs(Mu @ v)
        assert Mu @ u < 0 and Mv @ v < 0


def test_restatement_equals_test_mg_cpu_on_a_nested_grid():
    levels, nested = hierarchy_any(256, *steps(256)), ref.hierarchy(256, *steps(256))
    assert [(L.N, L.hx, L.hy) for L in levels] == [(L.N, L.hx, L.hy) for L in nested]
    r = np.random.default_rng(5).standard_normal(int(levels[0].mask.sum()))
    assert np.array_equal(apply_M(levels, r), ref.apply_M(nested, r))


@pytest.mark.parametrize("N", [258, 1000])
def test_restatement_pcg_converges_in_at_most_10_iterations(N):
    levels = hierarchy_any(N, *steps(N))
    L = levels[0]
    b = np.random.default_rng(N).standard_normal(int(L.mask.sum()))
    x, it = pcg(levels, b)
    assert it <= 10, it
    true_r = b - ref.packed(L, ref.apply_A(L, ref.grid(L, x)))
    assert np.linalg.norm(true_r) <= 2e-8 * np.linalg.norm(b)
