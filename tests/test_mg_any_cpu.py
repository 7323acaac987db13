"""MI355CG_PRECOND_MG_ANY without a GPU: the ladder of mi355cg_mg_hierarchy, and the non-nested levels of the NumPy restatement
(tests/mg_model.py; include/mi355cg.h), which tests/test_gpu_mg_any.py compares the device against."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model as ref  # noqa: E402


# ---- the library's ladder (host arithmetic: no GPU) --------------------------------------------------------------------
LADDERS = [(6, (6,)), (32, (32,)), (34, (34, 16)), (258, (258, 128, 64, 32)), (1000, (1000, 500, 250, 124, 62, 30)),
           (4098, (4098, 2048, 1024, 512, 256, 128, 64, 32)),
           (10000, (10000, 5000, 2500, 1250, 624, 312, 156, 78, 38, 18))]


@pytest.mark.parametrize("n,expected", LADDERS)
def test_mg_hierarchy_in_python(n, expected):
    import iterative_solvers_amd as isa
    assert isa.mg_hierarchy(n) == expected
    assert isa.mg_hierarchy(n, kind=isa.PRECOND_MG_ANY) == expected
    assert tuple(ref.ladder(n)) == expected


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
        assert list(ns) == ref.ladder(n)
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
    W = ref.weights(Nf, Nc)
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
    assert np.array_equal(ref.restrict(F, Cl, s, nested=False), ref.restrict(F, Cl, s))
    assert np.array_equal(ref.prolong(F, Cl, e, nested=False), ref.prolong(F, Cl, e))


@pytest.mark.parametrize("Nf", [34, 50, 258])
def test_restriction_is_a_multiple_of_the_transposed_prolongation(Nf):
    Nc = ref.ladder(Nf)[1]
    assert Nf != 2 * Nc
    F, Cl = ref.Level(Nf, 1 / Nf, 1 / Nf), ref.Level(Nc, 1 / Nc, 1 / Nc)
    F.W = ref.weights(Nf, Nc)
    rng = np.random.default_rng(Nf)
    for _ in range(3):
        s = ref.grid(F, rng.standard_normal(int(F.mask.sum())))
        e = ref.grid(Cl, rng.standard_normal(int(Cl.mask.sum())))
        lhs = ref.packed(Cl, ref.restrict(F, Cl, s)) @ ref.packed(Cl, e)          # (R s, e)
        rhs = (Nc * Nc / (Nf * Nf)) * (ref.packed(F, s) @ ref.packed(F, ref.prolong(F, Cl, e)))   # (N_c/N_f)^2 (s, P e)
        assert abs(lhs - rhs) <= 1e-13 * abs(lhs)
    # each fine node is covered by weights summing to 1 in each direction: P reproduces constants away from the boundary
    assert np.allclose(F.W.sum(axis=0), 1.0, rtol=0, atol=1e-15)


def test_restatement_ladder_and_steps():
    levels = ref.hierarchy_any(1000, *ref.steps(1000))
    assert [L.N for L in levels] == [1000, 500, 250, 124, 62, 30]
    for L in levels:                                    # every level spans the same domain (to rounding on non-nested levels)
        assert L.hx * L.N == pytest.approx(1.0, rel=1e-15) and L.hy * L.N == pytest.approx(1.0, rel=1e-15)
    assert levels[1].hx == 2 * levels[0].hx and levels[2].hx == 2 * levels[1].hx     # nested: exactly doubled


@pytest.mark.parametrize("N", [34, 50, 258])
def test_restatement_is_symmetric_and_negative_definite(N):
    levels = ref.hierarchy_any(N, *ref.steps(N))
    rng = np.random.default_rng(N)
    n = int(levels[0].mask.sum())
    for _ in range(3):
        u, v = rng.standard_normal(n), rng.standard_normal(n)
        Mu, Mv = ref.apply_M(levels, u), ref.apply_M(levels, v)
        assert abs(Mu @ v - u @ Mv) <= 1e-12 * abs(Mu @ v)
        assert Mu @ u < 0 and Mv @ v < 0


def test_restatement_equals_test_mg_cpu_on_a_nested_grid():
    levels, nested = ref.hierarchy_any(256, *ref.steps(256)), ref.hierarchy(256, *ref.steps(256))
    assert [(L.N, L.hx, L.hy) for L in levels] == [(L.N, L.hx, L.hy) for L in nested]
    r = np.random.default_rng(5).standard_normal(int(levels[0].mask.sum()))
    assert np.array_equal(ref.apply_M(levels, r), ref.apply_M(nested, r))


@pytest.mark.parametrize("N", [34, 64])
def test_the_default_smoother_is_the_point_smoother(N):
    levels = ref.hierarchy_any(N, *ref.steps(N))
    r = np.random.default_rng(N).standard_normal(int(levels[0].mask.sum()))
    assert np.array_equal(ref.apply_M(levels, r, smoother=ref.smooth), ref.apply_M(levels, r))


@pytest.mark.parametrize("N", [258, 1000])
def test_restatement_pcg_converges_in_at_most_10_iterations(N):
    levels = ref.hierarchy_any(N, *ref.steps(N))
    L = levels[0]
    b = np.random.default_rng(N).standard_normal(int(L.mask.sum()))
    x, it = ref.pcg(levels, b)
    assert it <= 10, it
    true_r = b - ref.packed(L, ref.apply_A(L, ref.grid(L, x)))
    assert np.linalg.norm(true_r) <= 2e-8 * np.linalg.norm(b)
