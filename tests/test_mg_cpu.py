"""The multigrid preconditioner without a GPU: the hierarchy rule of mi355cg_mg_levels, and the NumPy restatement of the algorithm
(tests/mg_model.py; include/mi355cg.h) that tests/test_gpu_mg.py compares the device against."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model as ref  # noqa: E402


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
    assert [L.N for L in ref.hierarchy(256, 1 / 256, 1 / 256)] == [256, 128, 64, 32]
    with pytest.raises(ValueError):
        ref.hierarchy(1000, 1e-3, 1e-3)


# ---- the restatement itself --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 64, 256])
def test_restatement_is_symmetric_and_negative_definite(N):
    levels = ref.hierarchy(N, 1 / N, 1 / N)
    rng = np.random.default_rng(N)
    n = int(levels[0].mask.sum())
    for _ in range(3):
        u, v = rng.standard_normal(n), rng.standard_normal(n)
        Mu, Mv = ref.apply_M(levels, u), ref.apply_M(levels, v)
        assert abs(Mu @ v - u @ Mv) <= 1e-12 * abs(Mu @ v)
        assert Mu @ u < 0 and Mv @ v < 0


def test_restatement_single_level_is_the_exact_inverse():
    levels = ref.hierarchy(16, 1 / 16, 1 / 16)
    L = levels[0]
    b = np.random.default_rng(1).standard_normal(int(L.mask.sum()))
    z = ref.apply_M(levels, b)
    assert np.abs(ref.packed(L, ref.apply_A(L, ref.grid(L, z))) - b).max() <= 1e-12 * np.abs(b).max()


def test_restatement_pcg_converges_in_at_most_10_iterations_at_n256():
    N = 256
    levels = ref.hierarchy(N, 1 / N, 1 / N)
    L = levels[0]
    b = np.random.default_rng(7).standard_normal(int(L.mask.sum()))
    x, it = ref.pcg(levels, b)
    assert it <= 10, it
    true_r = b - ref.packed(L, ref.apply_A(L, ref.grid(L, x)))
    assert np.linalg.norm(true_r) <= 2e-8 * np.linalg.norm(b)
