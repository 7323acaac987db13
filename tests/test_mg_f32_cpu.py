"""MI355CG_CYCLE_F32 without a GPU: the float32 run of the NumPy restatement (tests/mg_model.py: apply_M32, the one V-cycle on a
float32 grid) inside the fp64 PCG, and the new entry points."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model as ref  # noqa: E402
from mg_cases import oracle_rhs  # noqa: E402

DOM = ref.DOM
STRETCHED = (0.0, 1.0, 0.0, 2.0)


def levels_on(N, dom=DOM):
    a, b, c, d = dom
    return ref.hierarchy_any(N, (b - a) / N, (d - c) / N)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 34, 50, 256, 258])
def test_fp32_cycle_is_float32_throughout_and_close_to_the_fp64_cycle(N):
    levels = levels_on(N)
    rng = np.random.default_rng(N)
    for _ in range(2):
        r = rng.standard_normal(int(levels[0].mask.sum()))
        z32, z64 = ref.apply_M32(levels, r), ref.apply_M(levels, r)
        assert z32.dtype == np.float64                       # what the PCG sees; the cycle asserts float32 on every level
        dev = np.abs(z32 - z64).max() / np.abs(z64).max()
        assert 1e-9 < dev <= 2e-6, dev                       # fp32 rounding: not the fp64 cycle, and nothing worse than rounding


@pytest.mark.parametrize("N", [34, 64])
def test_the_cycle_works_in_the_dtype_it_is_given(N):
    levels = levels_on(N)
    F, Cl = levels[0], levels[1]
    r = np.random.default_rng(N).standard_normal(int(F.mask.sum()))
    for dt in (np.float64, np.float32):
        g = ref.grid(F, r.astype(dt))
        assert ref.vcycle(levels, 0, g).dtype == dt                 # and on every level: the cycle asserts it of each correction
        for op in (ref.apply_A(F, g), ref.smooth(F, g, g), ref.restrict(F, Cl, g), ref.prolong(F, Cl, ref.restrict(F, Cl, g))):
            assert op.dtype == dt
    if F.N != 2 * Cl.N:                                             # the non-nested restriction multiplies by float32((N_c / N_f)^2)
        s32, W32 = ref.grid(F, r.astype(np.float32)), F.W.astype(np.float32)
        expect = np.float32(Cl.N * Cl.N / (F.N * F.N)) * (W32 @ s32 @ W32.T)
        expect[~Cl.mask] = 0
        assert np.array_equal(ref.restrict(F, Cl, s32), expect)


def test_zero_residual_gives_zero():
    levels = levels_on(34)
    z = ref.apply_M32(levels, np.zeros(int(levels[0].mask.sum())))
    assert z.dtype == np.float64 and not z.any()


@pytest.mark.parametrize("N,dom", [(34, DOM), (100, DOM), (258, DOM), (1000, DOM), (258, STRETCHED)])
def test_pcg_with_the_fp32_cycle_takes_the_iterations_of_the_fp64_cycle(N, dom):
    levels = levels_on(N, dom)
    L = levels[0]
    b = oracle_rhs(N, dom)
    x64, it64 = ref.pcg(levels, b)
    x32, it32 = ref.pcg(levels, b, M=lambda r: ref.apply_M32(levels, r))
    print(f"N={N} dom={dom}: iterations fp64 cycle {it64}, fp32 cycle {it32}")
    assert it32 == it64
    true_r = b - ref.packed(L, ref.apply_A(L, ref.grid(L, x32)))
    rel = np.linalg.norm(true_r) / np.linalg.norm(b)
    print(f"  true residual {rel:.3e}")
    assert rel <= 2e-8


@pytest.mark.parametrize("k", [-140, 140])
def test_the_cycle_commutes_with_powers_of_two(k):
    levels = levels_on(258)
    r = oracle_rhs(258)
    z0 = ref.apply_M32(levels, r)
    zk = ref.apply_M32(levels, np.ldexp(r, k))
    assert np.isfinite(zk).all() and zk.any()
    assert np.array_equal(zk, np.ldexp(z0, k))
    # without the scale the float32 copy of r overflows (k > 0) or falls among the subnormals and loses its digits (k < 0)
    naive = ref.apply_M32(levels, np.ldexp(r, k), scaled=False)
    assert not np.isfinite(naive).all() or np.abs(naive - zk).max() > 1e-3 * np.abs(zk).max()


@pytest.mark.parametrize("k", [-140, 140])
def test_a_whole_solve_scales_exactly(k):
    levels = levels_on(258)
    L = levels[0]
    b = oracle_rhs(258)
    x0, it0 = ref.pcg(levels, b, M=lambda r: ref.apply_M32(levels, r))
    xk, itk = ref.pcg(levels, np.ldexp(b, k), M=lambda r: ref.apply_M32(levels, r))
    assert itk == it0
    assert np.array_equal(xk, np.ldexp(x0, k))


@pytest.mark.parametrize("N", [6, 10, 16, 32])
def test_one_level_grids_take_a_second_iteration(N):
    levels = levels_on(N)
    assert len(levels) == 1
    L = levels[0]
    b = oracle_rhs(N)
    assert ref.pcg(levels, b)[1] == 1
    x, it = ref.pcg(levels, b, M=lambda r: ref.apply_M32(levels, r))
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
