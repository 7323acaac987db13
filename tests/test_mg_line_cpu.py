"""The line smoother of the fp64 V-cycle without a GPU (mi355cg_set_smoother): the NumPy restatement of
tests/line_reference.py is a symmetric negative definite preconditioner whose iteration count does not grow with the stretch of
the domain, it can tell the two line directions apart, its rounding floor keeps the tolerance of every case of
tests/test_gpu_mg_line.py under the project's cap, every stop test of the PCG cases keeps its margin, and the C ABI declares,
exports and guards the two new entry points."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import line_reference as LR  # noqa: E402

R = LR.R
CAP = 1e-11                                                        # mg_cases's: no cycle tolerance may need more
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def normal(levels, seed):
    return np.random.default_rng(seed).standard_normal(int(levels[0].mask.sum()))


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_direction_zero_is_the_point_cycle_bit_for_bit():
    lv = R.levels_for(50, LR.STRETCH_X, R.MG_ANY)
    r = normal(lv, 1)
    assert np.array_equal(LR.apply_M_line(lv, r, LR.JACOBI), R.apply_M(lv, r))


@pytest.mark.parametrize("direction", [LR.LINE_X, LR.LINE_Y])
def test_the_line_solve_inverts_the_line_operator(direction):
    """T e = s back through the three-point formula along the lines, the short lines and the long ones"""
    lv = R.levels_for(50, LR.STRETCH_Y, R.MG_ANY)
    L = lv[0]
    s = R.model.grid(L, normal(lv, 2))
    e = LR.line_solve(L, s, direction)
    k = L.xk if direction == LR.LINE_X else L.yk
    g = e if direction == LR.LINE_X else e.T
    back = L.diag * g
    back[:, 1:] += k * g[:, :-1]
    back[:, :-1] += k * g[:, 1:]
    back = back if direction == LR.LINE_X else back.T
    assert np.all(e[~L.mask] == 0)
    assert np.abs(back[L.mask] - s[L.mask]).max() <= 1e-13 * np.abs(s).max()


@pytest.mark.parametrize("dom", [LR.STRETCH_X, LR.STRETCH_Y], ids=["10x1", "1x10"])
def test_restatement_is_symmetric_and_negative_definite(dom):
    lv = R.levels_for(50, dom, R.MG_ANY)
    d = LR.auto_direction(lv)
    rng = np.random.default_rng(50)
    n = int(lv[0].mask.sum())
    for _ in range(3):
        u, v = rng.standard_normal(n), rng.standard_normal(n)
        Mu, Mv = LR.apply_M_line(lv, u, d), LR.apply_M_line(lv, v, d)
        print(f"asymmetry {abs(Mu @ v - u @ Mv) / abs(Mu @ v):.1e}")
        assert abs(Mu @ v - u @ Mv) <= 1e-12 * abs(Mu @ v)
        assert Mu @ u < 0 and Mv @ v < 0


def test_auto_takes_the_strongly_coupled_direction():
    assert LR.auto_direction(R.levels_for(64, LR.STRETCH_X, R.MG)) == LR.LINE_Y
    assert LR.auto_direction(R.levels_for(64, LR.STRETCH_Y, R.MG)) == LR.LINE_X
    assert LR.auto_direction(R.levels_for(64, LR.SQUARE, R.MG)) == LR.LINE_X


@pytest.mark.parametrize("N", [64, 128])
@pytest.mark.parametrize("dom", LR.DOMAINS, ids=lambda d: f"{int(d[1])}x{int(d[3])}")
def test_line_auto_takes_at_most_8_iterations_on_every_domain(N, dom):
    lv = R.levels_for(N, dom, R.MG)
    t = R.pcg_trace(lv, normal(lv, N), M=LR.M_of(lv, LR.auto_direction(lv)))
    print(f"N={N} {dom}: {t.iterations} iterations")
    assert t.converged and t.iterations <= 8


@pytest.mark.parametrize("N", [64, 128])
def test_point_jacobi_takes_at_least_40_iterations_at_aspect_10(N):
    lv = R.levels_for(N, LR.STRETCH_X, R.MG)
    t = R.pcg_trace(lv, normal(lv, N))
    print(f"N={N}: {t.iterations} iterations")
    assert t.converged and t.iterations >= 40


@pytest.mark.parametrize("N,kind", [(50, R.MG_ANY), (64, R.MG)])
@pytest.mark.parametrize("dom", [LR.STRETCH_X, LR.STRETCH_Y], ids=["10x1", "1x10"])
def test_the_wrong_direction_is_far_from_the_right_one(N, kind, dom):
    lv = R.levels_for(N, dom, kind)
    d = LR.auto_direction(lv)
    # the standard-normal vector carries the teeth: a smooth r has little for a smoother to tell apart (printed, not asserted)
    for r, rough in zip(LR.cycle_vectors(N, dom), (True, False)):
        z, zw = LR.apply_M_line(lv, r, d), LR.apply_M_line(lv, r, LR.LINE_X + LR.LINE_Y - d)
        dev = np.abs(zw - z).max() / np.abs(z).max()
        print(f"N={N} {dom} {'standard-normal' if rough else 'smooth'} r: the other direction differs by {dev:.2f} of the max-norm")
        assert dev > 0.1 or not rough


# ---- what the GPU tests rely on ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", LR.CYCLE_CASES, ids=LR.case_id)
def test_cycle_floor(c):
    N, kind, dom, direction = c
    lv = R.levels_for(N, dom, kind)
    for r in LR.cycle_vectors(N, dom):
        floor = LR.cycle_floor_line(lv, r, direction)
        print(f"{LR.case_id(c)}: floor {floor:.2e}, tol_M = {R.tol_M(floor):.2e}")
        assert 16.0 * floor <= CAP


def test_shifted_cycle_floor():
    N, kind, dom, sigma = LR.SHIFT_CASE
    lv = LR.shifted_levels(N, dom, kind, sigma)
    r = LR.cycle_vectors(N, dom)[0]
    assert 16.0 * LR.cycle_floor_line(lv, r, LR.auto_direction(lv)) <= CAP
    base = R.levels_for(N, dom, kind)
    z, z0 = LR.apply_M_line(lv, r, LR.LINE_Y), LR.apply_M_line(base, r, LR.LINE_Y)
    assert np.abs(z - z0).max() > 0.1 * np.abs(z).max()           # the shift shows: tables kept from sigma = 0 would be told


@pytest.mark.parametrize("c", LR.PCG_CASES, ids=LR.pcg_id)
def test_pcg_cases_keep_their_stop_margin(c):
    ref = LR.pcg_reference(c)
    t = ref.trace
    print(f"{LR.pcg_id(c)}: {t.iterations} iterations, reason {t.reason}, margin {100 * ref.margin:.1f} %, "
          f"tol x {ref.tol['x'][-1]:.1e} r2 {ref.tol['r2'][-1]:.1e}")
    assert t.converged and 2 <= t.iterations <= 8
    assert ref.margin >= LR.MARGIN
    assert ref.tol["x"].max() <= CAP


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_the_smoother_entry_points_are_declared_and_exported():
    from iterative_solvers_amd import _capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355cg.h")).read(), flags=re.S)
    lib = _capi.load()
    for name in ("mi355cg_set_smoother", "mi355cg_get_smoother"):
        assert re.search(rf"\b{name}\s*\(", text) and name in _capi.EXPORTS and hasattr(lib, name)
    for name, value in (("JACOBI", 0), ("LINE_X", 1), ("LINE_Y", 2), ("LINE_AUTO", 3)):
        assert re.search(rf"#define\s+MI355CG_SMOOTHER_{name}\s+{value}\b", text)
        assert getattr(_capi, f"SMOOTHER_{name}") == value
    import iterative_solvers_amd as isa
    assert (isa.SMOOTHER_JACOBI, isa.SMOOTHER_LINE_X, isa.SMOOTHER_LINE_Y, isa.SMOOTHER_LINE_AUTO) == (0, 1, 2, 3)
    assert (LR.JACOBI, LR.LINE_X, LR.LINE_Y) == (0, 1, 2)


def test_a_null_handle_is_refused():
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    assert lib.mi355cg_set_smoother.argtypes == [C.c_void_p, C.c_int]
    assert lib.mi355cg_get_smoother.argtypes == [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    s, d = C.c_int(-5), C.c_int(-5)
    for value in (0, 1, 2, 3, 4, -1):
        assert lib.mi355cg_set_smoother(None, value) == _capi.ERR_INVALID
        assert b"null handle" in lib.mi355cg_last_error()
    assert lib.mi355cg_get_smoother(None, C.byref(s), C.byref(d)) == _capi.ERR_INVALID
    assert (s.value, d.value) == (-5, -5)


def test_the_python_layers_have_the_two_methods():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd.solver import _Handle
    for cls in (isa.MatrixFreeSystem, _Handle):
        assert callable(getattr(cls, "set_smoother")) and callable(getattr(cls, "smoother_info"))


def test_the_compat_header_has_set_smoother():
    text = open(os.path.join(ROOT, "iterative_solvers_amd", "compat", "mi355cg_compat.hpp")).read()
    assert re.search(r"void\s+setSmoother\s*\(\s*int\s+\w+\s*\)", text)
