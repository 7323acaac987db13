"""The diagonal shift and the theta-scheme stepper without a GPU: the shifted restatement of
tests/shift_reference.py is a valid preconditioner, every iteration count the GPU tests compare is decided well away from its
threshold, the step's right-hand side has the steady state as a fixed point, and the new entry points refuse a null handle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model  # noqa: E402
import shift_reference as S  # noqa: E402

R = S.R


@pytest.mark.parametrize("N", [10, 34])
@pytest.mark.parametrize("sigma", [1.0, 1e3, 1e5])
def test_shifted_restatement_is_symmetric_and_negative_definite(N, sigma):
    levels = S.shifted_levels(N, R.ISO, R.MG_ANY, sigma)
    n = int(levels[0].mask.sum())
    eye = np.eye(n)
    A = np.stack([R.apply_A(levels, eye[j]) for j in range(n)], axis=1)
    M = np.stack([R.apply_M(levels, eye[j]) for j in range(n)], axis=1)
    for name, Q in (("A - sigma I", A), ("M", M)):
        asym = np.abs(Q - Q.T).max() / np.abs(Q).max()
        top = np.linalg.eigvalsh(0.5 * (Q + Q.T)).max()
        print(f"N={N} sigma={sigma:g} {name}: asymmetry {asym:.2e}, largest eigenvalue {top:.3e}")
        assert asym <= 1e-12
        assert top < 0
    base = R.levels_for(N, R.ISO, R.MG_ANY)
    v = np.random.default_rng(N).standard_normal(n)
    assert np.abs(A @ v - (R.apply_A(base, v) - sigma * v)).max() <= 1e-12 * np.abs(A @ v).max()


@pytest.mark.parametrize("N", [34, 64])
def test_the_sigma_of_the_hierarchy_is_the_shifted_levels(N):
    sigma = S.SIGMAS[3]
    assert sigma != 0
    hx, hy = mg_model.steps(N)
    levels, shifted, base = mg_model.hierarchy_any(N, hx, hy, sigma), S.shifted_levels(N, R.ISO, R.MG_ANY, sigma), R.levels_for(N, R.ISO, R.MG_ANY)
    assert [L.diag for L in levels] == [L.diag for L in shifted] == [L.diag - sigma for L in base]
    assert np.array_equal(levels[-1].inv, shifted[-1].inv) and not np.array_equal(levels[-1].inv, base[-1].inv)
    assert np.array_equal(levels[-1].inv, mg_model.coarse_inverse(levels[-1]))          # the inverse of the diagonal the level has now


@pytest.mark.parametrize("N,kind,dom", S.GRIDS, ids=lambda v: str(v) if isinstance(v, int) else None)
def test_cold_solves_stop_away_from_their_threshold(N, kind, dom):
    b = S.rhs_vector(N)
    for sigma in S.SIGMAS:
        t = R.pcg_trace(S.shifted_levels(N, dom, kind, sigma), b, eps=S.EPS)
        m = R.stop_margin(t, R.REL_2NORM, S.EPS)
        print(f"N={N} kind={kind} sigma={sigma:g}: {t.iterations} iterations, margin {m:.3f}")
        assert t.converged and 1 <= t.iterations <= 20
        assert m >= S.MARGIN


@pytest.mark.parametrize("N,kind,dom,theta,tau", S.STEPPER + ((34, None, R.ISO, 1.0, 1e-4),),
                         ids=lambda v: str(v) if isinstance(v, (int, float)) else None)
def test_stepper_chain_stops_away_from_its_threshold(N, kind, dom, theta, tau):
    """kind None: the step solved without a preconditioner (identity M)"""
    sigma = 1.0 / (theta * tau)
    base = R.levels_for(N, dom, R.MG_ANY if kind is None else kind)
    levels = S.shifted_levels(N, dom, R.MG_ANY if kind is None else kind, sigma)
    M = (lambda r: r) if kind is None else None
    u, g = S.stepper_inputs(N)
    for k in range(S.STEPS if kind is not None else 1):
        st = S.step_reference(base, levels, u, g, sigma, theta, M=M)
        print(f"N={N} theta={theta} tau={tau:g} step {k}: {st.trace.iterations} iterations, margin {st.margin:.3f}")
        assert st.trace.converged and st.trace.iterations >= 1
        assert st.margin >= S.MARGIN
        u = st.u


@pytest.mark.parametrize("theta", [1.0, 0.5, 0.25])
def test_theta_rhs_has_the_steady_state_as_a_fixed_point(theta):
    """(A - sigma I) u = theta_rhs(u) exactly when A u = g"""
    N, tau = 34, 1e-2
    sigma = 1.0 / (theta * tau)
    base = R.levels_for(N, R.ISO, R.MG_ANY)
    shifted = S.shifted_levels(N, R.ISO, R.MG_ANY, sigma)
    u = np.random.default_rng(5).standard_normal(int(base[0].mask.sum()))
    g = R.apply_A(base, u)
    lhs, rhs = R.apply_A(shifted, u), S.theta_rhs(base, u, g, sigma, theta)
    dev = np.abs(lhs - rhs).max() / np.abs(rhs).max()
    print(f"theta={theta}: max|(A - sigma I) u - b_step| / max|b_step| = {dev:.2e}")
    assert dev <= 1e-13
    off = S.theta_rhs(base, u, g + 1.0, sigma, theta)               # not a fixed point for another g
    assert np.abs(lhs - off).max() >= 0.5 / theta


def test_null_handles_are_refused_through_the_c_abi():
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    assert lib.mi355cg_set_shift(None, 1.0) == _capi.ERR_INVALID
    s = C.c_double(-1.0)
    assert lib.mi355cg_get_shift(None, C.byref(s)) == _capi.ERR_INVALID and s.value == -1.0
    p = _capi.Params()
    lib.mi355cg_default_params(C.byref(p), _capi.RULE_REL_2NORM)
    p.use_true_solution = 0
    res, done = (_capi.Results * 1)(), C.c_int(-7)
    assert lib.mi355cg_time_steps(None, C.byref(p), 1e-3, 1.0, 1, None, res, C.byref(done)) == _capi.ERR_INVALID
    assert done.value == -7
    assert lib.mi355cg_get_solution_device(None, None) == _capi.ERR_INVALID
