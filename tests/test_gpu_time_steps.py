"""Device-resident theta-scheme steps on the GPU (mi355cg_time_steps) against tests/shift_reference.py: every
step compared with the reference step computed from the device's own previous state, one call against the chain of single-step
calls, the steady state, what the handle keeps, the two ways a step can fail to converge, the refusals, and device tensors.
tests/test_shift_cpu.py asserts the stop margins of the configurations whose iteration counts are compared here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shift_reference as S  # noqa: E402

R = S.R
pytestmark = pytest.mark.gpu


def system(N, dom, kind, g):
    import iterative_solvers_amd as isa
    s = isa.MatrixFreeSystem(N, N, *dom)
    s._handle.set_rhs(g)
    if kind is not None:
        s.set_preconditioner(kind)
    return s


def params(eps=S.EPS, max_iterations=10000):
    import iterative_solvers_amd as isa
    p = isa.default_params(isa.RULE_REL_2NORM)
    p.eps_rel, p.max_iterations, p.use_true_solution = eps, max_iterations, 0
    return p


def show(what, dev, tol):
    print(f"  {what}: deviation {dev:.2e}, tolerance {tol:.2e}")
    return dev <= tol


def check_chain(N, kind, dom, theta, tau, steps):
    """single-step calls, each against the reference step from the device's own previous state; returns the device's states"""
    sigma = 1.0 / (theta * tau)
    ref_kind = R.MG_ANY if kind is None else kind
    base, levels = R.levels_for(N, dom, ref_kind), S.shifted_levels(N, dom, ref_kind, sigma)
    M = (lambda r: r) if kind is None else None
    u0, g = S.stepper_inputs(N)
    s = system(N, dom, kind, g)
    u, states, ok = u0, [], True
    for k in range(steps):
        st = S.step_reference(base, levels, u, g, sigma, theta, M=M)
        assert st.margin >= S.MARGIN                                # tests/test_shift_cpu.py: it holds along the reference's own chain
        un, res, done = s.time_steps(u, tau, theta, 1)
        print(f"N={N} theta={theta} tau={tau:g} step {k}: {res[0].iterations} iterations (reference {st.trace.iterations}, margin {st.margin:.3f})")
        assert done == 1 and len(res) == 1 and res[0].converged
        assert res[0].iterations == st.trace.iterations >= 1
        ok &= show("u, max|u - u_ref| / max|u_ref|", np.abs(un - st.u).max() / np.abs(st.u).max(), st.tol)
        # r0 = b_step - (A - sigma I) u is a difference of vectors of the size of b_step, each element a handful of roundings: its
        # norm is bounded relative to ||b_step||, where 1e-13 is the floor of mg_reference.tol_pcg
        ok &= show("initial_r_norm2 over ||b_step||", abs(res[0].initial_r_norm2 - st.trace.r0_norm2) / st.trace.b_norm2, 1e-13)
        u = un
        states.append(un)
    assert ok
    assert s.shift == sigma
    return s, u0, g, states


@pytest.mark.parametrize("N,kind,dom,theta,tau", S.STEPPER, ids=lambda v: str(v) if isinstance(v, (int, float)) else None)
def test_steps_match_the_reference_and_one_call_is_the_chain(N, kind, dom, theta, tau):
    s, u0, g, states = check_chain(N, kind, dom, theta, tau, S.STEPS)
    fresh = system(N, dom, kind, g)
    u, res, done = fresh.time_steps(u0, tau, theta, S.STEPS)
    assert done == S.STEPS and len(res) == S.STEPS and all(r.converged for r in res)
    assert np.array_equal(u, states[-1])
    # continuation on the device: k calls of one step, each from the solution of the last
    h = system(N, dom, kind, g)._handle
    h.set_initial_guess(u0)
    its = []
    for k in range(S.STEPS):
        if k:
            h.use_solution_as_initial_guess()
        r1, d1 = h.time_steps(params(), tau, theta, 1)
        assert d1 == 1
        its.append(r1[0].iterations)
        assert np.array_equal(h.solution(), states[k])
    assert its == [r.iterations for r in res]


def test_steps_without_a_preconditioner():
    check_chain(34, None, R.ISO, 1.0, 1e-4, 1)


def test_the_steady_state_is_a_fixed_point():
    N, theta, tau = 34, 0.5, 1e-2
    _, g = S.stepper_inputs(N)
    s = system(N, R.ISO, R.MG_ANY, g)
    h = s._handle
    res = h.solve(params(eps=1e-12))
    assert res.converged
    u = h.solution()
    un, rs, done = s.time_steps(u, tau, theta, 1)
    assert done == 1 and rs[0].iterations == 0 and rs[0].converged
    assert np.array_equal(un, u)


def test_the_handle_keeps_its_rhs_and_the_shift_stays():
    N, theta, tau = 34, 0.5, 1e-2
    u0, g = S.stepper_inputs(N)
    s = system(N, R.ISO, R.MG_ANY, g)
    un, _, done = s.time_steps(u0, tau, theta, 2)
    assert done == 2
    assert np.array_equal(s.get_rhs(), g)
    assert s.shift == 1.0 / (theta * tau)
    # the device's b too: a plain solve afterwards is the shifted solve of g, the bits of a handle that never stepped
    h = s._handle
    x = (h.solve(params()), h.solution())[1]
    other = system(N, R.ISO, R.MG_ANY, g)
    other.set_shift(1.0 / (theta * tau))
    assert np.array_equal(x, (other._handle.solve(params()), other._handle.solution())[1])
    un2, _, _ = s.time_steps(un, tau, theta, 1)                     # the same (tau, theta): the shift is already there
    assert s.shift == 1.0 / (theta * tau) and not np.array_equal(un2, un)


def test_a_step_that_hits_the_iteration_cap_ends_the_stepping():
    import iterative_solvers_amd as isa
    N = 34
    u0, g = S.stepper_inputs(N)
    s = system(N, R.ISO, R.MG_ANY, g)
    h = s._handle
    h.set_initial_guess(u0)
    res, done = h.time_steps(params(max_iterations=1), 1e-2, 0.5, 3)
    assert done == 0 and len(res) == 1
    assert res[0].stop_reason == isa.StopCriterion.ITERATIONS and not res[0].converged and res[0].iterations == 1
    assert not np.array_equal(h.solution(), u0)                     # x holds that step's last iterate


@pytest.mark.parametrize("kind", [None, R.MG_ANY], ids=["plain", "mg"])
def test_a_stop_request_ends_the_stepping(kind):
    import iterative_solvers_amd as isa
    N = 34
    u0, g = S.stepper_inputs(N)
    s = system(N, R.ISO, kind, g)
    h = s._handle
    h.set_initial_guess(u0)
    res, done = h.time_steps(params(), 1e-2, 0.5, 3, stop_flag=C.c_int(1))
    assert done == 0 and len(res) == 1
    assert res[0].stop_reason == isa.StopCriterion.INTERRUPTED and not res[0].converged


def test_refusals():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    from iterative_solvers_amd.solver import _Handle
    from oracle.oracle import OracleGrid
    N = 34
    u0, g = S.stepper_inputs(N)
    s = system(N, R.ISO, R.MG_ANY, g)
    h = s._handle
    lib = h._lib
    p = params()
    out, done = (_capi.Results * 2)(), C.c_int(-7)

    def call(prm=p, tau=1e-2, theta=0.5, nsteps=1, res=out, dn=done, handle=h._h):
        return lib.mi355cg_time_steps(handle, C.byref(prm) if prm is not None else None, tau, theta, nsteps, None, res,
                                      C.byref(dn) if dn is not None else None)
    assert call() == _capi.ERR_STATE and b"starting state" in lib.mi355cg_last_error()      # no pending guess
    h.set_initial_guess(u0)
    for kw in (dict(prm=None), dict(res=None), dict(dn=None), dict(tau=0.0), dict(tau=-1.0), dict(tau=float("nan")),
               dict(tau=float("inf")), dict(theta=0.0), dict(theta=-0.5), dict(theta=1.0 + 1e-12), dict(theta=float("nan")),
               dict(nsteps=-1)):
        assert call(**kw) == _capi.ERR_INVALID, kw
    for field in ("diagnostics", "use_true_solution"):
        q = params()
        setattr(q, field, 1)
        assert call(prm=q) == _capi.ERR_INVALID, field
    assert done.value == -7 and s.shift == 0.0                      # nothing was written
    assert call(nsteps=0) == _capi.OK and done.value == 0 and s.shift == 0.0
    assert call(nsteps=1) == _capi.OK and done.value == 1           # the guess was still pending: the handle was left as it was
    assert s.shift == 1.0 / (0.5 * 1e-2)
    with pytest.raises(ValueError, match="theta"):
        s.time_steps(u0, 1e-2, theta=1.5)
    with pytest.raises(ValueError, match="shape"):
        s.time_steps(u0[:-1], 1e-2)

    mixed = isa.MatrixFreeSystem(64, 64, *R.ISO, dtype=isa.F32_MIXED)
    csr = isa.CrsMatrix(*OracleGrid(16, 16, *R.ISO).csr())
    slab = _Handle.__new__(_Handle)
    slab._lib, slab._h, slab._device = _capi.load(), C.c_void_p(), 0
    _capi.check(slab._lib.mi355cg_create_slab(64, 64, *R.ISO, _capi.F64, 0, 1, 31, C.byref(slab._h)))
    slab.size = int(slab._lib.mi355cg_size(slab._h))
    for other, why in ((mixed._handle, b"fp64 only"), (csr._handle, b"CSR"), (slab, b"single-GPU")):
        done.value = -7
        assert call(handle=other._h) == _capi.ERR_INVALID and why in lib.mi355cg_last_error()
        assert done.value == -7
    slab.close()


def test_a_device_tensor_state_gives_the_bits_of_the_numpy_path():
    import torch
    N, theta, tau = 64, 0.5, 1e-4
    u0, g = S.stepper_inputs(N)
    a, b = system(N, R.WIDE_Y, R.MG, g), system(N, R.WIDE_Y, R.MG, g)
    un, rn, dn = a.time_steps(u0, tau, theta, 2)
    t0 = torch.from_numpy(u0).cuda()
    ut, rt, dt = b.time_steps(t0, tau, theta, 2)
    assert isinstance(ut, torch.Tensor) and ut.is_cuda and ut.dtype == torch.float64 and ut.data_ptr() != t0.data_ptr()
    assert dn == dt == 2 and [r.iterations for r in rn] == [r.iterations for r in rt]
    assert np.array_equal(ut.cpu().numpy(), un)
    assert np.array_equal(t0.cpu().numpy(), u0)                     # the caller's tensor is read, not written
