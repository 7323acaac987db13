"""The on-chip solve mode: chunks of CG iterations in one launch of one workgroup, for plain fp64 grid handles up
to the cap.  It must take the two-launch path's steps bit for bit.  In every test "same" means np.array_equal on x and on the recursive
residual and == on iterations, stop reason, converged, r_norm2 (and the initial norm), final_precision, final_residual_norm and
final_error_norm, against a second handle of the same grid in the default mode; and every test asserts that the on-chip handle
reports on-chip launches for its solve, so that a silent fall-through to the two launches cannot pass."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from onchip_support import DOMAIN, cap as _cap, system as _system  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_pairs = {}


def pair(n, domain=DOMAIN):
    """(on-chip system, default system) of a grid, created once."""
    key = (n, domain)
    if key not in _pairs:
        _pairs[key] = (_system(n, True, domain), _system(n, False, domain))
    return _pairs[key]


def params(rule, **kw):
    """onchip_support.params with the true solution kept: these solves report final_error_norm"""
    import iterative_solvers_amd as isa
    p = isa.default_params(rule)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def run(s, p, callback=None, stop_flag=None):
    """One solve on a system: everything a caller can see, and the on-chip launches of that solve."""
    res = s._handle.solve(p, callback, stop_flag)
    return {"x": s._handle.solution(), "r": s._handle.recursive_residual(),
            "res": (res.iterations, res.stop_reason, res.converged, res.r_norm2, res.initial_r_norm2, res.final_precision,
                    res.final_residual_norm, res.final_error_norm),
            "launches": s.solve_mode_info()["onchip_launches"]}


def same(on, off, what):
    print(what, "on-chip", on["res"], "launches", on["launches"], "| default", off["res"])
    assert on["launches"] > 0, what
    assert off["launches"] == 0, what
    assert on["res"] == off["res"], what
    assert np.array_equal(on["x"], off["x"]), what
    assert np.array_equal(on["r"], off["r"]), what


SIZES = [6, 8, 10, 12, 16, 20, 30, 64, 66, 100, "cap"]     # 12, 20, 100: the shapes of the plan the others leave out
REL = dict(eps_rel=1e-10, sync_every=7)
MSG = dict(eps_precision=1e-9, eps_residual=1e-9, eps_exact_error=1e-9, sync_every=7)


def test_the_sizes_below_cover_every_shape_of_the_plan():
    """Workgroups of 64, 128, 256 and 512 threads and every unroll class of the kernel (1, 2, 4, 8, 16, 24 unknowns per thread)."""
    import iterative_solvers_amd as isa
    plans = [isa.onchip_plan(_cap() if n == "cap" else n) for n in SIZES]
    assert {p["threads"] for p in plans} == {64, 128, 256, 512}
    assert {p["elems_per_thread"] for p in plans} == {1, 2, 4, 8, 16, 24}


@pytest.mark.parametrize("n", SIZES)
def test_converged_solves_both_rules(n):
    """A grid smaller than one wave, N/2 odd and even, every workgroup size and unroll class of the plan; chunks of 7 iterations, so a
    solve spans many launches."""
    from iterative_solvers_amd import _capi
    n = _cap() if n == "cap" else n
    on, off = pair(n)
    for rule, kw in ((_capi.RULE_REL_2NORM, REL), (_capi.RULE_MSG_MAXNORM, MSG)):
        a, b = run(on, params(rule, **kw)), run(off, params(rule, **kw))
        same(a, b, (n, rule))
        assert a["res"][2] == 1                                   # converged
        if a["res"][0] > 7:
            assert a["launches"] >= a["res"][0] // 7              # many launches


def test_oracle_parity_with_exact_inner_products():
    """N = 16, as tests/test_gpu_launch_boundary.py compares: REL_2NORM x, iteration count and norms against OracleGrid.mf_solve under
    oracle.exact_dots() (its result carries no residual vector), MSG x and r against msg_solve."""
    from iterative_solvers_amd import _capi
    from oracle import oracle
    n = 16
    on, _ = pair(n)
    og = oracle.OracleGrid(n, n)
    with oracle.exact_dots():
        mf = og.mf_solve(eps=1e-10, max_iterations=10000)
        ms = og.msg_solve(eps_precision=1e-9, eps_residual=1e-9, eps_exact_error=1e-9)
    a = run(on, params(_capi.RULE_REL_2NORM, **REL))
    assert a["launches"] > 0 and mf.converged
    assert (a["res"][0], a["res"][3], a["res"][4]) == (mf.iterations, mf.r_norm, mf.initial_r_norm)
    assert np.array_equal(a["x"], mf.x)
    m = run(on, params(_capi.RULE_MSG_MAXNORM, **MSG))
    assert m["launches"] > 0
    assert m["res"][:3] == (ms.iterations, ms.stop_reason, int(ms.converged))
    assert m["res"][3:] == (ms.r_norm2, ms.initial_r_norm2, ms.final_precision, ms.final_residual_norm, ms.final_error_norm)
    assert np.array_equal(m["x"], ms.x) and np.array_equal(m["r"], ms.r)


@pytest.mark.parametrize("fixed", [0, 1])
@pytest.mark.parametrize("cap_it", [1, 2, 3, 5, 8])
def test_iteration_caps(cap_it, fixed):
    from iterative_solvers_amd import _capi
    on, off = pair(64)
    for rule, kw in ((_capi.RULE_REL_2NORM, dict(eps_rel=1e-10)), (_capi.RULE_MSG_MAXNORM, dict(eps_precision=1e-9, eps_residual=1e-9, eps_exact_error=1e-9))):
        kw = dict(kw, max_iterations=cap_it, fixed_iterations=fixed)
        a, b = run(on, params(rule, **kw)), run(off, params(rule, **kw))
        same(a, b, (cap_it, fixed, rule))
        assert a["res"][0] == cap_it


def test_msg_callbacks():
    """N = 30 with the true solution and callback_every = 3: the callbacks of it = 0, it = 1, every third iteration and the final one."""
    from iterative_solvers_amd import _capi
    on, off = pair(30)
    got = []
    for s in (on, off):
        cbs = []
        out = run(s, params(_capi.RULE_MSG_MAXNORM, eps_precision=1e-9, eps_residual=1e-9, eps_exact_error=1e-9, callback_every=3),
                  callback=lambda *a: cbs.append(tuple(a)))
        got.append((out, cbs))
    same(got[0][0], got[1][0], "callbacks")
    cbs = got[0][1]
    assert cbs == got[1][1]
    its = [c[0] for c in cbs]
    assert its[:4] == [0, 1, 3, 6] and its[-1] == got[0][0]["res"][0] and len(cbs) >= 6
    assert all(c[3] < 1e300 for c in cbs)                         # the error norm was there on every callback


def test_stop_request_from_the_first_callback():
    """Raised from the it == 1 callback: the first chunk of a watched solve is one iteration, so both modes stop after it."""
    from iterative_solvers_amd import _capi
    on, off = pair(30)
    outs = []
    for s in (on, off):
        flag = C.c_int(0)

        def cb(it, p, r, e, flag=flag):
            if it == 1:
                flag.value = 1
        outs.append(run(s, params(_capi.RULE_MSG_MAXNORM, eps_precision=1e-12, eps_residual=1e-12, eps_exact_error=1e-12), callback=cb, stop_flag=flag))
    same(outs[0], outs[1], "stop request")
    assert outs[0]["res"][1] == _capi.STOP_INTERRUPTED and outs[0]["res"][2] == 0 and outs[0]["res"][0] == 1


def test_anisotropic_domain():
    from iterative_solvers_amd import _capi
    on, off = pair(32, (0.0, 1.0, -1.0, 3.0))
    for rule, kw in ((_capi.RULE_REL_2NORM, REL), (_capi.RULE_MSG_MAXNORM, MSG)):
        same(run(on, params(rule, **kw)), run(off, params(rule, **kw)), ("anisotropic", rule))


def test_shift_warm_start_and_time_steps():
    from iterative_solvers_amd import _capi
    n = 16
    on, off = _system(n, True), _system(n, False)
    x0 = np.random.default_rng(0).standard_normal(on.size())
    for s in (on, off):
        s.set_shift(3.0)
    for rule, kw in ((_capi.RULE_REL_2NORM, REL), (_capi.RULE_MSG_MAXNORM, MSG)):
        outs = []
        for s in (on, off):
            s._handle.set_initial_guess(x0)
            outs.append(run(s, params(rule, **kw)))
        same(outs[0], outs[1], ("shift + warm start", rule))
    u0 = np.random.default_rng(0).standard_normal(on.size())
    steps = []
    for s in (on, off):
        u, res, done = s.time_steps(u0, 1e-3, theta=0.5, nsteps=5)
        steps.append((u, [r.iterations for r in res], done, s.solve_mode_info()["onchip_launches"]))
    assert steps[0][3] > 0 and steps[1][3] == 0
    assert steps[0][1] == steps[1][1] and steps[0][2] == steps[1][2] == 5
    assert np.array_equal(steps[0][0], steps[1][0])
    for s in (on, off):
        s._handle.close()


def test_continuation_across_modes():
    """Five on-chip iterations, then the solve continued to convergence in the default mode, against the same sequence in the default mode alone."""
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    n = 64
    a, b = _system(n, True), _system(n, False)
    first = [run(s, params(_capi.RULE_REL_2NORM, eps_rel=1e-10, max_iterations=5)) for s in (a, b)]
    same(first[0], first[1], "the capped start")
    a._handle.use_solution_as_initial_guess()
    a.set_solve_mode(isa.SOLVE_LAUNCHES)
    b._handle.use_solution_as_initial_guess()
    second = [run(s, params(_capi.RULE_REL_2NORM, eps_rel=1e-10)) for s in (a, b)]
    assert second[0]["launches"] == 0 and second[0]["res"][2] == 1
    assert second[0]["res"] == second[1]["res"]
    assert np.array_equal(second[0]["x"], second[1]["x"]) and np.array_equal(second[0]["r"], second[1]["r"])
    for s in (a, b):
        s._handle.close()


def test_refusals_and_reporting():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    from oracle.oracle import OracleGrid
    cap = _cap()
    lib = _capi.load()
    big = _system(cap + 2, False)
    assert lib.mi355cg_set_solve_mode(big._handle._h, _capi.SOLVE_ONCHIP) == _capi.ERR_INVALID
    assert str(cap).encode() in lib.mi355cg_last_error()
    with pytest.raises(ValueError):
        big.set_solve_mode(isa.SOLVE_ONCHIP)
    assert big.solve_mode_info()["plan"] is None
    big._handle.close()
    mg = _system(16, False)
    mg.set_preconditioner(isa.PRECOND_MG_ANY)
    with pytest.raises(ValueError):
        mg.set_solve_mode(isa.SOLVE_ONCHIP)
    mg.set_preconditioner(isa.PRECOND_NONE)
    mg.set_solve_mode(isa.SOLVE_ONCHIP)                          # eligible again ...
    with pytest.raises(ValueError):
        mg.set_preconditioner(isa.PRECOND_MG_ANY)                # ... and an on-chip handle refuses a preconditioner
    mg.set_preconditioner(isa.PRECOND_NONE)
    assert mg.solve_mode_info()["mode"] == isa.SOLVE_ONCHIP and mg.preconditioner_info()[0] == isa.PRECOND_NONE
    mg._handle.close()
    csr = isa.CrsMatrix(*OracleGrid(8, 8).csr())
    with pytest.raises(ValueError):
        csr._handle.set_solve_mode(isa.SOLVE_ONCHIP)
    mixed = isa.MatrixFreeSystem(16, 16, *DOMAIN, dtype=isa.F32_MIXED)
    with pytest.raises(ValueError):
        mixed.set_solve_mode(isa.SOLVE_ONCHIP)
    mixed._handle.close()
    with pytest.raises(ValueError):
        _system(16, False).set_solve_mode(7)

    # a diagnostics solve keeps the two launches in either mode
    on, off = pair(16)
    outs = []
    for s in (on, off):
        cbs = []
        sol = isa.MatrixFreeSolver(s, s.get_rhs(), 1e-10, 10000)
        sol.setIterationCallback(lambda *a: cbs.append(tuple(a)))
        x = sol.solve(s.get_true_solution_vector())
        outs.append((x, s._handle.recursive_residual(), sol.getIterations(), sol.last_results.r_norm2, cbs, s.solve_mode_info()["onchip_launches"]))
    assert outs[0][5] == 0 and outs[1][5] == 0
    assert outs[0][2:5] == outs[1][2:5] and len(outs[0][4]) == outs[0][2]
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    same(run(on, params(_capi.RULE_REL_2NORM, **REL)), run(off, params(_capi.RULE_REL_2NORM, **REL)), "after the diagnostics solve")

    # the environment knob: eligible handles are in the mode, the others are not
    old = os.environ.get("MI355CG_ONCHIP")
    os.environ["MI355CG_ONCHIP"] = "1"
    try:
        small, large = isa.MatrixFreeSystem(16, 16, *DOMAIN), isa.MatrixFreeSystem(256, 256, *DOMAIN)
    finally:
        if old is None:
            os.environ.pop("MI355CG_ONCHIP")
        else:
            os.environ["MI355CG_ONCHIP"] = old
    assert small.solve_mode_info()["mode"] == isa.SOLVE_ONCHIP and large.solve_mode_info()["mode"] == isa.SOLVE_LAUNCHES
    same(run(small, params(_capi.RULE_REL_2NORM, **REL)), run(off, params(_capi.RULE_REL_2NORM, **REL)), "a handle created under MI355CG_ONCHIP=1")
    small._handle.close()
    large._handle.close()


def test_cpp_host_reaches_the_mode_through_dirichlet_solver():
    """The reference's top-level class at its default n = m = 10: the same iteration count, norms and solution with and without setSolveMode."""
    from iterative_solvers_amd import build as b
    b.build()
    src = os.path.join(ROOT, "tests", "cpp", "onchip_compat_driver.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "onchip_compat_driver")
    headers = [os.path.join(ROOT, "iterative_solvers_amd", "compat", "mi355cg_compat.hpp"), os.path.join(ROOT, "include", "mi355cg.h")]
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(f) for f in [src] + headers):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                               "-I", os.path.join(ROOT, "iterative_solvers_amd", "compat"), src,
                               "-L", os.path.join(ROOT, "iterative_solvers_amd"), "-lmi355cg",
                               "-Wl,-rpath," + os.path.join(ROOT, "iterative_solvers_amd"), "-o", exe])
    env = {k: v for k, v in os.environ.items() if k != "MI355CG_ONCHIP"}
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    j = json.loads(out.stdout)
    on, off = j["onchip"], j["launches"]
    assert (on["mode"], off["mode"]) == (1, 0) and on["launches"] > 0 and off["launches"] == 0
    for key in ("iterations", "converged", "residual_norm", "error_norm", "solution"):
        assert on[key] == off[key], key
    assert on["converged"] == 1 and on["iterations"] > 1
