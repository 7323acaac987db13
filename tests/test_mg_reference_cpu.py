"""The cases of tests/test_gpu_mg_pcg.py without a GPU: the one table both files use, and the proof that
the GPU tests can fail for the right reasons and cannot hide a failure.
  teeth     a restatement with hx and hy exchanged is far from the right one on every stretched case
  floors    the reference's own uncertainty, from which the GPU tolerances come by formula: the fp64 cycle against the long double
            cycle (tol_M = max(1e-13, 16 floor)) and the PCG trace against itself with naive reversed sums (tol_pcg = max(1e-13,
            64 spread), per case, iteration and quantity); both must stay <= 1e-11
  margins   wherever a GPU test asserts an iteration count or a stop reason, the deciding numbers miss their thresholds by >= 1 %
Run with -s to see the table that DESIGN section 10.5 records."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model as model  # noqa: E402
import mg_reference as R  # noqa: E402
from mg_cases import (CAP, CAPPED, CASES, CYCLES, FIXED, Cycle, ISO, MG, MG_ANY, MSG, REL, REL_F32, SYMMETRY, WIDE_X,  # noqa: E402
                      WIDE_Y, case_id, checked, levels, reference, vectors)


def test_every_capped_entry_names_a_case():
    assert {e[0] for e in CAPPED} <= {case_id(c) for c in FIXED + REL + MSG}


# ---- teeth ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in CASES if c.dom != ISO], ids=case_id)
def test_exchanged_steps_are_far_from_the_right_restatement(c):
    right, wrong = levels(c), R.levels_for(c.N, c.dom, c.kind, exchanged=True)
    if isinstance(c, Cycle):
        rs = vectors(c)
    else:
        rs = [vectors(c)[0]]
    for r in rs:
        z, zw = R.apply_M(right, r), R.apply_M(wrong, r)
        dev = np.abs(zw - z).max() / np.abs(z).max()
        x = R.pcg_trace(right, r, iterations=1).x[0]
        xw = R.pcg_trace(wrong, r, iterations=1).x[0]
        devx = np.abs(xw - x).max() / np.abs(x).max()
        print(f"{case_id(c)}: exchanged hx, hy: apply_M differs by {dev:.2f}, x after one iteration by {devx:.2f} of the max-norm")
        assert dev > 0.1 and devx > 0.1


# ---- floors --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CYCLES + [SYMMETRY], ids=case_id)
def test_cycle_floor(c):
    lv = levels(c)
    for r in vectors(c):
        floor = R.cycle_floor(lv, r)
        print(f"{case_id(c)}: floor max|M r - M_longdouble r| / max|M_longdouble r| = {floor:.2e}, tol_M = {R.tol_M(floor):.2e}")
        assert R.tol_M(floor) <= CAP


@pytest.mark.parametrize("c", FIXED + REL + [REL_F32] + MSG, ids=case_id)
def test_pcg_spread_and_margin(c):
    ref = reference(c)
    t, sp = ref.trace, ref.spread
    reason = {R.ITERATIONS: "iterations", R.PRECISION: "precision", R.RESIDUAL: "residual", R.EXACT_ERROR: "exact error"}[t.reason]
    if c.rule == R.REL_2NORM:
        reason = "fixed" if c.k is not None else ("converged" if t.converged else "iterations")
    worst = {q: max((sp[q][i] for qq, i in checked(c, t) if qq == q), default=None) for q in sp}
    shown = ", ".join(f"{q} {v:.1e}" for q, v in worst.items() if v is not None)
    margin = "-" if ref.margin is None else f"{100 * ref.margin:.1f} %"
    print(f"{case_id(c)}: {t.iterations} iterations, stop {reason}, margin {margin}; largest spread where checked: {shown or '-'}")
    if c.k is None:
        assert t.converged and ref.margin >= 0.01
    needed = set()
    for q, i in checked(c, t):
        formula = R.tol_pcg(sp[q])[i]                                # never the clamped ref.tol
        if (case_id(c), q) in CAPPED:
            assert ref.tol[q][i] == min(formula, CAP)
            if formula > CAP:
                needed.add((case_id(c), q))
        else:
            assert ref.tol[q][i] == formula <= CAP, (q, i, formula)
    assert needed == {e for e in CAPPED if e[0] == case_id(c)}       # an exception that is not needed must go


def test_the_fp32_case_takes_the_iterations_of_test_mg_f32_cpu():
    ref = reference(REL_F32)
    _, it = model.pcg(ref.levels, ref.b, eps=REL_F32.eps, M=lambda r: model.apply_M32(ref.levels, r))
    assert it == ref.trace.iterations


# ---- the reference itself ------------------------------------------------------------------------------------------------------
def test_trace_agrees_with_the_plain_pcg_of_the_restatement():
    c = FIXED[1]
    ref = reference(c)
    x, it = model.pcg(ref.levels, ref.b, eps=0.0, max_iterations=c.k)
    assert it == c.k
    assert np.abs(x - ref.trace.x[-1]).max() <= 1e-12 * np.abs(x).max()
    assert ref.trace.true2[-1] == pytest.approx(np.linalg.norm(ref.b - R.apply_A(ref.levels, x)), rel=1e-9)


@pytest.mark.parametrize("N,kind,dom", [(50, MG_ANY, WIDE_X), (64, MG, WIDE_Y), (100, MG_ANY, ISO)])
def test_long_double_cycle_is_the_fp64_cycle_to_rounding(N, kind, dom):
    lv = R.levels_for(N, dom, kind)
    r = np.random.default_rng(N).standard_normal(int(lv[0].mask.sum()))
    zl = R.apply_M_longdouble(lv, r)
    assert zl.dtype == np.longdouble
    assert np.abs(R.apply_M(lv, r) - zl).max() <= 1e-14 * np.abs(zl).max()


def test_msg_order_and_switches():
    c = MSG[0]
    ref = reference(c)
    t = ref.trace
    assert t.reason in (R.PRECISION, R.RESIDUAL, R.EXACT_ERROR)
    huge = R.pcg_trace(ref.levels, ref.b, u=ref.u, rule=R.MSG, eps=1e300)                 # every test fires: the first in order wins
    assert huge.iterations == 1 and huge.reason == R.PRECISION
    off = R.pcg_trace(ref.levels, ref.b, u=ref.u, rule=R.MSG, eps=-1.0, eps_exact_error=1e300)
    assert off.iterations == 1 and off.reason == R.EXACT_ERROR
    none = R.pcg_trace(ref.levels, ref.b, u=ref.u, rule=R.MSG, eps=-1.0, eps_exact_error=-1.0, max_iterations=3)
    assert none.iterations == 3 and none.reason == R.ITERATIONS and not none.converged
