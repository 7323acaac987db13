"""The cases of tests/test_gpu_mg_pcg.py without a GPU: the one table both files use, and the proof that
the GPU tests can fail for the right reasons and cannot hide a failure.
  teeth     a restatement with hx and hy exchanged is far from the right one on every stretched case
  floors    the reference's own uncertainty, from which the GPU tolerances come by formula: the fp64 cycle against the long double
            cycle (tol_M = max(1e-13, 16 floor)) and the PCG trace against itself with naive reversed sums (tol_pcg = max(1e-13,
            64 spread), per case, iteration and quantity); both must stay <= 1e-11
  margins   wherever a GPU test asserts an iteration count or a stop reason, the deciding numbers miss their thresholds by >= 1 %
Run with -s to see the table that DESIGN section 10.5 records."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_reference as R  # noqa: E402
import test_mg_f32_cpu as ref32  # noqa: E402

ISO, WIDE_Y, WIDE_X, MG, MG_ANY = R.ISO, R.WIDE_Y, R.WIDE_X, R.MG, R.MG_ANY
DOM_NAME = {ISO: "ISO", WIDE_Y: "WIDE_Y", WIDE_X: "WIDE_X"}
CAP = 1e-11                                                        # no tolerance may need more than this

# ---- the case table ------------------------------------------------------------------------------------------------------------
# V-cycle cases (groups a, b): nvec seeded standard_normal vectors r; f32 = the fp32 cycle is checked on the same vectors
Cycle = namedtuple("Cycle", "group N kind dom seed nvec f32")
# PCG cases (groups c - f): b = A u for a seeded standard_normal u where an error norm is involved (with_u), else b itself is the
# standard_normal vector.  k: fixed iterations traced (group c checks its prefixes); None = the rule stops the solve.
# exact_error = False switches the MSG exact-error test off (setExactErrorEps(-1)).  f32 = the fp32 cycle.
Pcg = namedtuple("Pcg", "group N kind dom seed with_u rule eps k exact_error f32", defaults=(True, False))

CYCLES = (
    [Cycle("a", 64, MG, d, 640 + i, 2, False) for i, d in enumerate((WIDE_Y, WIDE_X))] +
    [Cycle("a", N, MG_ANY, d, 10 * N + i, 2, N in (50, 258)) for N in (50, 100, 258) for i, d in enumerate((WIDE_Y, WIDE_X))] +
    [Cycle("b", 2050, MG_ANY, ISO, 20500, 1, True), Cycle("b", 2050, MG_ANY, WIDE_Y, 20501, 1, True),
     Cycle("b", 4100, MG_ANY, ISO, 41000, 1, True)])
SYMMETRY = Cycle("a", 258, MG_ANY, WIDE_X, 2583, 2, True)          # (M r1, r2) = (r1, M r2)

_GRIDS = ((50, MG_ANY), (258, MG_ANY), (64, MG))
# seeds are base + 10 j for the first j at which the case keeps every tolerance it needs <= CAP and its stop margin >= 3 %
_J = {("c", 258, ISO): 2, ("d", 50, WIDE_X): 1, ("d", 258, ISO): 3, ("d", 258, WIDE_X): 5, ("e", 258, ISO): 1, ("e", 258, WIDE_X): 1,
      ("e", 64, ISO): 1, ("e", 64, WIDE_X): 1}


def _seed(group, N, d, base):
    return base + 10 * _J.get((group, N, d), 0)


_DOMS = (ISO, WIDE_Y, WIDE_X)
FIXED_K = (1, 2, 5)
FIXED = ([Pcg("c", N, kind, d, _seed("c", N, d, 1000 * N + i), False, R.REL_2NORM, 1e-8, max(FIXED_K)) for N, kind in _GRIDS for i, d in enumerate(_DOMS)] +
         [Pcg("c", 2050, MG_ANY, ISO, 2050000, False, R.REL_2NORM, 1e-8, 3)])
REL = ([Pcg("d", N, MG_ANY, d, _seed("d", N, d, 2000 * N + i), True, R.REL_2NORM, 1e-8, None) for N in (50, 258) for i, d in enumerate((ISO, WIDE_X))] +
       [Pcg("d", 64, MG, WIDE_Y, 128001, True, R.REL_2NORM, 1e-8, None)])
REL_F32 = Pcg("d", 258, MG_ANY, WIDE_X, 516009, True, R.REL_2NORM, 1e-8, None, True, True)
MSG = ([Pcg("e", N, kind, d, _seed("e", N, d, 3000 * N + i), True, R.MSG, 1e-6, None) for N, kind in _GRIDS for i, d in enumerate(_DOMS)] +
       [Pcg("e", 258, MG_ANY, WIDE_Y, 774009, True, R.MSG, 1e-6, None, False)])
BATCH = FIXED[-1]                                                  # group f: system 0 is group c's N = 2050 case ...
BATCH_MORE_SEEDS = (2050001, 2050002)                              # ... beside two more right-hand sides
CASES = CYCLES + [SYMMETRY] + FIXED + REL + [REL_F32] + MSG


def case_id(c):
    extra = "" if isinstance(c, Cycle) else ("" if c.exact_error else "-noexact") + ("-f32" if c.f32 else "")
    return f"{c.group}-{c.N}-{'mg' if c.kind == MG else 'any'}-{DOM_NAME[c.dom]}{extra}"


def vectors(c):
    """the seeded inputs of a case: Cycle -> [r, ...]; Pcg -> (b, u) with u = None where no error norm is involved"""
    rng = np.random.default_rng(c.seed)
    n = int(R.ref.interior_mask(c.N).sum())
    if isinstance(c, Cycle):
        return [rng.standard_normal(n) for _ in range(c.nvec)]
    v = rng.standard_normal(n)
    return (R.apply_A(levels(c), v), v) if c.with_u else (v, None)


@functools.lru_cache(maxsize=4)
def levels(c):
    return R.levels_for(c.N, c.dom, c.kind)


Reference = namedtuple("Reference", "levels b u trace spread tol margin")


@functools.lru_cache(maxsize=None)
def reference(c):
    """what a PCG case is compared with: the fsum trace, its spread, tol[quantity][iteration] = tol_pcg of the quantity's own
    spread (the entries of CAPPED: CAP where the formula gives more), and the stop margin (None for a fixed-iteration case).
    The fp32 case traces the float32 restatement of the cycle (its iteration count and margin only)."""
    lv = levels(c)
    b, u = vectors(c)
    M = None
    if c.f32:
        lv32 = ref32.hierarchy32(lv)
        M = lambda r: ref32.apply_M32(lv32, r)
    eee = c.eps if c.exact_error else -1.0
    t = R.pcg_trace(lv, b, u=u, iterations=c.k, rule=c.rule, eps=c.eps, eps_exact_error=eee, M=M)
    sp = R.spread(lv, b, t.iterations, u=u, M=M, exact=t)
    tol = {q: np.minimum(R.tol_pcg(v), CAP) if (case_id(c), q) in CAPPED else R.tol_pcg(v) for q, v in sp.items()}
    margin = None if c.k is not None else R.stop_margin(t, c.rule, c.eps, eee)
    return Reference(lv, b, u, t, sp, tol, margin)


def checked(c, t):
    """(quantity, iteration index) pairs whose tol_pcg the GPU test of the case uses -- the ones the cap is about"""
    last = t.iterations - 1
    if c.group == "c":
        ks = [k - 1 for k in FIXED_K] if c.k == max(FIXED_K) else [last]
        return [(q, i) for q in ("x", "r2", "b2") for i in ks]
    if c.group == "d":                                               # the fp32 case: only the last callback against the returned x
        return [("true2", last)] if c.f32 else [(q, i) for q in ("dx2", "true2", "x") for i in range(t.iterations)]
    return [(q, i) for q in ("dx_max", "r_max", "x") for i in sorted({0, last})]


# The error norms ||x - u||_2 and max|x - u| are differences of nearly equal vectors: | ||xa - u|| - ||xb - u|| | <= ||xa - xb||, and
# no better relative to ||x - u|| itself, which falls to 1e-8 ||x|| by the end of a REL_2NORM 1e-8 solve (the relative difference
# of the two summation orders reaches 6e-10 there, and is a poor sample: 3.5e-11, 4.0e-13, 7.3e-11 at iterations 11, 12, 13 of
# d-50-any-WIDE_X).  So the GPU tests bound them as they bound x: |e - e_ref| <= tol_pcg('x') ||x_ref||, in the norm of e, and 'x'
# is the quantity that must keep tol_pcg <= CAP for them.  They are also pinned to the returned x, exactly (max-norm) and within
# 1e-13 (2-norm).
# (case, quantity) whose formula exceeds CAP at the size the case is there for (a block marching over two rows): the naive
# reversed sum over 3.15 million terms is itself no better than 2e-13, and ||r_2|| / ||r_3|| = 20 carries that into ||r_3||.  The
# GPU test allows CAP there, less than the formula.
CAPPED = {("c-2050-any-ISO", "r2")}


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
    lv32 = ref32.hierarchy32(ref.levels)
    _, it = ref32.pcg(lambda r: ref32.apply_M32(lv32, r), ref.levels[0], ref.b, eps=REL_F32.eps)
    assert it == ref.trace.iterations


# ---- the reference itself ------------------------------------------------------------------------------------------------------
def test_trace_agrees_with_the_plain_pcg_of_the_restatement():
    c = FIXED[1]
    ref = reference(c)
    x, it = R.ref_any.pcg(ref.levels, ref.b, eps=0.0, max_iterations=c.k)
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
