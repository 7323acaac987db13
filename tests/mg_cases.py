"""The inputs the CPU and the GPU tests of multigrid-preconditioned CG share: the case table of tests/test_gpu_mg_pcg.py and
tests/test_mg_reference_cpu.py with its seeded vectors and cached references, the right-hand sides of the
batch tests (tools/mg_bits.batch_rhs, passed on), and the oracle's right-hand side.  A plain module: no test in here, nothing
that needs a GPU."""
import functools
import os
import sys
from collections import namedtuple

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import mg_model as model  # noqa: E402
import mg_reference as R  # noqa: E402
from mg_bits import batch_rhs, checkerboard  # noqa: E402,F401  (stated in the tool that records the bits; shared from here)

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
    n = int(model.interior_mask(c.N).sum())
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
    The fp32 case traces the float32 run of the cycle (its iteration count and margin only)."""
    lv = levels(c)
    b, u = vectors(c)
    M = None
    if c.f32:
        M = lambda r: model.apply_M32(lv, r)
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


def oracle_rhs(N, dom=model.DOM):
    from oracle.oracle import OracleGrid
    return np.asarray(OracleGrid(N, N, *dom).rhs(), dtype=np.float64)
