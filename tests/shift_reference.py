"""The reference of the shifted operator A - sigma I and of the theta-scheme stepper, built on the
restatement of tests/mg_reference.py without editing it: the hierarchy with every level's diagonal shifted, the right-hand side of
a step, and the margin and order-of-summation spread of a warm-started trace (mg_reference.stop_margin and .spread know cold
starts only).  A plain module: no test in here, nothing that needs a GPU.

The cases the CPU and the GPU tests share are listed here, so that the CPU test asserts the stop margins of exactly the inputs
the GPU tests compare iteration counts on."""
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_reference as R  # noqa: E402
import mg_model as ref  # noqa: E402

EPS = 1e-8
MARGIN = 0.01                          # iteration counts are compared only where the reference's deciding ratio stays this far from 1
SIGMAS = (0.0, 1.0, 1e3, 1e5, 1e7)
# (N, kind, domain): a non-nested pair; nested with the graph replay of small grids; a mixed ladder, anisotropic
GRIDS = ((34, R.MG_ANY, R.ISO), (64, R.MG, R.ISO), (258, R.MG_ANY, R.WIDE_Y))
# (N, kind, domain, theta, tau) of the stepper; four steps each
STEPPER = ((34, R.MG_ANY, R.ISO, 1.0, 1e-4), (34, R.MG_ANY, R.ISO, 0.5, 1e-2),
           (64, R.MG, R.WIDE_Y, 0.5, 1e-4), (64, R.MG, R.WIDE_Y, 1.0, 1.0))
STEPS = 4


def shifted_levels(N, dom, kind, sigma):
    """mg_reference.levels_for with every level's diagonal shifted by sigma (the same sigma on every level, no scaling) and the
    coarsest level's dense inverse that of the shifted matrix"""
    return R.levels_for(N, dom, kind, sigma=sigma)


def theta_rhs(base_levels, u, g, sigma, theta):
    """b_step = -sigma u - ((1 - theta) / theta) A u + g / theta with the unshifted A of base_levels"""
    return -sigma * u - ((1.0 - theta) / theta) * R.apply_A(base_levels, u) + g / theta


def rhs_vector(N, seed=0):
    """the seeded standard-normal right-hand side of the solve cases"""
    n = int(ref.interior_mask(N).sum())
    return np.random.default_rng(1000 * N + seed).standard_normal(n)


def stepper_inputs(N):
    """u0 = 1e-4 x standard normal, g standard normal"""
    rng = np.random.default_rng(N)
    n = int(ref.interior_mask(N).sum())
    return 1e-4 * rng.standard_normal(n), rng.standard_normal(n)


def warm_margin(t, eps=EPS):
    """mg_reference.stop_margin of a REL_2NORM trace that started from a guess: the threshold is eps ||b||_2"""
    if not t.converged:
        return 0.0
    thr = eps * t.b_norm2
    m = []
    for i, v in enumerate([t.r0_norm2] + t.r2):
        ratio = v / thr
        assert (ratio <= 1.0) == (i == t.iterations)
        m.append(abs(ratio - 1.0))
    return min(m)


def warm_spread(levels, b, x0, iterations, exact=None, M=None):
    """mg_reference.spread for a trace from the guess x0: per iteration the largest relative difference between the trace with
    exactly rounded sums and the one with naive sums in reversed order, over x, ||dx||, ||r|| and their max-norms"""
    a = R.pcg_trace(levels, b, x0=x0, iterations=iterations, M=M) if exact is None else exact
    v = R.pcg_trace(levels, b, x0=x0, iterations=iterations, M=M, total=R._reversed_sum)
    out = [np.array([np.abs(xa - xv).max() / np.abs(xa).max() for xa, xv in zip(a.x[:iterations], v.x)])]
    for name in ("dx2", "r2", "dx_max", "r_max"):
        sa, sv = np.array(getattr(a, name)[:iterations]), np.array(getattr(v, name))
        out.append(np.abs(sa - sv) / np.abs(sa))
    return np.max(np.stack(out), axis=0)


def step_reference(base_levels, levels, u, g, sigma, theta, M=None):
    """one step from the state u: the rule-driven warm trace of (A - sigma I) u+ = b_step, its margin, and the tolerance of its
    last iterate (None for a step of 0 iterations, whose state is the start's bits)"""
    b = theta_rhs(base_levels, u, g, sigma, theta)
    t = R.pcg_trace(levels, b, x0=u, eps=EPS, M=M)
    tol = None
    if t.iterations:
        tol = R.tol_pcg(warm_spread(levels, b, u, t.iterations, exact=t, M=M))[-1]
    return SimpleNamespace(b=b, trace=t, margin=warm_margin(t), tol=tol, u=t.x[-1] if t.iterations else u)
