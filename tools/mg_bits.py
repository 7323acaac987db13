#!/usr/bin/env python3
"""Record the bits of the fp64 multigrid path, single and batched, into tests/golden/mg_bits.json on one GPU.

tests/test_gpu_mg_batch.py pins batch == single and tests/test_gpu_mg*.py pin single ~ the NumPy restatement to a tolerance, so a
change that moves both kernel families by one ulp passes them.  This file pins the bits themselves: tests/test_gpu_mg_bits.py
asserts that the tree under test reproduces it.  It is recorded from a build of the commit whose results are the contract
(--tree DIR: that built checkout, whose package is imported instead of this one, the way tools/mg_timing.py takes
--baseline-tree; --commit HASH: noted in the file).

Cases (CASES): the smallest grids at which each element-wise body of csrc/mg_kernels.h can still go wrong, fp64 cycle, right-hand
sides from batch_rhs below (tests/mg_cases.py hands the same function to the batch tests).  Per case: the sha256 of the right-hand sides' bytes (a changed input is then
reported as such); per system iterations, stop_reason, the hex of r_norm2 and initial_r_norm2 and the sha256 of x, from single
solves and from one batch; and the sha256 of apply_preconditioner(last right-hand side).
Usage: python tools/mg_bits.py --commit HASH [--tree DIR] [--out FILE]"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "mg_bits.json")
DOM = (1.0, 2.0, 1.0, 2.0)
# rows of batch_rhs(N, b, scaled=False): 0 the grid's b, 1 zeros, 2 ones, 3 checkerboard, 4 seeded standard-normal.  REL_2NORM
# 1e-8 stops the zero vector at once and the others later: the batch freezes a system.  The MSG rule has no test before the
# first iteration, and 0 / 0 in alpha gives NaN, whose bits are no contract: no zero vector there.
CASES = [
    # name, N, kind, rule, rows                  what only this case reaches
    ("n16", 16, "any", "rel", (0, 1, 4)),        # level 0 is the coarsest: the coarse solve and dot
    ("n34", 34, "any", "rel", (0, 1, 4)),        # one non-nested transfer onto the coarsest grid
    ("n256", 256, "mg", "rel", (0, 1, 4)),       # nested levels only; cb != 0: mg_at's left-of-storage branch
    ("n258", 258, "any", "rel", (0, 1, 4)),      # one non-nested level, three nested; rows longer than a block
    ("n2050", 2050, "any", "rel", (0, 4)),       # more interior rows than kMgMaxGrid: the row stride loop iterates
    ("n34_msg", 34, "any", "msg", (0, 2, 4)),    # the MSG rule's tests
]


def checkerboard(N):
    """+-1 on the interior of the L-shaped grid (tests/mg_model.interior_mask) by the parity of x + y, packed order"""
    y, x = np.mgrid[0:N + 1, 0:N + 1]
    h = N // 2
    interior = (y >= 1) & (y <= N - 1) & (x <= N - 1) & (x >= np.where(y <= h, h + 1, 1))
    return np.where((x + y) % 2 == 0, 1.0, -1.0)[interior]


def batch_rhs(N, b, scaled=True):
    """The right-hand sides of the bit-identity tests, in this order: the grid's b, zeros, ones, the interior checkerboard,
    seeded standard-normal [, b * 2^200, b * 2^-200].  They are part of what the recorded file pins, so they are stated here,
    where nothing under tests/ is needed to record or replay it."""
    n = b.size
    out = [b.copy(), np.zeros(n), np.ones(n), checkerboard(N), np.random.default_rng(N).standard_normal(n)]
    if scaled:
        out += [np.ldexp(b, 200), np.ldexp(b, -200)]
    return np.ascontiguousarray(np.stack(out))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def system_record(res, x):
    return {"iterations": int(res.iterations), "stop_reason": int(res.stop_reason), "r_norm2": float(res.r_norm2).hex(),
            "initial_r_norm2": float(res.initial_r_norm2).hex(), "x_sha256": sha(x)}


def case_params(isa, rule):
    p = isa.default_params(isa.RULE_REL_2NORM if rule == "rel" else isa.RULE_MSG_MAXNORM)
    if rule == "rel":
        p.eps_rel, p.max_iterations = 1e-8, 1000
    p.use_true_solution = 0
    return p


def compute(case):
    """One case's record by the package that is importable now."""
    import iterative_solvers_amd as isa
    name, N, kind, rule, rows = case
    s = isa.MatrixFreeSystem(N, N, *DOM)
    s.set_preconditioner(isa.PRECOND_MG if kind == "mg" else isa.PRECOND_MG_ANY)
    h = s._handle
    rhs = np.ascontiguousarray(batch_rhs(N, s.get_rhs(), scaled=False)[list(rows)])
    p = case_params(isa, rule)
    rec = {"name": name, "N": N, "kind": kind, "rule": rule, "rows": list(rows), "rhs_sha256": sha(rhs),
           "precond_sha256": sha(h.apply_preconditioner(rhs[-1])), "single": [], "batch": []}
    for v in rhs:
        h.set_rhs(v)
        res = h.solve(p)
        rec["single"].append(system_record(res, h.solution()))
    xb, rb = h.solve_batch(p, rhs)
    rec["batch"] = [system_record(r, x) for r, x in zip(rb, xb)]
    h.close()
    return rec


def main(args):
    out, commit, tree = OUT, None, ROOT
    while args:
        a = args.pop(0)
        if a == "--tree":
            tree = os.path.abspath(args.pop(0))
        elif a == "--commit":
            commit = args.pop(0)
        elif a == "--out":
            out = os.path.abspath(args.pop(0))
        else:
            sys.exit(__doc__)
    if not commit:
        sys.exit("--commit HASH: the commit the recorded build is of")
    sys.path.insert(0, tree)                                           # before iterative_solvers_amd is imported
    import iterative_solvers_amd as isa
    doc = {"commit": commit, "cases": [compute(c) for c in CASES]}
    for c in doc["cases"]:
        print(c["name"], "iterations", [r["iterations"] for r in c["single"]], "batch == single:", c["batch"] == c["single"], flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("package", os.path.dirname(isa.__file__), "-> wrote", out)


if __name__ == "__main__":
    main(sys.argv[1:])
