#!/usr/bin/env python3
"""Time to solution, plain CG against multigrid-preconditioned CG (mi355cg_set_preconditioner), on one GPU.

For every N and rule: one handle, the plain solve, then set_preconditioner(MG) (its set-up time is reported on its own) and the
preconditioned solve; each solve twice, the faster wall time reported.  Rules: REL_2NORM eps 1e-8 (no iteration cap in effect)
and the MSG rule with mi355cg_default_params (eps 1e-6, at most 10 000 iterations, the true solution in the error norm).
The true relative residual ||b - A x|| / ||b|| comes from mi355cg_get_true_residual.
--kind any: the plain solve, MG where the grid has a nested hierarchy, and MG_ANY (MI355CG_PRECOND_MG_ANY), each preconditioner
built afresh on the handle.
Usage: python tools/mg_timing.py [N ...]      (default 256 1024 4096 8192; writes profiles/mg_time_to_solution.txt)
       python tools/mg_timing.py --kind any [N ...]   (default 100 258 1000 1002 4096 4098 10000;
                                                      writes profiles/mg_any_time_to_solution.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import iterative_solvers_amd as isa  # noqa: E402
from iterative_solvers_amd import _capi  # noqa: E402

OUT = {"mg": os.path.join(ROOT, "profiles", "mg_time_to_solution.txt"),
       "any": os.path.join(ROOT, "profiles", "mg_any_time_to_solution.txt")}
SIZES = {"mg": [256, 1024, 4096, 8192], "any": [100, 258, 1000, 1002, 4096, 4098, 10000]}
RULES = {"REL_2NORM 1e-8": _capi.RULE_REL_2NORM, "MSG defaults": _capi.RULE_MSG_MAXNORM}


def params(rule):
    p = isa.default_params(rule)
    if rule == _capi.RULE_REL_2NORM:
        p.eps_rel, p.max_iterations = 1e-8, 1_000_000
    return p


def run(h, rule, b_norm):
    best = None
    for _ in range(2):
        t0 = time.perf_counter()
        res = h.solve(params(rule))
        wall = time.perf_counter() - t0
        if best is None or wall < best[0]:
            best = (wall, res)
    wall, res = best
    rel = np.linalg.norm(h.true_residual()) / b_norm
    return wall, res, rel


def main(ns, kind="mg"):
    pw = 5 if kind == "mg" else 6
    what = "MG-preconditioned CG" if kind == "mg" else "MG- and MG_ANY-preconditioned CG"
    lines = [f"# time to solution on one MI355X: plain CG against {what} (tools/mg_timing.py{' --kind any' if kind == 'any' else ''})",
             "# wall = host wall time of mi355cg_solve (best of 2); solve_s = mi355cg_results.solve_seconds; true_rel = ||b - A x|| / ||b||",
             f"# {'N':>5} {'rule':<15} {'path':<{pw}} {'iters':>7} {'stop':>5} {'conv':>4} {'wall_s':>10} {'solve_s':>10} {'true_rel':>9}  speed-up"]
    print("\n".join(lines), flush=True)
    for n in ns:
        s = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
        h = s._handle
        b_norm = np.linalg.norm(s.get_rhs())
        kinds = [("MG", isa.PRECOND_MG)]
        if kind == "any":
            try:
                isa.mg_levels(n)
            except ValueError:
                kinds = []
            kinds.append(("MG_ANY", isa.PRECOND_MG_ANY))
        for name, rule in RULES.items():
            h.set_preconditioner(isa.PRECOND_NONE)
            wp, rp, tp = run(h, rule, b_norm)
            rows = [("plain", wp, rp, tp, "")]
            for path, pk in kinds:
                h.set_preconditioner(isa.PRECOND_NONE)                      # every kind builds its own hierarchy
                t0 = time.perf_counter()
                h.set_preconditioner(pk)
                setup = time.perf_counter() - t0
                wm, rm, tm = run(h, rule, b_norm)
                rows.append((path, wm, rm, tm, f"  {wp / wm:8.1f}x  ({path} set-up {setup:.3f} s)"))
            for path, w, r, t, extra in rows:
                line = (f"  {n:>5} {name:<15} {path:<{pw}} {r.iterations:>7} {r.stop_reason:>5} {r.converged:>4} {w:>10.4f} "
                        f"{r.solve_seconds:>10.4f} {t:>9.2e}{extra}")
                lines.append(line)
                print(line, flush=True)
        h.close()
    with open(OUT[kind], "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", OUT[kind])


if __name__ == "__main__":
    args = sys.argv[1:]
    kind = "mg"
    if "--kind" in args:
        i = args.index("--kind")
        kind = args[i + 1]
        del args[i:i + 2]
        if kind not in OUT:
            sys.exit(f"--kind must be one of {sorted(OUT)}")
    main([int(a) for a in args] or SIZES[kind], kind)
