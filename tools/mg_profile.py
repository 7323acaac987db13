#!/usr/bin/env python3
"""Per-kernel device time of one multigrid-preconditioned solve, from rocprofv3 kernel traces.

  solve:    one REL_2NORM 1e-8 solve with the given kind (run it under rocprofv3 --kernel-trace --stats); --record FILE keeps N,
            kind and iterations as JSON next to the trace.
  summary:  a table per trace directory: launches, total and per-PCG-iteration device time of every k_mg_* kernel (the kernels
            of the solve; the set-up's fills are left out), and the solve's sum.
            --cycle f32 runs the V-cycle in fp32 (MI355CG_CYCLE_F32; its kernels are the k_mg32_* ones).
            --batch NRHS solves NRHS seeded standard-normal right-hand sides by one batched solve instead (mi355cg_solve_batch; its
            kernels are the k_mgb_* ones); "iterations" is then the largest count of the batch.
Usage: python tools/mg_profile.py solve --kind {mg,any} [--cycle {f64,f32}] [--batch NRHS] N [--record FILE]
       python tools/mg_profile.py summary OUT.txt DIR [DIR ...]      (each DIR holds a trace and the FILE of its solve)"""
import csv
import glob
import json
import os
import re
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def solve(args):
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    record = None
    if "--record" in args:
        i = args.index("--record")
        record = args[i + 1]
        del args[i:i + 2]
    i = args.index("--kind")
    kind = {"mg": isa.PRECOND_MG, "any": isa.PRECOND_MG_ANY}[args[i + 1]]
    del args[i:i + 2]
    cycle = "f64"
    if "--cycle" in args:
        i = args.index("--cycle")
        cycle = args[i + 1]
        del args[i:i + 2]
    nrhs = 0
    if "--batch" in args:
        i = args.index("--batch")
        nrhs = int(args[i + 1])
        del args[i:i + 2]
    n = int(args[0])
    s = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
    s.set_preconditioner(kind, {"f64": isa.CYCLE_F64, "f32": isa.CYCLE_F32}[cycle])
    p = isa.default_params(_capi.RULE_REL_2NORM)
    p.eps_rel, p.max_iterations = 1e-8, 1000
    if nrhs:
        import numpy as np
        p.use_true_solution = 0
        _, all_res = s._handle.solve_batch(p, np.random.default_rng(n).standard_normal((nrhs, s.size())))
        res = max(all_res, key=lambda r: r.iterations)
        res.converged = int(all(r.converged for r in all_res))
    else:
        res = s._handle.solve(p)
    out = {"n": n, "kind": ("MG_ANY" if kind == isa.PRECOND_MG_ANY else "MG") + (", fp32 V-cycle" if cycle == "f32" else "")
           + (f", one batch of {nrhs} right-hand sides" if nrhs else ""),
           "levels": list(isa.mg_hierarchy(n, kind)),
           "iterations": res.iterations, "converged": res.converged, "solve_seconds": res.solve_seconds}
    print(json.dumps(out))
    if record:
        os.makedirs(os.path.dirname(os.path.abspath(record)), exist_ok=True)
        with open(record, "w") as f:
            json.dump(out, f)
    return 0 if res.converged else 1


def kernel_times(d):
    dur = defaultdict(list)
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"k_mg(32|b)?_\w+(<[^>]*>)?", row["Kernel_Name"])
                if m:
                    dur[m.group(0)].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return dur


def summary(args):
    out_path, dirs = args[0], args[1:]
    lines = ["# device time of one REL_2NORM 1e-8 multigrid-preconditioned solve on one MI355X, per kernel",
             "# (rocprofv3 --kernel-trace; tools/mg_profile.py; us = microseconds, per it = per PCG iteration)"]
    for d in dirs:
        rec = json.load(open(glob.glob(os.path.join(d, "**", "solve.json"), recursive=True)[0]))
        dur = kernel_times(d)
        it = rec["iterations"]
        lines += ["", f"N = {rec['n']}, {rec['kind']}, levels {rec['levels']}, {it} iterations, converged {rec['converged']}",
                  f"  {'kernel':<32} {'launches':>8} {'total_us':>10} {'avg_us':>9} {'us_per_it':>10}"]
        total = 0.0
        for k, v in sorted(dur.items(), key=lambda kv: -sum(kv[1])):
            t = sum(v)
            total += t
            lines.append(f"  {k:<32} {len(v):>8} {t:>10.1f} {t / len(v):>9.2f} {t / it:>10.1f}")
        lines.append(f"  {'sum':<32} {sum(len(v) for v in dur.values()):>8} {total:>10.1f} {'':>9} {total / it:>10.1f}")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    cmd, rest = sys.argv[1], sys.argv[2:]
    sys.exit(solve(rest) if cmd == "solve" else summary(rest))
