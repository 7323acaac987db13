#!/usr/bin/env python3
"""Time to solution, plain CG against multigrid-preconditioned CG (mi355cg_set_preconditioner), on one GPU.

For every N and rule: one handle, the plain solve, then set_preconditioner(MG) (its set-up time is reported on its own) and the
preconditioned solve; each solve twice, the faster wall time reported.  Rules: REL_2NORM eps 1e-8 (no iteration cap in effect)
and the MSG rule with mi355cg_default_params (eps 1e-6, at most 10 000 iterations, the true solution in the error norm).
The true relative residual ||b - A x|| / ||b|| comes from mi355cg_get_true_residual.
--kind any: the plain solve, MG where the grid has a nested hierarchy, and MG_ANY (MI355CG_PRECOND_MG_ANY), each preconditioner
built afresh on the handle.
--cycle f32 (with --kind any): MG_ANY with the fp64 V-cycle against MG_ANY with the fp32 V-cycle (MI355CG_CYCLE_F32), one handle per
N, one warm-up solve per setting, then three timed solves of each setting alternating, the best of each.  --baseline-tree DIR adds the
same fp64-cycle solves by another checkout of the project (built, e.g. the commit before the option), whose package a child process
of the same job imports instead of this one, on the same GPU: the yardstick for what the option gains over the code before it.
Usage: python tools/mg_timing.py [N ...]      (default 256 1024 4096 8192; writes profiles/mg_time_to_solution.txt)
       python tools/mg_timing.py --kind any [N ...]   (default 100 258 1000 1002 4096 4098 10000;
                                                      writes profiles/mg_any_time_to_solution.txt)
       python tools/mg_timing.py --kind any --cycle f32 [--baseline-tree DIR] [N ...]
                                                     (default 100 1000 4096 4098 8192 10000;
                                                      writes profiles/mg_f32_time_to_solution.txt)
--batch: batched solves (mi355cg_solve_batch_device) against one solve per right-hand side, MG_ANY, fp64 cycle, REL_2NORM 1e-8, seeded
standard-normal right-hand sides.  Per N and nrhs: one warm-up of each path, then three repetitions alternating {nrhs single solves, one
batch}; reported are the best sum of the single solves' wall times (set_rhs / get_solution not timed) and the best wall time of the batch
call on vectors that are already in device memory.  --baseline-tree DIR adds the same measurement of another built checkout (the
commit before a change) in a child process of the same job: the yardstick.  Its single solves, and its batch call if it has one.
       python tools/mg_timing.py --batch [--baseline-tree DIR] [--nrhs 4,16] [--out FILE] [N ...]
                                                     (default 100 258 1000 2002 4096, nrhs 4 16 64, at N >= 4096 only 4;
                                                      writes profiles/mg_batch_time_to_solution.txt)
--smoother: the point smoother against the line smoother of the fp64 V-cycle (mi355cg_set_smoother, MI355CG_SMOOTHER_LINE_AUTO) on the
square and on stretched domains: MG_ANY, REL_2NORM 1e-8, one seeded standard-normal right-hand side per N.  Per N and domain: one
handle, one warm-up solve per smoother, then three timed solves of each alternating (set_smoother switches in place; the hierarchy's
set-up is not timed), the best wall time of each.  --baseline-tree DIR adds the same point-smoother solves of another built checkout
(the commit before the option) in child processes of the same job, one before and one after this build's solves: the yardstick.
--traces DIR adds the device time of one level-0 sweep of each kind from rocprofv3 kernel traces found under DIR, each of
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR/NAME -- python tools/mg_timing.py --smoother-solve N a b c d {jacobi,line}`:
the sweep that carries the (r, z) partials runs on level 0 only, so its kernel name tells level 0 from the coarser levels.
       python tools/mg_timing.py --smoother [--baseline-tree DIR] [--traces DIR] [--out FILE] [N ...]
                                                     (default 1024 4096; writes profiles/mg_line_time_to_solution.txt)"""
import json
import subprocess
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("MG_TIMING_TREE") or ROOT)     # --baseline-tree: the child imports that checkout's package
import iterative_solvers_amd as isa  # noqa: E402
from iterative_solvers_amd import _capi  # noqa: E402

OUT = {"mg": os.path.join(ROOT, "profiles", "mg_time_to_solution.txt"),
       "any": os.path.join(ROOT, "profiles", "mg_any_time_to_solution.txt")}
SIZES = {"mg": [256, 1024, 4096, 8192], "any": [100, 258, 1000, 1002, 4096, 4098, 10000]}
RULES = {"REL_2NORM 1e-8": _capi.RULE_REL_2NORM, "MSG defaults": _capi.RULE_MSG_MAXNORM}
OUT_F32 = os.path.join(ROOT, "profiles", "mg_f32_time_to_solution.txt")
SIZES_F32 = [100, 1000, 4096, 4098, 8192, 10000]
OUT_BATCH = os.path.join(ROOT, "profiles", "mg_batch_time_to_solution.txt")
SIZES_BATCH = [100, 258, 1000, 2002, 4096]


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


def best_of_three(h, settings, rule, b_norm):
    """settings: {name: callable that sets the preconditioner}.  One warm-up solve per setting, then three timed solves of each
    alternating; per setting the best wall time, its results and the true relative residual of the last solve."""
    best = {}
    for name, setp in settings.items():
        setp()
        h.solve(params(rule))
    for _ in range(3):
        for name, setp in settings.items():
            setp()
            t0 = time.perf_counter()
            res = h.solve(params(rule))
            wall = time.perf_counter() - t0
            rel = float(np.linalg.norm(h.true_residual()) / b_norm)
            if name not in best or wall < best[name][0]:
                best[name] = (wall, res.iterations, res.stop_reason, res.converged, res.solve_seconds, rel)
    return best


def baseline_worker(ns):
    """Child process of --baseline-tree: the package is the other checkout's, which may only have mi355cg_set_preconditioner.  Prints one
    JSON line: {N: {rule: [wall, iterations, stop, converged, solve_seconds, true_rel]}}."""
    lib = _capi.load()
    out = {}
    for n in ns:
        s = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
        h = s._handle
        b_norm = np.linalg.norm(s.get_rhs())
        setp = lambda: _capi.check(lib.mi355cg_set_preconditioner(h._h, isa.PRECOND_MG_ANY))  # noqa: E731
        out[n] = {name: best_of_three(h, {"base": setp}, rule, b_norm)["base"] for name, rule in RULES.items()}
        h.close()
    print("BASELINE " + json.dumps(out), flush=True)


def main_f32(ns, baseline_tree):
    base = None
    if baseline_tree:
        env = dict(os.environ, MG_TIMING_TREE=os.path.abspath(baseline_tree))
        txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--baseline-worker"] + [str(n) for n in ns], env=env, check=True,
                             capture_output=True, text=True, timeout=900).stdout
        base = json.loads([l for l in txt.splitlines() if l.startswith("BASELINE ")][-1][len("BASELINE "):])
    lines = ["# time to solution on one MI355X: MG_ANY-preconditioned CG with the fp64 V-cycle against the fp32 V-cycle "
             "(MI355CG_CYCLE_F32; tools/mg_timing.py --kind any --cycle f32)",
             "# one warm-up solve per setting, then three timed solves of each alternating on one handle; wall = best host wall time of "
             "mi355cg_solve; true_rel = ||b - A x|| / ||b||",
             "# f64 = the fp64 cycle of this build, f32 = the fp32 cycle"
             + (", base = the fp64 cycle of the --baseline-tree checkout (the commit before the option) in a child process of the same job"
                if base else ""),
             "# ratio = wall / wall of " + ("base" if base else "f64"),
             f"# {'N':>5} {'rule':<15} {'cycle':<5} {'iters':>5} {'stop':>4} {'conv':>4} {'wall_s':>9} {'solve_s':>9} {'true_rel':>9} {'ratio':>6}"]
    print("\n".join(lines), flush=True)
    for n in ns:
        s = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
        h = s._handle
        b_norm = np.linalg.norm(s.get_rhs())
        settings = {"f64": lambda: h.set_preconditioner(isa.PRECOND_MG_ANY, isa.CYCLE_F64),
                    "f32": lambda: h.set_preconditioner(isa.PRECOND_MG_ANY, isa.CYCLE_F32)}
        for name, rule in RULES.items():
            rows = dict(best_of_three(h, settings, rule, b_norm))
            if base:
                rows = {"base": tuple(base[str(n)][name]), **rows}
            ref_wall = rows["base" if base else "f64"][0]
            for cyc, (w, it, stop, conv, ss, rel) in rows.items():
                line = f"  {n:>5} {name:<15} {cyc:<5} {it:>5} {stop:>4} {conv:>4} {w:>9.5f} {ss:>9.5f} {rel:>9.2e} {w / ref_wall:>6.3f}"
                lines.append(line)
                print(line, flush=True)
        h.close()
    with open(OUT_F32, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", OUT_F32)


# ---- --smoother -------------------------------------------------------------------------------------------------------------------
OUT_LINE = os.path.join(ROOT, "profiles", "mg_line_time_to_solution.txt")
SIZES_LINE = [1024, 4096]
DOMAINS_LINE = [(1.0, 2.0, 1.0, 2.0), (0.0, 3.0, 0.0, 1.0), (0.0, 10.0, 0.0, 1.0), (0.0, 1.0, 0.0, 10.0), (0.0, 32.0, 0.0, 1.0)]


def dom_name(dom):
    return "(" + ",".join(f"{v:g}" for v in dom) + ")"


def line_system(n, dom):
    """the handle of one (N, domain) with MG_ANY set and the seeded standard-normal right-hand side in place"""
    s = isa.MatrixFreeSystem(n, n, *dom)
    s.set_preconditioner(isa.PRECOND_MG_ANY)
    b = np.random.default_rng(n).standard_normal(s.size())
    s._handle.set_rhs(b)
    return s, float(np.linalg.norm(b))


def line_params():
    p = params(_capi.RULE_REL_2NORM)
    p.use_true_solution = 0
    return p


def line_best_of_three(h, settings, b_norm):
    """best_of_three without the error norm: the right-hand side has no known solution"""
    best = {}
    for name, setp in settings.items():
        setp()
        h.solve(line_params())
    for _ in range(3):
        for name, setp in settings.items():
            setp()
            t0 = time.perf_counter()
            res = h.solve(line_params())
            wall = time.perf_counter() - t0
            rel = float(np.linalg.norm(h.true_residual()) / b_norm)
            if name not in best or wall < best[name][0]:
                best[name] = (wall, res.iterations, res.stop_reason, res.converged, res.solve_seconds, rel)
    return best


def smoother_baseline_worker(ns):
    """Child process of --smoother --baseline-tree: the other checkout's package, which has the point smoother only.  Prints one JSON
    line: {N: {domain: [wall, iterations, stop, converged, solve_seconds, true_rel]}}."""
    out = {}
    for n in ns:
        out[n] = {}
        for dom in DOMAINS_LINE:
            s, b_norm = line_system(n, dom)
            out[n][dom_name(dom)] = line_best_of_three(s._handle, {"base": lambda: None}, b_norm)["base"]
            s._handle.close()
    print("BASELINE " + json.dumps(out), flush=True)


def smoother_solve(args):
    """one converged solve for a kernel trace: N a b c d {jacobi,line}"""
    n, dom, which = int(args[0]), tuple(float(v) for v in args[1:5]), args[5]
    s, _ = line_system(n, dom)
    s.set_smoother(isa.SMOOTHER_LINE_AUTO if which == "line" else isa.SMOOTHER_JACOBI)
    res = s._handle.solve(line_params())
    print(json.dumps({"n": n, "domain": dom_name(dom), "smoother": which, "direction": s.smoother_info()[1],
                      "iterations": res.iterations, "converged": res.converged}))
    return 0 if res.converged else 1


def sweep_times(traces):
    """{trace name: {kernel: (launches, average us)}} of the level-0 sweeps with the (r, z) partials and of all sweeps by kernel name"""
    import csv
    import glob
    import re
    out = {}
    for d in sorted(glob.glob(os.path.join(traces, "*"))):
        dur = {}
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            with open(f, newline="") as fh:
                for row in csv.DictReader(fh):
                    m = re.search(r"k_mg_(smooth|line)<[^>]*>", row["Kernel_Name"])
                    if m:
                        dur.setdefault(m.group(0), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
        if dur:
            out[os.path.basename(d)] = {k: (len(v), sum(v) / len(v)) for k, v in dur.items()}
    return out


def main_smoother(ns, baseline_tree, traces, out_path):
    def base_pass():
        env = dict(os.environ, MG_TIMING_TREE=os.path.abspath(baseline_tree))
        txt = subprocess.run([sys.executable, os.path.abspath(__file__), "--smoother-baseline-worker"] + [str(n) for n in ns], env=env,
                             check=True, capture_output=True, text=True, timeout=900).stdout
        return json.loads([l for l in txt.splitlines() if l.startswith("BASELINE ")][-1][len("BASELINE "):])
    lines = ["# time to solution on one MI355X: MG_ANY-preconditioned CG with damped point Jacobi against damped line Jacobi "
             "(MI355CG_SMOOTHER_LINE_AUTO) in the fp64 V-cycle (tools/mg_timing.py --smoother)",
             "# REL_2NORM 1e-8, b = numpy.random.default_rng(N).standard_normal(size); one handle per (N, domain), the hierarchy's set-up not "
             "timed; one warm-up solve per smoother, then three timed solves of each alternating; wall = best host wall time of mi355cg_solve",
             "# jacobi, line = this build; dir = the direction LINE_AUTO took (1 x, 2 y); true_rel = ||b - A x|| / ||b||",
             "# base1, base2 = the point smoother of the --baseline-tree checkout (the commit before the option) in child processes of the same "
             "job, one before and one after this build's solves" if baseline_tree else "# no --baseline-tree: the parent commit not measured",
             "# ratio = wall / the better base wall" if baseline_tree else "# ratio = wall / wall of jacobi",
             f"# {'N':>5} {'domain':<12} {'smoother':<8} {'dir':>3} {'iters':>5} {'conv':>4} {'wall_ms':>9} {'solve_ms':>9} {'ms_per_it':>9} {'true_rel':>9} {'ratio':>6}"]
    print("\n".join(lines), flush=True)
    base1 = base_pass() if baseline_tree else None
    rows = []
    for n in ns:
        for dom in DOMAINS_LINE:
            s, b_norm = line_system(n, dom)
            settings = {"jacobi": lambda: s.set_smoother(isa.SMOOTHER_JACOBI), "line": lambda: s.set_smoother(isa.SMOOTHER_LINE_AUTO)}
            best = line_best_of_three(s._handle, settings, b_norm)
            s.set_smoother(isa.SMOOTHER_LINE_AUTO)
            rows.append((n, dom, best, s.smoother_info()[1]))
            s._handle.close()
    base2 = base_pass() if baseline_tree else None
    for n, dom, best, direction in rows:
        named = {}
        if baseline_tree:
            named["base1"], named["base2"] = tuple(base1[str(n)][dom_name(dom)]), tuple(base2[str(n)][dom_name(dom)])
        named.update(best)
        ref_wall = min(named["base1"][0], named["base2"][0]) if baseline_tree else named["jacobi"][0]
        for name, (w, it, stop, conv, ss, rel) in named.items():
            line = (f"  {n:>5} {dom_name(dom):<12} {name:<8} {direction if name == 'line' else 0:>3} {it:>5} {conv:>4} {w * 1e3:>9.3f} {ss * 1e3:>9.3f} "
                    f"{w * 1e3 / max(it, 1):>9.3f} {rel:>9.2e} {w / ref_wall:>6.3f}")
            lines.append(line)
            print(line, flush=True)
    if traces:
        first = len(lines)
        lines += ["#", "# device time of the sweeps of one converged solve (rocprofv3 --kernel-trace of tools/mg_timing.py --smoother-solve): the sweep with",
                  "# the (r, z) partials, <.., false, true>, runs on level 0 only -- one level-0 sweep; the other names average over all levels",
                  f"# {'trace':<28} {'kernel':<34} {'launches':>8} {'avg_us':>9}"]
        for name, ks in sweep_times(traces).items():
            for k, (cnt, avg) in sorted(ks.items()):
                lines.append(f"  {name:<28} {k:<34} {cnt:>8} {avg:>9.2f}")
        print("\n".join(lines[first:]), flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


NRHS = None                                          # --nrhs: these counts at every N


def batch_counts(n):
    return NRHS or ([4] if n >= 4096 else [4, 16, 64])


def batch_rhs(n, size, nrhs):
    return np.random.default_rng(1000 * n + nrhs).standard_normal((nrhs, size))


def batch_params():
    p = params(_capi.RULE_REL_2NORM)
    p.use_true_solution = 0
    return p


def sequential_solves(h, rhs, p):
    """sum of the wall times of mi355cg_solve over the right-hand sides, and the iteration counts"""
    total, its = 0.0, []
    for v in rhs:
        h.set_rhs(v)
        t0 = time.perf_counter()
        res = h.solve(p)
        total += time.perf_counter() - t0
        its.append(res.iterations)
    return total, its


def batch_best_of_three(h, rhs, with_batch=True):
    """One warm-up of each path, then three repetitions alternating {the single solves, one batch on device vectors}: the best sum
    of the single solves' wall times, the best wall time of the batch call (None without one) and the iteration counts."""
    import torch
    p = batch_params()
    dev = torch.from_numpy(rhs).cuda() if with_batch else None
    sequential_solves(h, rhs, p)
    if with_batch:
        h.solve_batch(p, dev)
    seq, bat, its = [], [], None
    for _ in range(3):
        t, its = sequential_solves(h, rhs, p)
        seq.append(t)
        if with_batch:
            t0 = time.perf_counter()
            _, res = h.solve_batch(p, dev)
            bat.append(time.perf_counter() - t0)
            assert [r.iterations for r in res] == its
    if with_batch:
        del dev
        h.batch_release()
    return min(seq), (min(bat) if with_batch else None), its


def batch_baseline_worker(ns):
    """Child process of --batch --baseline-tree: the other checkout's package, which may have no batched solve.  Prints one JSON line:
    {N: {nrhs: [best sum of wall times, best wall time of the batch call or null]}}."""
    out = {}
    for n in ns:
        s = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
        s.set_preconditioner(isa.PRECOND_MG_ANY)
        h = s._handle
        out[n] = {nrhs: batch_best_of_three(h, batch_rhs(n, s.size(), nrhs), hasattr(h, "solve_batch"))[:2] for nrhs in batch_counts(n)}
        h.close()
    print("BASELINE " + json.dumps(out), flush=True)


def main_batch(ns, baseline_tree, out_path):
    base = None
    if baseline_tree:
        env = dict(os.environ, MG_TIMING_TREE=os.path.abspath(baseline_tree))
        cmd = [sys.executable, os.path.abspath(__file__), "--batch-baseline-worker"] + (["--nrhs", ",".join(map(str, NRHS))] if NRHS else [])
        txt = subprocess.run(cmd + [str(n) for n in ns], env=env, check=True, capture_output=True, text=True, timeout=900).stdout
        base = json.loads([l for l in txt.splitlines() if l.startswith("BASELINE ")][-1][len("BASELINE "):])
    lines = ["# time to solution of nrhs right-hand sides on one MI355X: one batched solve (mi355cg_solve_batch_device) against nrhs single "
             "solves (tools/mg_timing.py --batch)",
             "# MG_ANY, fp64 cycle, REL_2NORM 1e-8, seeded standard-normal right-hand sides; one warm-up of each path, then three "
             "repetitions alternating, the best of each",
             "# seq = sum of the wall times of mi355cg_solve (set_rhs / get_solution not timed); batch = wall time of the batch call, "
             "vectors already in device memory",
             "# base_seq, base_batch = seq and batch of the --baseline-tree checkout (the commit before the change; '-': it has no batched "
             "solve) in a child process of the same job"
             if base else "# no --baseline-tree: base_seq and base_batch not measured",
             f"# {'N':>5} {'nrhs':>4} {'iters':>7} {'base_seq_ms':>11} {'seq_ms':>9} {'batch_ms':>9} {'batch/base':>10} {'batch/seq':>9} {'seq/base':>8} "
             f"{'base_batch_ms':>13} {'batch/base_batch':>16}"]
    print("\n".join(lines), flush=True)
    num = lambda v, w, scale=1.0, prec=3: f"{v * scale:>{w}.{prec}f}" if v is not None else f"{'-':>{w}}"      # noqa: E731
    for n in ns:
        s = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
        s.set_preconditioner(isa.PRECOND_MG_ANY)
        for nrhs in batch_counts(n):
            seq, bat, its = batch_best_of_three(s._handle, batch_rhs(n, s.size(), nrhs))
            b, bb = base[str(n)][str(nrhs)] if base else (None, None)
            line = (f"  {n:>5} {nrhs:>4} {f'{min(its)}..{max(its)}':>7} {num(b, 11, 1e3)} {seq * 1e3:>9.3f} {bat * 1e3:>9.3f} "
                    f"{num(b and bat / b, 10)} {bat / seq:>9.3f} {num(b and seq / b, 8)} {num(bb, 13, 1e3)} {num(bb and bat / bb, 16)}")
            lines.append(line)
            print(line, flush=True)
        s._handle.close()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    args = sys.argv[1:]
    if "--nrhs" in args:
        i = args.index("--nrhs")
        NRHS = [int(v) for v in args[i + 1].split(",")]
        del args[i:i + 2]
    if args and args[0] == "--baseline-worker":
        baseline_worker([int(a) for a in args[1:]])
        sys.exit(0)
    if args and args[0] == "--batch-baseline-worker":
        batch_baseline_worker([int(a) for a in args[1:]])
        sys.exit(0)
    if args and args[0] == "--smoother-baseline-worker":
        smoother_baseline_worker([int(a) for a in args[1:]])
        sys.exit(0)
    if args and args[0] == "--smoother-solve":
        sys.exit(smoother_solve(args[1:]))
    kind = "mg"
    cycle, baseline_tree, out_path = "f64", None, None
    if "--out" in args:
        i = args.index("--out")
        out_path = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    smoother = "--smoother" in args
    if smoother:
        args.remove("--smoother")
    traces = None
    if "--traces" in args:
        i = args.index("--traces")
        traces = args[i + 1]
        del args[i:i + 2]
    batch = "--batch" in args
    if batch:
        args.remove("--batch")
    if "--cycle" in args:
        i = args.index("--cycle")
        cycle = args[i + 1]
        del args[i:i + 2]
        if cycle not in ("f64", "f32"):
            sys.exit("--cycle must be f64 or f32")
    if "--baseline-tree" in args:
        i = args.index("--baseline-tree")
        baseline_tree = args[i + 1]
        del args[i:i + 2]
    if "--kind" in args:
        i = args.index("--kind")
        kind = args[i + 1]
        del args[i:i + 2]
        if kind not in OUT:
            sys.exit(f"--kind must be one of {sorted(OUT)}")
    if smoother:
        main_smoother([int(a) for a in args] or SIZES_LINE, baseline_tree, traces, out_path or OUT_LINE)
    elif batch:
        main_batch([int(a) for a in args] or SIZES_BATCH, baseline_tree, out_path or OUT_BATCH)
    elif cycle == "f32":
        if kind != "any":
            sys.exit("--cycle f32 goes with --kind any")
        main_f32([int(a) for a in args] or SIZES_F32, baseline_tree)
    else:
        main([int(a) for a in args] or SIZES[kind], kind)
