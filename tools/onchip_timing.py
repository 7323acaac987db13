"""Time to solution of the on-chip solve mode against the two-launch path of the commit before it, on one MI355X.

For every N and both rules (REL_2NORM 1e-8, the MSG defaults): one warm-up solve and five timed solves of the on-chip mode in this
process, ALTERNATING solve by solve with the same solve on the --baseline-tree checkout (a built checkout of the parent commit), which
runs in a child process of this job that imports that checkout's package.  Per solve: mi355cg_results.loop_seconds / iterations (the
device time between the two events around the iteration loop) and solve_seconds (host wall time of mi355cg_solve).  The CPU oracle's
one-core time per iteration on the same host is measured once per row.

Acceptance (printed per row as `apart`): the SLOWEST on-chip loop time per iteration of the five is below the FASTEST of the parent's.

       python tools/onchip_timing.py [--baseline-tree DIR] [--resources FILE] [--out FILE] [N ...]
                                                  (default 6 10 16 32 64 128; writes profiles/onchip_time_to_solution.txt)
       python tools/onchip_timing.py --compile-report FILE
                                                  (no GPU: compiles csrc/mi355cg.hip for the device with -Rpass-analysis=kernel-resource-usage
                                                   and writes the registers, LDS and scratch of every k_onchip instantiation; --resources
                                                   FILE copies that report into the timing file)"""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "onchip_time_to_solution.txt")
SIZES = [6, 10, 16, 32, 64, 128]
TIMED = 5
RULES = ("REL_2NORM 1e-8", "MSG defaults")


def compile_report(path):
    sys.path.insert(0, ROOT)
    from iterative_solvers_amd import build as b
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC", "-pthread")]
    cmd = [b._hipcc()] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", os.path.join(b.CSRC, "mi355cg.hip"), "-o", os.devnull]
    txt = subprocess.run(cmd, cwd=b.CSRC, check=True, capture_output=True, text=True).stderr
    rows, cur = [], None
    for ln in txt.splitlines():
        m = re.search(r"remark: +(.*?) \[-Rpass-analysis", ln)
        if not m:
            continue
        key, _, val = m.group(1).strip().partition(":")
        if key == "Function Name":
            cur = {"name": val.strip()} if "k_onchip" in val else None
            if cur:
                rows.append(cur)
        elif cur is not None:
            cur[key.strip()] = val.strip()
    lines = ["# k_onchip<E, MSG> as hipcc builds it for gfx950 (-Rpass-analysis=kernel-resource-usage, the library's flags): E = unknowns per thread,",
             "# MSG = the max-norm rule (u in registers).  __launch_bounds__(512): two waves per SIMD, 256 VGPRs per wave.  Scratch must be 0.",
             f"# {'kernel':<26} {'VGPRs':>5} {'AGPRs':>5} {'SGPRs':>5} {'scratch_B_per_lane':>18} {'LDS_B':>7} {'waves_per_SIMD':>14}"]
    for r in rows:
        m = re.search(r"k_onchipILi(\d+)ELb([01])E", r["name"])
        name = f"k_onchip<{m.group(1)}, {'true' if m.group(2) == '1' else 'false'}>" if m else r["name"]
        lines.append(f"  {name:<26} {r.get('VGPRs', '?'):>5} {r.get('AGPRs', '?'):>5} {r.get('TotalSGPRs', '?'):>5} {r.get('ScratchSize [bytes/lane]', '?'):>18} "
                     f"{r.get('LDS Size [bytes/block]', '?'):>7} {r.get('Occupancy [waves/SIMD]', '?'):>14}")
    assert rows, "no k_onchip kernel in the compiler's remarks"
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if all(r.get("ScratchSize [bytes/lane]") == "0" for r in rows) else 1


if len(sys.argv) > 2 and sys.argv[1] == "--compile-report":
    sys.exit(compile_report(sys.argv[2]))

sys.path.insert(0, os.environ.get("ONCHIP_TIMING_TREE") or ROOT)     # --baseline-tree: the child imports that checkout's package
import iterative_solvers_amd as isa  # noqa: E402
from iterative_solvers_amd import _capi  # noqa: E402


def params(rule):
    p = isa.default_params(_capi.RULE_REL_2NORM if rule == RULES[0] else _capi.RULE_MSG_MAXNORM)
    if rule == RULES[0]:
        p.eps_rel, p.max_iterations = 1e-8, 1_000_000
    return p


class Solves:
    """The handles of one process, one per N; solve(n, rule) -> [iterations, converged, loop_seconds, solve_seconds, on-chip launches]."""
    def __init__(self, onchip):
        self.onchip, self.sys = onchip, {}

    def solve(self, n, rule):
        if n not in self.sys:
            os.environ.pop("MI355CG_ONCHIP", None)
            self.sys[n] = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
            if self.onchip:
                self.sys[n].set_solve_mode(isa.SOLVE_ONCHIP)
        s = self.sys[n]
        res = s._handle.solve(params(rule))
        launches = s.solve_mode_info()["onchip_launches"] if self.onchip else 0
        return [res.iterations, res.converged, res.loop_seconds, res.solve_seconds, launches]


def baseline_worker():
    """Child process of --baseline-tree: the other checkout's package (no solve modes there).  One line in ("N rule-index"), one JSON line out."""
    solves = Solves(False)
    print("READY", flush=True)
    for ln in sys.stdin:
        f = ln.split()
        if not f or f[0] == "quit":
            break
        print("R " + json.dumps(solves.solve(int(f[0]), RULES[int(f[1])])), flush=True)


def oracle_us_per_iteration(n, rule):
    sys.path.insert(0, ROOT)
    from oracle.oracle import OracleGrid
    og = OracleGrid(n, n)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        res = og.mf_solve(eps=1e-8, max_iterations=1_000_000) if rule == RULES[0] else og.msg_solve(eps_exact_error=1e-6)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best / max(res.iterations, 1) * 1e6, res.iterations


def _cap():
    """the largest N the mode takes"""
    n = 6
    while True:
        try:
            isa.onchip_plan(n + 2)
        except ValueError:
            return n
        n += 2


def main(ns, baseline_tree, resources, out_path):
    child = None
    if baseline_tree:
        env = dict(os.environ, ONCHIP_TIMING_TREE=os.path.abspath(baseline_tree))
        env.pop("MI355CG_ONCHIP", None)
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--baseline-worker"], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert child.stdout.readline().strip() == "READY"

    def base_solve(n, ri):
        child.stdin.write(f"{n} {ri}\n")
        child.stdin.flush()
        ln = child.stdout.readline()
        assert ln.startswith("R "), ln
        return json.loads(ln[2:])

    lines = ["# time to solution on one MI355X: the on-chip solve mode (one launch of one workgroup per chunk of iterations) against the two launches",
             "# per iteration of the parent commit (tools/onchip_timing.py).  Domain (1, 2, 1, 2), default sync_every; one handle per N and process.",
             f"# per row: one warm-up solve, then {TIMED} timed solves, the on-chip solve of this build and the parent commit's solve (a child process of the",
             "# same job on the same GPU) taking turns solve by solve" if baseline_tree else "# no --baseline-tree: the parent commit not measured",
             "# us_it = mi355cg_results.loop_seconds / iterations, min / median / max of the timed solves; solve_ms = best solve_seconds (host wall time)",
             "# cpu_us_it = the CPU oracle on one core of the same host (best of 3 solves) / its iterations; base/on = ratio of the median us_it;",
             "# cpu/on = cpu_us_it / median on-chip us_it (below 1: one CPU core is faster); apart = the slowest on-chip us_it is below the fastest parent us_it",
             f"# {'N':>4} {'rule':<15} {'iters':>5} {'launches':>8} | {'on_us_it min':>12} {'med':>8} {'max':>8} {'solve_ms':>8} | {'base_us_it min':>14} {'med':>8} {'max':>8} {'solve_ms':>8} | "
             f"{'cpu_us_it':>9} | {'base/on':>7} {'cpu/on':>7} {'apart':>5}"]
    print("\n".join(lines), flush=True)
    mine = Solves(True)
    ns = [n for n in ns if n <= _cap()]                  # "or up to the cap"
    all_apart = True
    for n in ns:
        for ri, rule in enumerate(RULES):
            on, base = [], []
            for k in range(TIMED + 1):                       # k = 0: the warm-up of both
                a = mine.solve(n, rule)
                b = base_solve(n, ri) if child else None
                if k:
                    on.append(a)
                    if b:
                        base.append(b)
            assert all(r[1] == 1 and r[4] > 0 for r in on), on
            assert not base or all(r[0] == on[0][0] and r[1] == 1 for r in base), (on, base)      # the same iteration count (the bits: tests/test_gpu_onchip.py)
            its = on[0][0]
            t_on = sorted(r[2] / its * 1e6 for r in on)
            t_base = sorted(r[2] / its * 1e6 for r in base) if base else None
            cpu, cpu_its = oracle_us_per_iteration(n, rule)
            apart = t_on[-1] < t_base[0] if t_base else None
            all_apart = all_apart and apart is not False
            line = (f"  {n:>4} {rule:<15} {its:>5} {on[0][4]:>8} | {t_on[0]:>12.2f} {t_on[TIMED // 2]:>8.2f} {t_on[-1]:>8.2f} {min(r[3] for r in on) * 1e3:>8.3f} | "
                    + (f"{t_base[0]:>14.2f} {t_base[TIMED // 2]:>8.2f} {t_base[-1]:>8.2f} {min(r[3] for r in base) * 1e3:>8.3f} | " if t_base else f"{'-':>14} {'-':>8} {'-':>8} {'-':>8} | ")
                    + f"{cpu:>9.2f} | " + (f"{t_base[TIMED // 2] / t_on[TIMED // 2]:>7.2f} " if t_base else f"{'-':>7} ")
                    + f"{cpu / t_on[TIMED // 2]:>7.2f} {('yes' if apart else 'NO') if apart is not None else '-':>5}")
            lines.append(line)
            print(line, flush=True)
    if child:
        child.stdin.write("quit\n")
        child.stdin.flush()
        child.wait(timeout=60)
        lines.append(f"# no overlap of the spreads at every row: {'yes' if all_apart else 'NO'}")
        print(lines[-1], flush=True)
    if resources and os.path.exists(resources):
        lines.append("#")
        lines += open(resources).read().splitlines()
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)
    return 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--baseline-worker":
        baseline_worker()
        sys.exit(0)
    baseline_tree = resources = None
    out_path = OUT
    for flag in ("--baseline-tree", "--resources", "--out"):
        if flag in args:
            i = args.index(flag)
            val = args[i + 1]
            del args[i:i + 2]
            if flag == "--baseline-tree":
                baseline_tree = val
            elif flag == "--resources":
                resources = val
            else:
                out_path = val
    sys.exit(main([int(a) for a in args] or SIZES, baseline_tree, resources, out_path))
