"""Time to solution of the batched on-chip solves (mi355cg_solve_many) on one MI355X.

For every N, batch size nsys and both rules (REL_2NORM 1e-8, the MSG defaults without the exact solution): right-hand sides = the
handle's own times (1 + 0.1 * seeded standard-normal numbers), a different one per system.  Per row one warm-up and then five timed
rounds; in every round, one after the other on the same GPU,
  (a) one solve_many call of all nsys systems (host vectors in, host vectors out: wall time of the call);
  (b) the same nsys systems one after another by single solves of a SOLVE_ONCHIP handle of the same build (set_rhs; solve;
      solution -- the wall time of the three, summed over the batch);
and then per row
  (c) the CPU oracle on one core of the host solving the same nsys systems one after another: a warm-up and five timed passes where a
      pass takes under 2 s, one timed pass otherwise.
Nothing is scaled.  Reported: median / min / max wall ms per batch, us per system and us per system-iteration (total iterations).

       python tools/onchip_many_timing.py [--resources FILE] [--out FILE] [N ...]
                                                  (default 6 10 16 32 64 128; writes profiles/onchip_many_time_to_solution.txt)
       python tools/onchip_many_timing.py --compile-report FILE
                                                  (no GPU: compiles csrc/mi355cg.hip for the device with -Rpass-analysis=kernel-resource-usage
                                                   and writes registers, LDS and scratch of every k_onchip / k_onchip_many instantiation;
                                                   exit status 1 if one of them uses scratch; --resources FILE copies it into the timing file)"""
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "onchip_many_time_to_solution.txt")
SIZES = [6, 10, 16, 32, 64, 128]
BATCHES = [1, 16, 256, 4096]
TIMED = 5
C_REPEAT_BELOW_MS = 2000.0      # (c) is timed TIMED times where one pass over the batch takes less than this, otherwise once
RULES = ("REL_2NORM 1e-8", "MSG defaults")
sys.path.insert(0, ROOT)


def compile_report(path):
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
    lines = ["# k_onchip<E, MSG>, k_onchip_many<E, MSG> and k_onchip_many_init<WARM> as hipcc builds them for gfx950 (-Rpass-analysis=kernel-resource-usage,",
             "# the library's flags): E = unknowns per thread, MSG = the max-norm rule.  __launch_bounds__(512): 256 VGPRs per wave at most.  Scratch must be 0.",
             "# static_LDS_B: k_onchip declares the image of the largest grid; the batch kernels take theirs dynamically, onchip_many_lds_bytes(N) per workgroup.",
             f"# {'kernel':<28} {'VGPRs':>5} {'AGPRs':>5} {'SGPRs':>5} {'scratch_B_per_lane':>18} {'static_LDS_B':>12}"]
    for r in rows:
        m = re.search(r"(k_onchip(?:_many)?)ILi(\d+)ELb([01])E", r["name"]) or re.search(r"(k_onchip_many_init)()ILb([01])E", r["name"])
        args = ", ".join(a for a in (m.group(2), "true" if m.group(3) == "1" else "false") if a) if m else ""
        name = f"{m.group(1)}<{args}>" if m else r["name"]
        lines.append(f"  {name:<28} {r.get('VGPRs', '?'):>5} {r.get('AGPRs', '?'):>5} {r.get('TotalSGPRs', '?'):>5} {r.get('ScratchSize [bytes/lane]', '?'):>18} "
                     f"{r.get('LDS Size [bytes/block]', '?'):>12}")
    assert len(rows) >= 26, "the compiler's remarks do not list every k_onchip / k_onchip_many instantiation"
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if all(r.get("ScratchSize [bytes/lane]") == "0" for r in rows) else 1


if len(sys.argv) > 2 and sys.argv[1] == "--compile-report":
    sys.exit(compile_report(sys.argv[2]))

import iterative_solvers_amd as isa  # noqa: E402
from iterative_solvers_amd import _capi  # noqa: E402
from oracle.oracle import OracleGrid  # noqa: E402


def params(rule):
    p = isa.default_params(_capi.RULE_REL_2NORM if rule == RULES[0] else _capi.RULE_MSG_MAXNORM)
    p.use_true_solution = 0
    if rule == RULES[0]:
        p.eps_rel, p.max_iterations = 1e-8, 1_000_000
    return p


def oracle_pass_ms(og, rule, b):
    """wall ms of the CPU oracle solving every row of b once, one after another on one core; its total iterations"""
    its = 0
    t0 = time.perf_counter()
    for row in b:
        res = og.mf_solve(b=row, eps=1e-8, max_iterations=1_000_000) if rule == RULES[0] else og.msg_solve(b=row, true_solution=None)
        its += res.iterations
    return (time.perf_counter() - t0) * 1e3, its


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main(ns, resources, out_path):
    lines = ["# time to solution of batches of small systems on one MI355X (tools/onchip_many_timing.py): (a) mi355cg_solve_many, one workgroup per",
             "# system; (b) the same systems one after another by single SOLVE_ONCHIP solves of this build; (c) the CPU oracle on one core of the host.",
             "# Domain (1, 2, 1, 2), default sync_every, right-hand sides = the handle's own times (1 + 0.1 * seeded standard-normal numbers).",
             f"# per row: one warm-up, then {TIMED} timed rounds of (a) then (b) on the same GPU, every round over ALL nsys systems; then (c), one pass = all nsys",
             f"# systems one after another: a warm-up and {TIMED} timed passes where a pass takes under {C_REPEAT_BELOW_MS / 1e3:.0f} s, otherwise ONE timed pass (c_n = passes timed).",
             "# Nothing is scaled or extrapolated.  ms = wall time per batch, median (min .. max).",
             "# us_sys = median ms / nsys; us_sys_it = median ms / total iterations of the batch; wg_cu = resident workgroups per CU (occupancy query);",
             "# b/a, c/a = ratio of the medians (above 1: the batch is faster).",
             f"# {'N':>4} {'nsys':>5} {'rule':<15} {'it/sys':>7} {'wg_cu':>5} | {'a_ms med':>9} {'min':>9} {'max':>9} {'us_sys':>9} {'us_sys_it':>9} | "
             f"{'b_ms med':>10} {'min':>10} {'max':>10} {'us_sys':>9} | {'c_ms med':>10} {'min':>10} {'max':>10} {'c_n':>3} {'us_sys':>9} | {'b/a':>7} {'c/a':>7}"]
    print("\n".join(lines), flush=True)
    for n in ns:
        os.environ.pop("MI355CG_ONCHIP", None)
        many = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
        single = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
        single.set_solve_mode(isa.SOLVE_ONCHIP)
        own = many.get_rhs()
        og = OracleGrid(n, n)
        for nsys in (BATCHES[:-1] + [1024] if n >= 128 else BATCHES):             # at the cap a workgroup has a CU to itself: up to 1024
            rng = np.random.default_rng(1000 * n + nsys)
            b = own[None, :] * (1.0 + 0.1 * rng.standard_normal((nsys, own.size)))
            info = many.solve_many_info(nsys)
            for rule in RULES:
                p = params(rule)
                ta, tb, its = [], [], 0
                for k in range(TIMED + 1):                   # k = 0: the warm-up of both
                    t0 = time.perf_counter()
                    x, res = many._handle.solve_many(p, b)
                    t1 = time.perf_counter()
                    for s in range(nsys):
                        single._handle.set_rhs(b[s])
                        single._handle.solve(p)
                        xs = single._handle.solution()
                    t2 = time.perf_counter()
                    if k == 0:
                        assert all(r.converged == 1 for r in res), (n, nsys, rule)
                        assert np.array_equal(xs, x[nsys - 1]), (n, nsys, rule)          # the same bits (tests/test_gpu_onchip_many.py)
                        its = sum(r.iterations for r in res)
                    else:
                        ta.append((t1 - t0) * 1e3)
                        tb.append((t2 - t1) * 1e3)
                oracle_pass_ms(og, rule, b[:min(nsys, 2)])                                # warm-up
                tc = [oracle_pass_ms(og, rule, b)[0]]
                while len(tc) < TIMED and tc[0] < C_REPEAT_BELOW_MS:
                    tc.append(oracle_pass_ms(og, rule, b)[0])
                a, b_, c = stats(ta), stats(tb), stats(tc)
                line = (f"  {n:>4} {nsys:>5} {rule:<15} {its / nsys:>7.1f} {info['workgroups_per_cu']:>5} | {a[0]:>9.3f} {a[1]:>9.3f} {a[2]:>9.3f} {a[0] * 1e3 / nsys:>9.2f} "
                        f"{a[0] * 1e3 / its:>9.3f} | {b_[0]:>10.3f} {b_[1]:>10.3f} {b_[2]:>10.3f} {b_[0] * 1e3 / nsys:>9.2f} | {c[0]:>10.3f} {c[1]:>10.3f} {c[2]:>10.3f} {len(tc):>3} "
                        f"{c[0] * 1e3 / nsys:>9.2f} | {b_[0] / a[0]:>7.2f} {c[0] / a[0]:>7.2f}")
                lines.append(line)
                print(line, flush=True)
        many._handle.close()
        single._handle.close()
    if resources and os.path.exists(resources):
        lines.append("#")
        lines += open(resources).read().splitlines()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)
    return 0


if __name__ == "__main__":
    args = sys.argv[1:]
    resources, out_path = None, OUT
    for flag in ("--resources", "--out"):
        if flag in args:
            i = args.index(flag)
            val = args[i + 1]
            del args[i:i + 2]
            if flag == "--resources":
                resources = val
            else:
                out_path = val
    sys.exit(main([int(a) for a in args] or SIZES, resources, out_path))
