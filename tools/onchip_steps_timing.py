"""Time to solution of on-chip ensemble time stepping (mi355cg_time_steps_many) on one MI355X.

For every N, ensemble size nsys and shift factor f: nsys members take 100 steps of implicit Euler (theta = 1) for u_t = A u - g_s from
u0 = 0 with tau such that sigma = 1 / tau = |A_diag| * f, REL_2NORM 1e-8, g_s = the handle's right-hand side times (1 + 0.1 * seeded
standard-normal numbers).  Per row one warm-up and then five timed rounds; in every round, one after the other on the same GPU,
  (a) one time_steps_many call on device tensors (wall time of the call);
  (b) the best a caller can do without it: per step b_step = g - sigma u formed with torch on the device (one multiply, one subtract:
      the stepper's roundings) and one solve_many(b_step, x0 = u, sigma) call on device tensors -- the wall time of the 100 steps; its
      final u is compared with (a)'s;
and then per row, for nsys <= 256,
  (c) time_steps member by member on a SOLVE_ONCHIP handle (set_rhs; set_initial_guess; time_steps; solution -- the wall time of
      all members): a warm-up member, then five timed passes where a pass takes under 2 s, one timed pass otherwise.
Nothing is scaled.  Reported: median / min / max wall ms and us per member-step (median ms / (nsys * 100)).

       python tools/onchip_steps_timing.py [--resources FILE] [--out FILE] [N ...]
                                                  (default 10 32 128; writes profiles/onchip_steps_time_to_solution.txt)
       python tools/onchip_steps_timing.py --compile-report FILE [--csrc DIR] [--title TEXT]
                                                  (no GPU: compiles csrc/mi355cg.hip -- or DIR/mi355cg.hip, a checkout of another commit --
                                                   for the device with -Rpass-analysis=kernel-resource-usage and writes registers and scratch of
                                                   every on-chip kernel; exit status 1 if one of them uses scratch)"""
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "onchip_steps_time_to_solution.txt")
SIZES = [10, 32, 128]
ENSEMBLES = [1, 256, 4096]
FACTORS = [10.0, 0.03]
NSTEPS = 100
TIMED = 5
C_MOST = 256
C_REPEAT_BELOW_MS = 2000.0
sys.path.insert(0, ROOT)


def compile_report(path, csrc, title):
    from iterative_solvers_amd import build as b
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC", "-pthread")]
    csrc = csrc or b.CSRC
    cmd = [b._hipcc()] + flags + ["--cuda-device-only", "-c", "-Rpass-analysis=kernel-resource-usage", os.path.join(csrc, "mi355cg.hip"), "-o", os.devnull]
    txt = subprocess.run(cmd, cwd=csrc, check=True, capture_output=True, text=True).stderr
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
    lines = [f"# {title}: the on-chip kernels as hipcc builds them for gfx950 (-Rpass-analysis=kernel-resource-usage, the library's flags).",
             f"# {'kernel':<34} {'VGPRs':>5} {'AGPRs':>5} {'SGPRs':>5} {'scratch_B_per_lane':>18} {'waves_per_SIMD':>14}"]
    for r in rows:
        m = (re.search(r"(k_onchip(?:_many|_steps|_wave_newmark)?)ILi(\d+)ELb([01])E", r["name"]) or re.search(r"(k_onchip_many_init)()ILb([01])E", r["name"])
             or re.search(r"(k_onchip_wave_verlet)ILi(\d+)E()", r["name"]) or re.search(r"(k_onchip_steps_init|k_onchip_wave_newmark_init|k_onchip_wave_newmark_finish)()()", r["name"]))
        args = ", ".join(a for a in (m.group(2), {"1": "true", "0": "false"}.get(m.group(3), "")) if a) if m else ""
        name = (f"{m.group(1)}<{args}>" if args else m.group(1)) if m else r["name"]
        lines.append(f"  {name:<34} {r.get('VGPRs', '?'):>5} {r.get('AGPRs', '?'):>5} {r.get('TotalSGPRs', '?'):>5} {r.get('ScratchSize [bytes/lane]', '?'):>18} "
                     f"{r.get('Occupancy [waves/SIMD]', '?'):>14}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0 if all(r.get("ScratchSize [bytes/lane]") == "0" for r in rows) else 1


def option(args, flag):
    if flag not in args:
        return None
    i = args.index(flag)
    val = args[i + 1]
    del args[i:i + 2]
    return val


if len(sys.argv) > 2 and sys.argv[1] == "--compile-report":
    rest = sys.argv[3:]
    csrc_dir, title_text = option(rest, "--csrc"), option(rest, "--title")
    sys.exit(compile_report(sys.argv[2], csrc_dir, title_text or "this commit"))

import torch  # noqa: E402

import iterative_solvers_amd as isa  # noqa: E402
from iterative_solvers_amd import _capi  # noqa: E402


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main(ns, resources, out_path):
    lines = ["# time to solution of ensembles of small time steppers on one MI355X (tools/onchip_steps_timing.py): 100 steps of implicit Euler per member,",
             "# sigma = 1 / tau = |A_diag| * factor, REL_2NORM 1e-8, u0 = 0, g_s = the handle's right-hand side times (1 + 0.1 * seeded standard-normal numbers).",
             "# (a) mi355cg_time_steps_many on device tensors, the step loop inside the launch; (b) per step b_step = g - sigma u with torch on the device and one",
             "# solve_many(b_step, x0 = u, sigma) call on device tensors; (c) time_steps member by member on a SOLVE_ONCHIP handle (nsys <= 256).",
             f"# Domain (1, 2, 1, 2), default sync_every.  Per row: one warm-up, then {TIMED} timed rounds of (a) then (b) on the same GPU; then (c): a warm-up member and",
             f"# {TIMED} timed passes where a pass takes under {C_REPEAT_BELOW_MS / 1e3:.0f} s, otherwise ONE timed pass (c_n = passes timed).  Nothing is scaled or extrapolated.",
             "# ms = wall time of all members' 100 steps, median (min .. max); us_ms = median ms * 1000 / (nsys * 100), per member-step; it/step = CG iterations per",
             "# member-step of (a); b=a: the final states of (b) and (a) agree bit for bit (otherwise the largest |difference|); b/a, c/a = ratio of the medians",
             "# (above 1: the new call is faster).",
             f"# {'N':>4} {'nsys':>5} {'factor':>6} {'it/step':>7} | {'a_ms med':>9} {'min':>9} {'max':>9} {'us_ms':>8} | {'b_ms med':>10} {'min':>10} {'max':>10} {'us_ms':>8} {'b=a':>9} | "
             f"{'c_ms med':>10} {'min':>10} {'max':>10} {'c_n':>3} {'us_ms':>8} | {'b/a':>7} {'c/a':>7}"]
    print("\n".join(lines), flush=True)
    p = isa.default_params(_capi.RULE_REL_2NORM)
    p.use_true_solution, p.eps_rel, p.max_iterations = 0, 1e-8, 1_000_000
    for n in ns:
        os.environ.pop("MI355CG_ONCHIP", None)
        many = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
        single = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
        single.set_solve_mode(isa.SOLVE_ONCHIP)
        own = many.get_rhs()
        e0 = np.zeros(own.size)
        e0[0] = 1.0
        adiag = abs(float(many.apply(e0)[0]))
        for nsys in (ENSEMBLES[:-1] + [1024] if n >= 128 else ENSEMBLES):           # at the cap a workgroup has a CU to itself: up to 1024
            rng = np.random.default_rng(1000 * n + nsys)
            g = own[None, :] * (1.0 + 0.1 * rng.standard_normal((nsys, own.size)))
            gd = torch.from_numpy(g).cuda()
            u0d = torch.zeros_like(gd)
            for factor in FACTORS:
                tau = np.full(nsys, 1.0 / (adiag * factor))
                sigma = 1.0 / (1.0 * tau)                                          # the library's own form of it
                sd = torch.from_numpy(sigma).cuda()
                ta, tb, its, agree = [], [], 0, ""
                for k in range(TIMED + 1):                                         # k = 0: the warm-up of both
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ua, res, done, step_it = many._handle.time_steps_many(p, u0d, tau, 1.0, NSTEPS, g=gd)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    ub = u0d
                    for _ in range(NSTEPS):
                        b = torch.sub(gd, torch.mul(sd[:, None], ub))
                        ub, _res = many._handle.solve_many(p, b, x0=ub, sigma=sd)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if k == 0:
                        assert (done == NSTEPS).all() and all(r.converged == 1 for r in res), (n, nsys, factor)
                        its = int(step_it.sum())
                        diff = float((ua - ub).abs().max())
                        agree = "yes" if torch.equal(ua, ub) else f"{diff:.1e}"
                    else:
                        ta.append((t1 - t0) * 1e3)
                        tb.append((t2 - t1) * 1e3)
                tc = []
                if nsys <= C_MOST:
                    def one_pass(rows):
                        t0 = time.perf_counter()
                        for s in rows:
                            single._handle.set_rhs(g[s])
                            single._handle.set_initial_guess(e0 * 0.0)
                            single._handle.time_steps(p, float(tau[s]), 1.0, NSTEPS)
                            us = single._handle.solution()
                        return (time.perf_counter() - t0) * 1e3, us
                    one_pass([0])                                                   # warm-up
                    ms, us = one_pass(range(nsys))
                    assert np.array_equal(us, ua[nsys - 1].cpu().numpy()), (n, nsys, factor)     # the same bits (tests/test_gpu_steps_many.py)
                    tc.append(ms)
                    while len(tc) < TIMED and tc[0] < C_REPEAT_BELOW_MS:
                        tc.append(one_pass(range(nsys))[0])
                    single._handle.set_shift(0.0)
                a, b_ = stats(ta), stats(tb)
                per = 1e3 / (nsys * NSTEPS)
                line = (f"  {n:>4} {nsys:>5} {factor:>6g} {its / (nsys * NSTEPS):>7.2f} | {a[0]:>9.3f} {a[1]:>9.3f} {a[2]:>9.3f} {a[0] * per:>8.3f} | "
                        f"{b_[0]:>10.3f} {b_[1]:>10.3f} {b_[2]:>10.3f} {b_[0] * per:>8.3f} {agree:>9} | ")
                if tc:
                    c = stats(tc)
                    line += f"{c[0]:>10.3f} {c[1]:>10.3f} {c[2]:>10.3f} {len(tc):>3} {c[0] * per:>8.3f} | {b_[0] / a[0]:>7.2f} {c[0] / a[0]:>7.2f}"
                else:
                    line += f"{'-':>10} {'-':>10} {'-':>10} {0:>3} {'-':>8} | {b_[0] / a[0]:>7.2f} {'-':>7}"
                lines.append(line)
                print(line, flush=True)
        many._handle.close()
        single._handle.close()
    for path in resources:
        if os.path.exists(path):
            lines.append("#")
            lines += open(path).read().splitlines()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)
    return 0


if __name__ == "__main__":
    args = sys.argv[1:]
    resources = []
    while "--resources" in args:
        resources.append(option(args, "--resources"))
    out_path = option(args, "--out") or OUT
    sys.exit(main([int(a) for a in args] or SIZES, resources, out_path))
