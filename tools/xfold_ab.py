#!/usr/bin/env python3
"""A/B runs of bench.py for the deferred x fold (profiles/xfold_ab.txt): this build against the library of a built checkout of the
commit before it, loaded through MI355CG_LIB, alternating on one box.  Every run is a fresh process under its own time limit; the
first failure ends the job.
    python tools/xfold_ab.py PARENT_LIB n4096 OUT    4 pairs at --steps 2000 --warmup 200, 4 pairs at --steps 20 --warmup 5, then the
                                                     fold launch's shapes and cache policies, one run each
    python tools/xfold_ab.py PARENT_LIB nt OUT       parent / fused / plain / nontemporal / grid-stride, three rounds
    python tools/xfold_ab.py PARENT_LIB large OUT    N = 8192 and 16384, one pair each for MI355CG_XFOLD = 32 and 16"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.abspath(sys.argv[1])
out = open(sys.argv[3], "a")


def say(s):
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


def bench(label, env, grid, steps, warmup, limit=150):
    e = dict(os.environ)
    e.update(env)
    t0 = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "bench.py", "--gpus", "1", "--grid", str(grid), "--steps", str(steps), "--warmup", str(warmup)],
                       cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        say(f"{label}: FAILED rc={p.returncode}\n{p.stderr[-1500:]}")
        sys.exit(1)
    j = json.loads(p.stdout.strip().splitlines()[-1])
    say(f"N={grid:6d} K={steps:5d} {label:34s} {j['value']:10.2f} it/s  ms/step {j['ms_per_step']:.5f}  loop-only ms/step {j['loop_only_ms_per_step']:.5f}  "
        f"x_fold={j['config']['layout'].get('x_fold', '-')}  ({time.time() - t0:.0f} s)")
    return j["value"]


def pairs(grid, steps, warmup, n, new_env=None, new_label="this build (default)"):
    a, b = [], []
    for _ in range(n):
        a.append(bench("parent (MI355CG_LIB)", {"MI355CG_LIB": PARENT}, grid, steps, warmup))
        b.append(bench(new_label, new_env or {}, grid, steps, warmup))
    sa, sb = sorted(a), sorted(b)
    med = lambda v: v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
    say(f"  -> N={grid} K={steps} [{new_label}]: parent min/median/max {sa[0]:.2f}/{med(sa):.2f}/{sa[-1]:.2f}  new min/median/max {sb[0]:.2f}/{med(sb):.2f}/{sb[-1]:.2f}  "
        f"median ratio {med(sb) / med(sa):.4f}  slowest new / fastest parent {sb[0] / sa[-1]:.4f}")


plan = sys.argv[2]
if plan == "n4096":
    pairs(4096, 2000, 200, 4)
    pairs(4096, 20, 5, 4)
    say("-- k_fold_x shape and cache policy at N = 4096 (one run each)")
    for label, env in (("one-shot plain", {"MI355CG_XFOLD_NT": "0"}), ("one-shot nontemporal", {"MI355CG_XFOLD_NT": "1"}),
                       ("grid-stride 2048 plain", {"MI355CG_XFOLD_GRID": "2048", "MI355CG_XFOLD_NT": "0"}), ("grid-stride 2048 nontemporal", {"MI355CG_XFOLD_GRID": "2048", "MI355CG_XFOLD_NT": "1"}),
                       ("grid-stride 8192 plain", {"MI355CG_XFOLD_GRID": "8192", "MI355CG_XFOLD_NT": "0"}), ("R = 16 one-shot plain", {"MI355CG_XFOLD": "16", "MI355CG_XFOLD_NT": "0"}),
                       ("MI355CG_XFOLD=0 (fused, this build)", {"MI355CG_XFOLD": "0"})):
        bench(label, env, 4096, 2000, 200)
elif plan == "large":
    big = {"MI355CG_DEVICE_SETUP": "1"}          # b and u generated on the device: no host pass over 50 - 200 M unknowns
    for grid, steps, warmup in ((8192, 1000, 100), (16384, 400, 64)):
        for R in ("32", "16"):
            pe = dict(big, MI355CG_LIB=PARENT)
            a = bench("parent (MI355CG_LIB)", pe, grid, steps, warmup, 280)
            b = bench(f"this build MI355CG_XFOLD={R}", dict(big, MI355CG_XFOLD=R), grid, steps, warmup, 280)
            say(f"  -> N={grid} R={R}: ratio {b / a:.4f}")
if plan == "nt":
    for _ in range(3):
        bench("parent (MI355CG_LIB)", {"MI355CG_LIB": PARENT}, 4096, 2000, 200)
        bench("this build MI355CG_XFOLD=0 (fused)", {"MI355CG_XFOLD": "0"}, 4096, 2000, 200)
        bench("one-shot plain (MI355CG_XFOLD_NT=0)", {"MI355CG_XFOLD_NT": "0"}, 4096, 2000, 200)
        bench("one-shot nontemporal (default)", {}, 4096, 2000, 200)
        bench("grid-stride 2048 nontemporal", {"MI355CG_XFOLD_GRID": "2048"}, 4096, 2000, 200)
say("done")
