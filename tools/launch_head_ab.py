#!/usr/bin/env python3
"""A/B runs of bench.py for the launch head (profiles/launch_head_ab.txt): this build against the library of a built checkout of
the commit before it, loaded through MI355CG_LIB, alternating on one box.  Every run is a fresh process under its own time limit;
the first failure ends the job.
    python tools/launch_head_ab.py PARENT_LIB OUT [PAIRS]    PAIRS (default 4) pairs each of: N = 4096 at --steps 2000 --warmup 200 and
                                                             at --steps 20 --warmup 5, N = 1024 and N = 2048 at --steps 2000"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.abspath(sys.argv[1])
out = open(sys.argv[2], "a")
PAIRS = int(sys.argv[3]) if len(sys.argv) > 3 else 4


def say(s):
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


def bench(label, env, args, limit=150):
    e = dict(os.environ)
    e.update(env)
    t0 = time.time()
    cmd = [sys.executable, "bench.py", "--gpus", "1"] + args
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        say(f"{label}: FAILED rc={p.returncode}\n{p.stderr[-1500:]}")
        sys.exit(1)
    j = json.loads(p.stdout.strip().splitlines()[-1])
    say(f"{' '.join(args):44s} {label:22s} {j['value']:10.2f} it/s  ms/step {j['ms_per_step']:.5f}  loop-only ms/step {j['loop_only_ms_per_step']:.5f}  ({time.time() - t0:.0f} s)")
    return j["value"]


def pairs(args):
    a, b = [], []
    for _ in range(PAIRS):
        a.append(bench("parent (MI355CG_LIB)", {"MI355CG_LIB": PARENT}, args))
        b.append(bench("this build", {}, args))
    sa, sb = sorted(a), sorted(b)
    med = lambda v: v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])
    say(f"  -> {' '.join(args)}: parent min/median/max {sa[0]:.2f}/{med(sa):.2f}/{sa[-1]:.2f}  new min/median/max {sb[0]:.2f}/{med(sb):.2f}/{sb[-1]:.2f}  "
        f"median ratio {med(sb) / med(sa):.4f}  slowest new / fastest parent {sb[0] / sa[-1]:.4f}")


pairs(["--steps", "2000", "--warmup", "200"])
pairs(["--grid", "1024", "--steps", "2000"])
pairs(["--grid", "2048", "--steps", "2000"])
pairs(["--steps", "20", "--warmup", "5"])
say("done")
