#!/usr/bin/env python3
"""A/B runs of bench.py for the launch boundary (profiles/launch_boundary_ab.txt): builds of the same ABI, loaded through
MI355CG_LIB, taking turns on one box.  Every run is a fresh process under its own time limit; the first failure ends the job.
    python tools/launch_boundary_ab.py OUT ROUNDS CASES LABEL=LIB [LABEL=LIB ...]
The first LABEL is the baseline of the ratios (the parent commit's library); LIB "-" is this tree's own build.  CASES:
    full     N = 4096 at --steps 2000 --warmup 200 and at --steps 20 --warmup 5; N = 1024, 2048, 8192 at --steps 2000; N = 16384 at --steps 400
    sweep    N = 4096 at --steps 2000 --warmup 200; N = 8192 at --steps 2000; N = 16384 at --steps 400   (many builds, e.g. store policies)
    n4096    N = 4096 at --steps 2000 --warmup 200 only
    n16384   N = 16384 at --steps 400 only"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out = open(sys.argv[1], "a")
ROUNDS = int(sys.argv[2])
BUILDS = [(a.split("=", 1)[0], a.split("=", 1)[1]) for a in sys.argv[4:]]
N4096 = (4096, 2000, 200)
CASES = {"full": [N4096, (1024, 2000, 200), (2048, 2000, 200), (8192, 2000, 200), (16384, 400, 64), (4096, 20, 5)],
         "sweep": [N4096, (8192, 2000, 200), (16384, 400, 64)], "n4096": [N4096], "n16384": [(16384, 400, 64)]}[sys.argv[3]]


def say(s):
    print(s, flush=True)
    out.write(s + "\n")
    out.flush()


def bench(label, lib, grid, steps, warmup):
    e = dict(os.environ)
    if lib != "-":
        e["MI355CG_LIB"] = os.path.abspath(lib)
    if grid >= 8192:
        e["MI355CG_DEVICE_SETUP"] = "1"          # b and u generated on the device: no host pass over 50 - 200 M unknowns
    t0 = time.time()
    p = subprocess.run(["timeout", "-k", "10", "280", sys.executable, "bench.py", "--gpus", "1", "--grid", str(grid), "--steps", str(steps), "--warmup", str(warmup)],
                       cwd=ROOT, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        say(f"{label}: FAILED rc={p.returncode}\n{p.stderr[-1500:]}")
        sys.exit(1)
    j = json.loads(p.stdout.strip().splitlines()[-1])
    say(f"N={grid:6d} K={steps:5d} {label:24s} {j['value']:10.2f} it/s  ms/step {j['ms_per_step']:.5f}  loop-only ms/step {j['loop_only_ms_per_step']:.5f}  ({time.time() - t0:.0f} s)")
    return j["value"]


def med(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


for grid, steps, warmup in CASES:
    runs = {label: [] for label, _ in BUILDS}
    for _ in range(ROUNDS):
        for label, lib in BUILDS:
            runs[label].append(bench(label, lib, grid, steps, warmup))
    base = runs[BUILDS[0][0]]
    for label, _ in BUILDS:
        v = runs[label]
        say(f"  -> N={grid} K={steps} {label:24s} min/median/max {min(v):.2f}/{med(v):.2f}/{max(v):.2f}  median ratio {med(v) / med(base):.4f}  "
            f"slowest / fastest {BUILDS[0][0]} {min(v) / max(base):.4f}  median / slowest {BUILDS[0][0]} {med(v) / min(base):.4f}")
say("done")
