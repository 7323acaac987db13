#!/usr/bin/env python3
"""Instruction mix of the loops of one kernel in a hipcc -S dump.
Usage: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 -w --cuda-device-only -S -o /tmp/dev.s iterative_solvers_amd/csrc/mi355cg.hip
       python tools/isa_loop_stats.py /tmp/dev.s <mangled-name-substring> [min_instructions]
Prints, for every backward branch (a loop), the number of instructions by class between its target label and the branch.
With --head as a last argument: the launch head of the kernel instead (profiles/launch_head.txt): kernel-argument bytes, registers,
scratch, code bytes, lane spills (v_writelane / v_readlane) in the kernel and in its largest loop, what precedes the first row
request, and every vmcnt wait between the first 128-bit row request and the largest loop (the main loop)."""
import collections
import re
import sys

head = sys.argv[-1] == "--head"
if head:
    sys.argv.pop()
path, pat = sys.argv[1], sys.argv[2]
minlen = int(sys.argv[3]) if len(sys.argv) > 3 else 40
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\S*:", l) and pat in l)
end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
body = lines[start:end + 1]
labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}


def klass(op):
    if op.startswith("buffer_load") or op.startswith("global_load"): return "vmem_load"
    if op.startswith("buffer_store") or op.startswith("global_store"): return "vmem_store"
    if op.startswith("s_load") or op.startswith("s_buffer_load"): return "smem"
    if op.startswith("ds_"): return "lds"
    if op.startswith("s_waitcnt"): return "waitcnt"
    if op.startswith("s_"): return "salu"
    if op.startswith("v_") and ("_f64" in op): return "valu_f64"
    if op.startswith("v_") and "dpp" in op: return "valu_dpp"
    if op.startswith("v_"): return "valu_other"
    return "other"


def instr(k):
    t = body[k].strip()
    return None if (not t or t.startswith(";") or t.startswith(".") or t.endswith(":")) else t


def loops():
    for i, l in enumerate(body):
        m = re.match(r"^\s+(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)", l)
        if m and m.group(2) in labels and labels[m.group(2)] <= i:
            yield labels[m.group(2)], i


if head:
    name = body[0].split(":")[0]
    meta = {}
    for l in lines[end:]:
        if l.startswith(".Lfunc_end") and l != lines[end]:
            break
        for key in ("codeLenInByte", "TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy"):
            if (m := re.match(rf"^; {key}\s*[:=]\s*(\d+)", l)):
                meta[key] = int(m.group(1))
    karg = None      # .amdhsa_kernarg_size stands in the kernel descriptor block that follows ".amdhsa_kernel <name>"
    for i, l in enumerate(lines):
        if l.strip() == f".amdhsa_kernel {name}":
            karg = next(int(m.group(1)) for k in range(i, i + 80) if (m := re.match(r"^\s+\.amdhsa_kernarg_size (\d+)", lines[k])))
    ins = [(k, t) for k in range(len(body)) if (t := instr(k))]
    cnt = lambda pred, a=0, b=len(body): sum(1 for k, t in ins if a <= k <= b and pred(t))
    first_row = next(k for k, t in ins if t.startswith("buffer_load_dwordx4"))
    # the main loop: the widest loop behind the first row request that stores rows (blocks laid out behind the kernel's end that
    # jump back into the prologue make wider "loops" that are none)
    stores = [k for k, t in ins if t.startswith("buffer_store_dwordx4")]
    real = [r for r in loops() if "Loop Header" in body[r[0]]]        # LLVM marks the header of every natural loop
    cand = [r for r in real if r[0] > first_row and any(r[0] <= k <= r[1] for k in stores)]
    if not cand:          # the header of the main loop lies in front of the first row request in the text (rotated layout): any loop with stores
        cand = [r for r in loops() if any(r[0] <= k <= r[1] for k in stores)]
    lo, hi = max(cand, key=lambda r: r[1] - r[0])
    # loops of the prologue itself: the tails of the reductions that take the partials beyond the two prefetched pairs (more than 512)
    small = [r for r in real if first_row < r[0] and r[1] < lo]
    first_vmem = next(k for k, t in ins if t.startswith("buffer_load") or t.startswith("global_load"))
    print(f"{name}")
    print(f"  kernarg bytes {karg}, VGPRs {meta.get('NumVgprs')}, SGPRs {meta.get('TotalNumSgprs')}, scratch {meta.get('ScratchSize')}, code bytes {meta.get('codeLenInByte')}, occupancy {meta.get('Occupancy')}")
    print(f"  whole kernel: {len(ins)} instructions, s_load {cnt(lambda t: t.startswith('s_load'))}, s_waitcnt lgkmcnt(0) {cnt(lambda t: t.startswith('s_waitcnt') and 'lgkmcnt(0)' in t)}, "
          f"v_writelane {cnt(lambda t: t.startswith('v_writelane'))}, v_readlane {cnt(lambda t: t.startswith('v_readlane'))}, ds_bpermute {cnt(lambda t: t.startswith('ds_bpermute'))}, global_atomic {cnt(lambda t: t.startswith('global_atomic'))}")
    print(f"  main loop (lines {lo}-{hi}): {cnt(lambda t: True, lo, hi)} instructions, v_writelane {cnt(lambda t: t.startswith('v_writelane'), lo, hi)}, v_readlane {cnt(lambda t: t.startswith('v_readlane'), lo, hi)}")
    print(f"  before the first vector load: {cnt(lambda t: True, 0, first_vmem - 1)} instructions, s_load {cnt(lambda t: t.startswith('s_load'), 0, first_vmem - 1)}, lgkmcnt(0) waits {cnt(lambda t: t.startswith('s_waitcnt') and 'lgkmcnt(0)' in t, 0, first_vmem - 1)}")
    print(f"  before the first 128-bit row request: {cnt(lambda t: True, 0, first_row - 1)} instructions, s_load {cnt(lambda t: t.startswith('s_load'), 0, first_row - 1)}, lgkmcnt(0) waits {cnt(lambda t: t.startswith('s_waitcnt') and 'lgkmcnt(0)' in t, 0, first_row - 1)}")
    waits = [(t, any(a <= k <= b for a, b in small)) for k, t in ins if first_row < k < lo and t.startswith("s_waitcnt") and "vmcnt" in t]
    print(f"  vmcnt waits between the first row request and the main loop ([tail]: inside a loop over partials beyond the 512 prefetched): "
          + (" | ".join(t + (" [tail]" if inner else "") for t, inner in waits) if waits else "none"))
    print(f"  vmcnt(0) among them outside those tails: {sum(1 for t, inner in waits if not inner and re.search(r'vmcnt[(]0[)]', t))}")
    sys.exit(0)

print(f"{pat}: {end - start} lines")
for i, l in enumerate(body):
    m = re.match(r"^\s+(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)", l)
    if not m or m.group(2) not in labels or labels[m.group(2)] > i:
        continue
    lo = labels[m.group(2)]
    cnt, ops = collections.Counter(), collections.Counter()
    n = 0
    for k in range(lo, i + 1):
        t = body[k].strip()
        if not t or t.startswith(";") or t.startswith(".") or t.endswith(":"):
            continue
        op = t.split()[0]
        if "dpp" in t and op.startswith("v_"):
            op += "_dpp"
        cnt[klass(op)] += 1
        ops[op] += 1
        n += 1
    if n < minlen:
        continue
    f64 = {o: c for o, c in ops.items() if "_f64" in o}
    print(f"loop {m.group(2)} lines {lo}-{i}: {n} instructions: " + ", ".join(f"{k} {v}" for k, v in sorted(cnt.items())))
    print("     f64 ops: " + ", ".join(f"{o} {c}" for o, c in sorted(f64.items(), key=lambda kv: -kv[1])))
    print("     waits: " + " | ".join(body[k].strip() for k in range(lo, i + 1) if body[k].strip().startswith("s_waitcnt"))[:400])
