"""Time to solution of the recorded explicit on-chip wave stepper with a damping field (mi355cg_wave_sponge_many, DESIGN section
12.6) on one MI355X.

For every N and ensemble size nsys, nsys members integrate u_tt + d_s o u_t = c2_s o (A u) - w(t) g_s over 1000 steps of velocity
Verlet, each at tau_s = 0.5 x its own bound wave_cfl(c2_s), from seeded (u0, v0); c2_s a seeded medium in [0.25, 4] per member,
d_s a sponge layer of N / 5 nodes on all four outer sides (sponge_damping) scaled per member to (0.25 tau_s) max d_s = 0.5,
g_s = the handle's right-hand side times (1 + 0.1 * seeded standard-normal numbers), w a Ricker wavelet shared by all members, 16
seeded receivers sampled at every step.  Per row one warm-up and then five timed calls of each of
  (a)  one wave_record_many(..., c2=..., damping=...) call on device tensors (wall time of the call);
  (b)  the same scheme with torch slicing on (nsys, N+1, N+1) images, the factor formed once, v scaled at both ends of a step;
       its final u, v and traces are compared with (a)'s bit for bit, and that is the check;
  (c)  this build's wave_record_many(..., c2=...) on the same inputs with the damping dropped: what the damping costs;
  (d)  that medium call (no damping) of this build and of the --baseline-tree checkout (a built checkout of the parent commit), each
       in a child process on the same GPU, taking turns call by call.  ok: this build's median is not above the parent's slowest
       call of five.
Every row of (a) - (c) runs in a child process of its own under a time limit, and so does every answer of a worker of (d); the tool
stops at the first failure.  Nothing is scaled.  Reported: median (min .. max) wall ms; us_ms = median ms * 1000 / (nsys * steps).
At the end the registers and scratch of the four explicit wave kernels' instantiations, read from the built library's code-object
notes.

       python tools/onchip_wave_sponge_timing.py [--baseline-tree DIR] [--out FILE] [N ...]
                                                  (default 10 32 64 128; writes profiles/onchip_wave_sponge_time_to_solution.txt)"""
import json
import os
import re
import select
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "onchip_wave_sponge_time_to_solution.txt")
SIZES = [10, 32, 64, 128]
ENSEMBLES = {10: [1, 256, 4096], 32: [1, 256, 4096], 64: [256], 128: [1, 256, 1024]}      # section 12.5's nine rows and N = 64; at the cap a workgroup has a CU to itself
STEPS, RECEIVERS = 1000, 16
TIMED = 5
ROW_LIMIT, CALL_LIMIT = 240, 60                                          # seconds: a row of (a) - (c) in its child; one answer of a worker of (d)
sys.path.insert(0, os.environ.get("ONCHIP_WAVE_SPONGE_TREE") or ROOT)    # a worker of --baseline-tree imports that checkout's package
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def option(args, flag):
    if flag not in args:
        return None
    i = args.index(flag)
    val = args[i + 1]
    del args[i:i + 2]
    return val


def ensembles(n):
    return ENSEMBLES.get(n, [1, 256])


def ricker(steps):
    """A Ricker wavelet centred at a quarter of the run, six of its periods long."""
    x = (np.arange(steps + 1) - steps / 4.0) / (steps / 24.0)
    return (1.0 - 2.0 * x * x) * np.exp(-x * x)


# ---- the processes that touch the GPU ------------------------------------------------------------------------------------------------
def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def inputs(n, nsys):
    """The system of a row and its seeded ensemble on the device."""
    import torch
    import iterative_solvers_amd as isa
    import wave_reference as W
    os.environ.pop("MI355CG_ONCHIP", None)
    many = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
    e0 = np.zeros(many.size())
    e0[0] = 1.0
    col = many.apply(e0)
    grid = W.Grid(n, col[0], col[1], col[n // 2 - 1])
    own = many.get_rhs()
    rng = np.random.default_rng(1000 * n + nsys)
    g = own[None, :] * (1.0 + 0.1 * rng.standard_normal((nsys, own.size)))
    u0 = rng.standard_normal((nsys, own.size))
    v0 = rng.standard_normal((nsys, own.size)) * np.sqrt(abs(grid.A0))
    receivers = sorted(int(r) for r in rng.permutation(own.size)[:RECEIVERS])
    c2 = rng.uniform(0.25, 4.0, (nsys, own.size))
    gd, ud, vd, cd = (torch.from_numpy(a).cuda() for a in (g, u0, v0, c2))
    return many, grid, gd, ud, vd, cd, c2, receivers


class TorchImages:
    """The ensemble as (nsys, N+1, N+1) images on the device: the scheme written with torch."""

    def __init__(self, grid, nsys):
        import torch
        self.grid, self.nsys = grid, nsys
        self.cells = torch.from_numpy(grid.cells).cuda()
        n1 = grid.n + 1
        mask = torch.zeros(n1 * n1, dtype=torch.float64, device="cuda")
        mask[self.cells] = 1.0
        self.mask = mask.view(1, n1, n1)[:, 1:-1, 1:-1]
        self.n1 = n1

    def image(self, packed):
        import torch
        img = torch.zeros((self.nsys, self.n1 * self.n1), dtype=torch.float64, device="cuda")
        img[:, self.cells] = packed
        return img.view(self.nsys, self.n1, self.n1)

    def au(self, u):
        g = self.grid
        return g.A0 * u[:, 1:-1, 1:-1] + g.xk * (u[:, 1:-1, :-2] + u[:, 1:-1, 2:]) + g.yk * (u[:, :-2, 1:-1] + u[:, 2:, 1:-1])

    def sponge(self, u0, v0, gg, c2, d, tau, w, receivers):
        import torch
        inner = lambda p: self.image(p)[:, 1:-1, 1:-1]
        u, v, gi, ci, di = self.image(u0), inner(v0).clone(), inner(gg), inner(c2), inner(d)
        rc = self.cells[torch.tensor(receivers, device="cuda")]
        t = torch.from_numpy(tau).cuda().view(-1, 1, 1)
        h = 0.5 * t
        e = (0.25 * t) * di
        s = (1.0 - e) / (1.0 + e)
        flat = u.view(self.nsys, -1)
        traces = torch.empty((self.nsys, len(w) - 1, len(receivers)), dtype=torch.float64, device="cuda")
        a = (ci * self.au(u) - float(w[0]) * gi) * self.mask
        for n in range(len(w) - 1):
            v = s * v
            v = v + h * a
            u[:, 1:-1, 1:-1] = u[:, 1:-1, 1:-1] + t * v
            a = (ci * self.au(u) - float(w[n + 1]) * gi) * self.mask
            v = v + h * a
            v = s * v
            traces[:, n, :] = flat[:, rc]
        vimg = torch.zeros((self.nsys, self.n1, self.n1), dtype=torch.float64, device="cuda")
        vimg[:, 1:-1, 1:-1] = v
        return flat[:, self.cells].contiguous(), vimg.view(self.nsys, -1)[:, self.cells].contiguous(), traces


def row(n, nsys):
    """Child process of (a) - (c): one row, one JSON line out."""
    import torch
    many, grid, gd, ud, vd, cd, c2, receivers = inputs(n, nsys)
    tau = 0.5 * np.atleast_1d(many.wave_cfl(c2))
    layer = many.sponge_damping(max(2, n // 5), 1.0)
    d = np.ascontiguousarray(layer[None, :] * (2.0 / tau)[:, None])          # (0.25 tau_s) max d_s = 0.5
    dd = torch.from_numpy(d).cuda()
    w = ricker(STEPS)
    wd = torch.from_numpy(w).cuda()
    ti = TorchImages(grid, nsys)
    call_a = lambda: many.wave_record_many(ud, vd, tau, STEPS, wd, g=gd, receivers=receivers, c2=cd, damping=dd)
    call_b = lambda: ti.sponge(ud, vd, gd, cd, dd, tau, w, receivers)
    call_c = lambda: many.wave_record_many(ud, vd, tau, STEPS, wd, g=gd, receivers=receivers, c2=cd)
    _, ra = timed(call_a)                                               # the warm-up of all
    _, rb = timed(call_b)
    timed(call_c)
    assert (ra[4] == STEPS).all() and bool(torch.isfinite(ra[0]).all()), (n, nsys)
    agree = bool(torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1]) and torch.equal(ra[2], rb[2]))
    a, b, c = (stats([timed(f)[0] for _ in range(TIMED)]) for f in (call_a, call_b, call_c))
    print("ROW " + json.dumps(dict(a=a, b=b, c=c, agree=agree, tau=[float(tau.min()), float(tau.max())])), flush=True)


def worker():
    """Child process of (d): the call in a medium of the package this process imports.  One line in ("N nsys"), one JSON line out."""
    import torch
    rows = {}
    print("READY", flush=True)
    for ln in sys.stdin:
        f = ln.split()
        if not f or f[0] == "quit":
            break
        key = (int(f[0]), int(f[1]))
        if key not in rows:
            many, _, gd, ud, vd, cd, c2, receivers = inputs(*key)
            rows = {key: (many, gd, ud, vd, cd, receivers, 0.5 * np.atleast_1d(many.wave_cfl(c2)), torch.from_numpy(ricker(STEPS)).cuda())}
        many, gd, ud, vd, cd, receivers, tau, wd = rows[key]
        ms, out = timed(lambda: many.wave_record_many(ud, vd, tau, STEPS, wd, g=gd, receivers=receivers, c2=cd))
        assert (out[4] == STEPS).all()
        print("R " + json.dumps(ms), flush=True)


# ---- no GPU from here on ---------------------------------------------------------------------------------------------------------------
KERNELS = ("k_onchip_wave_verlet", "k_oc_wave_record", "k_oc_wave_medium", "k_oc_wave_sponge")


def resources():
    """The wave kernels of the built library: registers and scratch from the code-object notes."""
    llvm = os.path.join(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")), "..", "lib", "llvm", "bin")
    lib = os.path.join(ROOT, "iterative_solvers_amd", "libmi355cg.so")
    if not os.path.exists(os.path.join(llvm, "clang-offload-bundler")) or not os.path.exists(lib):
        return ["# (no ROCm LLVM tools or no built library here: the kernels' resources are not listed)"]
    tmp = tempfile.mkdtemp(prefix="onchip_wave_sponge_")
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "gfx950.co")
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={fat}", f"--output={co}"])
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    shutil.rmtree(tmp)
    found = {}
    for entry in notes[notes.index("amdhsa.kernels"):].split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        m = re.search(r"\d+(" + "|".join(KERNELS) + r")ILi(\d+)E", name)
        if m:
            field = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", entry).group(1))
            found[(m.group(1), int(m.group(2)))] = (field("vgpr_count"), field("sgpr_count"), field("private_segment_fixed_size"))
    lines = ["# the explicit wave kernels as built for gfx950 (the library's code-object notes).  E = unknowns per thread, __launch_bounds__(512).  Scratch must be 0;",
             "# waves_per_SIMD = min(8, 512 / VGPRs rounded up to 8), computed here.  The first three kernels: the parent commit's figures.",
             f"# {'kernel':<28} {'VGPRs':>5} {'SGPRs':>5} {'scratch_B_per_lane':>18} {'waves_per_SIMD':>14}"]
    for kernel in KERNELS:
        for e in (1, 2, 4, 8, 16, 24):
            v, s, p = found[(kernel, e)]
            lines.append(f"  {kernel + '<' + str(e) + '>':<28} {v:>5} {s:>5} {p:>18} {min(8, 512 // ((v + 7) // 8 * 8)):>14}")
    return lines


def answer(child, limit):
    """One line of a child within `limit` seconds, or None."""
    ready, _, _ = select.select([child.stdout], [], [], limit)
    return child.stdout.readline() if ready else None


def main(ns, baseline_tree, out_path):
    lines = ["# time to solution of ensembles of recorded explicit wave steppers with a damping field on one MI355X (tools/onchip_wave_sponge_timing.py).",
             f"# {STEPS} steps of velocity Verlet of u_tt + d_s o u_t = c2_s o (A u) - w(t) g_s, member s at tau_s = 0.5 x wave_cfl(c2_s), c2_s seeded in [0.25, 4], d_s a sponge",
             "# layer of N / 5 nodes on all outer sides scaled to (0.25 tau_s) max d_s = 0.5, a Ricker wavelet for all members,",
             f"# {RECEIVERS} receivers sampled at every step, seeded (u0, v0), g_s = the handle's right-hand side times (1 + 0.1 * seeded standard-normal numbers).",
             "# Domain (1, 2, 1, 2), default steps_per_launch.  (a) mi355cg_wave_sponge_many on device tensors; (b) the scheme with torch slicing on images, b=a: final",
             "# u, v and traces agree with (a)'s bit for bit; (c) this build's mi355cg_wave_medium_many, the same inputs without the damping.",
             f"# Per row, in a child process of its own: one warm-up of each, then {TIMED} timed calls of (a), of (b), of (c).  ms = wall time of all members' steps,",
             "# median (min .. max); us_ms = median ms * 1000 / (nsys * steps), per member-step; b/a, a/c = ratios of the medians.  Nothing is scaled or extrapolated.",
             f"# {'N':>4} {'nsys':>5} | {'a_ms med':>9} {'min':>9} {'max':>9} {'us_ms':>8} | {'b_ms med':>10} {'min':>10} {'max':>10} {'b=a':>4} | {'c_ms med':>9} {'min':>9} {'max':>9} | {'b/a':>7} {'a/c':>6}"]
    print("\n".join(lines), flush=True)
    env = dict(os.environ)
    env.pop("MI355CG_ONCHIP", None)
    env.pop("MI355CG_LIB", None)
    failed = None
    for n in ns:
        for nsys in ensembles(n):
            try:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", str(n), str(nsys)], env=env, capture_output=True, text=True, timeout=ROW_LIMIT)
            except subprocess.TimeoutExpired:
                failed = f"row N = {n}, nsys = {nsys}: no result within {ROW_LIMIT} s"
                break
            got = [ln for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
            if out.returncode != 0 or not got:
                failed = f"row N = {n}, nsys = {nsys}: exit status {out.returncode}: {out.stderr[-400:]!r}"
                break
            r = json.loads(got[0][4:])
            a, b, c = r["a"], r["b"], r["c"]
            line = (f"  {n:>4} {nsys:>5} | {a[0]:>9.3f} {a[1]:>9.3f} {a[2]:>9.3f} {a[0] * 1e3 / (nsys * STEPS):>8.3f} | {b[0]:>10.3f} {b[1]:>10.3f} {b[2]:>10.3f} "
                    f"{'yes' if r['agree'] else 'NO':>4} | {c[0]:>9.3f} {c[1]:>9.3f} {c[2]:>9.3f} | {b[0] / a[0]:>7.2f} {a[0] / c[0]:>6.2f}")
            lines.append(line)
            print(line, flush=True)
            if not r["agree"]:
                failed = f"row N = {n}, nsys = {nsys}: (b) and (a) differ"
                break
        if failed:
            break

    medium_lines = []
    if not failed:
        children = {}
        trees = {"this": ROOT}
        if baseline_tree:
            trees["parent"] = os.path.abspath(baseline_tree)
        for name, tree in trees.items():
            children[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], env=dict(env, ONCHIP_WAVE_SPONGE_TREE=tree),
                                              stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            if (answer(children[name], CALL_LIMIT) or "").strip() != "READY":
                failed = f"(d): the worker of {name} did not start"

        def medium(name, n, nsys):
            child = children[name]
            child.stdin.write(f"{n} {nsys}\n")
            child.stdin.flush()
            ln = answer(child, CALL_LIMIT)
            return json.loads(ln[2:]) if ln and ln.startswith("R ") else None

        medium_lines = [f"# (d) the call in a medium without a damping (wave_record_many(..., c2=)), {STEPS} steps, {RECEIVERS} receivers: this build and the parent commit, each in a child process, taking turns call by call"
                        if baseline_tree else "# (d) no --baseline-tree: the parent commit not measured; this build's call in a medium in a child process",
                        f"# {'N':>4} {'nsys':>5} | {'this_ms med':>11} {'min':>9} {'max':>9} | {'parent_ms med':>13} {'min':>9} {'max':>9} | {'this med <= parent max':>22}"]
        all_ok = True
        for n in ns:
            for nsys in ensembles(n):
                mine, base = [], []
                for k in range(TIMED + 1):                                          # k = 0: the warm-up of both
                    m = medium("this", n, nsys) if not failed else None
                    b = medium("parent", n, nsys) if baseline_tree and not failed and m is not None else None
                    if m is None or (baseline_tree and b is None):
                        failed = failed or f"(d) N = {n}, nsys = {nsys}: a worker gave no answer within {CALL_LIMIT} s"
                        break
                    if k:
                        mine.append(m)
                        if b is not None:
                            base.append(b)
                if failed:
                    break
                m = stats(mine)
                if base:
                    b = stats(base)
                    ok = m[0] <= b[2]
                    all_ok = all_ok and ok
                    medium_lines.append(f"  {n:>4} {nsys:>5} | {m[0]:>11.3f} {m[1]:>9.3f} {m[2]:>9.3f} | {b[0]:>13.3f} {b[1]:>9.3f} {b[2]:>9.3f} | {'yes' if ok else 'NO':>22}")
                else:
                    medium_lines.append(f"  {n:>4} {nsys:>5} | {m[0]:>11.3f} {m[1]:>9.3f} {m[2]:>9.3f} | {'-':>13} {'-':>9} {'-':>9} | {'-':>22}")
                print(medium_lines[-1], flush=True)
            if failed:
                break
        for child in children.values():
            if failed:
                child.kill()
            else:
                child.stdin.write("quit\n")
                child.stdin.flush()
            child.wait(timeout=60)
        if baseline_tree and not failed:
            medium_lines.append(f"# this build's median is not above the parent's slowest call in every row: {'yes' if all_ok else 'NO'}")
    lines += ["#"] + medium_lines
    if failed:
        lines.append("# STOPPED at the first failure: " + failed)
        print(lines[-1], flush=True)
    lines += ["#"] + resources()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)
    return 1 if failed else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--worker":
        worker()
        sys.exit(0)
    if args and args[0] == "--row":
        row(int(args[1]), int(args[2]))
        sys.exit(0)
    baseline_tree = option(args, "--baseline-tree")
    out_path = option(args, "--out") or OUT
    sys.exit(main([int(a) for a in args] or SIZES, baseline_tree, out_path))
