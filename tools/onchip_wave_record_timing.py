"""Time to solution of the explicit on-chip wave stepper with a source time function and receiver traces (mi355cg_wave_record_many,
DESIGN section 12.4) on one MI355X.

For every N and ensemble size nsys, nsys members integrate u_tt = A u - w(t) g_s over 1000 steps of velocity Verlet at tau = 0.5 x the
bound of wave_cfl() from seeded (u0, v0); g_s = the handle's right-hand side times (1 + 0.1 * seeded standard-normal numbers), w a
Ricker wavelet shared by all members, 16 seeded receivers, a sample every step and every 10th.  Per row one warm-up and then five
timed calls of each of
  (a)  one wave_record_many call on device tensors (wall time of the call);
  (b)  what the interface without it allows on the same GPU.  One wave_steps_many call holds the forcing constant over its steps, and
       the scheme takes w[n] in the first half kick of step n and w[n + 1] in the second, so no sequence of such calls gives these
       bits.  Two stand-ins are timed:
       (b1) a loop of wave_steps_many(nsteps = 1) with g rescaled by torch per step (w[n] in both half kicks: first order in tau where
            w changes) and the receivers gathered by torch indexing -- the launch-bound loop; its largest |difference| of the final u
            from (a)'s, relative to the largest |u|, is reported, not zero by construction;
       (b2) the scheme's own expressions with torch slicing on (nsys, N+1, N+1) images, in their order, the receivers gathered by
            torch indexing: its final u and traces are compared with (a)'s bit for bit;
  (c)  this build's plain wave_steps_many for the same steps (a constant forcing, no traces): what the source and the receivers cost;
  (d)  the plain wave_steps_many of this build and of the --baseline-tree checkout (a built checkout of the parent commit), each in a
       child process of the same job on the same GPU, taking turns call by call.
Nothing is scaled.  Reported: median (min .. max) wall ms; us_ms = median ms * 1000 / (nsys * steps).  (d) ok: this build's median is
not above the parent's slowest call.

       python tools/onchip_wave_record_timing.py [--baseline-tree DIR] [--resources FILE] [--out FILE] [N ...]
                                                  (default 10 32 128; writes profiles/onchip_wave_record_time_to_solution.txt)"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "onchip_wave_record_time_to_solution.txt")
SIZES = [10, 32, 128]
ENSEMBLES = [1, 256, 4096]
STEPS, RECEIVERS, CADENCES = 1000, 16, (1, 10)
TIMED = 5
sys.path.insert(0, os.environ.get("ONCHIP_WAVE_RECORD_TREE") or ROOT)     # a worker of --baseline-tree imports that checkout's package
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import iterative_solvers_amd as isa  # noqa: E402
import wave_reference as W  # noqa: E402


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


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def ensembles(n):
    return ENSEMBLES[:-1] + [1024] if n >= 128 else ENSEMBLES         # at the cap a workgroup has a CU to itself: up to 1024


class Case:
    """One system per N and process; the seeded ensemble of a row on the device."""

    def __init__(self):
        self.sys = {}

    def row(self, n, nsys):
        if n not in self.sys:
            os.environ.pop("MI355CG_ONCHIP", None)
            many = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
            e0 = np.zeros(many.size())
            e0[0] = 1.0
            col = many.apply(e0)
            self.sys[n] = (many, W.Grid(n, col[0], col[1], col[n // 2 - 1]))
        many, grid = self.sys[n]
        own = many.get_rhs()
        rng = np.random.default_rng(1000 * n + nsys)
        g = own[None, :] * (1.0 + 0.1 * rng.standard_normal((nsys, own.size)))
        u0 = rng.standard_normal((nsys, own.size))
        v0 = rng.standard_normal((nsys, own.size)) * np.sqrt(abs(grid.A0))
        receivers = sorted(int(r) for r in rng.permutation(own.size)[:RECEIVERS])
        tau = np.full(nsys, 0.5 * many.wave_cfl())
        gd, ud, vd = (torch.from_numpy(a).cuda() for a in (g, u0, v0))
        return many, grid, gd, ud, vd, tau, receivers


def ricker(steps):
    """A Ricker wavelet centred at a quarter of the run, six of its periods long."""
    x = (np.arange(steps + 1) - steps / 4.0) / (steps / 24.0)
    return (1.0 - 2.0 * x * x) * np.exp(-x * x)


def worker():
    """Child process of (d): the plain call of the package this process imports.  One line in ("N nsys"), one JSON line out (wall ms)."""
    case = Case()
    print("READY", flush=True)
    for ln in sys.stdin:
        f = ln.split()
        if not f or f[0] == "quit":
            break
        many, _, gd, ud, vd, tau, _ = case.row(int(f[0]), int(f[1]))
        ms, out = timed(lambda: many.wave_steps_many(ud, vd, tau, STEPS, g=gd))
        assert (out[3] == STEPS).all()
        print("R " + json.dumps(ms), flush=True)


class TorchImages:
    """The ensemble as (nsys, N+1, N+1) images on the device: the scheme written with torch."""

    def __init__(self, grid, nsys):
        self.grid, self.nsys = grid, nsys
        self.cells = torch.from_numpy(grid.cells).cuda()
        n1 = grid.n + 1
        mask = torch.zeros(n1 * n1, dtype=torch.float64, device="cuda")
        mask[self.cells] = 1.0
        self.mask = mask.view(1, n1, n1)[:, 1:-1, 1:-1]
        self.n1 = n1

    def image(self, packed):
        img = torch.zeros((self.nsys, self.n1 * self.n1), dtype=torch.float64, device="cuda")
        img[:, self.cells] = packed
        return img.view(self.nsys, self.n1, self.n1)

    def au(self, u):
        g = self.grid
        return g.A0 * u[:, 1:-1, 1:-1] + g.xk * (u[:, 1:-1, :-2] + u[:, 1:-1, 2:]) + g.yk * (u[:, :-2, 1:-1] + u[:, 2:, 1:-1])

    def record(self, u0, v0, gg, tau, w, receivers, every):
        u, v, gi = self.image(u0), self.image(v0)[:, 1:-1, 1:-1].clone(), self.image(gg)[:, 1:-1, 1:-1]
        rc = self.cells[torch.tensor(receivers, device="cuda")]
        t = torch.from_numpy(tau).cuda().view(-1, 1, 1)
        h = 0.5 * t
        flat = u.view(self.nsys, -1)
        traces = torch.empty((self.nsys, (len(w) - 1) // every, len(receivers)), dtype=torch.float64, device="cuda")
        a = (self.au(u) - float(w[0]) * gi) * self.mask
        for n in range(len(w) - 1):
            v = v + h * a
            u[:, 1:-1, 1:-1] = u[:, 1:-1, 1:-1] + t * v
            a = (self.au(u) - float(w[n + 1]) * gi) * self.mask
            v = v + h * a
            if (n + 1) % every == 0:
                traces[:, (n + 1) // every - 1, :] = flat[:, rc]
        return flat[:, self.cells].contiguous(), traces


def step_loop(many, ud, vd, gd, tau, w, receivers, every):
    """(b1): one call per step, the forcing of the step w[n] g."""
    rc = torch.tensor(receivers, device="cuda")
    traces = torch.empty((ud.shape[0], (len(w) - 1) // every, len(receivers)), dtype=torch.float64, device="cuda")
    u, v = ud, vd
    for n in range(len(w) - 1):
        u, v = many.wave_steps_many(u, v, tau, 1, g=float(w[n]) * gd)[:2]
        if (n + 1) % every == 0:
            traces[:, (n + 1) // every - 1, :] = u[:, rc]
    return u, traces


def main(ns, baseline_tree, resources, out_path):
    children = {}
    trees = {"this": ROOT}
    if baseline_tree:
        trees["parent"] = os.path.abspath(baseline_tree)
    for name, tree in trees.items():
        env = dict(os.environ, ONCHIP_WAVE_RECORD_TREE=tree)
        env.pop("MI355CG_ONCHIP", None)
        env.pop("MI355CG_LIB", None)
        children[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert children[name].stdout.readline().strip() == "READY"

    def plain(name, n, nsys):
        child = children[name]
        child.stdin.write(f"{n} {nsys}\n")
        child.stdin.flush()
        ln = child.stdout.readline()
        assert ln.startswith("R "), ln
        return json.loads(ln[2:])

    lines = ["# time to solution of ensembles of explicit wave steppers with a source and receiver traces on one MI355X (tools/onchip_wave_record_timing.py).",
             f"# {STEPS} steps of velocity Verlet at tau = 0.5 x wave_cfl(), a Ricker wavelet for all members, {RECEIVERS} receivers, seeded (u0, v0), g_s = the handle's",
             "# right-hand side times (1 + 0.1 * seeded standard-normal numbers).  Domain (1, 2, 1, 2), default steps_per_launch.",
             "# (a) mi355cg_wave_record_many on device tensors; (b1) a loop of wave_steps_many(nsteps = 1), g rescaled by torch per step (the forcing constant",
             "# over a step: not the scheme of (a), du = largest |u_b1 - u_a| / largest |u_a|), receivers gathered by torch; (b2) the scheme with torch slicing on",
             "# images, b2=a: final u and traces agree with (a)'s bit for bit; (c) this build's plain wave_steps_many, the same steps.",
             f"# Per row: one warm-up of each, then {TIMED} timed calls of (a), of (b1), of (b2), of (c).  ms = wall time of all members' steps, median (min .. max);",
             "# us_ms = median ms * 1000 / (nsys * steps), per member-step; b1/a, b2/a, a/c = ratios of the medians.  Nothing is scaled or extrapolated.",
             f"# {'N':>4} {'nsys':>5} {'every':>5} | {'a_ms med':>9} {'min':>9} {'max':>9} {'us_ms':>8} | {'b1_ms med':>10} {'min':>10} {'max':>10} {'du':>8} | "
             f"{'b2_ms med':>10} {'min':>10} {'max':>10} {'b2=a':>5} | {'c_ms med':>9} {'min':>9} {'max':>9} | {'b1/a':>7} {'b2/a':>7} {'a/c':>6}"]
    print("\n".join(lines), flush=True)
    case = Case()
    w = ricker(STEPS)
    plain_lines = [f"# (d) the plain wave_steps_many call, {STEPS} steps: this build and the parent commit, each in a child process, taking turns call by call"
                   if baseline_tree else "# (d) no --baseline-tree: the parent commit not measured; this build's plain call in a child process",
                   f"# {'N':>4} {'nsys':>5} | {'this_ms med':>11} {'min':>9} {'max':>9} | {'parent_ms med':>13} {'min':>9} {'max':>9} | {'this med <= parent max':>22}"]
    all_ok = True
    for n in ns:
        for nsys in ensembles(n):
            many, grid, gd, ud, vd, tau, receivers = case.row(n, nsys)
            ti = TorchImages(grid, nsys)
            wd = torch.from_numpy(w).cuda()
            for every in CADENCES:
                call_a = lambda: many.wave_record_many(ud, vd, tau, STEPS, wd, g=gd, receivers=receivers, record_every=every)
                call_b1 = lambda: step_loop(many, ud, vd, gd, tau, w, receivers, every)
                call_b2 = lambda: ti.record(ud, vd, gd, tau, w, receivers, every)
                call_c = lambda: many.wave_steps_many(ud, vd, tau, STEPS, g=gd)
                _, ra = timed(call_a)                                               # the warm-up of all
                _, rb1 = timed(call_b1)
                _, rb2 = timed(call_b2)
                timed(call_c)
                assert (ra[4] == STEPS).all() and bool(torch.isfinite(ra[0]).all()), (n, nsys)
                du = float((rb1[0] - ra[0]).abs().max() / ra[0].abs().max())
                agree = "yes" if torch.equal(ra[0], rb2[0]) and torch.equal(ra[2], rb2[1]) else "NO"
                a, b1, b2, c = (stats([timed(f)[0] for _ in range(TIMED)]) for f in (call_a, call_b1, call_b2, call_c))
                per = 1e3 / (nsys * STEPS)
                line = (f"  {n:>4} {nsys:>5} {every:>5} | {a[0]:>9.3f} {a[1]:>9.3f} {a[2]:>9.3f} {a[0] * per:>8.3f} | {b1[0]:>10.3f} {b1[1]:>10.3f} {b1[2]:>10.3f} {du:>8.1e} | "
                        f"{b2[0]:>10.3f} {b2[1]:>10.3f} {b2[2]:>10.3f} {agree:>5} | {c[0]:>9.3f} {c[1]:>9.3f} {c[2]:>9.3f} | {b1[0] / a[0]:>7.2f} {b2[0] / a[0]:>7.2f} {a[0] / c[0]:>6.2f}")
                lines.append(line)
                print(line, flush=True)
            mine, base = [], []
            for k in range(TIMED + 1):                                              # k = 0: the warm-up of both
                m = plain("this", n, nsys)
                b = plain("parent", n, nsys) if baseline_tree else None
                if k:
                    mine.append(m)
                    if b is not None:
                        base.append(b)
            m = stats(mine)
            if base:
                b = stats(base)
                ok = m[0] <= b[2]
                all_ok = all_ok and ok
                plain_lines.append(f"  {n:>4} {nsys:>5} | {m[0]:>11.3f} {m[1]:>9.3f} {m[2]:>9.3f} | {b[0]:>13.3f} {b[1]:>9.3f} {b[2]:>9.3f} | {'yes' if ok else 'NO':>22}")
            else:
                plain_lines.append(f"  {n:>4} {nsys:>5} | {m[0]:>11.3f} {m[1]:>9.3f} {m[2]:>9.3f} | {'-':>13} {'-':>9} {'-':>9} | {'-':>22}")
            print(plain_lines[-1], flush=True)
    for child in children.values():
        child.stdin.write("quit\n")
        child.stdin.flush()
        child.wait(timeout=60)
    if baseline_tree:
        plain_lines.append(f"# this build's median is not above the parent's slowest call in every row: {'yes' if all_ok else 'NO'}")
    lines += ["#"] + plain_lines
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
    if args and args[0] == "--worker":
        worker()
        sys.exit(0)
    resources = []
    while "--resources" in args:
        resources.append(option(args, "--resources"))
    baseline_tree = option(args, "--baseline-tree")
    out_path = option(args, "--out") or OUT
    sys.exit(main([int(a) for a in args] or SIZES, baseline_tree, resources, out_path))
