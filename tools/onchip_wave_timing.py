"""Time to solution of the on-chip ensemble wave steppers (mi355cg_wave_steps_many) on one MI355X.

For every N and ensemble size nsys, nsys members integrate u_tt = A u - g_s from seeded (u0, v0), g_s = the handle's right-hand side
times (1 + 0.1 * seeded standard-normal numbers):
  Verlet    200 steps of velocity Verlet at tau = 0.5 x the bound of wave_cfl();
  Newmark    20 steps of Newmark at sigma = 4 / tau^2 = 10 |A_diag|, REL_2NORM 1e-8.
Per row one warm-up and then five timed calls of each of
  (a) one wave_steps_many call on device tensors (wall time of the call);
  (b) the best the interface without it allows on the same GPU.  Verlet: torch slicing on an (nsys, N+1, N+1) image, the scheme's
      expressions in their order, the state kept as images over all steps.  Newmark: per step the right-hand side with torch (the same
      slicing) and one solve_many(b, x0 = u, sigma) call on device tensors, the velocity with torch.  Its final u is compared with (a)'s;
  (c) the NumPy model of tests/wave_reference.py on one core, for nsys <= 256: five timed calls where a call takes under 2 s, one
      otherwise (Newmark: the model's own CG to 1e-8, member by member).
Nothing is scaled.  Reported: median / min / max wall ms and us per member-step (median ms / (nsys * steps)).  At the end, for the
default steps_per_launch of the explicit scheme: the device time of ONE launch of that many steps at N = 128 (the latency of a stop
request), from the call's loop_seconds.

       python tools/onchip_wave_timing.py [--resources FILE] [--out FILE] [N ...]
                                                  (default 10 32 128; writes profiles/onchip_wave_time_to_solution.txt)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "onchip_wave_time_to_solution.txt")
SIZES = [10, 32, 128]
ENSEMBLES = [1, 256, 4096]
VERLET_STEPS, NEWMARK_STEPS = 200, 20
TIMED = 5
C_MOST = 256
C_REPEAT_BELOW_MS = 2000.0
DEFAULT_LAUNCH = 512                    # kOnchipWaveDefaultSteps (csrc/onchip_plan.h)
# us per member-step of time_steps_many (implicit Euler, factor 10 / factor 0.03) from profiles/onchip_steps_time_to_solution.txt
STEPS_MANY_US = {(10, 1): "13.7/9.1", (10, 256): ".056/.039", (10, 4096): ".009/.006", (32, 1): "23.6/35.2", (32, 256): ".099/.150",
                 (32, 4096): ".038/.058", (128, 1): "91.1/324", (128, 256): ".408/1.33", (128, 1024): ".404/1.32"}
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import iterative_solvers_amd as isa  # noqa: E402
import wave_reference as W  # noqa: E402
from iterative_solvers_amd import _capi  # noqa: E402


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


class TorchImages:
    """The ensemble as (nsys, N+1, N+1) images on the device: what a caller without the new entry point would write."""

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

    def packed(self, img):
        return img.reshape(self.nsys, -1)[:, self.cells].contiguous()

    def au(self, u):
        """A0 uc + xk (left + right) + yk (down + up) on the interior of the image, in that order."""
        g = self.grid
        return g.A0 * u[:, 1:-1, 1:-1] + g.xk * (u[:, 1:-1, :-2] + u[:, 1:-1, 2:]) + g.yk * (u[:, :-2, 1:-1] + u[:, 2:, 1:-1])

    def verlet(self, u0, v0, gg, tau, nsteps):
        u, v, gi = self.image(u0), self.image(v0)[:, 1:-1, 1:-1].clone(), self.image(gg)[:, 1:-1, 1:-1]
        t = torch.from_numpy(tau).cuda().view(-1, 1, 1)
        h = 0.5 * t
        a = (self.au(u) - gi) * self.mask
        for _ in range(nsteps):
            v = v + h * a
            u[:, 1:-1, 1:-1] = u[:, 1:-1, 1:-1] + t * v
            a = (self.au(u) - gi) * self.mask
            v = v + h * a
        return self.packed(u)

    def newmark(self, handle, p, u0, v0, gg, tau, nsteps):
        t = torch.from_numpy(tau).cuda().view(-1, 1)
        sigma, hv = 4.0 / (t * t), 2.0 / t
        sd = sigma.view(-1).contiguous()
        u, v = u0, v0
        for _ in range(nsteps):
            w = u + t * v
            b = (gg + gg) - sigma * w
            b = b - self.packed_interior(self.au(self.image(u)))
            x, _res = handle.solve_many(p, b.contiguous(), x0=u, sigma=sd)
            v = hv * (x - u) - v
            u = x
        return u

    def packed_interior(self, interior):
        img = torch.zeros((self.nsys, self.n1, self.n1), dtype=torch.float64, device="cuda")
        img[:, 1:-1, 1:-1] = interior
        return self.packed(img)


def timed(fn, sync):
    if sync:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    if sync:
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def numpy_rows(fn):
    """(c): a warm-up is the first timed call itself when a call is slow."""
    ms, _ = timed(fn, False)
    t = [ms]
    while len(t) < TIMED and t[0] < C_REPEAT_BELOW_MS:
        t.append(timed(fn, False)[0])
    return t


def main(ns, resources, out_path):
    lines = ["# time to solution of ensembles of small wave-equation steppers u_tt = A u - g on one MI355X (tools/onchip_wave_timing.py).",
             f"# Verlet: {VERLET_STEPS} steps at tau = 0.5 x wave_cfl().  Newmark: {NEWMARK_STEPS} steps at sigma = 4 / tau^2 = 10 |A_diag|, REL_2NORM 1e-8.  Seeded (u0, v0),",
             "# g_s = the handle's right-hand side times (1 + 0.1 * seeded standard-normal numbers).  Domain (1, 2, 1, 2), default sync_every and steps_per_launch.",
             "# (a) mi355cg_wave_steps_many on device tensors; (b) without it on the same GPU -- Verlet: torch slicing on (nsys, N+1, N+1) images; Newmark: the",
             "# right-hand side and the velocity with torch, one solve_many(b, x0 = u, sigma) per step; (c) the NumPy model on one core (nsys <= 256).",
             f"# Per row: one warm-up, then {TIMED} timed calls of (a), then of (b); (c): {TIMED} timed calls where a call takes under {C_REPEAT_BELOW_MS / 1e3:.0f} s, otherwise ONE (c_n).",
             "# Nothing is scaled or extrapolated.  ms = wall time of all members' steps, median (min .. max); us_ms = median ms * 1000 / (nsys * steps), per",
             "# member-step; b=a: the final u of (b) and (a) agree bit for bit (otherwise the largest |difference|); b/a, c/a = ratio of the medians (above 1:",
             "# the new call is faster); tsm_us: us per member-step of time_steps_many at this N and nsys, sigma factor 10 / 0.03 (profiles/onchip_steps_time_to_solution.txt).",
             f"# {'scheme':<8} {'N':>4} {'nsys':>5} {'it/step':>7} | {'a_ms med':>9} {'min':>9} {'max':>9} {'us_ms':>8} | {'b_ms med':>10} {'min':>10} {'max':>10} {'us_ms':>8} {'b=a':>9} | "
             f"{'c_ms med':>10} {'min':>10} {'max':>10} {'c_n':>3} {'us_ms':>8} | {'b/a':>7} {'c/a':>7} {'tsm_us':>9}"]
    print("\n".join(lines), flush=True)
    p = isa.default_params(_capi.RULE_REL_2NORM)
    p.use_true_solution, p.eps_rel, p.max_iterations = 0, 1e-8, 1_000_000
    launch_lines = []
    for n in ns:
        os.environ.pop("MI355CG_ONCHIP", None)
        many = isa.MatrixFreeSystem(n, n, 1.0, 2.0, 1.0, 2.0)
        own = many.get_rhs()
        e0 = np.zeros(own.size)
        e0[0] = 1.0
        col = many.apply(e0)
        grid = W.Grid(n, col[0], col[1], col[n // 2 - 1])
        bound = many.wave_cfl()
        for nsys in (ENSEMBLES[:-1] + [1024] if n >= 128 else ENSEMBLES):           # at the cap a workgroup has a CU to itself: up to 1024
            rng = np.random.default_rng(1000 * n + nsys)
            g = own[None, :] * (1.0 + 0.1 * rng.standard_normal((nsys, own.size)))
            u0 = rng.standard_normal((nsys, own.size))
            v0 = rng.standard_normal((nsys, own.size)) * np.sqrt(abs(grid.A0))
            gd, ud, vd = (torch.from_numpy(a).cuda() for a in (g, u0, v0))
            ti = TorchImages(grid, nsys)
            for scheme, steps, tau in (("verlet", VERLET_STEPS, np.full(nsys, 0.5 * bound)),
                                       ("newmark", NEWMARK_STEPS, np.full(nsys, 2.0 / np.sqrt(10.0 * abs(grid.A0))))):
                verlet = scheme == "verlet"
                if verlet:
                    call_a = lambda: many.wave_steps_many(ud, vd, tau, steps, g=gd)
                    call_b = lambda: ti.verlet(ud, vd, gd, tau, steps)
                    call_c = lambda: W.verlet(grid, u0, v0, g, tau, steps)
                else:
                    call_a = lambda: many._handle.wave_steps_many(p, ud, vd, tau, steps, scheme=_capi.WAVE_NEWMARK, g=gd, step_iterations=True)
                    call_b = lambda: ti.newmark(many._handle, p, ud, vd, gd, tau, steps)
                    call_c = lambda: [W.newmark(grid, u0[s], v0[s], g[s], float(tau[s]), steps, tol=1e-8) for s in range(nsys)]
                _, ra = timed(call_a, True)                                         # the warm-up of both
                _, ub = timed(call_b, True)
                assert (ra[3] == steps).all() and all(r.converged == 1 for r in ra[2]), (scheme, n, nsys)
                its = 0.0 if verlet else float(ra[4].sum()) / (nsys * steps)
                agree = "yes" if torch.equal(ra[0], ub) else f"{float((ra[0] - ub).abs().max()):.1e}"
                ta = [timed(call_a, True)[0] for _ in range(TIMED)]
                tb = [timed(call_b, True)[0] for _ in range(TIMED)]
                tc = numpy_rows(call_c) if nsys <= C_MOST else []
                a, b_ = stats(ta), stats(tb)
                per = 1e3 / (nsys * steps)
                line = (f"  {scheme:<8} {n:>4} {nsys:>5} {its:>7.2f} | {a[0]:>9.3f} {a[1]:>9.3f} {a[2]:>9.3f} {a[0] * per:>8.3f} | "
                        f"{b_[0]:>10.3f} {b_[1]:>10.3f} {b_[2]:>10.3f} {b_[0] * per:>8.3f} {agree:>9} | ")
                if tc:
                    c = stats(tc)
                    line += f"{c[0]:>10.3f} {c[1]:>10.3f} {c[2]:>10.3f} {len(tc):>3} {c[0] * per:>8.3f} | {b_[0] / a[0]:>7.2f} {c[0] / a[0]:>7.2f}"
                else:
                    line += f"{'-':>10} {'-':>10} {'-':>10} {0:>3} {'-':>8} | {b_[0] / a[0]:>7.2f} {'-':>7}"
                line += f" {STEPS_MANY_US.get((n, nsys), '-'):>9}"
                lines.append(line)
                print(line, flush=True)
            if n == 128:                                                            # one launch of the default length: the latency of a stop request
                tau = np.full(nsys, 0.5 * bound)
                t = []
                for _ in range(TIMED + 1):
                    res = many.wave_steps_many(ud, vd, tau, DEFAULT_LAUNCH, g=gd, steps_per_launch=DEFAULT_LAUNCH)[2]
                    t.append(res[0].loop_seconds * 1e3)
                m = stats(t[1:])
                launch_lines.append(f"# one launch of {DEFAULT_LAUNCH} Verlet steps at N = {n}, nsys = {nsys}: {m[0]:.3f} ms device time, median of {TIMED} ({m[1]:.3f} .. {m[2]:.3f})")
                print(launch_lines[-1], flush=True)
        many._handle.close()
    lines += ["#"] + launch_lines
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
