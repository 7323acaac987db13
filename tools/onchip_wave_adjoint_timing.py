"""Time to solution of the adjoint of the recorded explicit on-chip wave stepper in a medium (mi355cg_wave_history_many,
mi355cg_wave_adjoint_many, wave_gradient_many) on one MI355X.

The rows, the ensembles and the inputs are tools/onchip_wave_medium_timing.py's: for every N and ensemble size nsys, nsys members
in seeded media c2_s in [0.25, 4], each at tau_s = 0.5 x its own bound, seeded (u0, v0), g_s = the handle's right-hand side times
(1 + 0.1 * seeded noise), a Ricker wavelet for all, 16 seeded receivers sampled at every step; the observed traces are those of the
medium 0.9 c2 + 0.1.  Per row, in a child process of its own, one warm-up and then five timed calls of each of
  (1)  200 steps: (f) wave_record_many(c2=), the forward step; (h) wave_history_many, the forward step that writes its history;
       (b) wave_adjoint_many on that history, the backward step.  us = median ms * 1000 / (nsys * steps), per member-step.  At
       N = 128 the bytes of history the backward run reads, per second, against the copy ceiling of profiles/r03_copy_ceiling.txt.
  (2)  1000 steps: (g) wave_gradient_many with segment=None where the history is at most HISTORY_LIMIT bytes, (s) with
       segment=100; (t) the same gradient by the adjoint recurrence written with torch slicing on (nsys, N+1, N+1) images, in
       segments of 100 from the same checkpoints, whose misfit-free results grad_c2, grad_u0, grad_v0 and traces are compared
       with (s)'s bit for bit, and that is the check; the arithmetic bound of the gradient by differences, size + 1 forward runs,
       computed from (f)'s time per member-step and not run.
  (3)  with --baseline-tree (a built checkout of the parent commit): wave_record_many with c2, and with c2 and damping, 1000
       steps, of this build and of the parent's, each in a child process on the same GPU, taking turns call by call.  ok: this
       build's median is not above the parent's slowest call of five; a row that is above is reported as NO.
Every row runs in a child process under a time limit; the tool stops at the first failure.  Nothing is scaled.

       python tools/onchip_wave_adjoint_timing.py [--baseline-tree DIR] [--out FILE] [N ...]
                                                   (default 10 32 128; writes profiles/onchip_wave_adjoint_time_to_solution.txt)"""
import json
import os
import select
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "onchip_wave_adjoint_time_to_solution.txt")
SIZES = [10, 32, 128]
ENSEMBLES = [1, 256, 4096]
STEPS, SHORT, SEGMENT, RECEIVERS = 1000, 200, 100, 16
TIMED = 5
HISTORY_LIMIT = 32 << 30                                                 # bytes: segment=None is run where the whole history is at most this
COPY_CEILING_GBS = None                                                  # read from profiles/r03_copy_ceiling.txt when it is there
ROW_LIMIT, CALL_LIMIT = 420, 60
sys.path.insert(0, os.environ.get("ONCHIP_WAVE_ADJOINT_TREE") or ROOT)   # a worker of --baseline-tree imports that checkout's package
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


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
    return ENSEMBLES[:-1] + [1024] if n >= 128 else ENSEMBLES         # at the cap a workgroup has a CU to itself: up to 1024


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


class TorchAdjoint:
    """The gradient with torch slicing on images: the forward scheme that keeps au(u), and the transpose of its steps."""

    def __init__(self, images, tau, receivers):
        import torch
        self.ti, self.nsys = images, images.nsys
        self.t = torch.from_numpy(tau).cuda().view(-1, 1, 1)
        self.h = 0.5 * self.t
        self.rc = images.cells[torch.tensor(receivers, device="cuda")]

    def forward(self, u, v, gi, ci, w, keep):
        """k = len(w) - 1 steps on the image u (in place) and the interior v: (v, traces [nsys, k, nrec], H or None)."""
        import torch
        ti = self.ti
        flat = u.view(self.nsys, -1)
        traces = torch.empty((self.nsys, len(w) - 1, len(self.rc)), dtype=torch.float64, device="cuda")
        t = ti.au(u) * ti.mask
        H = [t] if keep else None
        a = (ci * t - float(w[0]) * gi) * ti.mask
        for n in range(len(w) - 1):
            v = v + self.h * a
            u[:, 1:-1, 1:-1] = u[:, 1:-1, 1:-1] + self.t * v
            t = ti.au(u) * ti.mask
            if keep:
                H.append(t)
            a = (ci * t - float(w[n + 1]) * gi) * ti.mask
            v = v + self.h * a
            traces[:, n, :] = flat[:, self.rc]
        return v, traces, H

    def backward(self, H, ci, r, lam, q, S):
        """The transpose of the len(H) - 1 steps: lam, q images (q's border stays zero), S interior; r [nsys, k, nrec], every step sampled."""
        ti = self.ti
        lflat = lam.view(self.nsys, -1)
        for s in range(len(H) - 1, 0, -1):
            for j in range(len(self.rc)):                            # ascending, one at a time: duplicates would add in this order
                lflat[:, self.rc[j]] = lflat[:, self.rc[j]] + r[:, s - 1, j]
            S = S + q[:, 1:-1, 1:-1] * H[s]
            lam[:, 1:-1, 1:-1] = lam[:, 1:-1, 1:-1] + self.h * (ti.au(q) * ti.mask)
            q[:, 1:-1, 1:-1] = q[:, 1:-1, 1:-1] + self.t * (ci * lam[:, 1:-1, 1:-1])
            S = S + q[:, 1:-1, 1:-1] * H[s - 1]
            lam[:, 1:-1, 1:-1] = lam[:, 1:-1, 1:-1] + self.h * (ti.au(q) * ti.mask)
        return S

    def gradient(self, u0, v0, gg, c2, w, observed, segment):
        import torch
        ti = self.ti
        gi, ci = ti.image(gg)[:, 1:-1, 1:-1], ti.image(c2)[:, 1:-1, 1:-1]
        u, v = ti.image(u0), ti.image(v0)[:, 1:-1, 1:-1].clone()
        steps = len(w) - 1
        cuts = [(a, min(segment, steps - a)) for a in range(0, steps, segment)]
        starts, parts = [], []
        for a, k in cuts:                                            # forward: the checkpoints and the traces
            starts.append((u.clone(), v))
            v, tr, _ = self.forward(u, v, gi, ci, w[a:a + k + 1], False)
            parts.append(tr)
        traces = torch.cat(parts, dim=1)
        r = traces - observed
        lam, q = torch.zeros_like(u), torch.zeros_like(u)
        S = torch.zeros_like(v)
        for (a, k), (us, vs) in zip(reversed(cuts), reversed(starts)):
            _, _, H = self.forward(us, vs, gi, ci, w[a:a + k + 1], True)
            S = self.backward(H, ci, r[:, a:a + k], lam, q, S)
        pack = lambda img: img.reshape(self.nsys, -1)[:, ti.cells].contiguous()
        full = lambda x: torch.nn.functional.pad(x, (1, 1, 1, 1))
        return self.h.view(-1, 1) * pack(full(S)) / c2, pack(lam), pack(q) / c2, traces


def row(n, nsys):
    """Child process of (1) and (2): one row, one JSON line out."""
    import torch
    import iterative_solvers_amd as isa
    import onchip_wave_medium_timing as MT
    many, grid, gd, ud, vd, cd, c2, receivers = MT.inputs(n, nsys)
    tau = 0.5 * np.atleast_1d(many.wave_cfl(c2))
    w = MT.ricker(STEPS)
    wd, ws = torch.from_numpy(w).cuda(), torch.from_numpy(np.ascontiguousarray(w[:SHORT + 1])).cuda()
    # (1) the three steps
    call_f = lambda: many.wave_record_many(ud, vd, tau, SHORT, ws, g=gd, receivers=receivers, c2=cd)
    call_h = lambda: many.wave_history_many(ud, vd, tau, SHORT, ws, g=gd, receivers=receivers, c2=cd)
    _, rf = timed(call_f)
    _, rh = timed(call_h)
    assert all(torch.equal(a, b) for a, b in zip(rf[:3], rh[:3])), "the history call changes the forward run"
    hist = rh[3]
    adj = torch.from_numpy(np.random.default_rng(7 * n + nsys).standard_normal((nsys, SHORT, RECEIVERS))).cuda()
    call_b = lambda: many.wave_adjoint_many(hist, tau, cd, adj, receivers=receivers)
    timed(call_b)
    f, h, b = (stats([timed(fn)[0] for _ in range(TIMED)]) for fn in (call_f, call_h, call_b))
    del hist, rh, rf
    # (2) the gradient
    observed = many.wave_record_many(ud, vd, tau, STEPS, wd, g=gd, receivers=receivers, c2=0.9 * cd + 0.1)[2]
    whole_fits = isa.wave_history_bytes(n, nsys, STEPS) <= HISTORY_LIMIT
    call_s = lambda: many.wave_gradient_many(ud, vd, tau, STEPS, wd, observed, g=gd, receivers=receivers, c2=cd, segment=SEGMENT)
    call_g = lambda: many.wave_gradient_many(ud, vd, tau, STEPS, wd, observed, g=gd, receivers=receivers, c2=cd)
    ta = TorchAdjoint(MT.TorchImages(grid, nsys), tau, receivers)
    call_t = lambda: ta.gradient(ud, vd, gd, cd, w, observed, SEGMENT)
    _, rs = timed(call_s)
    _, rt = timed(call_t)
    agree = all(bool(torch.equal(x, y)) for x, y in zip(rs[1:], rt))
    finite = all(bool(torch.isfinite(x).all()) for x in rs)
    g = None
    if whole_fits:
        _, rg = timed(call_g)
        agree = agree and all(bool(torch.equal(x, y)) for x, y in zip(rs, rg))
        del rg
        g = stats([timed(call_g)[0] for _ in range(TIMED)])
    s, t = (stats([timed(fn)[0] for _ in range(TIMED)]) for fn in (call_s, call_t))
    print("ROW " + json.dumps(dict(f=f, h=h, b=b, g=g, s=s, t=t, agree=agree, finite=finite, size=many.size())), flush=True)


def worker():
    """Child process of (3): the two existing calls of the package this process imports.  One line in ("N nsys kind"), one JSON line out."""
    import torch
    import iterative_solvers_amd                                     # this process's tree, before the other tool puts its own in front
    import onchip_wave_medium_timing as MT
    assert os.path.realpath(iterative_solvers_amd.__file__).startswith(os.path.realpath(os.environ.get("ONCHIP_WAVE_ADJOINT_TREE") or ROOT))
    rows = {}
    print("READY", flush=True)
    for ln in sys.stdin:
        f = ln.split()
        if not f or f[0] == "quit":
            break
        key = (int(f[0]), int(f[1]))
        if key not in rows:
            many, _, gd, ud, vd, cd, c2, receivers = MT.inputs(*key)
            dd = torch.from_numpy(many.sponge_damping(max(2, key[0] // 8), 1.0)).cuda()
            rows = {key: (many, gd, ud, vd, cd, dd, receivers, 0.5 * np.atleast_1d(many.wave_cfl(c2)), torch.from_numpy(MT.ricker(STEPS)).cuda())}
        many, gd, ud, vd, cd, dd, receivers, tau, wd = rows[key]
        extra = dict(c2=cd, damping=dd) if f[2] == "sponge" else dict(c2=cd)
        ms, out = timed(lambda: many.wave_record_many(ud, vd, tau, STEPS, wd, g=gd, receivers=receivers, **extra))
        assert (out[4] == STEPS).all()
        print("R " + json.dumps(ms), flush=True)


# ---- no GPU from here on ---------------------------------------------------------------------------------------------------------------
def copy_ceiling():
    """The read rate of profiles/r03_copy_ceiling.txt in GB/s (the backward run streams its history in), or None."""
    import re
    path = os.path.join(ROOT, "profiles", "r03_copy_ceiling.txt")
    if not os.path.exists(path):
        return None
    rates = [float(m.group(1)) for m in re.finditer(r"^\s*read\s+1 float4/thread\s.*?->\s*([0-9.]+) GB/s", open(path).read(), re.M)]
    return rates[-1] if rates else None                              # the median of the plain read stream at the largest size


def answer(child, limit):
    ready, _, _ = select.select([child.stdout], [], [], limit)
    return child.stdout.readline() if ready else None


def main(ns, baseline_tree, out_path):
    fmt = lambda x: f"{x[0]:>9.3f} {x[1]:>9.3f} {x[2]:>9.3f}"
    ceiling = COPY_CEILING_GBS or copy_ceiling()
    head1 = [f"# the adjoint of the recorded explicit wave stepper in a medium on one MI355X (tools/onchip_wave_adjoint_timing.py).  The rows and inputs of",
             f"# tools/onchip_wave_medium_timing.py: members in seeded media at 0.5 x their own bound, a Ricker wavelet, {RECEIVERS} receivers sampled at every step, domain (1, 2, 1, 2),",
             f"# default steps_per_launch.  Per row, in a child process of its own: one warm-up, then {TIMED} timed calls of each; ms = wall time, median (min .. max).",
             f"# (1) {SHORT} steps.  (f) wave_record_many(c2=); (h) wave_history_many; (b) wave_adjoint_many on that history.  us = median ms * 1000 / (nsys * {SHORT}), per member-step.",
             f"#     GB/s = the history (b) reads, 8 * size * nsys * {SHORT} bytes, over its median" + (f"; of_copy = that over the read stream of profiles/r03_copy_ceiling.txt at 4 GiB, {ceiling:.0f} GB/s." if ceiling else "."),
             f"# {'N':>4} {'nsys':>5} | {'f_ms med':>9} {'min':>9} {'max':>9} {'f_us':>7} | {'h_ms med':>9} {'min':>9} {'max':>9} {'h_us':>7} | {'b_ms med':>9} {'min':>9} {'max':>9} {'b_us':>7} | {'h/f':>5} {'b/f':>5} {'GB/s':>7} {'of_copy':>7}"]
    head2 = ["#",
             f"# (2) {STEPS} steps.  (g) wave_gradient_many, segment=None (-: the history of the row is above {HISTORY_LIMIT >> 30} GiB, not run); (s) segment={SEGMENT}; (t) the same gradient with torch",
             f"#     slicing on images, segments of {SEGMENT}; t=s: grad_c2, grad_u0, grad_v0 and the traces of (t), and all of (g), agree with (s)'s bit for bit.  fd_ms = (size + 1) forward runs of",
             f"#     {STEPS} steps at (f)'s time per member-step: the gradient with respect to c2 by one-sided differences, computed, not run.",
             f"# {'N':>4} {'nsys':>5} | {'g_ms med':>9} {'min':>9} {'max':>9} | {'s_ms med':>9} {'min':>9} {'max':>9} | {'t_ms med':>10} {'min':>10} {'max':>10} {'t=s':>4} | {'t/s':>7} {'fd_ms':>12} {'fd/s':>8}"]
    print("\n".join(head1), flush=True)
    env = dict(os.environ)
    env.pop("MI355CG_ONCHIP", None)
    env.pop("MI355CG_LIB", None)
    failed = None
    rows1, rows2 = [], []
    for n in ns:
        for nsys in ensembles(n):
            try:
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--row", str(n), str(nsys)], env=env, capture_output=True, text=True, timeout=ROW_LIMIT)
            except subprocess.TimeoutExpired:
                failed = f"row N = {n}, nsys = {nsys}: no result within {ROW_LIMIT} s"
                break
            got = [ln for ln in out.stdout.splitlines() if ln.startswith("ROW ")]
            if out.returncode != 0 or not got:
                failed = f"row N = {n}, nsys = {nsys}: exit status {out.returncode}: {out.stderr[-600:]!r}"
                break
            r = json.loads(got[0][4:])
            us = lambda x: x[0] * 1e3 / (nsys * SHORT)
            gbs = 8.0 * r["size"] * nsys * SHORT / (r["b"][0] * 1e-3) / 1e9
            rows1.append(f"  {n:>4} {nsys:>5} | {fmt(r['f'])} {us(r['f']):>7.3f} | {fmt(r['h'])} {us(r['h']):>7.3f} | {fmt(r['b'])} {us(r['b']):>7.3f} | "
                         f"{r['h'][0] / r['f'][0]:>5.2f} {r['b'][0] / r['f'][0]:>5.2f} {gbs:>7.1f} {(f'{gbs / ceiling:.3f}' if ceiling else '-'):>7}")
            fd = (r["size"] + 1) * us(r["f"]) * nsys * STEPS * 1e-3
            gtxt = fmt(r["g"]) if r["g"] else f"{'-':>9} {'-':>9} {'-':>9}"
            rows2.append(f"  {n:>4} {nsys:>5} | {gtxt} | {fmt(r['s'])} | {r['t'][0]:>10.3f} {r['t'][1]:>10.3f} {r['t'][2]:>10.3f} {'yes' if r['agree'] else 'NO':>4} | "
                         f"{r['t'][0] / r['s'][0]:>7.2f} {fd:>12.1f} {fd / r['s'][0]:>8.1f}")
            print(rows1[-1] + "\n" + rows2[-1], flush=True)
            if not r["agree"] or not r["finite"]:
                failed = f"row N = {n}, nsys = {nsys}: the gradients differ or are not finite"
                break
        if failed:
            break
    lines = head1 + rows1 + head2 + rows2

    if baseline_tree and not failed:
        trees = {"this": ROOT, "parent": os.path.abspath(baseline_tree)}
        children = {}
        for name, tree in trees.items():
            children[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], env=dict(env, ONCHIP_WAVE_ADJOINT_TREE=tree, ONCHIP_WAVE_MEDIUM_TREE=tree),
                                              stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            if (answer(children[name], CALL_LIMIT) or "").strip() != "READY":
                failed = f"(3): the worker of {name} did not start"

        def call(name, n, nsys, kind):
            child = children[name]
            child.stdin.write(f"{n} {nsys} {kind}\n")
            child.stdin.flush()
            ln = answer(child, CALL_LIMIT)
            return json.loads(ln[2:]) if ln and ln.startswith("R ") else None

        lines += ["#", f"# (3) the existing calls, {STEPS} steps, {RECEIVERS} receivers: wave_record_many with c2 (medium) and with c2 and damping (sponge), this build and the parent commit,",
                  "#     each in a child process, taking turns call by call.",
                  f"# {'N':>4} {'nsys':>5} {'call':>7} | {'this_ms med':>11} {'min':>9} {'max':>9} | {'parent_ms med':>13} {'min':>9} {'max':>9} | {'this med <= parent max':>22}"]
        all_ok = True
        for n in ns:
            for nsys in ensembles(n):
                for kind in ("medium", "sponge"):
                    mine, base = [], []
                    for k in range(TIMED + 1):                           # k = 0: the warm-up of both
                        m = call("this", n, nsys, kind) if not failed else None
                        b = call("parent", n, nsys, kind) if m is not None else None
                        if m is None or b is None:
                            failed = failed or f"(3) N = {n}, nsys = {nsys}: a worker gave no answer within {CALL_LIMIT} s"
                            break
                        if k:
                            mine.append(m)
                            base.append(b)
                    if failed:
                        break
                    m, b = stats(mine), stats(base)
                    ok = m[0] <= b[2]
                    all_ok = all_ok and ok
                    lines.append(f"  {n:>4} {nsys:>5} {kind:>7} | {m[0]:>11.3f} {m[1]:>9.3f} {m[2]:>9.3f} | {b[0]:>13.3f} {b[1]:>9.3f} {b[2]:>9.3f} | {'yes' if ok else 'NO':>22}")
                    print(lines[-1], flush=True)
                if failed:
                    break
            if failed:
                break
        for child in children.values():
            if failed:
                child.kill()
            else:
                child.stdin.write("quit\n")
                child.stdin.flush()
            child.wait(timeout=60)
        if not failed:
            lines.append(f"# this build's median is not above the parent's slowest call in every row: {'yes' if all_ok else 'NO'}")
    elif not baseline_tree:
        lines += ["#", "# (3) no --baseline-tree: the parent commit not measured"]
    if failed:
        lines.append("# STOPPED at the first failure: " + failed)
        print(lines[-1], flush=True)
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
