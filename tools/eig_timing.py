#!/usr/bin/env python3
"""Time to solution of the lowest eigenpairs on one MI355X: mi355cg_eigs_device (the block multigrid-preconditioned iteration,
DESIGN section 10.7) against what a caller could do before it existed: block inverse iteration through
mi355cg_solve_batch_device_from, the block kept in device memory as a torch tensor, K X by mi355cg_apply_device per column, the
Gram matrices by torch on the device and the Rayleigh-Ritz step in NumPy on the host, run to the same relative residual.

  N = 258, 1000, 4096; (nev, block) = (6, 8), (12, 16); tol 1e-8; MG_ANY, fp64 cycle; the same seeded standard-normal start block
  the inner solves of the baseline warm-start from X / theta and stop at REL_2NORM eps = 0.01 x the smallest residual that has
  not converged yet (at most 1e-2): about two digits per outer iteration, the cheapest setting that still converges
  each side: one warm-up (the same call cut after two iterations: it allocates the workspaces), then one timed run

Usage: python tools/eig_timing.py [out.txt]                 the table (default profiles/eigs_time_to_solution.txt)
       python tools/eig_timing.py --one N                   one solve of nev 12 / block 16 at N, for a kernel trace
       python tools/eig_timing.py --summarise DIR [out.txt] per-kernel totals of a rocprofv3 --kernel-trace run of --one
No threshold: the file records what came out."""
import csv
import glob
import os
import re
import sys
import time
from collections import defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DOM = (1.0, 2.0, 1.0, 2.0)
TOL = 1e-8
GRIDS = (258, 1000, 4096)
CASES = ((6, 8), (12, 16))


def system(N):
    import iterative_solvers_amd as isa
    s = isa.MatrixFreeSystem(N, N, *DOM)
    s.set_preconditioner(isa.PRECOND_MG_ANY)
    return s


def start(s, block):
    import torch
    return torch.from_numpy(np.random.default_rng(0).standard_normal((block, s.size()))).cuda()


def eigs(s, x0, nev, max_iterations=200):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lam, V, info = s.eigs(nev, block=x0.shape[0], tol=TOL, max_iterations=max_iterations, x0=x0)
    return time.perf_counter() - t0, lam, info


def whitened_ritz(G, H):
    d = 1 / np.sqrt(np.diag(G))
    L = np.linalg.cholesky(d[:, None] * (0.5 * (G + G.T)) * d[None, :])
    Li = np.linalg.inv(L)
    M = Li @ (d[:, None] * (0.5 * (H + H.T)) * d[None, :]) @ Li.T
    theta, Y = np.linalg.eigh(0.5 * (M + M.T))
    return theta, d[:, None] * (Li.T @ Y)


def inverse_iteration(s, x0, nev, max_outer=400):
    """(seconds, lambda[nev], outer iterations, inner PCG iterations in total, converged)"""
    import iterative_solvers_amd as isa
    import torch
    h = s._handle
    lib = h._lib
    p = isa.default_params(isa.RULE_REL_2NORM)
    p.max_iterations, p.use_true_solution = 1000, 0
    X = x0.clone()
    KX = torch.empty_like(X)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    outer = inner = 0
    while True:
        torch.cuda.synchronize()                                         # the library works on its own stream
        for j in range(X.shape[0]):
            isa._capi.check(lib.mi355cg_apply_device(h._h, X[j].data_ptr(), KX[j].data_ptr()))
        KX.neg_()
        theta, Cm = whitened_ritz((X @ X.T).cpu().numpy(), (X @ KX.T).cpu().numpy())
        Ct = torch.from_numpy(np.ascontiguousarray(Cm.T)).cuda()
        X, KX = Ct @ X, Ct @ KX
        th = torch.from_numpy(theta).cuda()
        res = (torch.linalg.norm(KX - th[:, None] * X, dim=1) / (th * torch.linalg.norm(X, dim=1))).cpu().numpy()
        if np.all(res[:nev] <= TOL) or outer >= max_outer:
            break
        todo = res[res > TOL]
        p.eps_rel = min(1e-2, 0.01 * float(todo.min()))
        guess = (X / th[:, None]).contiguous()
        Y, results = h.solve_batch(p, (-X).contiguous(), x0=guess)       # A y = -x, i.e. K y = x
        inner += sum(r.iterations for r in results)
        X = Y
        KX = torch.empty_like(X)
        outer += 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0, theta[:nev], outer, inner, bool(np.all(res[:nev] <= TOL))


def table(out_path):
    lines = ["# time to solution of the lowest eigenpairs on one MI355X (tools/eig_timing.py): mi355cg_eigs_device against block inverse iteration",
             "# through mi355cg_solve_batch_device_from (block in device memory, K X by mi355cg_apply_device, Gram matrices by torch on the",
             "# device, Rayleigh-Ritz in NumPy), both to a relative residual of 1e-8 for the first nev pairs; MG_ANY, fp64 cycle, the same seeded",
             "# start block; inner solves of the baseline: warm start X / theta, REL_2NORM eps = min(1e-2, 0.01 x smallest unconverged residual)",
             "# each side: one warm-up (the same call cut after two iterations), then one timed run; eigs_ms = wall time of the Python call",
             "# around mi355cg_eigs_device, which clones the start block on the device; ratio = eigs_ms / inv_ms",
             "#     N nev block eigs_its p_drops   eigs_ms inv_outer inv_inner     inv_ms   ratio  max|lam_eigs - lam_inv| / lam"]
    for N in GRIDS:
        s = system(N)
        for nev, block in CASES:
            x0 = start(s, block)
            eigs(s, x0, nev, max_iterations=2)
            inverse_iteration(s, x0, nev, max_outer=2)
            t_e, lam, info = eigs(s, x0, nev)
            t_i, lam_i, outer, inner, conv = inverse_iteration(s, x0, nev)
            dev = float(np.abs(lam - lam_i).max() / lam.max())
            lines.append(f"{N:7d} {nev:3d} {block:5d} {info['iterations']:8d} {info['p_drops']:7d} {1e3 * t_e:9.2f} {outer:9d} {inner:9d} {1e3 * t_i:10.2f} "
                         f"{t_e / t_i:7.3f}  {dev:.2e}{'' if info['converged'] else '  (eigs did not converge)'}{'' if conv else '  (inverse iteration did not converge)'}")
            print(lines[-1], flush=True)
            del x0
        s.eigs_release()
        s.batch_release()
        del s
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print(text, end="")


def one(N):
    s = system(N)
    x0 = start(s, 16)
    t, lam, info = eigs(s, x0, 12)
    print(f"N = {N}, nev 12, block 16: {info['iterations']} iterations, {1e3 * t:.2f} ms, lambda_1 = {lam[0]:.10g}")


def summarise(d, out_path):
    dur = defaultdict(list)
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f, newline="") as fh:
            for row in csv.DictReader(fh):
                m = re.search(r"\bk_[a-z0-9_]+", row["Kernel_Name"])
                dur[m.group(0) if m else row["Kernel_Name"][:40]].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    total = sum(sum(v) for v in dur.values())
    lines = ["# rocprofv3 --kernel-trace of one mi355cg_eigs_device solve (tools/eig_timing.py --one: nev 12, block 16, tol 1e-8, MG_ANY), per kernel",
             f"{'kernel':24s} {'launches':>8s} {'avg_us':>10s} {'total_ms':>10s} {'share':>7s}"]
    for k, v in sorted(dur.items(), key=lambda kv: -sum(kv[1])):
        lines.append(f"{k:24s} {len(v):8d} {sum(v) / len(v):10.2f} {sum(v) / 1e3:10.3f} {100 * sum(v) / total:6.1f}%")
    block = sum(sum(v) for k, v in dur.items() if k.startswith("k_eig_"))
    lines.append(f"# k_eig_* (gram, reduce, combine, resid): {100 * block / total:.1f}% of {total / 1e3:.3f} ms of kernel time")
    text = "\n".join(lines) + "\n"
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--one":
        one(int(sys.argv[2]))
    elif len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else None)
    else:
        table(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "eigs_time_to_solution.txt"))
