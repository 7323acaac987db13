#!/usr/bin/env python3
"""Device-resident theta-scheme steps (mi355cg_time_steps) against the same steps through the host API, N = 4096, PRECOND_MG,
theta = 1 (implicit Euler), 20 steps, on one handle: one tau with sigma = 1 / tau about |diag| of the Laplacian and one with
sigma about 1e-3 |diag|.  The host loop does per step what a caller without the stepper has to do: b = g - sigma u in NumPy,
set_rhs(b), solve(x0 = u), get_solution.  Best of two runs of each, after one warm-up run.  Writes profiles/time_steps.txt (or the
path given as the first argument).  No threshold: the file records what came out."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import iterative_solvers_amd as isa  # noqa: E402

N, STEPS, THETA, EPS = 4096, 20, 1.0, 1e-8
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "time_steps.txt")


def params():
    p = isa.default_params(isa.RULE_REL_2NORM)
    p.eps_rel, p.max_iterations, p.use_true_solution = EPS, 1000, 0
    return p


def stepper(s, u0, tau):
    t0 = time.perf_counter()
    u, res, done = s.time_steps(u0, tau, THETA, STEPS, params=params())
    return time.perf_counter() - t0, u, [r.iterations for r in res], done


def host_loop(s, u0, g, tau):
    h = s._handle
    sigma = 1.0 / (THETA * tau)
    s.set_shift(sigma)
    u, its = u0, []
    t0 = time.perf_counter()
    for _ in range(STEPS):
        h.set_rhs(g - sigma * u)
        h.set_initial_guess(u)
        its.append(h.solve(params()).iterations)
        u = h.solution()
    dt = time.perf_counter() - t0
    h.set_rhs(g)
    return dt, u, its


def main():
    s = isa.MatrixFreeSystem(N, N, 1.0, 2.0, 1.0, 2.0)
    s.set_preconditioner(isa.PRECOND_MG)
    g = s.get_rhs()
    u0 = np.zeros(s.size())
    diag = 2.0 * (N * N + N * N)                                    # |A_diag| on the unit-step domain (1, 2) x (1, 2): 2 (x_k + y_k)
    lines = [f"mi355cg_time_steps against the host API, N = {N}, PRECOND_MG (fp64 cycle), theta = {THETA:g}, {STEPS} steps from u = 0, "
             f"REL_2NORM {EPS:g}, one handle, best of two after a warm-up run; |diag| = {diag:.4g}",
             f"packed vector: {8 * s.size() / 1e6:.1f} MB"]
    for name, frac in (("sigma ~ |diag|", 1.0), ("sigma ~ 1e-3 |diag|", 1e-3)):
        tau = 1.0 / (THETA * frac * diag)
        stepper(s, u0, tau)
        host_loop(s, u0, g, tau)
        best_dev, best_host = np.inf, np.inf
        for _ in range(2):
            dt, ud, its_d, done = stepper(s, u0, tau)
            best_dev = min(best_dev, dt)
            dt, uh, its_h = host_loop(s, u0, g, tau)
            best_host = min(best_host, dt)
        dev = float(np.abs(ud - uh).max() / np.abs(uh).max())
        lines.append(f"{name}: tau = {tau:.4g}, sigma = {s.shift:.4g}")
        lines.append(f"  stepper   {1e3 * best_dev:9.2f} ms for {done} steps ({1e3 * best_dev / STEPS:7.3f} ms a step, the upload of u0 and the download of u included), iterations {its_d}")
        lines.append(f"  host API  {1e3 * best_host:9.2f} ms for {STEPS} steps ({1e3 * best_host / STEPS:7.3f} ms a step), iterations {its_h}")
        lines.append(f"  host / stepper = {best_host / best_dev:.2f}; max|u_stepper - u_host| / max|u_host| = {dev:.2e}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
