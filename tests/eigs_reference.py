"""A NumPy restatement of the block eigensolver (include/mi355cg.h, mi355cg_eigs) on top of the multigrid
restatement of tests/mg_model.py: K = -A, T = -M (one V-cycle), a locally optimal block
preconditioned iteration with soft locking, and the Rayleigh-Ritz step exactly as the header states it.  tests/test_eigs_cpu.py
checks it against the dense operator; tests/test_gpu_eigs.py bounds the device's iteration counts by its own."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model as ref  # noqa: E402

CONVERGED, ITERATIONS, INTERRUPTED, BREAKDOWN = range(4)


def levels_for(N, dom=(1.0, 2.0, 1.0, 2.0)):
    """The hierarchy MI355CG_PRECOND_MG_ANY builds (where MI355CG_PRECOND_MG has one it is the same)."""
    a, b, c, d = dom
    return ref.hierarchy_any(N, (b - a) / N, (d - c) / N)


def apply_K(levels, v):
    L = levels[0]
    return -ref.packed(L, ref.apply_A(L, ref.grid(L, v)))


def apply_T(levels, r):
    return -ref.apply_M(levels, r)


def dense_K(levels):
    n = int(levels[0].mask.sum())
    K = np.empty((n, n))
    e = np.zeros(n)
    for j in range(n):
        e[j] = 1.0
        K[:, j] = apply_K(levels, e)
        e[j] = 0.0
    return K


def rayleigh_ritz(G, H):
    """(theta ascending, C) with C.T G C = I, C.T H C = diag(theta), or None for a refused basis."""
    G, H = 0.5 * (G + G.T), 0.5 * (H + H.T)
    g = np.diag(G)
    if not (np.all(np.isfinite(g)) and np.all(g > 0)):
        return None
    d = 1.0 / np.sqrt(g)
    Gs, Hs = d[:, None] * G * d[None, :], d[:, None] * H * d[None, :]
    if not (np.all(np.isfinite(Gs)) and np.all(np.isfinite(Hs))):
        return None
    try:
        L = np.linalg.cholesky(Gs)
    except np.linalg.LinAlgError:
        return None
    if np.diag(L).min() < 1e-6:
        return None
    Li = np.linalg.inv(L)
    M = Li @ Hs @ Li.T
    theta, Y = np.linalg.eigh(0.5 * (M + M.T))
    return theta, d[:, None] * (Li.T @ Y)


def lobpcg(levels, X0, nev, tol=1e-8, max_iterations=200, stop=False):
    """X0: [m, size] start block.  Returns (theta[m], X[m, size], info) with info = dict(iterations, converged, stop_reason,
    p_drops, residuals)."""
    m = X0.shape[0]
    X = X0.T.copy()                                                 # columns
    KX = np.stack([apply_K(levels, X[:, j]) for j in range(m)], axis=1)
    info = dict(iterations=0, converged=False, stop_reason=ITERATIONS, p_drops=0, residuals=np.full(m, np.inf))
    rr = rayleigh_ritz(X.T @ X, X.T @ KX)
    if rr is None:
        info["stop_reason"] = BREAKDOWN
        return np.zeros(m), X0.copy(), info
    theta, C = rr
    X, KX = X @ C, KX @ C
    P = KP = None
    it = 0
    while True:
        R = KX - X * theta[None, :]
        res = np.linalg.norm(R, axis=0) / (theta * np.linalg.norm(X, axis=0))
        info["residuals"] = res
        if np.all(res[:nev] <= tol):
            info["converged"], info["stop_reason"] = True, CONVERGED
            break
        if it >= max_iterations:
            info["stop_reason"] = ITERATIONS
            break
        if stop:
            info["stop_reason"] = INTERRUPTED
            break
        act = np.flatnonzero(~(res <= tol))
        W = np.stack([apply_T(levels, R[:, j]) for j in act], axis=1)
        W = W - X @ (X.T @ W)
        KW = np.stack([apply_K(levels, W[:, k]) for k in range(W.shape[1])], axis=1)
        S, KS = [X, W], [KX, KW]
        if P is not None:
            S.append(P[:, act])
            KS.append(KP[:, act])
        S, KS = np.concatenate(S, axis=1), np.concatenate(KS, axis=1)
        rr = rayleigh_ritz(S.T @ S, S.T @ KS)
        if rr is None and P is not None:
            info["p_drops"] += 1
            k2 = m + act.size
            S, KS = S[:, :k2], KS[:, :k2]
            rr = rayleigh_ritz(S.T @ S, S.T @ KS)
        if rr is None:
            info["stop_reason"] = BREAKDOWN
            break
        th, C = rr
        C = C[:, :m]
        C0 = C.copy()
        C0[:m] = 0.0
        X, KX, P, KP = S @ C, KS @ C, S @ C0, KS @ C0
        theta = th[:m]
        it += 1
    info["iterations"] = it
    return theta, X.T.copy(), info
