"""A NumPy model of the adjoint of the recorded explicit wave stepper in a medium (csrc/onchip_plan.h): the
forward run that keeps its history H[n] = au(u_n), and the exact transpose of the scheme, every expression written operation by
operation in the kernels' order, so that a GPU result can be compared with np.array_equal.  Not a test module:
tests/test_onchip_wave_adjoint_cpu.py checks the model's own properties, tests/test_gpu_wave_adjoint.py compares the kernels with
it.  The grid is tests/wave_reference.py's."""
import numpy as np

from wave_reference import Grid  # noqa: F401  (the model's grid, for the callers too)


def _members(u, tau, w, nsteps):
    if u.ndim == 2:
        tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (len(u),))[:, None]
        w = np.broadcast_to(w, (len(u), nsteps + 1))
        return tau, (lambda n: w[:, n][:, None])
    assert w.ndim == 1
    return tau, (lambda n: w[n])


def verlet_history(grid, u, v, g, c2, tau, nsteps, source, receivers=(), record_every=1):
    """wave_medium_reference.verlet_medium with the history: (u, v, traces, H), H [..., nsteps + 1, size] with H[n] = au(u_n), the
    stencil value t of the state after n steps before a = c2 * t - f scales it."""
    u, v = np.array(u, dtype=np.float64), np.array(v, dtype=np.float64)
    w = np.asarray(source, dtype=np.float64)
    c2 = np.asarray(c2, dtype=np.float64)
    assert w.shape[-1] == nsteps + 1 and record_every >= 1 and c2.shape in (u.shape, u.shape[-1:])
    receivers = np.asarray(receivers, dtype=np.int64).reshape(-1)
    tau, amplitude = _members(u, tau, w, nsteps)
    h = 0.5 * tau
    f = amplitude(0) * g
    t = grid.au(u)
    rows = [t]
    a = c2 * t - f
    samples = []
    for n in range(nsteps):
        vh = v + h * a
        u = u + tau * vh
        f = amplitude(n + 1) * g
        t = grid.au(u)
        rows.append(t)
        a = c2 * t - f
        v = vh + h * a
        if (n + 1) % record_every == 0:
            samples.append(u[..., receivers])
    traces = np.stack(samples, axis=-2) if samples else np.zeros(u.shape[:-1] + (0, len(receivers)))
    return u, v, traces, np.stack(rows, axis=-2)


def adjoint(grid, H, c2, tau, adj, receivers=(), record_every=1, lam=None, q=None, S=None):
    """The transpose of nsteps = H.shape[-2] - 1 steps, from state index s = nsteps down to 1: (lam, q, S).
    H: [nsteps + 1, size] with a scalar tau, or [members, nsteps + 1, size] with tau [members] (or a scalar); c2 [size] or
    [members, size]; adj [..., nsteps // record_every, len(receivers)], row j the adjoint source of the sample after step
    (j + 1) * record_every; lam, q, S: the incoming state, None = zeros.  With h = 0.5 tau:
        if s % record_every == 0:  lam[rec[j]] = lam[rec[j]] + adj[s / record_every - 1][j],  j ascending
        S = S + q H[s];  lam = lam + h au(q);  q = q + tau (c2 lam);  S = S + q H[s - 1];  lam = lam + h au(q)"""
    H = np.asarray(H, dtype=np.float64)
    nsteps = H.shape[-2] - 1
    shape = H.shape[:-2] + H.shape[-1:]
    c2 = np.asarray(c2, dtype=np.float64)
    receivers = np.asarray(receivers, dtype=np.int64).reshape(-1)
    adj = np.asarray(adj, dtype=np.float64)
    assert record_every >= 1 and c2.shape in (shape, shape[-1:])
    assert len(receivers) == 0 or adj.shape[-2:] == (nsteps // record_every, len(receivers))
    lam, q, S = (np.zeros(shape) if a is None else np.array(a, dtype=np.float64) for a in (lam, q, S))
    assert lam.shape == q.shape == S.shape == shape
    if len(shape) == 2:
        tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (shape[0],))[:, None]
        if len(receivers):
            adj = np.broadcast_to(adj, (shape[0],) + adj.shape[-2:])
    h = 0.5 * tau
    for s in range(nsteps, 0, -1):
        if s % record_every == 0:
            for j, r in enumerate(receivers):                       # one at a time: a duplicated receiver adds twice, in this order
                lam[..., r] = lam[..., r] + adj[..., s // record_every - 1, j]
        S = S + q * H[..., s, :]
        lam = lam + h * grid.au(q)
        q = q + tau * (c2 * lam)
        S = S + q * H[..., s - 1, :]
        lam = lam + h * grid.au(q)
    return lam, q, S


def gradient(grid, u0, v0, g, c2, tau, nsteps, source, observed, receivers, record_every=1):
    """What wave_gradient_many returns, from the model: (misfit [members], grad_c2, grad_u0, grad_v0, traces) of
    J = 1/2 sum (traces - observed)^2 per member: the adjoint source is traces - observed, and
    grad_c2 = h S / c2, grad_u0 = lam, grad_v0 = q / c2."""
    u, v, traces, H = verlet_history(grid, u0, v0, g, c2, tau, nsteps, source, receivers, record_every)
    r = traces - observed
    lam, q, S = adjoint(grid, H, c2, tau, r, receivers, record_every)
    h = 0.5 * (np.broadcast_to(np.asarray(tau, dtype=np.float64), (H.shape[0],))[:, None] if H.ndim == 3 else tau)
    J = 0.5 * np.sum((r * r).reshape(r.shape[:-2] + (-1,)), axis=-1)
    return J, h * S / c2, lam, q / c2, traces
