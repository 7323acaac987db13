"""A NumPy model of the recorded explicit wave stepper in a medium (csrc/onchip_plan.h): velocity Verlet for
u_tt = c2 o (A u) - w(t) g with the squared wave speed c2 > 0 of every unknown, every expression written operation by operation in
the kernel's order, so that a GPU result can be compared with np.array_equal.  Not a test module:
tests/test_onchip_wave_medium_cpu.py checks the model's own properties, tests/test_gpu_wave_medium.py compares the kernel with it.
The grid is tests/wave_reference.py's."""
import numpy as np

from wave_reference import Grid  # noqa: F401  (the model's grid, for the callers too)


def medium_cfl(grid, c2max):
    """onchip_wave_medium_cfl: 2 / sqrt((2 |A0|) c2max), a float or an array; c2max = 1 gives the bits of grid.cfl()."""
    return 2.0 / np.sqrt(2.0 * abs(grid.A0) * c2max)


def verlet_medium(grid, u, v, g, c2, tau, nsteps, source, receivers=(), record_every=1):
    """nsteps steps from (u, v) in the medium c2 with the amplitudes source[..., n] at the local times n tau: (u, v, traces).
    u, v, g: [size] with a scalar tau, c2 [size] and source [nsteps + 1]; or [members, size] with tau [members] (or a scalar), c2
    [size] (one medium for all) or [members, size] and source [nsteps + 1] (one row for all) or [members, nsteps + 1].  traces:
    [..., nsteps // record_every, len(receivers)], sample j is u at the receivers (packed indices) after step (j + 1) * record_every.
    With h = 0.5 tau and t = au(u), a = c2 * t - f (two roundings after t):
        f = w[n] g;  a = c2 au(u) - f;  vh = v + h a;  u = u + tau vh;  f = w[n + 1] g;  a = c2 au(u) - f;  v = vh + h a,
    the second a of a step carried into the next."""
    u, v = np.array(u, dtype=np.float64), np.array(v, dtype=np.float64)
    w = np.asarray(source, dtype=np.float64)
    c2 = np.asarray(c2, dtype=np.float64)
    assert w.shape[-1] == nsteps + 1 and record_every >= 1 and c2.shape in (u.shape, u.shape[-1:])
    receivers = np.asarray(receivers, dtype=np.int64).reshape(-1)
    if u.ndim == 2:
        tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (len(u),))[:, None]
        w = np.broadcast_to(w, (len(u), nsteps + 1))
        amplitude = lambda n: w[:, n][:, None]
    else:
        assert w.ndim == 1
        amplitude = lambda n: w[n]
    h = 0.5 * tau
    f = amplitude(0) * g
    t = grid.au(u)
    a = c2 * t - f
    samples = []
    for n in range(nsteps):
        vh = v + h * a
        u = u + tau * vh
        f = amplitude(n + 1) * g
        t = grid.au(u)
        a = c2 * t - f
        v = vh + h * a
        if (n + 1) % record_every == 0:
            samples.append(u[..., receivers])
    traces = np.stack(samples, axis=-2) if samples else np.zeros(u.shape[:-1] + (0, len(receivers)))
    return u, v, traces


def modified_energy(grid, u, v, c2, tau):
    """1/2 v^T C^-1 v - 1/2 u^T A u - (tau^2 / 8) a^T C^-1 a with a = c2 au(u) and C = diag(c2): what the scheme conserves (up to
    rounding) without a forcing."""
    t = grid.au(u)
    a = c2 * t
    return 0.5 * float(v @ (v / c2)) - 0.5 * float(u @ t) - (tau * tau / 8.0) * float(a @ (a / c2))


def plain_energy(grid, u, v, c2):
    """1/2 v^T C^-1 v - 1/2 u^T A u: the exact flow's invariant, which the scheme only shadows."""
    return 0.5 * float(v @ (v / c2)) - 0.5 * float(u @ grid.au(u))
