"""A NumPy model of the explicit wave stepper with a source time function and receiver traces (csrc/onchip_plan.h, DESIGN section
12.4): velocity Verlet for u_tt = A u - w(t) g, every expression written operation by operation in the kernel's order, so that a
GPU result can be compared with np.array_equal.  Not a test module: tests/test_onchip_wave_record_cpu.py checks the model's own
properties, tests/test_gpu_wave_record.py compares the kernel with it.  The grid is tests/wave_reference.py's."""
import numpy as np

from wave_reference import Grid  # noqa: F401  (the model's grid, for the callers too)


def verlet_record(grid, u, v, g, tau, nsteps, source, receivers=(), record_every=1):
    """nsteps steps from (u, v) with the amplitudes source[..., n] at the local times n tau: (u, v, traces) after them.
    u, v, g: [size] with a scalar tau and source [nsteps + 1]; or [members, size] with tau [members] (or a scalar) and source
    [nsteps + 1] (one row for all) or [members, nsteps + 1].  traces: [..., nsteps // record_every, len(receivers)], sample j is u
    at the receivers (packed indices) after step (j + 1) * record_every.
    With h = 0.5 tau:   f = w[n] g;  a = au(u) - f;  vh = v + h a;  u = u + tau vh;  f = w[n + 1] g;  a = au(u) - f;  v = vh + h a,
    the second a of a step carried into the next."""
    u, v = np.array(u, dtype=np.float64), np.array(v, dtype=np.float64)
    w = np.asarray(source, dtype=np.float64)
    assert w.shape[-1] == nsteps + 1 and record_every >= 1
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
    a = grid.au(u) - f
    samples = []
    for n in range(nsteps):
        vh = v + h * a
        u = u + tau * vh
        f = amplitude(n + 1) * g
        a = grid.au(u) - f
        v = vh + h * a
        if (n + 1) % record_every == 0:
            samples.append(u[..., receivers])
    traces = np.stack(samples, axis=-2) if samples else np.zeros(u.shape[:-1] + (0, len(receivers)))
    return u, v, traces
