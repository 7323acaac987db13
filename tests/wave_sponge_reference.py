"""A NumPy model of the recorded explicit wave stepper with a damping field (csrc/onchip_plan.h): velocity
Verlet for u_tt + d o u_t = c2 o (A u) - w(t) g, the damping rate d >= 0 of every unknown entering as one factor on v at both ends
of a step, every expression written operation by operation in the kernel's order, so that a GPU result can be compared with
np.array_equal.  Not a test module: tests/test_onchip_wave_sponge_cpu.py checks the model's own properties,
tests/test_gpu_wave_sponge.py compares the kernel with it.  The grid is tests/wave_reference.py's, the medium's bound and energies
tests/wave_medium_reference.py's."""
import numpy as np

from wave_medium_reference import medium_cfl, modified_energy, plain_energy  # noqa: F401  (for the callers too)
from wave_reference import Grid  # noqa: F401


def sponge_factor(tau, d):
    """onchip_wave_sponge_factor: e = (0.25 tau) d; s = (1 - e) / (1 + e), every operation rounded once.  tau and d broadcast."""
    e = (0.25 * np.asarray(tau, dtype=np.float64)) * np.asarray(d, dtype=np.float64)
    return (1.0 - e) / (1.0 + e)


def verlet_sponge(grid, u, v, g, c2, d, tau, nsteps, source, receivers=(), record_every=1):
    """nsteps steps from (u, v) in the medium c2 with the damping d and the amplitudes source[..., n] at the local times n tau:
    (u, v, traces).  wave_medium_reference.verlet_medium's arguments with d behind c2, [size] (one field for all members) or
    [members, size] like c2.  With h = 0.5 tau and s = sponge_factor(tau, d):
        v = s v;  f = w[n] g;  a = c2 au(u) - f;  vh = v + h a;  u = u + tau vh;  f = w[n + 1] g;  a = c2 au(u) - f;  v = vh + h a;  v = s v,
    the second a of a step carried into the next (damping does not touch u); the v returned is the one after the closing multiply."""
    u, v = np.array(u, dtype=np.float64), np.array(v, dtype=np.float64)
    w = np.asarray(source, dtype=np.float64)
    c2, d = np.asarray(c2, dtype=np.float64), np.asarray(d, dtype=np.float64)
    assert w.shape[-1] == nsteps + 1 and record_every >= 1 and c2.shape in (u.shape, u.shape[-1:]) and d.shape in (u.shape, u.shape[-1:])
    receivers = np.asarray(receivers, dtype=np.int64).reshape(-1)
    if u.ndim == 2:
        tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (len(u),))[:, None]
        w = np.broadcast_to(w, (len(u), nsteps + 1))
        amplitude = lambda n: w[:, n][:, None]
    else:
        assert w.ndim == 1
        amplitude = lambda n: w[n]
    h = 0.5 * tau
    s = sponge_factor(tau, d)
    f = amplitude(0) * g
    t = grid.au(u)
    a = c2 * t - f
    samples = []
    for n in range(nsteps):
        v = s * v
        vh = v + h * a
        u = u + tau * vh
        f = amplitude(n + 1) * g
        t = grid.au(u)
        a = c2 * t - f
        v = vh + h * a
        v = s * v
        if (n + 1) % record_every == 0:
            samples.append(u[..., receivers])
    traces = np.stack(samples, axis=-2) if samples else np.zeros(u.shape[:-1] + (0, len(receivers)))
    return u, v, traces
