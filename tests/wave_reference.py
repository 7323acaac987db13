"""A NumPy model of the on-chip wave steppers (csrc/onchip_plan.h): u_tt = A u - g on the L-shaped grid in packed
order, every expression written operation by operation in the order the kernels use, so that a GPU result can be compared with
np.array_equal.  Not a test module: tests/test_onchip_wave_cpu.py checks the model's own invariants, tests/test_gpu_wave_many.py
compares the kernels with it."""
import numpy as np


def packed_cells(n):
    """The image cell of every unknown in packed order: the bottom-right block row by row, then the upper block (onchip_plan.h)."""
    half, pitch = n // 2, n + 1
    cells = [y * pitch + x for y in range(1, half + 1) for x in range(half + 1, n)]
    cells += [y * pitch + x for y in range(half + 1, n) for x in range(1, n)]
    return np.array(cells), pitch


class Grid:
    """An n x n grid with the coefficients of its operator: A0 (the UNSHIFTED diagonal), xk, yk."""

    def __init__(self, n, A0, xk, yk):
        self.n, self.A0, self.xk, self.yk = n, float(A0), float(xk), float(yk)
        self.cells, self.pitch = packed_cells(n)
        self.size = len(self.cells)

    @classmethod
    def of_domain(cls, n, a, b, c, d):
        """grid_setup.cpp: the steps (b - a) / n and (d - c) / n, xk = 1 / hx^2, yk = 1 / hy^2, A0 = -2 (xk + yk)."""
        hx, hy = (b - a) / n, (d - c) / n
        return cls(n, -2 * (1 / (hx * hx) + 1 / (hy * hy)), 1 / (hx * hx), 1 / (hy * hy))

    def image(self, u):
        """u: [size] or [members, size]."""
        u = np.asarray(u, dtype=np.float64)
        img = np.zeros(u.shape[:-1] + ((self.n + 1) ** 2,))
        img[..., self.cells] = u
        return img

    def au(self, u, A0=None):
        """A0 uc + xk (left + right) + yk (down + up), in that order; A0: another diagonal (a shifted operator)."""
        img, c, p = self.image(u), self.cells, self.pitch
        A0 = self.A0 if A0 is None else A0
        return A0 * img[..., c] + self.xk * (img[..., c - 1] + img[..., c + 1]) + self.yk * (img[..., c - p] + img[..., c + p])

    def cfl(self):
        return 2.0 / np.sqrt(2.0 * abs(self.A0))


def verlet(grid, u, v, g, tau, nsteps):
    """nsteps steps of velocity Verlet; (u, v) after them.  u, v, g: [size] with a scalar tau, or [members, size] with tau [members]."""
    u, v = np.array(u, dtype=np.float64), np.array(v, dtype=np.float64)
    if u.ndim == 2:
        tau = np.broadcast_to(np.asarray(tau, dtype=np.float64), (len(u),))[:, None]
    h = 0.5 * tau
    a = grid.au(u) - g
    for _ in range(nsteps):
        vh = v + h * a
        u = u + tau * vh
        a = grid.au(u) - g
        v = vh + h * a
    return u, v


def newmark_coefficients(tau):
    """(sigma, hv) of a step: 4 / tau^2 and 2 / tau."""
    return 4.0 / (tau * tau), 2.0 / tau


def newmark_rhs(grid, u, v, g, tau):
    """The right-hand side of (A - sigma I) x = b for one Newmark step from (u, v)."""
    sigma, _ = newmark_coefficients(tau)
    w = u + tau * v
    b = (g + g) - sigma * w
    b = b - grid.au(u)
    return b


def newmark_velocity(tau, x, u, v):
    _, hv = newmark_coefficients(tau)
    return hv * (x - u) - v


def cg(grid, diag, b, x0, tol=1e-12, max_iterations=100000):
    """Plain CG on the NEGATIVE definite (A - sigma I), diag = A0 - sigma, from x0 until ||r|| <= tol ||b||.  The model's own
    solver for its Newmark invariant; the GPU tests solve with a reference handle instead."""
    x = np.array(x0, dtype=np.float64)
    r = b - grid.au(x, diag)
    p = r.copy()
    rr = float(r @ r)
    stop = (tol * np.linalg.norm(b)) ** 2
    for _ in range(max_iterations):
        if rr <= stop:
            break
        ap = grid.au(p, diag)
        alpha = rr / float(p @ ap)
        x = x + alpha * p
        r = r - alpha * ap
        rr_new = float(r @ r)
        p = r + (rr_new / rr) * p
        rr = rr_new
    return x


def newmark(grid, u, v, g, tau, nsteps, tol=1e-12):
    """nsteps Newmark steps with the model's CG; (u, v) after them."""
    u, v = np.array(u, dtype=np.float64), np.array(v, dtype=np.float64)
    sigma, _ = newmark_coefficients(tau)
    for _ in range(nsteps):
        x = cg(grid, grid.A0 - sigma, newmark_rhs(grid, u, v, g, tau), u, tol)
        v = newmark_velocity(tau, x, u, v)
        u = x
    return u, v


def energy(grid, u, v, g):
    """1/2 |v|^2 - 1/2 u^T A u + g^T u: what the exact flow and the Newmark scheme conserve."""
    return 0.5 * float(v @ v) - 0.5 * float(u @ grid.au(u)) + float(g @ u)


def verlet_energy(grid, u, v, g, tau):
    """The energy minus (tau^2 / 8) |A u - g|^2: what velocity Verlet conserves exactly (up to rounding) for a linear force."""
    a = grid.au(u) - g
    return energy(grid, u, v, g) - (tau * tau / 8.0) * float(a @ a)
