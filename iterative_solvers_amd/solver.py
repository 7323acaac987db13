"""Host-side mirror of the reference's operator / solver interface for the hot path, over the
C ABI (include/mi355cg.h).  Same class and method names, argument meaning and error behaviour
as the reference's C++ classes, so the parity tests read like the reference's own usage:

  MatrixFreeSystem / MatrixFreeSolver   solver/matrix_free_system.hpp:12-127
  GridSystem                            solver/grid_system.h:16-88
  Solver / MSGSolver / StopCriterion    solver/solver.hpp:17-66, solver/msg_solver.hpp:9-120
  DirichletSolver / SolverResults       solver/dirichlet_solver.hpp:11-24,79-184

All compute runs in libmi355cg.so on the GPU; nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
import enum
import sys
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

from . import _capi

DBL_MAX = sys.float_info.max
BATCH_MAX = _capi.BATCH_MAX


class StopCriterion(enum.IntEnum):          # solver/msg_solver.hpp:9-15
    ITERATIONS = 0
    PRECISION = 1
    RESIDUAL = 2
    EXACT_ERROR = 3
    INTERRUPTED = 4


_STOP_TEXT = {                              # solver/msg_solver.hpp:85-100
    StopCriterion.ITERATIONS: "Достигнуто максимальное число итераций",
    StopCriterion.PRECISION: "Достигнута требуемая точность по норме разности xn и xn-1",
    StopCriterion.RESIDUAL: "Достигнута требуемая точность по норме невязки",
    StopCriterion.EXACT_ERROR: "Достигнута требуемая точность по норме разности с истинным решением",
    StopCriterion.INTERRUPTED: "Прервано пользователем",
}


class _Handle:
    """Owns one mi355cg context (one GPU)."""

    def __init__(self, n, m, a, b, c, d, dtype=_capi.F64, device=0):
        self._lib = _capi.load()
        self._h = C.c_void_p()
        rc = self._lib.mi355cg_create(int(n), int(m), float(a), float(b), float(c), float(d),
                                      int(dtype), int(device), C.byref(self._h))
        self._check_rc(rc)
        self.size = int(self._lib.mi355cg_size(self._h))
        self._device = int(device)

    @classmethod
    def from_csr(cls, row_map, entries, values, device=0):
        """Handle for a caller-supplied CSR matrix (mi355cg_create_csr).  The library reads row_map[-1] entries and values
        through bare pointers, so the arrays' lengths and integer ranges are checked here first: ValueError, and the library has
        not been called when it is raised."""
        row_map, entries, values = cls._check_csr(row_map, entries, values)
        self = cls.__new__(cls)
        self._lib = _capi.load()
        self._h = C.c_void_p()
        rc = self._lib.mi355cg_create_csr(len(row_map) - 1, row_map, entries, values, int(device), C.byref(self._h))
        self._check_rc(rc)
        self.size = int(self._lib.mi355cg_size(self._h))
        self._device = int(device)
        return self

    @staticmethod
    def _check_csr(row_map, entries, values):
        """(row_map int32, entries int32, values float64), contiguous, or ValueError: row_map is one-dimensional and not empty,
        row_map and entries hold integers that fit in int32 (compared before the cast, which would wrap), and entries and values
        have exactly row_map[-1] elements.  Monotone offsets and the column range are the library's to check."""
        row_map, entries, values = np.asarray(row_map), np.asarray(entries), np.asarray(values)
        if row_map.ndim != 1 or row_map.size == 0:
            raise ValueError(f"row_map has shape {row_map.shape}, expected (rows + 1,) with at least one offset")
        if entries.ndim != 1 or values.ndim != 1:
            raise ValueError(f"entries and values have shapes {entries.shape} and {values.shape}, expected one dimension each")
        i32 = np.iinfo(np.int32)
        for name, a in (("row_map", row_map), ("entries", entries)):
            if a.size == 0:                                       # an empty list arrives as float64 and holds nothing to misread
                continue
            if a.dtype.kind not in "iu":
                raise ValueError(f"{name} has dtype {a.dtype}, expected an integer type")
            if int(a.min()) < i32.min or int(a.max()) > i32.max:
                raise ValueError(f"{name} holds values in [{int(a.min())}, {int(a.max())}], which do not fit in int32")
        nnz = int(row_map[-1])
        if len(entries) != nnz or len(values) != nnz:
            raise ValueError(f"row_map[-1] = {nnz}, but entries has {len(entries)} and values has {len(values)} elements")
        try:
            values = np.ascontiguousarray(values, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"values has dtype {values.dtype}, expected real numbers") from e
        return np.ascontiguousarray(row_map, dtype=np.int32), np.ascontiguousarray(entries, dtype=np.int32), values

    def set_true_solution(self, u):
        u = np.ascontiguousarray(u, dtype=np.float64)
        if u.shape != (self.size,):
            raise ValueError(f"true solution has shape {u.shape}, expected ({self.size},)")
        _capi.check(self._lib.mi355cg_set_true_solution(self._h, u))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.mi355cg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # thin wrappers -------------------------------------------------------------------------
    def _vec_out(self, fn) -> np.ndarray:
        out = np.empty(self.size)
        _capi.check(fn(self._h, out))
        return out

    def rhs(self): return self._vec_out(self._lib.mi355cg_get_rhs)
    def true_solution(self): return self._vec_out(self._lib.mi355cg_get_true_solution)
    def solution(self): return self._vec_out(self._lib.mi355cg_get_solution)
    def recursive_residual(self): return self._vec_out(self._lib.mi355cg_get_recursive_residual)
    def true_residual(self): return self._vec_out(self._lib.mi355cg_get_true_residual)

    def node_coords(self):
        xs, ys = np.empty(self.size), np.empty(self.size)
        _capi.check(self._lib.mi355cg_get_node_coords(self._h, xs, ys))
        return xs, ys

    def set_rhs(self, b):
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.shape != (self.size,):
            raise ValueError(f"rhs has shape {b.shape}, expected ({self.size},)")
        _capi.check(self._lib.mi355cg_set_rhs(self._h, b))

    def apply(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.size,):
            raise ValueError(f"vector has shape {x.shape}, expected ({self.size},)")
        y = np.empty(self.size)
        _capi.check(self._lib.mi355cg_apply(self._h, x, y))
        return y

    @staticmethod
    def _check_guess(x0, size):
        """True if the guess x0 is in device memory: a NumPy array or a CUDA torch tensor, [size] float64, contiguous.
        ValueError for anything else; the library has not been called when it is raised."""
        on_device = not isinstance(x0, np.ndarray)
        if on_device:
            if not (type(x0).__module__.split(".")[0] == "torch" and hasattr(x0, "data_ptr")):
                raise ValueError(f"an initial guess is a NumPy array or a CUDA torch tensor, not {type(x0).__name__}")
            import torch
            if not x0.is_cuda:
                raise ValueError("a torch guess must be in device memory (a CPU tensor: pass tensor.numpy())")
            if x0.dtype != torch.float64:
                raise ValueError(f"initial guess has dtype {x0.dtype}, expected torch.float64")
            if not x0.is_contiguous():
                raise ValueError("initial guess tensor must be contiguous")
        elif x0.dtype != np.float64:
            raise ValueError(f"initial guess has dtype {x0.dtype}, expected float64")
        if tuple(x0.shape) != (size,):
            raise ValueError(f"initial guess has shape {tuple(x0.shape)}, expected ({size},)")
        return on_device

    def _check_rc(self, rc):
        if rc == _capi.ERR_INVALID:
            raise ValueError(self._lib.mi355cg_last_error().decode())     # std::invalid_argument
        _capi.check(rc)

    def set_initial_guess(self, x0):
        """Extension (no reference twin): the next solve() starts from x0 and r0 = b - A x0 instead of from zero, and REL_2NORM
        stops relative to ||b|| (mi355cg_set_initial_guess).  One-shot.  x0: NumPy [size] float64, or a contiguous CUDA
        torch.Tensor on the handle's device, which is read in place (mi355cg_set_initial_guess_device); None withdraws a
        pending guess.  Until the next solve solution() and the residuals raise.  ValueError on CSR and F32_MIXED handles."""
        if x0 is None:
            return self._check_rc(self._lib.mi355cg_set_initial_guess(self._h, None))
        if self._check_guess(x0, self.size):
            import torch
            if x0.device.index != self._device:
                raise ValueError(f"initial guess is on {x0.device}, the handle on device {self._device}")
            torch.cuda.current_stream(x0.device).synchronize()       # the library works on its own stream
            return self._check_rc(self._lib.mi355cg_set_initial_guess_device(self._h, x0.data_ptr()))
        x0 = np.ascontiguousarray(x0)
        self._check_rc(self._lib.mi355cg_set_initial_guess(self._h, x0.ctypes.data))

    def use_solution_as_initial_guess(self):
        """The x of the last solve is the next solve's starting point, without a copy: after a solve that was interrupted or hit
        its iteration cap this continues it (mi355cg_use_solution_as_initial_guess)."""
        self._check_rc(self._lib.mi355cg_use_solution_as_initial_guess(self._h))

    def set_shift(self, sigma: float):
        """Extension (no reference twin): the handle's operator becomes A - sigma I, for apply(), every solve, the preconditioner
        and the batched solves (mi355cg_set_shift).  sigma is finite and >= 0; 0 restores the Laplacian bit for bit.  ValueError
        if refused (a bad sigma; CSR, slab and F32_MIXED handles); the handle then keeps what it had."""
        self._check_rc(self._lib.mi355cg_set_shift(self._h, float(sigma)))

    def get_shift(self) -> float:
        s = C.c_double()
        _capi.check(self._lib.mi355cg_get_shift(self._h, C.byref(s)))
        return s.value

    def solution_device(self, out):
        """The x of the last solve into `out`, a contiguous CUDA float64 tensor [size] on the handle's device
        (mi355cg_get_solution_device); complete on return."""
        _capi.check(self._lib.mi355cg_get_solution_device(self._h, out.data_ptr()))
        return out

    def time_steps(self, params: _capi.Params, tau: float, theta: float, nsteps: int, stop_flag: Optional[C.c_int] = None):
        """nsteps theta-scheme steps of u_t = A u - g from the pending starting state (mi355cg_time_steps).  Returns
        ([Results of the steps taken, the unfinished one included], steps_done)."""
        n = int(nsteps)
        res = (_capi.Results * max(n, 1))()
        done = C.c_int(0)
        sp = C.cast(C.pointer(stop_flag), C.c_void_p) if stop_flag is not None else None
        rc = self._lib.mi355cg_time_steps(self._h, C.byref(params), float(tau), float(theta), n, sp, res, C.byref(done))
        self._check_rc(rc)
        return list(res[:min(n, done.value + 1)]), done.value

    def solve(self, params: _capi.Params, callback=None, stop_flag: Optional[C.c_int] = None) -> _capi.Results:
        res = _capi.Results()
        cb = _capi.ITER_CB(lambda user, it, p, r, e: callback(it, p, r, e)) if callback else _capi.ITER_CB()
        sp = C.cast(C.pointer(stop_flag), C.c_void_p) if stop_flag is not None else None
        rc = self._lib.mi355cg_solve(self._h, C.byref(params), cb, None, sp, C.byref(res))
        self._check_rc(rc)
        return res

    def set_preconditioner(self, kind: int, cycle: int = _capi.CYCLE_F64):
        """Extension (no reference twin): _capi.PRECOND_MG (grids with a nested hierarchy, see mg_levels) or _capi.PRECOND_MG_ANY
        (every grid, see mg_hierarchy) builds the multigrid hierarchy, after which solve() runs preconditioned CG;
        _capi.PRECOND_NONE frees it (include/mi355cg.h, mi355cg_set_preconditioner).  cycle: _capi.CYCLE_F64, or _capi.CYCLE_F32
        for the V-cycle in fp32 inside the fp64 PCG (mi355cg_set_preconditioner_ex).  ValueError if refused; the handle then
        keeps what it had."""
        rc = self._lib.mi355cg_set_preconditioner_ex(self._h, int(kind), int(cycle))
        self._check_rc(rc)

    def set_solve_mode(self, mode: int):
        """Extension (no reference twin): _capi.SOLVE_ONCHIP runs every chunk of a plain fp64 solve as one launch of one workgroup
        (grids up to N = 128, bit-identical to the default), _capi.SOLVE_LAUNCHES goes back to two launches per iteration
        (include/mi355cg.h, mi355cg_set_solve_mode).  ValueError if refused; the handle then keeps its mode."""
        rc = self._lib.mi355cg_set_solve_mode(self._h, int(mode))
        self._check_rc(rc)

    def solve_mode_info(self):
        """(mode, on-chip chunk launches of the last solve)."""
        mode, n = C.c_int(), C.c_longlong()
        _capi.check(self._lib.mi355cg_get_solve_mode(self._h, C.byref(mode), C.byref(n)))
        return mode.value, n.value

    def preconditioner_info(self):
        """(kind, cycle, levels) of the preconditioner that is set; (PRECOND_NONE, CYCLE_F64, 0) without one."""
        k, cy, lv = C.c_int(), C.c_int(), C.c_int()
        _capi.check(self._lib.mi355cg_preconditioner_info(self._h, C.byref(k), C.byref(cy), C.byref(lv)))
        return k.value, cy.value, lv.value

    def set_smoother(self, smoother: int):
        """Extension (no reference twin): the smoother of the fp64 V-cycle, _capi.SMOOTHER_JACOBI (the default) or line Jacobi
        _capi.SMOOTHER_LINE_X / _LINE_Y / _LINE_AUTO for stretched domains (include/mi355cg.h, mi355cg_set_smoother).  Before or
        after set_preconditioner.  ValueError if refused; the handle then keeps what it had."""
        rc = self._lib.mi355cg_set_smoother(self._h, int(smoother))
        self._check_rc(rc)

    def smoother_info(self):
        """(smoother, direction): the smoother as set, and the line direction it means on this grid (0 none, 1 x, 2 y)."""
        s, d = C.c_int(), C.c_int()
        _capi.check(self._lib.mi355cg_get_smoother(self._h, C.byref(s), C.byref(d)))
        return s.value, d.value

    def apply_preconditioner(self, r):
        """z = M r for a packed vector r (needs set_preconditioner(PRECOND_MG or PRECOND_MG_ANY) first)."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        if r.shape != (self.size,):
            raise ValueError(f"vector has shape {r.shape}, expected ({self.size},)")
        z = np.empty(self.size)
        _capi.check(self._lib.mi355cg_apply_preconditioner(self._h, r, z))
        return z

    @staticmethod
    def _check_batch(b, size, most=_capi.BATCH_MAX):
        """(nrhs, on_device) of a batch of right-hand sides: a NumPy array or a CUDA torch tensor, [nrhs, size] float64, at most
        `most` rows.  ValueError for anything else; the library has not been called when it is raised."""
        on_device = not isinstance(b, np.ndarray)
        if on_device:
            if not (type(b).__module__.split(".")[0] == "torch" and hasattr(b, "data_ptr")):
                raise ValueError(f"a batch of right-hand sides is a NumPy array or a CUDA torch tensor, not {type(b).__name__}")
            import torch
            if not b.is_cuda:
                raise ValueError("a torch batch must be in device memory (a CPU tensor: pass tensor.numpy())")
            if b.dtype != torch.float64:
                raise ValueError(f"batch has dtype {b.dtype}, expected torch.float64")
            if not b.is_contiguous():
                raise ValueError("batch tensor must be contiguous")
        elif b.dtype != np.float64:
            raise ValueError(f"batch has dtype {b.dtype}, expected float64")
        shape = tuple(b.shape)
        if len(shape) != 2 or shape[1] != size:
            raise ValueError(f"batch has shape {shape}, expected (nrhs, {size})")
        if not 1 <= shape[0] <= most:
            raise ValueError(f"a batch has 1 .. {most} right-hand sides, not {shape[0]}")
        return shape[0], on_device

    def _batched(self, main, other, names, most, stop_flag):
        """What solve_batch, solve_many and time_steps_many check before they call the library: (count, on_device, stop pointer).
        main: the batch; other: its optional companion of the same kind and shape; names: what the messages call main, other, the
        others and the whole, e.g. ("b", "x0", "guesses", "batch").  The return code then goes through _check_rc."""
        n, on_device = self._check_batch(main, self.size, most)
        m_name, o_name, o_plural, whole = names
        if other is not None and self._check_batch(other, self.size, most) != (n, on_device):
            raise ValueError(f"{o_name} has shape {tuple(other.shape)}: the {o_plural} are of the kind (NumPy / CUDA tensor) and shape of {m_name}, "
                             f"{tuple(main.shape)}")
        if on_device:
            if main.device.index != self._device:
                raise ValueError(f"{whole} is on {main.device}, the handle on device {self._device}")
            if other is not None and other.device != main.device:
                raise ValueError(f"{o_name} is on {other.device}, {m_name} on {main.device}")
        return n, on_device, C.cast(C.pointer(stop_flag), C.c_void_p) if stop_flag is not None else None

    def solve_batch(self, params: _capi.Params, b, stop_flag: Optional[C.c_int] = None, x0=None):
        """Extension (no reference twin): solve b[s] for every row s of b by one multigrid-preconditioned CG loop
        (mi355cg_solve_batch; needs set_preconditioner first).  Returns (x, [Results per system]); system s gets the bits
        set_rhs(b[s]); solve(params); solution() gives.  b: NumPy [nrhs, size] float64 -> NumPy x; or a contiguous CUDA
        torch.Tensor [nrhs, size] float64 on the handle's device -> a new tensor there (mi355cg_solve_batch_device; torch's
        current stream is synchronised first, since the library works on its own stream).  params.use_true_solution and
        params.diagnostics must be 0.  x0: a guess per system, of b's kind and shape (mi355cg_solve_batch_from): system s then
        gets the bits of set_rhs(b[s]); set_initial_guess(x0[s]); solve(params); solution().  x0 is not modified."""
        nrhs, on_device, sp = self._batched(b, x0, ("b", "x0", "guesses", "batch"), _capi.BATCH_MAX, stop_flag)
        res = (_capi.Results * nrhs)()
        if on_device:
            import torch
            x = torch.empty_like(b) if x0 is None else x0.clone()
            torch.cuda.current_stream(b.device).synchronize()
            fn = self._lib.mi355cg_solve_batch_device if x0 is None else self._lib.mi355cg_solve_batch_device_from
            rc = fn(self._h, C.byref(params), nrhs, b.data_ptr(), x.data_ptr(), sp, res)
        else:
            b = np.ascontiguousarray(b)
            x = np.empty_like(b) if x0 is None else np.array(x0, dtype=np.float64, order="C", copy=True)
            fn = self._lib.mi355cg_solve_batch if x0 is None else self._lib.mi355cg_solve_batch_from
            rc = fn(self._h, C.byref(params), nrhs, b.ctypes.data, x.ctypes.data, sp, res)
        self._check_rc(rc)
        return x, list(res)

    def batch_release(self):
        """Free the workspaces solve_batch and solve_many keep on the handle (nothing to free is fine)."""
        _capi.check(self._lib.mi355cg_batch_release(self._h))

    def solve_many(self, params: _capi.Params, b, stop_flag: Optional[C.c_int] = None, x0=None, sigma=None):
        """Extension (no reference twin): many small systems on this grid, one workgroup each (mi355cg_solve_many; plain fp64 grid
        handles up to the on-chip cap, no preconditioner).  Returns (x, [Results per system]); system s gets the bits
        set_shift(sigma[s]); set_rhs(b[s]); [set_initial_guess(x0[s]);] solve(params); solution() gives, and the handle itself is
        left as it was.  b: NumPy [nsys, size] float64 -> NumPy x; or a contiguous CUDA torch.Tensor of that shape on the handle's
        device -> a new tensor there (torch's current stream is synchronised first).  x0: a guess per system, of b's kind and
        shape; not modified.  sigma: a shift per system, [nsys] float64 of b's kind (a sequence is fine beside a NumPy b); None =
        the handle's current shift for all.  params.use_true_solution and params.diagnostics must be 0."""
        nsys, on_device, sp = self._batched(b, x0, ("b", "x0", "guesses", "batch"), _capi.MANY_MAX, stop_flag)
        res = (_capi.Results * nsys)()
        if on_device:
            import torch
            if sigma is not None:
                if not (hasattr(sigma, "data_ptr") and sigma.is_cuda and sigma.device == b.device and sigma.dtype == torch.float64
                        and tuple(sigma.shape) == (nsys,) and sigma.is_contiguous()):
                    raise ValueError(f"sigma beside a CUDA batch is a contiguous float64 tensor of shape ({nsys},) on {b.device}")
            x = torch.empty_like(b) if x0 is None else x0.clone()
            torch.cuda.current_stream(b.device).synchronize()
            fn = self._lib.mi355cg_solve_many_device if x0 is None else self._lib.mi355cg_solve_many_device_from
            rc = fn(self._h, C.byref(params), nsys, b.data_ptr(), x.data_ptr(), sigma.data_ptr() if sigma is not None else None, sp, res)
        else:
            b = np.ascontiguousarray(b)
            if sigma is not None:
                sigma = np.ascontiguousarray(sigma, dtype=np.float64)
                if sigma.shape != (nsys,):
                    raise ValueError(f"sigma has shape {sigma.shape}, expected ({nsys},)")
            x = np.empty_like(b) if x0 is None else np.array(x0, dtype=np.float64, order="C", copy=True)
            fn = self._lib.mi355cg_solve_many if x0 is None else self._lib.mi355cg_solve_many_from
            rc = fn(self._h, C.byref(params), nsys, b.ctypes.data, x.ctypes.data, sigma.ctypes.data if sigma is not None else None, sp, res)
        self._check_rc(rc)
        return x, list(res)

    @staticmethod
    def _ensemble_steps(nsys, tau, nsteps, step_iterations):
        """What time_steps_many and wave_steps_many make of their step arguments: (tau as contiguous float64 [nsys], nsteps as an
        int in range, the Results array, steps_done, step_it or None without step_iterations)."""
        if hasattr(tau, "data_ptr"):
            tau = tau.detach().cpu().numpy()
        tau = np.ascontiguousarray(np.broadcast_to(np.asarray(tau, dtype=np.float64), (nsys,)) if np.ndim(tau) == 0 else tau, dtype=np.float64)
        if tau.shape != (nsys,):
            raise ValueError(f"tau has shape {tau.shape}, expected a scalar or ({nsys},)")
        nsteps = int(nsteps)
        if not 0 <= nsteps <= _capi.STEPS_MANY_MAX_STEPS:
            raise ValueError(f"nsteps {nsteps} rejected: it must be 0 .. {_capi.STEPS_MANY_MAX_STEPS}")
        if step_iterations and nsys * nsteps > 1 << 26:
            raise ValueError(f"{nsys} members x {nsteps} steps: more than 2^26 iteration counts")
        step_it = np.full((nsys, nsteps), -1, dtype=np.int32) if step_iterations else None
        return tau, nsteps, (_capi.Results * nsys)(), np.zeros(nsys, dtype=np.int32), step_it

    def time_steps_many(self, params: _capi.Params, u0, tau, theta: float, nsteps: int, g=None, stop_flag: Optional[C.c_int] = None):
        """Extension (no reference twin): an ensemble of time steppers on this grid, one workgroup per member with the step loop
        inside the launch (mi355cg_time_steps_many; the handles solve_many takes).  Member s is integrated over nsteps steps of the
        theta scheme for u_t = A u - g[s] from u0[s] with its own time step tau[s] and gets the bits set_rhs(g[s]);
        set_initial_guess(u0[s]); time_steps(params, tau[s], theta, nsteps) give; the handle itself is left as it was.  Returns
        (u, [Results of the last step attempted per member], steps_done int32 [nsys], step_iterations int32 [nsys, nsteps], -1 =
        step not taken).  u0: NumPy [nsys, size] float64 -> NumPy u; or a contiguous CUDA torch.Tensor of that shape on the
        handle's device -> a new tensor there (torch's current stream is synchronised first); not modified.  g: of u0's kind and
        shape, None = the handle's right-hand side for every member.  tau: a scalar or [nsys] (host values).
        params.use_true_solution and params.diagnostics must be 0."""
        nsys, on_device, sp = self._batched(u0, g, ("u0", "g", "forcings", "ensemble"), _capi.MANY_MAX, stop_flag)
        tau, nsteps, res, steps_done, step_it = self._ensemble_steps(nsys, tau, nsteps, True)
        if on_device:
            import torch
            u = u0.clone()
            torch.cuda.current_stream(u0.device).synchronize()
            rc = self._lib.mi355cg_time_steps_many_device(self._h, C.byref(params), nsys, nsteps, float(theta), tau.ctypes.data,
                                                          g.data_ptr() if g is not None else None, u.data_ptr(), sp, res,
                                                          steps_done.ctypes.data, step_it.ctypes.data)
        else:
            u = np.array(u0, dtype=np.float64, order="C", copy=True)
            if g is not None:
                g = np.ascontiguousarray(g)
            rc = self._lib.mi355cg_time_steps_many(self._h, C.byref(params), nsys, nsteps, float(theta), tau.ctypes.data,
                                                   g.ctypes.data if g is not None else None, u.ctypes.data, sp, res,
                                                   steps_done.ctypes.data, step_it.ctypes.data)
        self._check_rc(rc)
        return u, list(res), steps_done, step_it

    def wave_steps_many(self, params: Optional[_capi.Params], u0, v0, tau, nsteps: int, scheme: int = _capi.WAVE_VERLET, g=None,
                        steps_per_launch: int = 0, stop_flag: Optional[C.c_int] = None, step_iterations: bool = False):
        """Extension (no reference twin): an ensemble of wave-equation steppers u_tt = A u - g[s] on this grid, one workgroup per
        member (mi355cg_wave_steps_many; the handles solve_many takes).  Member s takes nsteps steps of velocity Verlet
        (WAVE_VERLET; tau[s] at most wave_cfl()) or of average-acceleration Newmark (WAVE_NEWMARK; params as in time_steps_many)
        from the state (u0[s], v0[s]) with its own time step tau[s]; the handle itself is left as it was.  Returns (u, v, [Results
        per member], steps_done int32 [nsys]) and, with step_iterations, int32 [nsys, nsteps] (-1 = step not taken; Verlet takes no
        iterations).  u0, v0: NumPy [nsys, size] float64 -> NumPy; or contiguous CUDA torch.Tensors of that shape on the handle's
        device -> new tensors there (torch's current stream is synchronised first); not modified.  g: of u0's kind and shape,
        None = the handle's right-hand side for every member.  tau: a scalar or [nsys] (host values).  params may be None for
        Verlet."""
        nsys, on_device, sp = self._batched(u0, g, ("u0", "g", "forcings", "ensemble"), _capi.MANY_MAX, stop_flag)
        if self._check_batch(v0, self.size, _capi.MANY_MAX) != (nsys, on_device) or (on_device and v0.device != u0.device):
            raise ValueError(f"v0 has shape {tuple(v0.shape)}: the velocities are of the kind (NumPy / CUDA tensor), shape and device of u0, {tuple(u0.shape)}")
        if scheme not in (_capi.WAVE_VERLET, _capi.WAVE_NEWMARK):
            raise ValueError(f"unknown wave scheme {scheme}")
        if scheme == _capi.WAVE_NEWMARK and params is None:
            raise ValueError("the Newmark scheme reads params")
        tau, nsteps, res, steps_done, step_it = self._ensemble_steps(nsys, tau, nsteps, step_iterations)
        pp = C.byref(params) if params is not None else None
        ip = step_it.ctypes.data if step_it is not None and scheme == _capi.WAVE_NEWMARK else None
        if on_device:
            import torch
            u, v = u0.clone(), v0.clone()
            torch.cuda.current_stream(u0.device).synchronize()
            rc = self._lib.mi355cg_wave_steps_many_device(self._h, pp, nsys, nsteps, int(scheme), tau.ctypes.data,
                                                          g.data_ptr() if g is not None else None, u.data_ptr(), v.data_ptr(),
                                                          int(steps_per_launch), sp, res, steps_done.ctypes.data, ip)
        else:
            u = np.array(u0, dtype=np.float64, order="C", copy=True)
            v = np.array(v0, dtype=np.float64, order="C", copy=True)
            if g is not None:
                g = np.ascontiguousarray(g)
            rc = self._lib.mi355cg_wave_steps_many(self._h, pp, nsys, nsteps, int(scheme), tau.ctypes.data,
                                                   g.ctypes.data if g is not None else None, u.ctypes.data, v.ctypes.data,
                                                   int(steps_per_launch), sp, res, steps_done.ctypes.data, ip)
        self._check_rc(rc)
        return (u, v, list(res), steps_done) + ((step_it,) if step_iterations else ())

    def wave_record_many(self, u0, v0, tau, nsteps: int, source, g=None, receivers=None, record_every: int = 1, steps_per_launch: int = 0,
                         stop_flag: Optional[C.c_int] = None, traces=None, c2=None, damping=None):
        """Extension (no reference twin): wave_steps_many with WAVE_VERLET, a source time function and receiver traces
        (mi355cg_wave_record_many).  damping (or None): a damping rate per unknown, [size] or [nsys, size] of u0's kind; the call is
        then mi355cg_wave_sponge_many, u_tt + d o u_t = c2 o (A u) - w(t) g, in a unit medium when c2 is None.  c2 (or None): a medium, [size] (one for all members) or [nsys, size] of u0's kind, the squared
        wave speed of every unknown; the call is then mi355cg_wave_medium_many, u_tt = c2 o (A u) - w(t) g.  source: the amplitudes, [nsteps + 1] (one row for all members) or [nsys, nsteps + 1], of u0's
        kind; the forcing of member s at its local time n tau[s] is source[s][n] * g[s].  receivers: a sequence of at most
        WAVE_MAX_RECEIVERS packed indices, or None; record_every: the cadence.  Returns (u, v, traces, [Results per member],
        steps_done): traces [nsys, nsteps // record_every, len(receivers)] of u0's kind, u at the receivers after every
        record_every-th step, None without receivers.  traces: an array of that shape to write into (a stop flag leaves the samples
        of steps that did not run as they are).  u0, v0, g, tau, steps_per_launch and stop_flag as in wave_steps_many."""
        return self._wave_recorded(u0, v0, tau, nsteps, source, g, receivers, record_every, steps_per_launch, stop_flag, traces, c2, damping, None)

    def _wave_recorded(self, u0, v0, tau, nsteps, source, g, receivers, record_every, steps_per_launch, stop_flag, traces, c2, damping, _hist):
        """wave_record_many, and with _hist ([nsys, nsteps + 1, size] of u0's kind, zeros; c2 given, no damping) wave_history_many."""
        nsys, on_device, sp = self._batched(u0, g, ("u0", "g", "forcings", "ensemble"), _capi.MANY_MAX, stop_flag)
        if self._check_batch(v0, self.size, _capi.MANY_MAX) != (nsys, on_device) or (on_device and v0.device != u0.device):
            raise ValueError(f"v0 has shape {tuple(v0.shape)}: the velocities are of the kind (NumPy / CUDA tensor), shape and device of u0, {tuple(u0.shape)}")
        tau, nsteps, res, steps_done, _ = self._ensemble_steps(nsys, tau, nsteps, False)
        record_every = int(record_every)
        if record_every < 1:
            raise ValueError(f"record_every {record_every} rejected: it must be >= 1")
        nodes = np.ascontiguousarray(receivers if receivers is not None else [], dtype=np.int32)
        if nodes.ndim != 1 or len(nodes) > _capi.WAVE_MAX_RECEIVERS:
            raise ValueError(f"receivers has shape {nodes.shape}: a sequence of at most {_capi.WAVE_MAX_RECEIVERS} packed indices")
        nrec = len(nodes)
        if not on_device and hasattr(source, "data_ptr"):
            raise ValueError("source is of the kind (NumPy / CUDA tensor) of u0")
        shapes = ((nsteps + 1,), (nsys, nsteps + 1))
        tshape = (nsys, nsteps // record_every, nrec)
        cshapes = ((self.size,), (nsys, self.size))
        if damping is not None and c2 is None:                       # a unit medium: 1.0 * t == t
            if on_device:
                import torch
                c2 = torch.ones(self.size, dtype=torch.float64, device=u0.device)
            else:
                c2 = np.ones(self.size)
        if not on_device:
            fields = {"c2": c2, "damping": damping}
            for name, a in fields.items():
                if a is None:
                    continue
                if hasattr(a, "data_ptr"):
                    raise ValueError(f"{name} is of the kind (NumPy / CUDA tensor) of u0")
                a = fields[name] = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape not in cshapes:
                    raise ValueError(f"{name} has shape {a.shape}, expected {cshapes[0]} or {cshapes[1]}")
            c2, damping = fields["c2"], fields["damping"]
        if on_device:
            import torch
            for name, a, want in (("source", source, shapes), ("traces", traces, (tshape,)), ("c2", c2, cshapes), ("damping", damping, cshapes)):
                if a is not None and not (hasattr(a, "data_ptr") and a.is_cuda and a.device == u0.device and a.dtype == torch.float64
                                          and tuple(a.shape) in want and a.is_contiguous()):
                    raise ValueError(f"{name} beside CUDA states is a contiguous float64 tensor of shape {' or '.join(map(str, want))} on {u0.device}")
            u, v = u0.clone(), v0.clone()
            if nrec and traces is None:
                traces = torch.zeros(tshape, dtype=torch.float64, device=u0.device)
            torch.cuda.current_stream(u0.device).synchronize()
            fn = (self._lib.mi355cg_wave_record_many_device if c2 is None else self._lib.mi355cg_wave_medium_many_device if damping is None
                  else self._lib.mi355cg_wave_sponge_many_device)
            medium = tuple(x for a in (c2, damping) if a is not None for x in (a.data_ptr(), self.size if a.dim() == 2 else 0))
            if _hist is not None:                                    # wave_history_many: checked there
                fn, medium = self._lib.mi355cg_wave_history_many_device, medium + (_hist.data_ptr(), (nsteps + 1) * self.size)
            rc = fn(self._h, nsys, nsteps, tau.ctypes.data, g.data_ptr() if g is not None else None, u.data_ptr(), v.data_ptr(), *medium, source.data_ptr(),
                    nsteps + 1 if source.dim() == 2 else 0, nrec, nodes.ctypes.data if nrec else None, record_every, traces.data_ptr() if nrec else None,
                    int(steps_per_launch), sp, res, steps_done.ctypes.data)
        else:
            source = np.ascontiguousarray(source, dtype=np.float64)
            if source.shape not in shapes:
                raise ValueError(f"source has shape {source.shape}, expected {shapes[0]} or {shapes[1]}")
            if traces is not None and not (isinstance(traces, np.ndarray) and traces.dtype == np.float64 and traces.shape == tshape and traces.flags.c_contiguous):
                raise ValueError(f"traces is a contiguous float64 array of shape {tshape}")
            u = np.array(u0, dtype=np.float64, order="C", copy=True)
            v = np.array(v0, dtype=np.float64, order="C", copy=True)
            if g is not None:
                g = np.ascontiguousarray(g)
            if nrec and traces is None:
                traces = np.zeros(tshape)
            fn = (self._lib.mi355cg_wave_record_many if c2 is None else self._lib.mi355cg_wave_medium_many if damping is None
                  else self._lib.mi355cg_wave_sponge_many)
            medium = tuple(x for a in (c2, damping) if a is not None for x in (a.ctypes.data, self.size if a.ndim == 2 else 0))
            if _hist is not None:
                fn, medium = self._lib.mi355cg_wave_history_many, medium + (_hist.ctypes.data, (nsteps + 1) * self.size)
            rc = fn(self._h, nsys, nsteps, tau.ctypes.data, g.ctypes.data if g is not None else None, u.ctypes.data, v.ctypes.data, *medium, source.ctypes.data,
                    nsteps + 1 if source.ndim == 2 else 0, nrec, nodes.ctypes.data if nrec else None, record_every, traces.ctypes.data if nrec else None,
                    int(steps_per_launch), sp, res, steps_done.ctypes.data)
        self._check_rc(rc)
        return u, v, (traces if nrec else None), list(res), steps_done

    def wave_history_many(self, u0, v0, tau, nsteps: int, source, g=None, receivers=None, record_every: int = 1, steps_per_launch: int = 0,
                          stop_flag: Optional[C.c_int] = None, traces=None, c2=None):
        """wave_record_many in the medium c2 (None: a unit medium) that also returns the history (mi355cg_wave_history_many):
        (u, v, traces, hist, [Results per member], steps_done), hist [nsys, nsteps + 1, size] of u0's kind with hist[s, n] = au(u_n)
        of member s, zeros in the rows of steps that did not run."""
        nsys, on_device = self._check_batch(u0, self.size, _capi.MANY_MAX)
        nsteps = int(nsteps)
        if not 0 <= nsteps <= _capi.STEPS_MANY_MAX_STEPS:
            raise ValueError(f"nsteps {nsteps} rejected: it must be 0 .. {_capi.STEPS_MANY_MAX_STEPS}")
        if on_device:
            import torch
            if c2 is None:
                c2 = torch.ones(self.size, dtype=torch.float64, device=u0.device)
            hist = torch.zeros((nsys, nsteps + 1, self.size), dtype=torch.float64, device=u0.device)
        else:
            if c2 is None:
                c2 = np.ones(self.size)
            hist = np.zeros((nsys, nsteps + 1, self.size))
        u, v, traces, res, done = self._wave_recorded(u0, v0, tau, nsteps, source, g, receivers, record_every, steps_per_launch, stop_flag, traces, c2, None, hist)
        return u, v, traces, hist, res, done

    def wave_adjoint_many(self, hist, tau, c2, adjoint_source, receivers=None, record_every: int = 1, lam=None, q=None, sens=None,
                          steps_per_launch: int = 0, stop_flag: Optional[C.c_int] = None, return_info: bool = False):
        """The transpose of the steps whose history is hist (mi355cg_wave_adjoint_many): (lam, q, sens) after nsteps =
        hist.shape[1] - 1 backward steps from the incoming (lam, q, sens), None = zeros; with return_info also ([Results per
        member], steps_done).  hist: [nsys, nsteps + 1, size] float64, NumPy or a contiguous CUDA tensor; c2 ([size] or [nsys,
        size], None: a unit medium), adjoint_source ([nsteps // record_every, nrec] for all members or [nsys, nsteps //
        record_every, nrec]; None without receivers) and lam, q, sens ([nsys, size]) of its kind.  Nothing passed in is modified."""
        on_device = not isinstance(hist, np.ndarray)
        if on_device:
            if not (type(hist).__module__.split(".")[0] == "torch" and hasattr(hist, "data_ptr")):
                raise ValueError(f"a history is a NumPy array or a CUDA torch tensor, not {type(hist).__name__}")
            import torch
            if not (hist.is_cuda and hist.dtype == torch.float64 and hist.is_contiguous()):
                raise ValueError("a torch history is a contiguous float64 tensor in device memory")
            if hist.device.index != self._device:
                raise ValueError(f"hist is on {hist.device}, the handle on device {self._device}")
        elif hist.dtype != np.float64:
            raise ValueError(f"hist has dtype {hist.dtype}, expected float64")
        shape = tuple(hist.shape)
        if len(shape) != 3 or shape[2] != self.size or shape[1] < 1 or not 1 <= shape[0] <= _capi.MANY_MAX:
            raise ValueError(f"hist has shape {shape}, expected (1 .. {_capi.MANY_MAX} members, nsteps + 1, {self.size})")
        nsys, nsteps = shape[0], shape[1] - 1
        tau, nsteps, res, steps_done, _ = self._ensemble_steps(nsys, tau, nsteps, False)
        record_every = int(record_every)
        if record_every < 1:
            raise ValueError(f"record_every {record_every} rejected: it must be >= 1")
        nodes = np.ascontiguousarray(receivers if receivers is not None else [], dtype=np.int32)
        if nodes.ndim != 1 or len(nodes) > _capi.WAVE_MAX_RECEIVERS:
            raise ValueError(f"receivers has shape {nodes.shape}: a sequence of at most {_capi.WAVE_MAX_RECEIVERS} packed indices")
        nrec = len(nodes)
        samples = nsteps // record_every
        cshapes = ((self.size,), (nsys, self.size))
        ashapes = ((samples, nrec), (nsys, samples, nrec))
        state = ((nsys, self.size),)
        sp = C.cast(C.pointer(stop_flag), C.c_void_p) if stop_flag is not None else None
        if nrec and adjoint_source is None:
            raise ValueError(f"{nrec} receivers need adjoint_source")
        if on_device:
            if c2 is None:
                c2 = torch.ones(self.size, dtype=torch.float64, device=hist.device)
            for name, a, want in (("c2", c2, cshapes), ("adjoint_source", adjoint_source if nrec else None, ashapes), ("lam", lam, state), ("q", q, state), ("sens", sens, state)):
                if a is not None and not (hasattr(a, "data_ptr") and a.is_cuda and a.device == hist.device and a.dtype == torch.float64
                                          and tuple(a.shape) in want and a.is_contiguous()):
                    raise ValueError(f"{name} beside a CUDA history is a contiguous float64 tensor of shape {' or '.join(map(str, want))} on {hist.device}")
            lam, q, sens = (torch.zeros(state[0], dtype=torch.float64, device=hist.device) if a is None else a.clone() for a in (lam, q, sens))
            torch.cuda.current_stream(hist.device).synchronize()
            rc = self._lib.mi355cg_wave_adjoint_many_device(
                self._h, nsys, nsteps, tau.ctypes.data, c2.data_ptr(), self.size if c2.dim() == 2 else 0, hist.data_ptr(), (nsteps + 1) * self.size, nrec,
                nodes.ctypes.data if nrec else None, record_every, adjoint_source.data_ptr() if nrec else None,
                samples * nrec if nrec and adjoint_source.dim() == 3 else 0, lam.data_ptr(), q.data_ptr(), sens.data_ptr(), int(steps_per_launch), sp, res,
                steps_done.ctypes.data)
        else:
            c2 = np.ones(self.size) if c2 is None else c2
            arrays = {"c2": (c2, cshapes), "adjoint_source": (adjoint_source if nrec else None, ashapes), "lam": (lam, state), "q": (q, state), "sens": (sens, state)}
            for name, (a, want) in arrays.items():
                if a is None:
                    continue
                if hasattr(a, "data_ptr"):
                    raise ValueError(f"{name} is of the kind (NumPy / CUDA tensor) of hist")
                a = np.ascontiguousarray(a, dtype=np.float64)
                if a.shape not in want:
                    raise ValueError(f"{name} has shape {a.shape}, expected {' or '.join(map(str, want))}")
                arrays[name] = (a, want)
            c2, adjoint_source = arrays["c2"][0], arrays["adjoint_source"][0]
            lam, q, sens = (np.zeros(state[0]) if arrays[k][0] is None else np.array(arrays[k][0], dtype=np.float64, order="C", copy=True) for k in ("lam", "q", "sens"))
            hist = np.ascontiguousarray(hist)
            rc = self._lib.mi355cg_wave_adjoint_many(
                self._h, nsys, nsteps, tau.ctypes.data, c2.ctypes.data, self.size if c2.ndim == 2 else 0, hist.ctypes.data, (nsteps + 1) * self.size, nrec,
                nodes.ctypes.data if nrec else None, record_every, adjoint_source.ctypes.data if nrec else None,
                samples * nrec if nrec and adjoint_source.ndim == 3 else 0, lam.ctypes.data, q.ctypes.data, sens.ctypes.data, int(steps_per_launch), sp, res,
                steps_done.ctypes.data)
        self._check_rc(rc)
        return (lam, q, sens, list(res), steps_done) if return_info else (lam, q, sens)

    def wave_gradient_many(self, u0, v0, tau, nsteps: int, source, observed, g=None, receivers=None, record_every: int = 1, c2=None, segment=None):
        """(misfit [nsys], grad_c2, grad_u0, grad_v0, traces) of J_s = 1/2 sum (traces_s - observed_s)^2 by one forward run with
        its history and one backward run; with segment=K in segments of K steps from checkpoints of (u, v).  Everything runs on
        the device; NumPy arguments go up once and the results come down once."""
        nsys, on_device = self._check_batch(u0, self.size, _capi.MANY_MAX)
        import torch
        dev = torch.device("cuda", self._device)
        nodes = [int(r) for r in (receivers if receivers is not None else [])]
        if not nodes:
            raise ValueError("wave_gradient_many needs receivers: the misfit is a sum over the traces")
        tau, nsteps, _, _, _ = self._ensemble_steps(nsys, tau, nsteps, False)
        record_every = int(record_every)
        if record_every < 1:
            raise ValueError(f"record_every {record_every} rejected: it must be >= 1")
        K = nsteps if segment is None else int(segment)
        if segment is not None and (K < 1 or K % record_every):
            raise ValueError(f"segment {segment} rejected: a positive multiple of record_every = {record_every}")
        samples = nsteps // record_every

        def up(name, a, shapes):
            if a is None:
                return None
            if on_device != (not isinstance(a, np.ndarray) and hasattr(a, "data_ptr")):
                raise ValueError(f"{name} is of the kind (NumPy / CUDA tensor) of u0")
            if not on_device:
                a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
            if tuple(a.shape) not in shapes or a.dtype != torch.float64 or not a.is_cuda:
                raise ValueError(f"{name} has shape {tuple(a.shape)}, expected float64 of shape {' or '.join(map(str, shapes))}")
            return a.contiguous()

        state = ((nsys, self.size),)
        u0d, v0d, gd = up("u0", u0, state), up("v0", v0, state), up("g", g, state)
        c2d = up("c2", c2, ((self.size,), (nsys, self.size)))
        if c2d is None:
            c2d = torch.ones(self.size, dtype=torch.float64, device=dev)
        wd = up("source", source, ((nsteps + 1,), (nsys, nsteps + 1)))
        od = up("observed", observed, ((nsys, samples, len(nodes)),))
        if wd is None or od is None:
            raise ValueError("source and observed are required")
        cuts = [(a, min(K, nsteps - a)) for a in range(0, nsteps, max(K, 1))]
        hist = None
        if len(cuts) <= 1:                                           # the whole history at once
            _, _, traces, hist, _, _ = self.wave_history_many(u0d, v0d, tau, nsteps, wd, g=gd, receivers=nodes, record_every=record_every, c2=c2d)
            starts = [(u0d, v0d)]
        else:                                                        # forward in segments: (u, v) at every segment start stays on the device
            traces = torch.zeros((nsys, samples, len(nodes)), dtype=torch.float64, device=dev)
            starts, u, v = [], u0d, v0d
            for a, k in cuts:
                starts.append((u, v))
                u, v, tr, _, _ = self.wave_record_many(u, v, tau, k, wd[..., a:a + k + 1].contiguous(), g=gd, receivers=nodes, record_every=record_every, c2=c2d)
                traces[:, a // record_every:(a + k) // record_every] = tr
        r = traces - od                                              # the adjoint source: one rounding
        rh = r.cpu().numpy()
        misfit = 0.5 * np.sum((rh * rh).reshape(nsys, -1), axis=-1)
        lam = q = sens = None
        for (a, k), (u, v) in zip(reversed(cuts), reversed(starts)):
            if hist is None:
                hist = self.wave_history_many(u, v, tau, k, wd[..., a:a + k + 1].contiguous(), g=gd, receivers=nodes, record_every=record_every, c2=c2d)[3]
            lam, q, sens = self.wave_adjoint_many(hist, tau, c2d, r[:, a // record_every:(a + k) // record_every].contiguous(), receivers=nodes,
                                                  record_every=record_every, lam=lam, q=q, sens=sens)
            hist = None
        if lam is None:                                              # no steps: nothing depends on anything
            lam = q = sens = torch.zeros((nsys, self.size), dtype=torch.float64, device=dev)
        h = torch.from_numpy(0.5 * tau).to(dev)[:, None]
        out = (h * sens / c2d, lam, q / c2d, traces)
        if on_device:
            return (torch.from_numpy(misfit).to(dev),) + out
        return (misfit,) + tuple(t.cpu().numpy() for t in out)

    def wave_cfl(self, c2=None):
        """The largest time step velocity Verlet takes on this grid, 2 / sqrt(2 |A_diag|) of the unshifted operator (mi355cg_wave_cfl).
        c2: a medium, [size] or [nsys, size] (NumPy or tensor): the bound 2 / sqrt(2 |A_diag| max c2) of that medium, or an array
        [nsys] of them (mi355cg_wave_medium_cfl); the max is NumPy's or torch's."""
        out = C.c_double()
        if c2 is not None:
            top = c2.amax(dim=-1).cpu().numpy() if hasattr(c2, "data_ptr") else np.max(np.asarray(c2, dtype=np.float64), axis=-1)
            if top.ndim > 1:
                raise ValueError(f"c2 has shape {tuple(c2.shape)}: a medium is [size] or [nsys, size]")
            bounds = []
            for c2max in np.atleast_1d(top):
                rc = self._lib.mi355cg_wave_medium_cfl(self._h, float(c2max), C.byref(out))
                self._check_rc(rc)
                bounds.append(out.value)
            return bounds[0] if top.ndim == 0 else np.array(bounds)
        self._check_rc(self._lib.mi355cg_wave_cfl(self._h, C.byref(out)))
        return out.value

    def solve_many_info(self, nsys: int):
        """{"lds_bytes_per_workgroup", "workgroups_per_cu", "workspace_bytes"} of a solve_many batch of nsys systems on this grid
        (mi355cg_solve_many_info); ValueError for handles solve_many refuses."""
        lds, wg, ws = C.c_int(), C.c_int(), C.c_longlong()
        rc = self._lib.mi355cg_solve_many_info(self._h, int(nsys), C.byref(lds), C.byref(wg), C.byref(ws))
        self._check_rc(rc)
        return {"lds_bytes_per_workgroup": lds.value, "workgroups_per_cu": wg.value, "workspace_bytes": ws.value}

    @staticmethod
    def _check_block(v, size, most, what):
        """A group of packed vectors for the block utilities: NumPy [n, size] float64, 1 <= n <= most, C-contiguous on return."""
        if not isinstance(v, np.ndarray):
            raise ValueError(f"{what} is a NumPy array, not {type(v).__name__}")
        if v.dtype != np.float64:
            raise ValueError(f"{what} has dtype {v.dtype}, expected float64")
        if v.ndim != 2 or v.shape[1] != size:
            raise ValueError(f"{what} has shape {tuple(v.shape)}, expected (n, {size})")
        if not 1 <= v.shape[0] <= most:
            raise ValueError(f"{what} has 1 .. {most} vectors, not {v.shape[0]}")
        return np.ascontiguousarray(v)

    def eigs(self, nev: int, block: int, tol: float, max_iterations: int, x, stop_flag: Optional[C.c_int] = None):
        """The nev lowest eigenpairs by the block multigrid-preconditioned iteration (mi355cg_eigs; needs set_preconditioner
        first).  x: the start block, NumPy [block, size] float64 (a new array comes back) or a contiguous CUDA torch tensor
        on the handle's device (mi355cg_eigs_device; a new tensor comes back).  Returns (lambda[block], Ritz vectors
        [block, size], resid[block], _capi.EigResults)."""
        nev, block = int(nev), int(block)
        on_device = not isinstance(x, np.ndarray)
        if on_device:
            if not (type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")):
                raise ValueError(f"a start block is a NumPy array or a CUDA torch tensor, not {type(x).__name__}")
            import torch
            if not x.is_cuda:
                raise ValueError("a torch start block must be in device memory (a CPU tensor: pass tensor.numpy())")
            if x.dtype != torch.float64:
                raise ValueError(f"start block has dtype {x.dtype}, expected torch.float64")
            if x.device.index != self._device:
                raise ValueError(f"start block is on {x.device}, the handle on device {self._device}")
        elif x.dtype != np.float64:
            raise ValueError(f"start block has dtype {x.dtype}, expected float64")
        if tuple(x.shape) != (block, self.size):
            raise ValueError(f"start block has shape {tuple(x.shape)}, expected ({block}, {self.size})")
        lam, res = np.zeros(max(block, 1)), np.zeros(max(block, 1))
        out = _capi.EigResults()
        sp = C.cast(C.pointer(stop_flag), C.c_void_p) if stop_flag is not None else None
        if on_device:
            v = x.contiguous().clone()
            torch.cuda.current_stream(x.device).synchronize()        # the library works on its own stream
            rc = self._lib.mi355cg_eigs_device(self._h, nev, block, float(tol), int(max_iterations), v.data_ptr(), lam.ctypes.data,
                                               res.ctypes.data, sp, C.byref(out))
        else:
            v = np.array(x, dtype=np.float64, order="C", copy=True)
            rc = self._lib.mi355cg_eigs(self._h, nev, block, float(tol), int(max_iterations), v.ctypes.data, lam.ctypes.data,
                                        res.ctypes.data, sp, C.byref(out))
        self._check_rc(rc)
        return lam[:block], v, res[:block], out

    def eigs_release(self):
        """Free the workspace eigs keeps on the handle (nothing to free is fine)."""
        _capi.check(self._lib.mi355cg_eigs_release(self._h))

    def block_gram(self, a, b, rows=None, cols=None):
        """C[i, j] = a[i] . b[j] on the device in a fixed summation order (mi355cg_block_gram).  rows / cols: index lists into a
        and b; the result then has the listed rows and columns only (mi355cg_block_gram_indexed)."""
        a = self._check_block(a, self.size, _capi.EIG_BASIS_MAX, "a")
        b = self._check_block(b, self.size, _capi.EIG_BASIS_MAX, "b")
        ia = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        ib = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32)
        out = np.empty((a.shape[0] if ia is None else ia.size, b.shape[0] if ib is None else ib.size))
        rc = self._lib.mi355cg_block_gram_indexed(self._h, a.shape[0], a.ctypes.data, 0 if ia is None else ia.size,
                                                  None if ia is None else ia.ctypes.data, b.shape[0], b.ctypes.data,
                                                  0 if ib is None else ib.size, None if ib is None else ib.ctypes.data, out.ctypes.data)
        self._check_rc(rc)
        return out

    def block_combine(self, s, coef):
        """y[j] = sum_i s[i] * coef[i, j], i ascending, unfused (mi355cg_block_combine); s: [k, size], coef: [k, m] -> [m, size]."""
        s = self._check_block(s, self.size, _capi.EIG_BASIS_MAX, "s")
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        if coef.ndim != 2 or coef.shape[0] != s.shape[0] or not 1 <= coef.shape[1] <= _capi.EIG_BLOCK_MAX:
            raise ValueError(f"coef has shape {tuple(coef.shape)}, expected ({s.shape[0]}, 1 .. {_capi.EIG_BLOCK_MAX})")
        y = np.empty((coef.shape[1], self.size))
        rc = self._lib.mi355cg_block_combine(self._h, s.shape[0], s.ctypes.data, coef.shape[1], coef.ctypes.data, y.ctypes.data)
        self._check_rc(rc)
        return y

    def setup_on_device(self):
        """Opt-in: regenerate b and u on the GPU (<= 1 ulp from the host values)."""
        _capi.check(self._lib.mi355cg_setup_on_device(self._h))

    def set_profiling(self, on: bool):
        _capi.check(self._lib.mi355cg_set_profiling(self._h, 1 if on else 0))

    def kernel_time(self, kernel: int):
        ms, n = C.c_double(), C.c_longlong()
        _capi.check(self._lib.mi355cg_get_kernel_time(self._h, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def layout(self):
        L = C.c_longlong()
        v = [C.c_int() for _ in range(5)]
        _capi.check(self._lib.mi355cg_get_layout(self._h, C.byref(L), *[C.byref(i) for i in v]))
        fold, extra = C.c_int(), C.c_int()
        if hasattr(self._lib, "mi355cg_get_xfold"):      # an older build of the ABI (MI355CG_LIB) has no deferred x fold
            _capi.check(self._lib.mi355cg_get_xfold(self._h, C.byref(fold), C.byref(extra)))
        # x_fold: depth of the deferred x fold in use (0 = fused update); x_fold_buffers: vectors its ring has allocated so far
        return {"padded_len": L.value, "pitch_bottom": v[0].value, "pitch_upper": v[1].value,
                "grid_stencil": v[2].value, "grid_update": v[3].value, "rows_per_item": v[4].value,
                "x_fold": fold.value, "x_fold_buffers": extra.value}


def default_params(rule: int) -> _capi.Params:
    p = _capi.Params()
    _capi.load().mi355cg_default_params(C.byref(p), rule)
    return p


def mg_levels(n: int):
    """(levels, coarsest n) of the multigrid hierarchy of an n x n grid (host arithmetic, no GPU); ValueError if it has none."""
    L, nc = C.c_int(), C.c_int()
    lib = _capi.load()
    rc = lib.mi355cg_mg_levels(int(n), C.byref(L), C.byref(nc))
    if rc == _capi.ERR_INVALID:
        raise ValueError(lib.mi355cg_last_error().decode())
    _capi.check(rc)
    return L.value, nc.value


def mg_hierarchy(n: int, kind: int = _capi.PRECOND_MG_ANY):
    """The intervals (N_0 = n, N_1, ..., N_L) of the multigrid levels kind builds for an n x n grid (host arithmetic, no GPU);
    ValueError if kind has none for n, n is odd or < 6, or kind is not a multigrid kind."""
    L = C.c_int()
    buf = (C.c_int * 64)()
    lib = _capi.load()
    rc = lib.mi355cg_mg_hierarchy(int(kind), int(n), len(buf), C.byref(L), buf)
    if rc == _capi.ERR_INVALID:
        raise ValueError(lib.mi355cg_last_error().decode())
    _capi.check(rc)
    return tuple(buf[:L.value])


def onchip_plan(n: int):
    """The layout of the on-chip solve mode for an n x n grid (host arithmetic, no GPU): a dict with the workgroup's `threads`, the
    `lds_bytes` in use and the unknowns per thread `elems_per_thread`; ValueError if n is odd, < 6 or above the mode's cap."""
    t, lds, e = C.c_int(), C.c_int(), C.c_int()
    lib = _capi.load()
    rc = lib.mi355cg_onchip_plan(int(n), C.byref(t), C.byref(lds), C.byref(e))
    if rc == _capi.ERR_INVALID:
        raise ValueError(lib.mi355cg_last_error().decode())
    _capi.check(rc)
    return {"threads": t.value, "lds_bytes": lds.value, "elems_per_thread": e.value}


def time_steps_many_workspace(n: int, nsys: int, nsteps: int, with_step_iterations: bool = True) -> int:
    """The device workspace bytes of MatrixFreeSystem.time_steps_many for nsys members and nsteps steps on an n x n grid (host
    arithmetic, no GPU; mi355cg_time_steps_many_workspace).  The Python interface always asks for the per-step iteration counts.
    ValueError for a grid or an ensemble the call refuses."""
    out = C.c_longlong()
    lib = _capi.load()
    rc = lib.mi355cg_time_steps_many_workspace(int(n), int(nsys), int(nsteps), 1 if with_step_iterations else 0, C.byref(out))
    if rc == _capi.ERR_INVALID:
        raise ValueError(lib.mi355cg_last_error().decode())
    _capi.check(rc)
    return out.value


def wave_steps_many_workspace(n: int, nsys: int, nsteps: int, scheme: int = _capi.WAVE_VERLET, with_step_iterations: bool = False) -> int:
    """The device workspace bytes of MatrixFreeSystem.wave_steps_many for nsys members and nsteps steps on an n x n grid (host
    arithmetic, no GPU; mi355cg_wave_steps_many_workspace).  ValueError for a grid, an ensemble or a scheme the call refuses."""
    out = C.c_longlong()
    lib = _capi.load()
    rc = lib.mi355cg_wave_steps_many_workspace(int(n), int(nsys), int(nsteps), int(scheme), 1 if with_step_iterations else 0, C.byref(out))
    if rc == _capi.ERR_INVALID:
        raise ValueError(lib.mi355cg_last_error().decode())
    _capi.check(rc)
    return out.value


def wave_record_many_workspace(n: int, nsys: int, nsteps: int, nrec: int = 0, record_every: int = 1) -> int:
    """The device workspace bytes of MatrixFreeSystem.wave_record_many for nsys members, nsteps steps and nrec receivers on an n x n
    grid (host arithmetic, no GPU; mi355cg_wave_record_many_workspace).  ValueError for what the call refuses."""
    out = C.c_longlong()
    lib = _capi.load()
    rc = lib.mi355cg_wave_record_many_workspace(int(n), int(nsys), int(nsteps), int(nrec), int(record_every), C.byref(out))
    if rc == _capi.ERR_INVALID:
        raise ValueError(lib.mi355cg_last_error().decode())
    _capi.check(rc)
    return out.value


def wave_medium_many_workspace(n: int, nsys: int, nsteps: int, nrec: int = 0, record_every: int = 1) -> int:
    """The device workspace bytes of MatrixFreeSystem.wave_record_many with a medium c2 (host arithmetic, no GPU;
    mi355cg_wave_medium_many_workspace): those of the call without it and 16 bytes per member.  ValueError for what the call refuses."""
    out = C.c_longlong()
    lib = _capi.load()
    rc = lib.mi355cg_wave_medium_many_workspace(int(n), int(nsys), int(nsteps), int(nrec), int(record_every), C.byref(out))
    if rc == _capi.ERR_INVALID:
        raise ValueError(lib.mi355cg_last_error().decode())
    _capi.check(rc)
    return out.value


def wave_sponge_many_workspace(n: int, nsys: int, nsteps: int, nrec: int = 0, record_every: int = 1) -> int:
    """The device workspace bytes of MatrixFreeSystem.wave_record_many with a damping field (host arithmetic, no GPU;
    mi355cg_wave_sponge_many_workspace): those of the call with c2 alone and 16 bytes per member.  ValueError for what the call refuses."""
    out = C.c_longlong()
    lib = _capi.load()
    rc = lib.mi355cg_wave_sponge_many_workspace(int(n), int(nsys), int(nsteps), int(nrec), int(record_every), C.byref(out))
    if rc == _capi.ERR_INVALID:
        raise ValueError(lib.mi355cg_last_error().decode())
    _capi.check(rc)
    return out.value


def wave_history_bytes(n: int, nsys: int, nsteps: int) -> int:
    """The bytes of the history MatrixFreeSystem.wave_history_many writes for nsys members and nsteps steps on an n x n grid: 8 *
    nsys * (nsteps + 1) * size (host arithmetic, no GPU; mi355cg_wave_history_bytes).  ValueError for what the call refuses."""
    out = C.c_longlong()
    lib = _capi.load()
    rc = lib.mi355cg_wave_history_bytes(int(n), int(nsys), int(nsteps), C.byref(out))
    if rc == _capi.ERR_INVALID:
        raise ValueError(lib.mi355cg_last_error().decode())
    _capi.check(rc)
    return out.value


def wave_adjoint_many_workspace(n: int, nsys: int, nsteps: int, nrec: int = 0, record_every: int = 1) -> int:
    """The device workspace bytes of MatrixFreeSystem.wave_adjoint_many (host arithmetic, no GPU;
    mi355cg_wave_adjoint_many_workspace): those of wave_record_many with a medium.  ValueError for what the call refuses."""
    out = C.c_longlong()
    lib = _capi.load()
    rc = lib.mi355cg_wave_adjoint_many_workspace(int(n), int(nsys), int(nsteps), int(nrec), int(record_every), C.byref(out))
    if rc == _capi.ERR_INVALID:
        raise ValueError(lib.mi355cg_last_error().decode())
    _capi.check(rc)
    return out.value


def sponge_damping(n: int, width: int, dmax: float, sides: str = "lrbt"):
    """A sponge layer for wave_record_many(damping=) on the L-shaped grid of n intervals a side, pure NumPy: the [size] field
    dmax * ((width - k) / width)^2 in the packed order, k the node distance of an unknown to the nearest chosen outer side of the
    bounding square, counted from the first interior line (k = 0 there: the field is dmax; the side itself holds no unknown), 0
    where k >= width: `width` lines of unknowns are damped.  sides: letters of "lrbt" -- left (ix = 0), right (ix = n), bottom
    (iy = 0), top (iy = n).  The two sides of the cut-out quadrant are not outer sides: they stay reflecting."""
    n, width = int(n), int(width)
    if n < 2 or n % 2:
        raise ValueError(f"n = {n} rejected: the grid has an even number of intervals a side")
    if width < 1:
        raise ValueError(f"width {width} rejected: a layer is at least one node wide")
    if not np.isfinite(dmax) or dmax < 0:
        raise ValueError(f"dmax {dmax} rejected: a damping rate is finite and >= 0")
    if not sides or set(sides) - set("lrbt"):
        raise ValueError(f"sides {sides!r} rejected: letters of 'lrbt'")
    half = n // 2
    # the packed order (packed_index): the bottom-right block row-major, then the upper block row-major
    ix = np.concatenate([np.tile(np.arange(half + 1, n), half), np.tile(np.arange(1, n), half - 1)])
    iy = np.concatenate([np.repeat(np.arange(1, half + 1), half - 1), np.repeat(np.arange(half + 1, n), n - 1)])
    k = np.full(ix.shape, width)
    for side, dist in (("l", ix), ("r", n - ix), ("b", iy), ("t", n - iy)):
        if side in sides:
            k = np.minimum(k, dist - 1)
    return float(dmax) * ((width - k) / width) ** 2


def rayleigh_ritz(g, h):
    """The Rayleigh-Ritz step of eigs on the host (mi355cg_rayleigh_ritz, no GPU): for the k x k pair G = S^T S, H = S^T K S
    (k <= 48) returns (theta[k] ascending, coef[k, k]) with coef.T @ G @ coef = I and coef.T @ H @ coef = diag(theta).
    ValueError for a bad shape; Mi355cgError (code ERR_STATE) for a basis that is refused as numerically dependent."""
    g = np.ascontiguousarray(g, dtype=np.float64)
    h = np.ascontiguousarray(h, dtype=np.float64)
    if g.ndim != 2 or g.shape[0] != g.shape[1] or h.shape != g.shape:
        raise ValueError(f"G and H are square matrices of one size, not {tuple(g.shape)} and {tuple(h.shape)}")
    k = g.shape[0]
    theta, coef = np.empty(max(k, 1)), np.empty((max(k, 1), max(k, 1)))
    lib = _capi.load()
    rc = lib.mi355cg_rayleigh_ritz(k, g.ctypes.data, h.ctypes.data, theta.ctypes.data, coef.ctypes.data)
    if rc == _capi.ERR_INVALID:
        raise ValueError(lib.mi355cg_last_error().decode())
    _capi.check(rc)
    return theta, coef


# ---------------------------------------------------------------------------------------------
class MatrixFreeSystem:
    """solver/matrix_free_system.hpp:12-70.  Constructor order is (m, n, a, b, c, d)."""

    def __init__(self, m, n, a, b, c, d, device: int = 0, dtype: int = _capi.F64):
        self.n, self.m = n, m
        self.domain = (a, b, c, d)
        self._handle = _Handle(n, m, a, b, c, d, dtype=dtype, device=device)

    def get_rhs(self) -> np.ndarray: return self._handle.rhs()
    def get_true_solution_vector(self) -> np.ndarray: return self._handle.true_solution()
    def size(self) -> int: return self._handle.size

    def apply(self, x, y=None) -> np.ndarray:
        out = self._handle.apply(x)
        if y is not None:
            y[...] = out
            return y
        return out

    def __mul__(self, x): return self.apply(x)             # operator* (matrix_free_system.hpp:59-63)

    def set_preconditioner(self, kind: int, cycle: int = _capi.CYCLE_F64):
        """Extension (no reference twin): _capi.PRECOND_MG / PRECOND_MG_ANY / PRECOND_NONE.  Every solver built on this system
        (MatrixFreeSolver, MSGSolver) runs preconditioned CG while it is set.  cycle = _capi.CYCLE_F32 runs the V-cycle in fp32;
        the CG vectors, inner products and stop tests stay fp64."""
        self._handle.set_preconditioner(kind, cycle)

    def preconditioner_info(self):
        """(kind, cycle, levels) of the preconditioner that is set; (PRECOND_NONE, CYCLE_F64, 0) without one."""
        return self._handle.preconditioner_info()

    def set_solve_mode(self, mode: int):
        """Extension (no reference twin): SOLVE_ONCHIP / SOLVE_LAUNCHES.  In the on-chip mode every plain fp64 solve built on this
        system (MatrixFreeSolver without diagnostics, MSGSolver, time_steps) runs its chunks of iterations as one launch of one
        workgroup: the same bits, a fraction of the launch cost, grids up to N = 128.  ValueError if the system is not eligible."""
        self._handle.set_solve_mode(mode)

    def solve_mode_info(self):
        """{"mode", "onchip_launches" of the last solve, "plan": onchip_plan(n) or None above the cap}."""
        mode, launches = self._handle.solve_mode_info()
        try:
            plan = onchip_plan(self.n)
        except ValueError:
            plan = None
        return {"mode": mode, "onchip_launches": launches, "plan": plan}

    def set_smoother(self, smoother: int):
        """Extension (no reference twin): _capi.SMOOTHER_JACOBI (the default) or SMOOTHER_LINE_X / _LINE_Y / _LINE_AUTO, line
        Jacobi along the strongly coupled direction of a stretched domain, for the fp64 V-cycle of this system's preconditioner
        and everything built on it.  Before or after set_preconditioner."""
        self._handle.set_smoother(smoother)

    def smoother_info(self):
        """(smoother, direction): the smoother as set, and the line direction it means on this grid (0 none, 1 x, 2 y)."""
        return self._handle.smoother_info()

    def set_shift(self, sigma: float):
        """Extension (no reference twin): this system's operator becomes A - sigma I (sigma finite, >= 0) for apply() and for every
        solver built on it, preconditioned and batched solves included; 0 restores the Laplacian bit for bit."""
        self._handle.set_shift(sigma)

    @property
    def shift(self) -> float:
        """The sigma that is set (0.0 without one)."""
        return self._handle.get_shift()

    def time_steps(self, u0, tau: float, theta: float = 1.0, nsteps: int = 1, eps: float = 1e-8, max_iterations: int = 10000,
                   rule: int = _capi.RULE_REL_2NORM, params=None):
        """Extension (no reference twin): nsteps steps of the theta scheme (1: implicit Euler, 0.5: Crank-Nicolson) for
        u_t = A u - g from the state u0, g = this system's right-hand side as it stands; the state stays on the device between
        steps and every step warm-starts from the previous one (mi355cg_time_steps).  The shift is left at 1 / (theta * tau).
        u0: NumPy [size()] float64 or a contiguous CUDA torch tensor; returns (u of u0's kind, [Results per step taken],
        steps_done).  Stepping ends after the first step that does not converge; u is then that step's last iterate.  eps,
        max_iterations, rule as in solve_batch; params, if given, is used as it is (use_true_solution and diagnostics 0)."""
        h = self._handle
        on_device = h._check_guess(u0, h.size)
        if params is None:
            params = default_params(rule)
            params.max_iterations = max_iterations
            params.eps_rel = params.eps_precision = params.eps_residual = eps
            params.use_true_solution = 0
        h.set_initial_guess(u0)
        try:
            res, done = h.time_steps(params, tau, theta, nsteps)
        except Exception:
            h.set_initial_guess(None)                             # a refused call takes no state with it
            raise
        if int(nsteps) == 0:
            h.set_initial_guess(None)
            return (u0.clone() if on_device else np.array(u0, dtype=np.float64, copy=True)), res, done
        if on_device:
            import torch
            return h.solution_device(torch.empty_like(u0)), res, done
        return h.solution(), res, done

    def solve_batch(self, b, eps: float = 1e-6, max_iterations: int = 10000, rule: int = _capi.RULE_REL_2NORM, params=None, x0=None):
        """Extension (no reference twin): many right-hand sides on this grid by one multigrid-preconditioned CG loop (needs
        set_preconditioner).  b: [nrhs, size()] float64, NumPy or a CUDA torch tensor; returns (x of the same kind, one
        _capi.Results per system), every system with the bits a MatrixFreeSolver / MSGSolver solve of it on this system
        gives.  eps: eps_rel (RULE_REL_2NORM) or the precision and residual thresholds (RULE_MSG_MAXNORM); params, if
        given, is used as it is.  x0: a starting vector per system, of b's kind and shape (for instance the solutions of
        the previous step); with it REL_2NORM stops relative to ||b[s]||."""
        if params is None:
            params = default_params(rule)
            params.max_iterations = max_iterations
            params.eps_rel = params.eps_precision = params.eps_residual = eps
            params.use_true_solution = 0
        return self._handle.solve_batch(params, b, x0=x0)

    def batch_release(self):
        """Free the device workspaces solve_batch and solve_many keep on this system."""
        self._handle.batch_release()

    def solve_many(self, b, eps: float = 1e-6, max_iterations: int = 10000, rule: int = _capi.RULE_REL_2NORM, params=None, x0=None,
                   sigma=None):
        """Extension (no reference twin): many independent small systems on this grid -- an ensemble, a parameter sweep, a time
        step per member -- by plain CG with ONE workgroup per system and one launch per chunk of iterations for all of them
        (grids up to the on-chip cap, N = 128; no preconditioner).  b: [nsys, size()] float64, NumPy or a CUDA torch tensor;
        x0: a starting vector per system; sigma: a shift per system (system s solves (A - sigma[s] I) x = b[s]), None = this
        system's own shift.  Returns (x of b's kind, one _capi.Results per system), every system with the bits a
        set_shift / MatrixFreeSolver or MSGSolver solve of it on this system gives; this system's own state stays as it was.
        eps, max_iterations, rule as in solve_batch; params, if given, is used as it is."""
        if params is None:
            params = default_params(rule)
            params.max_iterations = max_iterations
            params.eps_rel = params.eps_precision = params.eps_residual = eps
            params.use_true_solution = 0
        return self._handle.solve_many(params, b, x0=x0, sigma=sigma)

    def time_steps_many(self, u0, tau, theta: float = 1.0, nsteps: int = 1, g=None, eps: float = 1e-8, max_iterations: int = 10000,
                        rule: int = _capi.RULE_REL_2NORM, params=None):
        """Extension (no reference twin): an ensemble of time steppers on this grid -- time_steps for many members at once, ONE
        workgroup per member from its first step to its last, the step loop inside the launch (grids up to the on-chip cap,
        N = 128; no preconditioner).  u0: [nsys, size()] float64, NumPy or a CUDA torch tensor, the start states; tau: a time
        step per member ([nsys]) or one for all; g: a forcing per member, of u0's kind and shape, None = this system's right-hand
        side for all; theta and nsteps are shared.  Returns (u of u0's kind, one _capi.Results per member for its last step
        attempted, steps_done [nsys], step_iterations [nsys, nsteps] with -1 for steps not taken), every member with the bits
        set_rhs(g[s]) and time_steps(u0[s], tau[s], theta, nsteps) give on this system.  A member ends after its first step that
        does not converge.  Unlike time_steps the call leaves this system as it was, the shift included.  eps, max_iterations
        (per step), rule as in time_steps; params, if given, is used as it is."""
        if params is None:
            params = default_params(rule)
            params.max_iterations = max_iterations
            params.eps_rel = params.eps_precision = params.eps_residual = eps
            params.use_true_solution = 0
        return self._handle.time_steps_many(params, u0, tau, theta, nsteps, g=g)

    def wave_steps_many(self, u0, v0, tau, nsteps: int = 1, scheme: int = _capi.WAVE_VERLET, g=None, eps: float = 1e-8,
                        max_iterations: int = 10000, rule: int = _capi.RULE_REL_2NORM, params=None, steps_per_launch: int = 0,
                        stop_flag: Optional[C.c_int] = None, step_iterations: bool = False):
        """Extension (no reference twin): an ensemble of wave-equation steppers on this grid -- u_tt = A u - g[s] for many
        members at once, ONE workgroup per member (grids up to the on-chip cap, N = 128; no preconditioner).  u0, v0: [nsys,
        size()] float64, NumPy or CUDA torch tensors, the start states and velocities; tau: a time step per member ([nsys]) or one
        for all; g: a forcing per member, None = this system's right-hand side for all; nsteps and the scheme are shared.
        WAVE_VERLET (explicit velocity Verlet): the step loop runs inside the launch, one stencil pass and two axpys per step;
        every tau is at most wave_cfl(), a larger one is a ValueError; steps_per_launch (0: the default) cuts the run into
        launches between which stop_flag is tested.  WAVE_NEWMARK (implicit, beta = 1/4, gamma = 1/2, no bound on tau): every
        step is the warm-started solve of time_steps_many with the shift 4 / tau^2, under eps, max_iterations (per step) and rule
        or params; a member ends after its first step that does not converge, its state that after its last converged step.
        Returns (u, v, one _capi.Results per member, steps_done [nsys]) and with step_iterations the iteration counts [nsys,
        nsteps], -1 for steps not taken.  One call of k steps gives the bits of k calls of one step.  This system's own state,
        right-hand side, shift and solve mode stay as they were."""
        if params is None and scheme == _capi.WAVE_NEWMARK:
            params = default_params(rule)
            params.max_iterations = max_iterations
            params.eps_rel = params.eps_precision = params.eps_residual = eps
            params.use_true_solution = 0
        return self._handle.wave_steps_many(params, u0, v0, tau, nsteps, scheme=scheme, g=g, steps_per_launch=steps_per_launch,
                                            stop_flag=stop_flag, step_iterations=step_iterations)

    def wave_record_many(self, u0, v0, tau, nsteps: int, source, g=None, receivers=None, record_every: int = 1, steps_per_launch: int = 0,
                         stop_flag: Optional[C.c_int] = None, traces=None, c2=None, damping=None):
        """Extension (no reference twin): wave_steps_many with WAVE_VERLET, a source time function and receiver traces, all inside
        the launch.  damping (None: none, exactly the call without it): a damping rate d >= 0 (1 / time) of every unknown, [size] or
        [nsys, size] of u0's kind, for absorbing layers (sponge_damping builds one); member s then integrates
        u_tt + d_s o u_t = c2_s o (A u) - source_s(t) g_s, in a unit medium when c2 is None, with v scaled by
        (1 - tau d / 4) / (1 + tau d / 4) at both ends of every step; tau_s * max d_s must not exceed 4, the bound on tau is
        unchanged, and d = 0 gives the bits of the call with c2 alone.  c2 (None: the homogeneous medium, exactly the call without it): the squared wave speed of every unknown,
        [size] (one medium for all members) or [nsys, size], positive, of u0's kind; member s then integrates
        u_tt = c2_s o (A u) - source_s(t) g_s (the source is not scaled), and its tau must not exceed wave_cfl(c2)[s].  c2 = 1
        gives the bits of the call without it.  source: [nsteps + 1] (one row for all members) or [nsys, nsteps + 1] amplitudes of u0's kind; member s feels
        the forcing source[s][n] * g[s] at its local time n tau[s], so a step from n to n + 1 uses source[n] in its first half
        kick and source[n + 1] in its second (second order in tau for a smooth source); source = 1 gives the bits of
        wave_steps_many.  receivers: at most WAVE_MAX_RECEIVERS packed indices (packed_index) shared by all members, None = no
        traces.  Returns (u, v, traces, results, steps_done) with traces [nsys, nsteps // record_every, len(receivers)] of u0's
        kind -- sample j is u at the receivers after step (j + 1) * record_every -- or None without receivers.  A call of k *
        record_every steps followed by a call from its state with the next slice of the source gives the bits of one long call.
        traces: an array of that shape to write into; a stop flag leaves the samples of steps that did not run untouched.  u0,
        v0, tau, g, steps_per_launch and stop_flag as in wave_steps_many; this system is left as it was."""
        return self._handle.wave_record_many(u0, v0, tau, nsteps, source, g=g, receivers=receivers, record_every=record_every,
                                             steps_per_launch=steps_per_launch, stop_flag=stop_flag, traces=traces, c2=c2, damping=damping)

    def wave_history_many(self, u0, v0, tau, nsteps: int, source, g=None, receivers=None, record_every: int = 1, steps_per_launch: int = 0,
                          stop_flag: Optional[C.c_int] = None, traces=None, c2=None):
        """Extension (no reference twin): wave_record_many in the medium c2 (None: a unit medium) that keeps its history, the
        forward half of an adjoint-state gradient.  Returns (u, v, traces, hist, results, steps_done): u, v and traces with the
        bits of wave_record_many(c2=), and hist [nsys, nsteps + 1, size()] of u0's kind, hist[s, n] = A u_n of member s -- the
        stencil value of its state after n steps, before c2 scales it.  wave_history_bytes(n, nsys, nsteps) is its size: 8 bytes
        per unknown, member and state.  The arguments are wave_record_many's; damping= is not taken."""
        return self._handle.wave_history_many(u0, v0, tau, nsteps, source, g=g, receivers=receivers, record_every=record_every,
                                              steps_per_launch=steps_per_launch, stop_flag=stop_flag, traces=traces, c2=c2)

    def wave_adjoint_many(self, hist, tau, c2, adjoint_source, receivers=None, record_every: int = 1, lam=None, q=None, sens=None,
                          steps_per_launch: int = 0, stop_flag: Optional[C.c_int] = None, return_info: bool = False):
        """Extension (no reference twin): the exact transpose of the steps wave_history_many took, ONE workgroup per member, the
        step loop inside the launch.  hist: [nsys, nsteps + 1, size()] as wave_history_many returns it (NumPy or a CUDA tensor);
        tau, c2, receivers and record_every those of the forward run; adjoint_source: the derivative of the misfit with respect
        to the traces, [nsys, nsteps // record_every, nrec] (or one table for all members without the first axis) -- traces -
        observed for a least-squares misfit.  From state index s = nsteps down to 1, with h = tau / 2:
            if s % record_every == 0:  lam[receivers[j]] += adjoint_source[s / record_every - 1][j]   (j ascending)
            sens += q * hist[s];  lam += h * A q;  q += tau * (c2 * lam);  sens += q * hist[s - 1];  lam += h * A q
        Returns (lam, q, sens), [nsys, size()] each, from the incoming ones (None: zeros); with return_info also (results,
        steps_done).  From zeros, dJ/dc2 = (tau / 2) * sens / c2, dJ/du0 = lam and dJ/dv0 = q / c2.  No division happens inside the
        call, so a backward run cut at multiples of record_every into calls that pass (lam, q, sens) on, each with its slice of
        the history and of the sources, gives the bits of one call.  A tau above wave_cfl(c2) is refused.  This system is left as
        it was."""
        return self._handle.wave_adjoint_many(hist, tau, c2, adjoint_source, receivers=receivers, record_every=record_every, lam=lam, q=q, sens=sens,
                                              steps_per_launch=steps_per_launch, stop_flag=stop_flag, return_info=return_info)

    def wave_gradient_many(self, u0, v0, tau, nsteps: int, source, observed, g=None, receivers=None, record_every: int = 1, c2=None, segment=None, damping=None):
        """Extension (no reference twin): the least-squares misfit of a recorded run and its gradient by the adjoint-state method:
        one forward run (wave_history_many) and one backward run (wave_adjoint_many) instead of one forward run per unknown.
        observed: [nsys, nsteps // record_every, nrec] of u0's kind.  Returns (misfit [nsys], grad_c2, grad_u0, grad_v0, traces):
        misfit_s = 1/2 sum (traces_s - observed_s)^2, the adjoint source is traces - observed (one rounding), grad_c2 = (tau / 2)
        sens / c2, grad_u0 = lam, grad_v0 = q / c2.  segment=K (a multiple of record_every): the forward run goes in segments of K
        steps and keeps (u, v) at every segment start on the device; the segments are then walked backwards, each with one
        history call of K steps from its checkpoint and one adjoint call, so never more than K + 1 history rows per member exist
        (wave_history_bytes(n, nsys, K)); the bits are those of segment=None.  c2=None is a unit medium.  NumPy arrays or CUDA
        tensors, as wave_record_many takes them; unlike that call this one needs torch for either kind: NumPy arguments go to the
        device once, everything runs there through the device entry points, and the results come down once.  The transpose of
        the damped step is not built: a damping that is not None is a ValueError."""
        if damping is not None:
            raise ValueError("wave_gradient_many takes no damping: the transpose of the damped step is not built")
        return self._handle.wave_gradient_many(u0, v0, tau, nsteps, source, observed, g=g, receivers=receivers, record_every=record_every, c2=c2, segment=segment)

    def sponge_damping(self, width: int, dmax: float, sides: str = "lrbt"):
        """The damping field of a sponge layer on this system's grid, for wave_record_many(damping=): the module's
        sponge_damping(n, width, dmax, sides).  ValueError on a grid that is not square (the packed order is packed_index's)."""
        if self.m != self.n:
            raise ValueError(f"sponge_damping is defined on square grids, not {self.m} x {self.n}")
        return sponge_damping(self.n, width, dmax, sides)

    def packed_index(self, ix: int, iy: int) -> int:
        """The packed index of grid node (ix, iy), 0 <= ix, iy <= n, in the order of the batch and ensemble calls (solve_many,
        wave_record_many's receivers): row by row, x fastest, first the rows 1 .. n/2 of the bottom-right block (columns n/2 + 1
        .. n - 1), then the rows n/2 + 1 .. n - 1 of the upper block (columns 1 .. n - 1).  -1: the node is not an unknown (a
        boundary node, or in the cut-out quadrant).  ValueError on a grid that is not square with an even n."""
        n = self.n
        if self.m != n or n % 2 or n < 4:
            raise ValueError(f"packed_index is defined on square grids with an even n, not {self.m} x {n}")
        half, ix, iy = n // 2, int(ix), int(iy)
        if 1 <= iy <= half and half + 1 <= ix <= n - 1:
            return (iy - 1) * (half - 1) + (ix - half - 1)
        if half + 1 <= iy <= n - 1 and 1 <= ix <= n - 1:
            return half * (half - 1) + (iy - half - 1) * (n - 1) + (ix - 1)
        return -1

    def wave_cfl(self, c2=None):
        """The largest time step wave_steps_many takes with WAVE_VERLET on this grid: 2 / sqrt(2 |A_diag|), Gershgorin's bound.
        c2: a medium of wave_record_many, [size] or [nsys, size]: its bound 2 / sqrt(2 |A_diag| max c2), one float or an array
        [nsys]; sufficient, not sharp."""
        return self._handle.wave_cfl(c2)

    def solve_many_info(self, nsys: int):
        """What a solve_many batch of nsys systems costs on this grid: the LDS bytes of one workgroup, how many workgroups the
        runtime lets reside on one CU, and the device workspace bytes."""
        return self._handle.solve_many_info(nsys)

    def eigs(self, nev: int, block: Optional[int] = None, tol: float = 1e-8, max_iterations: int = 200, x0=None, seed: int = 0,
             stop_flag: Optional[C.c_int] = None):
        """Extension (no reference twin): the nev lowest eigenpairs of this system's operator by a block preconditioned
        iteration (LOBPCG) with one multigrid V-cycle per vector and iteration (needs set_preconditioner with the fp64 cycle).
        Returns (lam[nev], V[nev, size()], info): lam > 0 ascending with A v = -lam v (with set_shift(sigma): (A - sigma I) v =
        -lam v, i.e. the unshifted values + sigma), the rows of V orthonormal.  block: vectors iterated, nev <= block <= 16; the
        extra ones are guard vectors (default min(16, nev + max(2, nev // 4)), capped by size()).  x0: the start block,
        [block, size()] float64, NumPy or a CUDA torch tensor (V is then a tensor too); without it
        numpy.random.default_rng(seed).standard_normal((block, size())).  info: iterations, converged, stop_reason
        (_capi.EIG_CONVERGED / EIG_ITERATIONS / EIG_INTERRUPTED / EIG_BREAKDOWN), p_drops, solve_seconds, residuals (the relative
        residuals of all block columns), ritz_values (all block Ritz values).  The system's right-hand side, last solution and
        shift are untouched."""
        nev = int(nev)
        if block is None:
            block = min(_capi.EIG_BLOCK_MAX, nev + max(2, nev // 4), self.size())
        block = int(block)
        if x0 is None:
            if not 1 <= nev <= block <= _capi.EIG_BLOCK_MAX:
                raise ValueError(f"1 <= nev <= block <= {_capi.EIG_BLOCK_MAX} is required, not nev = {nev}, block = {block}")
            x0 = np.random.default_rng(seed).standard_normal((block, self.size()))
        lam, v, res, out = self._handle.eigs(nev, block, tol, max_iterations, x0, stop_flag)
        info = {"iterations": out.iterations, "converged": bool(out.converged), "stop_reason": out.stop_reason, "p_drops": out.p_drops,
                "solve_seconds": out.solve_seconds, "residuals": res, "ritz_values": lam}
        return lam[:nev].copy(), v[:nev], info

    def eigs_release(self):
        """Free the device workspace eigs keeps on this system."""
        self._handle.eigs_release()

    def block_gram(self, a, b, rows=None, cols=None):
        """a @ b.T for two groups of <= 48 packed vectors, summed on the device in a fixed order (two calls: the same bits)."""
        return self._handle.block_gram(a, b, rows, cols)

    def block_combine(self, s, coef):
        """coef.T @ s for <= 48 packed vectors s and <= 16 output columns, as an ascending sum of unfused multiply-adds."""
        return self._handle.block_combine(s, coef)


class GridSystem(MatrixFreeSystem):
    """solver/grid_system.h:16-88: same geometry; the CSR matrix is never materialised on the
    hot path -- get_matrix() hands back the operator itself."""

    def get_matrix(self): return self
    def get_x_coords(self): return self._handle.node_coords()[0]
    def get_y_coords(self): return self._handle.node_coords()[1]

    def get_node_coordinates(self, solution_index: int):
        if solution_index < 0 or solution_index >= self.size():
            return (0.0, 0.0)                                   # grid_system.cpp:339-341
        xs, ys = self._handle.node_coords()
        return (float(xs[solution_index]), float(ys[solution_index]))


class CrsMatrix:
    """A caller-supplied sparse matrix (KokkosCrsMatrix, solver/solver.hpp:15) as the operator of
    `MSGSolver(a, b, ...)` / `MatrixFreeSolver(a, b, ...)`: the generic path of the abstract `Solver` contract."""

    def __init__(self, row_map, entries, values, device: int = 0):
        self._handle = _Handle.from_csr(row_map, entries, values, device=device)

    def numRows(self): return self._handle.size
    def numCols(self): return self._handle.size
    def size(self): return self._handle.size
    def apply(self, x): return self._handle.apply(x)
    def __mul__(self, x): return self.apply(x)


class MatrixFreeSolver:
    """solver/matrix_free_system.hpp:73-127, MatrixFreeSolver::solve (.cpp:383-482):
    textbook CG, relative 2-norm stop rule."""

    def __init__(self, system: MatrixFreeSystem, b, eps: float = 1e-6, maxIterations: int = 10000,
                 name: str = "Matrix-free solver"):
        self.system, self.b, self.eps, self.maxIterations, self.name = system, b, eps, maxIterations, name
        self.iterations = 0
        self.iteration_callback = None
        self.completion_callback = None
        self.last_results = None

    def setIterationCallback(self, cb): self.iteration_callback = cb
    def setCompletionCallback(self, cb): self.completion_callback = cb
    def getIterations(self): return self.iterations
    def getName(self): return self.name

    def solve(self, true_solution=None, fixed_iterations: bool = False, sync_every: int = 0,
              inner_eps: float = 0.0, x0=None) -> np.ndarray:
        """inner_eps only matters for a MatrixFreeSystem created with dtype=F32_MIXED (config 3).  x0 (extension): the starting
        vector of this solve instead of zero (_Handle.set_initial_guess); the rule is then relative to ||b||."""
        h = self.system._handle
        h.set_rhs(self.b)
        if x0 is not None:
            h.set_initial_guess(x0)
        if true_solution is not None and len(true_solution) > 0:
            h.set_true_solution(true_solution)                   # matrix_free_system.cpp:451-455 uses the caller's vector
        p = default_params(_capi.RULE_REL_2NORM)
        p.eps_rel, p.max_iterations = self.eps, self.maxIterations
        p.diagnostics = 1 if self.iteration_callback else 0
        p.fixed_iterations = 1 if fixed_iterations else 0
        p.sync_every = sync_every
        p.inner_eps = inner_eps
        res = h.solve(p, self.iteration_callback)
        self.iterations, self.last_results = res.iterations, res
        if self.completion_callback:                              # matrix_free_system.cpp:472-479
            ok = bool(res.converged)
            self.completion_callback(ok, "Converged successfully" if ok else
                                     "Failed to converge within maximum iterations")
        return h.solution()


class MSGSolver:
    """solver/msg_solver.hpp:17-120, MSGSolver::solve (msg_solver.cpp:10-212)."""

    def __init__(self, a: MatrixFreeSystem, b, eps: float = 1e-6, maxIterations: int = 10000):
        self.a, self.b = a, b
        self.eps, self.maxIterations = eps, maxIterations
        self.name = "Метод серединных градиентов"
        self.eps_precision = self.eps_residual = self.eps_exact_error = eps
        self.converged = False
        self.stop_reason = StopCriterion.ITERATIONS
        self.final_residual_norm = self.final_error_norm = self.final_precision = 0.0
        self.iterations = 0
        self.iteration_callback = None
        self.completion_callback = None
        self._stop = C.c_int(0)
        self.last_results = None

    def setPrecisionEps(self, eps): self.eps_precision = eps
    def setResidualEps(self, eps): self.eps_residual = eps
    def setExactErrorEps(self, eps): self.eps_exact_error = eps
    def hasConverged(self): return self.converged
    def getStopReason(self): return self.stop_reason
    def getStopReasonText(self): return _STOP_TEXT.get(self.stop_reason, "Неизвестная причина остановки")
    def requestStop(self): self._stop.value = 1
    def resetStop(self): self._stop.value = 0
    def isStopRequested(self): return bool(self._stop.value)
    def getFinalResidualNorm(self): return self.final_residual_norm
    def getFinalErrorNorm(self): return self.final_error_norm
    def getFinalPrecision(self): return self.final_precision
    def setIterationCallback(self, cb): self.iteration_callback = cb
    def setCompletionCallback(self, cb): self.completion_callback = cb
    def getIterations(self): return self.iterations
    def getName(self): return self.name

    def solve(self, true_solution=None, callback_every: int = 100, x0=None) -> np.ndarray:
        """true_solution: None / empty = extent 0 (error criterion and norm off).  x0 (extension): the starting vector of this
        solve instead of zero (_Handle.set_initial_guess); the residual and exact-error tests then also run on the start."""
        self.converged = False
        self._stop.value = 0                                     # msg_solver.cpp:12-13
        h = self.a._handle
        h.set_rhs(self.b)
        if x0 is not None:
            h.set_initial_guess(x0)
        if true_solution is not None and len(true_solution) > 0:
            h.set_true_solution(true_solution)                   # the error norms use the vector that was passed in (msg_solver.cpp:64-72,132-139)
        p = default_params(_capi.RULE_MSG_MAXNORM)
        p.max_iterations = self.maxIterations
        p.eps_precision, p.eps_residual, p.eps_exact_error = self.eps_precision, self.eps_residual, self.eps_exact_error
        p.use_true_solution = 0 if true_solution is None or len(true_solution) == 0 else 1
        p.callback_every = callback_every
        res = h.solve(p, self.iteration_callback, self._stop)
        self.last_results = res
        self.iterations = res.iterations                         # msg_solver.cpp:187-190
        self.converged = bool(res.converged)
        self.stop_reason = StopCriterion(res.stop_reason)
        self.final_residual_norm, self.final_precision, self.final_error_norm = \
            res.final_residual_norm, res.final_precision, res.final_error_norm
        return h.solution()


@dataclass
class SolverResults:                        # solver/dirichlet_solver.hpp:11-24
    solution: np.ndarray = field(default_factory=lambda: np.empty(0))
    true_solution: np.ndarray = field(default_factory=lambda: np.empty(0))
    residual: np.ndarray = field(default_factory=lambda: np.empty(0))      # A x - b (true)
    error: np.ndarray = field(default_factory=lambda: np.empty(0))         # x - u
    x_coords: np.ndarray = field(default_factory=lambda: np.empty(0))
    y_coords: np.ndarray = field(default_factory=lambda: np.empty(0))
    residual_norm: float = 0.0              # recursive max-norm (dirichlet_solver.cpp:122)
    error_norm: float = 0.0
    iterations: int = 0
    precision: float = 0.0                  # never assigned by the reference; kept at 0
    converged: bool = False
    stop_reason: str = ""


class DirichletSolver:
    """Facade, solver/dirichlet_solver.hpp:79-184 / .cpp:11-131."""

    def __init__(self, n: int = 10, m: int = 10, a: float = 0.0, b: float = 1.0, c: float = 0.0,
                 d: float = 1.0, device: int = 0):
        self._device = device
        self.eps_precision = self.eps_residual = self.eps_exact_error = 1e-6     # .cpp:14
        self.max_iterations = 10000
        self.use_precision, self.use_residual, self.use_error, self.use_max_iterations = True, True, False, True  # .cpp:15-16
        self.iteration_callback = None
        self.completion_callback = None
        self.solver: Optional[MSGSolver] = None
        self.solution = np.empty(0)
        self.true_solution = np.empty(0)
        self.setGridParameters(n, m, a, b, c, d)

    def setGridParameters(self, n, m, a, b, c, d):
        self.n, self.m, self.a, self.b, self.c, self.d = n, m, a, b, c, d
        self.grid = GridSystem(m, n, a, b, c, d, device=self._device)     # note (m, n): .cpp:24

    def setSolverParameters(self, eps_p, eps_r, eps_e, max_iter):
        self.eps_precision, self.eps_residual, self.eps_exact_error, self.max_iterations = eps_p, eps_r, eps_e, max_iter

    def enablePrecisionStopping(self, on): self.use_precision = on
    def enableResidualStopping(self, on): self.use_residual = on
    def enableErrorStopping(self, on): self.use_error = on
    def enableMaxIterationsStopping(self, on): self.use_max_iterations = on      # never read (as in the reference)
    def setIterationCallback(self, cb): self.iteration_callback = cb
    def setCompletionCallback(self, cb): self.completion_callback = cb
    def getMethodName(self): return self.solver.getName() if self.solver is not None else "МСГ"    # dirichlet_solver.hpp:159-161
    def getGridSystem(self): return self.grid
    def getSolution(self): return self.solution
    def getTrueSolution(self): return self.true_solution

    def requestStop(self):
        if self.solver is not None:
            self.solver.requestStop()

    def solve(self) -> SolverResults:
        if self.grid is None:
            raise RuntimeError("Grid system not initialized")                     # .cpp:62-64
        eps = min(self.eps_precision, self.eps_residual, self.eps_exact_error)    # .cpp:67-68
        s = MSGSolver(self.grid.get_matrix(), self.grid.get_rhs(), eps, self.max_iterations)
        s.setPrecisionEps(self.eps_precision if self.use_precision else -1.0)     # .cpp:71-87
        s.setResidualEps(self.eps_residual if self.use_residual else -1.0)
        s.setExactErrorEps(self.eps_exact_error if self.use_error else -1.0)
        if self.iteration_callback:
            s.setIterationCallback(self.iteration_callback)
        self.solver = s
        u = self.grid.get_true_solution_vector()                                   # .cpp:95
        x = s.solve(u)                                                             # .cpp:98
        r = SolverResults()
        r.solution, r.true_solution = x, u
        r.residual = self.grid._handle.true_residual()                             # A x - b, .cpp:106,147-161
        r.error = x - u                                                            # .cpp:110,164-180
        r.x_coords, r.y_coords = self.grid.get_x_coords(), self.grid.get_y_coords()
        r.iterations, r.converged = s.getIterations(), s.hasConverged()
        r.stop_reason = s.getStopReasonText()
        r.residual_norm, r.error_norm = s.getFinalResidualNorm(), s.getFinalErrorNorm()
        self.solution, self.true_solution = x, u
        if self.completion_callback:
            self.completion_callback(r)
        return r
