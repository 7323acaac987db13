"""Warm starts (mi355cg_set_initial_guess*, mi355cg_use_solution_as_initial_guess, mi355cg_solve_batch*_from)
without a GPU: the declared and exported symbols, the refusals that need no device, the Python wrappers' argument checks, the
compiled kernels, and a NumPy restatement of warm multigrid-PCG (on the apply_A and apply_M of
tests/mg_model.py) that establishes the identities tests/test_gpu_warm_start.py leans on."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOM = ref.DOM
GUESS_SYMBOLS = ("mi355cg_set_initial_guess", "mi355cg_set_initial_guess_device", "mi355cg_use_solution_as_initial_guess")
BATCH_SYMBOLS = ("mi355cg_solve_batch_from", "mi355cg_solve_batch_device_from")


def test_header_declares_the_five_entry_points():
    header = open(os.path.join(ROOT, "include", "mi355cg.h")).read()
    assert re.search(r"int\s+mi355cg_set_initial_guess\(mi355cg_handle h, const double \*x0\);", header)
    assert re.search(r"int\s+mi355cg_set_initial_guess_device\(mi355cg_handle h, const double \*x0_dev\);", header)
    assert re.search(r"int\s+mi355cg_use_solution_as_initial_guess\(mi355cg_handle h\);", header)
    for name in BATCH_SYMBOLS:
        assert re.search(rf"int\s+{name}\(mi355cg_handle h, const mi355cg_params \*params, int nrhs,", header), name


def test_library_exports_them():
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    for name in GUESS_SYMBOLS + BATCH_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _capi.EXPORTS


def test_null_handles_are_invalid_without_a_device():
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    buf = np.zeros(8)
    assert lib.mi355cg_set_initial_guess(None, buf.ctypes.data) == _capi.ERR_INVALID
    assert lib.mi355cg_set_initial_guess(None, None) == _capi.ERR_INVALID
    assert lib.mi355cg_set_initial_guess_device(None, buf.ctypes.data) == _capi.ERR_INVALID
    assert lib.mi355cg_use_solution_as_initial_guess(None) == _capi.ERR_INVALID
    assert b"null handle" in lib.mi355cg_last_error()
    p = _capi.Params()
    lib.mi355cg_default_params(C.byref(p), _capi.RULE_REL_2NORM)
    p.use_true_solution = 0
    res = (_capi.Results * 2)()
    for fn in (lib.mi355cg_solve_batch_from, lib.mi355cg_solve_batch_device_from):
        assert fn(None, C.byref(p), 1, buf.ctypes.data, buf.ctypes.data + 32, None, res) == _capi.ERR_INVALID
        assert fn(None, None, 1, None, None, None, None) == _capi.ERR_INVALID


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def _stub(size=10):
    from iterative_solvers_amd.solver import _Handle
    h = _Handle.__new__(_Handle)
    h._lib, h._h, h.size, h._device = _NoLibrary(), None, size, 0
    return h


@pytest.mark.parametrize("x0, what", [
    (np.zeros(9), "shape"), (np.zeros((1, 10)), "shape"), (np.zeros(10, dtype=np.float32), "dtype"),
    (np.zeros(10, dtype=np.int64), "dtype"), ([0.0] * 10, "NumPy array or a CUDA torch tensor"),
])
def test_set_initial_guess_checks_shape_and_dtype_before_calling_the_library(x0, what):
    with pytest.raises(ValueError, match=what):
        _stub().set_initial_guess(x0)


def test_set_initial_guess_refuses_host_tensors_before_calling_the_library():
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="device memory"):
        _stub().set_initial_guess(torch.zeros(10, dtype=torch.float64))


@pytest.mark.parametrize("x0, what", [
    (np.zeros((3, 10)), "x0 has shape"), (np.zeros((2, 9)), "shape"), (np.zeros((2, 10), dtype=np.float32), "dtype"),
    (np.zeros(10), "shape"),
])
def test_solve_batch_checks_the_guesses_before_calling_the_library(x0, what):
    from iterative_solvers_amd import _capi
    with pytest.raises(ValueError, match=what):
        _stub().solve_batch(_capi.Params(), np.zeros((2, 10)), x0=x0)


def test_solver_classes_check_the_guess_before_the_library_sees_it():
    import iterative_solvers_amd as isa

    class _System:
        pass

    s = _System()
    s._handle = _stub()
    s._handle.set_rhs = lambda b: None
    for solver in (isa.MatrixFreeSolver(s, np.zeros(10)), isa.MSGSolver(s, np.zeros(10))):
        with pytest.raises(ValueError, match="shape"):
            solver.solve(x0=np.zeros(11))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_the_warm_start_kernels_are_compiled_without_scratch(tmp_path, monkeypatch):
    """The device code of build()'s flags (-O3 -ffp-contract=off, the atomic-optimizer switch), compiled device-only to assembly."""
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    import isa_store_hazard_check as chk
    monkeypatch.setenv("PATH", os.environ.get("PATH", "") + ":/opt/rocm/bin")
    dump = str(tmp_path / "dev.s")
    chk.compile_to_asm(dump)
    text = open(dump).read()
    meta = text[text.index("amdhsa.kernels"):]
    found = {}
    for entry in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        found[name] = (int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1)),
                       int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1)))
    for k, instances in (("k_init_guess", 2), ("k_guess_state", 1), ("k_mgb_init_guess", 1)):
        mine = {n: v for n, v in found.items() if re.search(rf"\d+{k}(E|I)", n)}
        print(k, mine)
        assert len(mine) == instances, (k, mine)
        assert all(scratch == 0 for scratch, _ in mine.values()), mine
        assert all(vgprs <= 128 for _, vgprs in mine.values()), mine          # two waves per SIMD and more: a streaming pass


# ---- the NumPy restatement -------------------------------------------------------------------------------------------------
def apply_A_packed(L, v):
    return ref.packed(L, ref.apply_A(L, ref.grid(L, v)))


def warm_pcg(levels, b, x0=None, eps=1e-8, max_iterations=100, fixed_iterations=False):
    """mg_model.pcg with a start: x = x0, r0 = b - A x0, REL_2NORM relative to ||b||.  x0 = None is that function's cold
    start (r0 = b, relative to ||r0|| = ||b||).  Returns (x, r, iterations, [||r_k||_2 for k = 0 .. iterations])."""
    L = levels[0]
    if x0 is None:
        x, r = np.zeros_like(b), b.copy()
        target = np.linalg.norm(r)
    else:
        x, r = x0.copy(), b - apply_A_packed(L, x0)
        target = np.linalg.norm(b)
    norms = [np.linalg.norm(r)]
    it, rho, p = 0, 0.0, None
    while it < max_iterations and (fixed_iterations or norms[-1] > eps * target):
        z = ref.apply_M(levels, r)
        rz = r @ z
        p = z if it == 0 else z + (rz / rho) * p
        rho = rz
        q = apply_A_packed(L, p)
        alpha = rho / (p @ q)
        x = x + alpha * p
        r = r - alpha * q
        it += 1
        norms.append(np.linalg.norm(r))
    return x, r, it, norms


def problem(N):
    from oracle.oracle import OracleGrid
    levels = ref.hierarchy_any(N, *ref.steps(N))
    return levels, OracleGrid(N, N, *DOM).rhs()


@pytest.mark.parametrize("N", [34, 64])
def test_a_zero_guess_reproduces_the_cold_solve_exactly(N):
    levels, b = problem(N)
    xc, rc, itc, nc = warm_pcg(levels, b)
    xw, rw, itw, nw = warm_pcg(levels, b, x0=np.zeros_like(b))
    assert itc == itw >= 1 and nc == nw
    assert np.array_equal(xc, xw) and np.array_equal(rc, rw)
    assert np.array_equal(xc, ref.pcg(levels, b)[0])                     # and the cold start is the existing restatement's


@pytest.mark.parametrize("N", [34, 64])
def test_a_guess_is_the_shifted_problem_exactly(N):
    """b with the guess x0 and b' = b - A x0 from zero have the same r0, and x never enters the recurrences of r, z, p: the
    residual sequences are the same bits; the iterates differ by x0 up to one rounding per step."""
    levels, b = problem(N)
    x0 = 1e-2 * np.random.default_rng(N).standard_normal(b.size)
    k = 8
    xw, rw, _, nw = warm_pcg(levels, b, x0=x0, max_iterations=k, fixed_iterations=True)
    xs, rs, _, ns = warm_pcg(levels, b - apply_A_packed(levels[0], x0), max_iterations=k, fixed_iterations=True)
    assert nw == ns and np.array_equal(rw, rs)
    assert np.all(np.abs(xw - (x0 + xs)) <= (k + 2) * 2.0 ** -52 * np.abs(xw).max())


@pytest.mark.parametrize("N, cold_its, warm_its", [(34, 7, 3), (64, 6, 3)])
def test_a_good_guess_takes_strictly_fewer_iterations(N, cold_its, warm_its):
    """x0 = the 1e-4 solution, then eps 1e-8.  NumPy counts (this restatement): N = 34: cold 7, the 1e-4 solve 4, warm 3;
    N = 64: cold 6, the 1e-4 solve 3, warm 3."""
    levels, b = problem(N)
    _, _, cold, _ = warm_pcg(levels, b, eps=1e-8)
    x4, _, first, _ = warm_pcg(levels, b, eps=1e-4)
    xw, rw, warm, norms = warm_pcg(levels, b, x0=x4, eps=1e-8)
    print(f"N={N}: cold {cold}, the 1e-4 solve {first}, warm {warm}")
    assert 1 <= warm < cold
    assert norms[-1] <= 1e-8 * np.linalg.norm(b)
    assert (cold, warm) == (cold_its, warm_its)
    # a start that already meets the rule: 0 iterations, x untouched
    xe, _, its, _ = warm_pcg(levels, b, x0=xw, eps=1e-7)
    assert its == 0 and np.array_equal(xe, xw)
