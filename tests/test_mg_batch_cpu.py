"""Batched multigrid-PCG solves (mi355cg_solve_batch) without a GPU: the exported symbols, the refusals that
need no device, the Python wrapper's argument checks, the compiled batched kernels (present, no scratch), and the right-hand
sides tests/test_gpu_mg_batch.py uses: that they stop after different numbers of iterations, so the freeze rule runs there."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mg_model as ref  # noqa: E402
from mg_cases import batch_rhs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOM = (1.0, 2.0, 1.0, 2.0)
BATCH_SYMBOLS = ("mi355cg_solve_batch", "mi355cg_solve_batch_device", "mi355cg_batch_release")
BATCH_KERNELS = ("k_mgb_smooth", "k_mgb_restrict", "k_mgb_prolong", "k_mgb_residual", "k_mgb_restrict_nn", "k_mgb_prolong_nn",
                 "k_mgb_coarse", "k_mgb_dir_apply", "k_mgb_update", "k_mgb_init", "k_mgb_dot", "k_mgb_reduce", "k_mgb_unpack",
                 "k_mgb_pack")


def test_library_exports_the_batch_entry_points():
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    for name in BATCH_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _capi.EXPORTS
    assert _capi.BATCH_MAX == 64
    header = open(os.path.join(ROOT, "include", "mi355cg.h")).read()
    assert re.search(r"#define\s+MI355CG_BATCH_MAX\s+64\b", header)


@pytest.mark.parametrize("nrhs", [1, 0, 65])
def test_null_handle_and_bad_counts_are_invalid_without_a_device(nrhs):
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    p = _capi.Params()
    lib.mi355cg_default_params(C.byref(p), _capi.RULE_REL_2NORM)
    p.use_true_solution = 0
    buf = np.zeros(8)
    res = (_capi.Results * 65)()
    for fn in (lib.mi355cg_solve_batch, lib.mi355cg_solve_batch_device):
        assert fn(None, C.byref(p), nrhs, buf.ctypes.data, buf.ctypes.data + 32, None, res) == _capi.ERR_INVALID
        assert fn(None, None, nrhs, None, None, None, None) == _capi.ERR_INVALID
        assert lib.mi355cg_last_error()
    assert lib.mi355cg_batch_release(None) == _capi.ERR_INVALID


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def _stub(size=10):
    from iterative_solvers_amd.solver import _Handle
    h = _Handle.__new__(_Handle)
    h._lib, h._h, h.size, h._device = _NoLibrary(), None, size, 0
    return h


@pytest.mark.parametrize("b, what", [
    (np.zeros(10), "shape"), (np.zeros((2, 9)), "shape"), (np.zeros((2, 2, 10)), "shape"), (np.zeros((0, 10)), "right-hand sides"),
    (np.zeros((65, 10)), "right-hand sides"), (np.zeros((2, 10), dtype=np.float32), "dtype"), (np.zeros((2, 10), dtype=np.int64), "dtype"),
    ([[0.0] * 10], "NumPy array or a CUDA torch tensor"),
])
def test_wrapper_checks_shape_and_dtype_before_calling_the_library(b, what):
    from iterative_solvers_amd import _capi
    with pytest.raises(ValueError, match=what):
        _stub().solve_batch(_capi.Params(), b)


def test_wrapper_refuses_host_and_wrong_type_tensors_before_calling_the_library():
    torch = pytest.importorskip("torch")
    from iterative_solvers_amd import _capi
    with pytest.raises(ValueError, match="device memory"):
        _stub().solve_batch(_capi.Params(), torch.zeros((2, 10), dtype=torch.float64))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_batched_kernels_are_compiled_without_scratch_and_without_store_hazards(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_store_hazard_check as chk
    os.environ["PATH"] = os.environ.get("PATH", "") + ":/opt/rocm/bin"
    dump = str(tmp_path / "dev.s")
    chk.compile_to_asm(dump)
    text = open(dump).read()
    meta = text[text.index("amdhsa.kernels"):]
    scratch = {}
    for entry in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        scratch[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1))
    for k in BATCH_KERNELS:
        mine = {n: v for n, v in scratch.items() if re.search(rf"\d+{k}(E|I)", n)}
        assert mine, f"{k} is not in the compiled code"
        assert all(v == 0 for v in mine.values()), mine
    # every template instance the host code launches
    assert sum(1 for n in scratch if "k_mgb_smoothILb" in n) == 3 and sum(1 for n in scratch if "k_mgb_dir_applyILb" in n) == 2
    single = [n for n in scratch if re.search(r"\d+k_mg_[a-z0-9_]+(E|I)", n)]
    assert len(single) >= 14 and all(scratch[n] == 0 for n in single)       # the single-system kernels are as they were
    assert not chk.findings(dump)


@pytest.mark.parametrize("N", [130, 258])
def test_the_right_hand_sides_of_the_gpu_tests_stop_at_different_iterations(N):
    """The freeze rule only runs if the systems of a batch stop at different iterations.  This is the NumPy restatement of the
    REL_2NORM PCG (mg_model.pcg, eps 1e-8) on the unscaled right-hand sides; it guards the inputs, not the device code."""
    from oracle.oracle import OracleGrid
    levels = ref.hierarchy_any(N, *ref.steps(N))
    b = OracleGrid(N, N, *DOM).rhs()
    rhs = batch_rhs(N, b, scaled=False)
    assert rhs.shape == (5, int(levels[0].mask.sum()))
    assert set(np.unique(rhs[3])) == {-1.0, 1.0} and abs(rhs[3].sum()) <= N
    its = [ref.pcg(levels, v)[1] for v in rhs]
    print("iterations (b, zeros, ones, checkerboard, normal):", its)
    assert len(set(its)) >= 2, its
    assert its[1] == 0 and all(1 <= k <= 12 for k in its[:1] + its[2:]), its
