"""The block eigensolver (mi355cg_eigs) without a GPU: the host Rayleigh-Ritz step through the C ABI
against NumPy, the bases it refuses, the argument refusals that need no device, the NumPy restatement of the iteration
(tests/eigs_reference.py) against the dense operator, and the compiled kernels (present, no scratch)."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eigs_reference as er  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIG_SYMBOLS = ("mi355cg_eigs", "mi355cg_eigs_device", "mi355cg_eigs_release", "mi355cg_block_gram", "mi355cg_block_gram_indexed",
               "mi355cg_block_combine", "mi355cg_rayleigh_ritz")
EIG_KERNELS = ("k_eig_gram", "k_eig_reduce", "k_eig_combine", "k_eig_resid")
# iterations of the prototype to a relative residual of 1e-8 (the larger figure where it gave a range), by (N, nev, block)
PROTOTYPE_ITERATIONS = {(16, 1, 1): 16, (16, 6, 8): 18, (16, 16, 16): 26, (34, 1, 1): 16, (34, 6, 8): 21, (34, 16, 16): 37,
                        (64, 1, 1): 15, (64, 6, 8): 20, (64, 16, 16): 37}


def spd_pair(k, seed):
    """G = S^T S and H = S^T K S of k random vectors of length 4 k + 8 and a random SPD K"""
    rng = np.random.default_rng(seed)
    n = 4 * k + 8
    S = rng.standard_normal((n, k))
    B = rng.standard_normal((n, n))
    K = B @ B.T + n * np.eye(n)
    return S.T @ S, S.T @ K @ S


def whitened_eigh(G, H):
    """the same quantities by numpy.linalg.eigh of the whitened pair"""
    G, H = 0.5 * (G + G.T), 0.5 * (H + H.T)
    d = 1 / np.sqrt(np.diag(G))
    L = np.linalg.cholesky(d[:, None] * G * d[None, :])
    Li = np.linalg.inv(L)
    M = Li @ (d[:, None] * H * d[None, :]) @ Li.T
    theta, Y = np.linalg.eigh(0.5 * (M + M.T))
    return theta, d[:, None] * (Li.T @ Y)


def errors(G, H, theta, coef, exact):
    k = G.shape[0]
    return (np.abs(theta - exact).max() / np.abs(exact).max(), np.abs(coef.T @ G @ coef - np.eye(k)).max(),
            np.abs(coef.T @ H @ coef - np.diag(theta)).max() / np.abs(exact).max())


def test_library_exports_the_eigen_entry_points():
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    for name in EIG_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _capi.EXPORTS
    assert _capi.EIG_BLOCK_MAX == 16
    header = open(os.path.join(ROOT, "include", "mi355cg.h")).read()
    assert re.search(r"#define\s+MI355CG_EIG_BLOCK_MAX\s+16\b", header)
    for i, name in enumerate(("CONVERGED", "ITERATIONS", "INTERRUPTED", "BREAKDOWN")):
        assert re.search(rf"#define\s+MI355CG_EIG_{name}\s+{i}\b", header) and getattr(_capi, "EIG_" + name) == i
    assert (er.CONVERGED, er.ITERATIONS, er.INTERRUPTED, er.BREAKDOWN) == (0, 1, 2, 3)


@pytest.mark.parametrize("k", [1, 3, 24, 48])
def test_rayleigh_ritz_against_numpy(k):
    import iterative_solvers_amd as isa
    for seed in range(3):
        G, H = spd_pair(k, 100 * k + seed)
        # the exact values: the generalised problem in extended precision is not at hand, so the yardstick is NumPy's own
        # error in the three quantities, measured on its solution of the same whitened pair
        theta_np, coef_np = whitened_eigh(G, H)
        theta, coef = isa.rayleigh_ritz(G, H)
        assert theta.shape == (k,) and coef.shape == (k, k) and np.all(np.diff(theta) >= 0)
        mine = errors(G, H, theta, coef, theta_np)
        numpys = errors(G, H, theta_np, coef_np, theta_np)
        # NumPy's error in theta against itself is 0: its yardstick is k ulps of the largest value, the error bound of eigh
        floor = (k * np.finfo(float).eps, numpys[1], numpys[2])
        print(k, seed, "library", mine, "numpy", numpys)
        for a, b in zip(mine, floor):
            assert a <= 100 * max(b, np.finfo(float).eps)


def test_rayleigh_ritz_is_invariant_to_the_scaling_of_the_basis():
    import iterative_solvers_amd as isa
    G, H = spd_pair(12, 7)
    s = np.ldexp(1.0, np.arange(12) * 7 - 40)                          # columns scaled by powers of two from 2^-40 to 2^37
    theta, coef = isa.rayleigh_ritz(G, H)
    theta_s, coef_s = isa.rayleigh_ritz(s[:, None] * G * s[None, :], s[:, None] * H * s[None, :])
    assert np.array_equal(theta, theta_s) and np.array_equal(coef, coef_s * s[:, None])


def test_refused_bases_return_err_state():
    from iterative_solvers_amd import _capi
    import iterative_solvers_amd as isa
    G, H = spd_pair(6, 1)
    zero = G.copy()
    zero[2, :] = 0.0
    zero[:, 2] = 0.0
    rng = np.random.default_rng(2)
    S = rng.standard_normal((40, 6))
    S[:, 4] = S[:, 1]                                                  # a duplicated column
    dup = S.T @ S
    # two unit vectors at an angle phi: the scaled Gram matrix has L = [[1, 0], [cos phi, sin phi]], so min diag(L) = sin phi
    near = lambda sphi: np.array([[1.0, np.sqrt(1 - sphi * sphi)], [np.sqrt(1 - sphi * sphi), 1.0]])
    nan = G.copy()
    nan[0, 0] = np.nan
    for bad, Hm in ((zero, H), (dup, H), (near(0.9e-6), np.eye(2)), (nan, H), (-G, H)):
        with pytest.raises(isa.Mi355cgError) as e:
            isa.rayleigh_ritz(bad, Hm)
        assert e.value.code == _capi.ERR_STATE and "refused" in str(e.value)
    theta, coef = isa.rayleigh_ritz(near(1.1e-6), np.eye(2))           # just above the threshold: accepted
    assert np.all(np.isfinite(theta)) and np.all(np.isfinite(coef))


def test_argument_refusals_that_need_no_device():
    from iterative_solvers_amd import _capi
    import iterative_solvers_amd as isa
    lib = _capi.load()
    buf = np.zeros(64)
    out = _capi.EigResults()
    p = buf.ctypes.data
    for fn in (lib.mi355cg_eigs, lib.mi355cg_eigs_device):
        assert fn(None, 1, 1, 1e-8, 10, p, p, p, None, C.byref(out)) == _capi.ERR_INVALID
        assert fn(None, 0, 0, 0.0, 0, None, None, None, None, None) == _capi.ERR_INVALID
        assert lib.mi355cg_last_error()
    assert lib.mi355cg_eigs_release(None) == _capi.ERR_INVALID
    assert lib.mi355cg_block_gram(None, 1, p, 1, p, p) == _capi.ERR_INVALID
    assert lib.mi355cg_block_combine(None, 1, p, 1, p, p) == _capi.ERR_INVALID
    for k in (0, -1, 49):
        assert lib.mi355cg_rayleigh_ritz(k, p, p, p, p) == _capi.ERR_INVALID
    assert lib.mi355cg_rayleigh_ritz(2, None, p, p, p) == _capi.ERR_INVALID
    with pytest.raises(ValueError, match="square"):
        isa.rayleigh_ritz(np.eye(3), np.eye(2))


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_wrapper_checks_the_start_block_before_calling_the_library():
    from iterative_solvers_amd.solver import _Handle
    h = _Handle.__new__(_Handle)
    h._lib, h._h, h.size, h._device = _NoLibrary(), None, 10, 0
    for x, what in ((np.zeros((3, 9)), "shape"), (np.zeros((2, 10)), "shape"), (np.zeros((3, 10), dtype=np.float32), "dtype"),
                    ([[0.0] * 10] * 3, "NumPy array or a CUDA torch tensor")):
        with pytest.raises(ValueError, match=what):
            h.eigs(2, 3, 1e-8, 10, x)
    with pytest.raises(ValueError, match="vectors"):
        h.block_gram(np.zeros((49, 10)), np.zeros((1, 10)))
    with pytest.raises(ValueError, match="coef"):
        h.block_combine(np.zeros((3, 10)), np.zeros((3, 17)))


@pytest.fixture(scope="module")
def dense():
    """levels and eigvalsh of the dense K per grid, built once"""
    cache = {}

    def get(N):
        if N not in cache:
            levels = er.levels_for(N)
            ev = np.linalg.eigvalsh(er.dense_K(levels))
            ev.setflags(write=False)
            cache[N] = (levels, ev)
        return cache[N]
    return get


@pytest.mark.parametrize("N", [16, 34, 64])
@pytest.mark.parametrize("nev, block", [(1, 1), (6, 8), (16, 16)])
def test_restatement_converges_to_the_dense_spectrum(dense, N, nev, block):
    levels, ev = dense(N)
    n = int(levels[0].mask.sum())
    X0 = np.random.default_rng(0).standard_normal((block, n))
    theta, X, info = er.lobpcg(levels, X0, nev, tol=1e-8)
    print(N, nev, block, "iterations", info["iterations"], "p_drops", info["p_drops"], "rel err", np.abs(theta[:nev] - ev[:nev]).max() / ev[nev - 1])
    assert info["converged"] and info["stop_reason"] == er.CONVERGED
    assert np.all(np.abs(theta[:nev] - ev[:nev]) <= 1e-10 * ev[:nev])
    assert info["iterations"] <= 2 * PROTOTYPE_ITERATIONS[(N, nev, block)]
    assert np.abs(X @ X.T - np.eye(block)).max() <= 1e-12
    for j in range(nev):
        assert np.linalg.norm(er.apply_K(levels, X[j]) - theta[j] * X[j]) <= 2e-8 * theta[j] * np.linalg.norm(X[j])


def test_restatement_stop_rules(dense):
    levels, ev = dense(34)
    n = int(levels[0].mask.sum())
    X0 = np.random.default_rng(0).standard_normal((8, n))
    theta, X, info = er.lobpcg(levels, X0, 6, max_iterations=2)
    assert info["iterations"] == 2 and info["stop_reason"] == er.ITERATIONS and np.all(np.isfinite(info["residuals"]))
    theta, X, info = er.lobpcg(levels, X0, 6, stop=True)
    assert info["iterations"] == 0 and info["stop_reason"] == er.INTERRUPTED
    theta, X, info = er.lobpcg(levels, X0, 6, tol=1e-10)
    theta2, X2, info2 = er.lobpcg(levels, X, 6, tol=1e-8)             # a converged start block: no iteration
    assert info2["iterations"] == 0 and info2["converged"]
    dup = X0.copy()
    dup[5] = dup[2]
    assert er.lobpcg(levels, dup, 6)[2]["stop_reason"] == er.BREAKDOWN


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_eigen_kernels_are_compiled_without_scratch(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_store_hazard_check as chk
    os.environ["PATH"] = os.environ.get("PATH", "") + ":/opt/rocm/bin"
    dump = str(tmp_path / "dev.s")
    chk.compile_to_asm(dump)
    text = open(dump).read()
    meta = text[text.index("amdhsa.kernels"):]
    scratch, vgprs = {}, {}
    for entry in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        scratch[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1))
        vgprs[name] = int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1))
    for k in EIG_KERNELS:
        mine = {n: v for n, v in scratch.items() if re.search(rf"\d+{k}(E|I)", n)}
        assert mine, f"{k} is not in the compiled code"
        assert all(v == 0 for v in mine.values()), mine
    # every template instance the host code launches: gram and reduce with and without symmetry, combine with and without a start
    for k in ("k_eig_gramILb", "k_eig_reduceILb", "k_eig_combineILb"):
        assert sum(1 for n in scratch if k in n) == 2, k
    assert all(v <= 128 for n, v in vgprs.items() if "k_eig_" in n), {n: v for n, v in vgprs.items() if "k_eig_" in n}
    assert not chk.findings(dump)
