"""The adjoint of the recorded explicit wave stepper in a medium (csrc/onchip_plan.h), without a GPU.
tests/cpp/onchip_wave_adjoint_plan_driver.cpp, a program of its own built with the sanitizers, (1) runs whole backward steps -- and
the forward steps that keep the history -- as the kernels run them, with the functions the kernels call, which is compared bit for
bit with the NumPy model of tests/wave_adjoint_reference.py, and (2) restates the two byte formulas for every even N from 6 to the
cap.  The model's own properties are checked here too: its three derivatives against central differences of the forward model's
misfit, a backward run may be split at a multiple of the cadence, nothing in gives nothing out, and the history does not touch the
forward run.  The header, the ctypes layer, the package and the built kernels must agree on the new entry points."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_adjoint_reference as A  # noqa: E402
import wave_medium_reference as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE, STRETCHED = (1.0, 2.0, 1.0, 2.0), (0.0, 1.0, 0.0, 1.7)
LLVM = os.path.join(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")), "..", "lib", "llvm", "bin")


def grid(n):
    """N = 20 is stretched: xk != yk."""
    return A.Grid.of_domain(n, *(STRETCHED if n == 20 else SQUARE))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("onchip_wave_adjoint") / "onchip_wave_adjoint_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "onchip_wave_adjoint_plan_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def lines(driver):
    out = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    return [ln.split() for ln in out.stdout.splitlines()]


def run_file(driver, tmp_path, values, *mode):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.atleast_1d(np.asarray(a, dtype=np.float64)).reshape(-1) for a in values]).tofile(src)
    out = subprocess.run([driver, src, dst, *mode], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-2000:]
    return np.fromfile(dst, dtype=np.float64)


def run_backward(driver, tmp_path, g, tau, H, c2, adj, receivers, every, lam, q, S):
    nsteps = len(H) - 1
    got = run_file(driver, tmp_path, [[float(g.n), tau, float(nsteps), g.A0, g.xk, g.yk, float(every), float(len(receivers))], g.image(q), lam, S, c2, H, adj,
                                      np.asarray(receivers, dtype=np.float64)])
    assert got.shape == (3 * g.size,)
    return got[:g.size], got[g.size:2 * g.size], got[2 * g.size:]


def seeded(g, seed, nsteps, every, frac=0.77):
    """The setup of the derivative check: states and a forcing, a medium in [0.25, 4], tau at `frac` of its bound, seeded amplitudes,
    the five receivers of tests/test_gpu_wave_medium.py -- three seeded nodes and both ends -- and observed traces."""
    rng = np.random.default_rng(seed)
    u, v = rng.standard_normal(g.size), rng.standard_normal(g.size) * np.sqrt(abs(g.A0))
    gv = rng.standard_normal(g.size) * abs(g.A0)
    c2 = rng.uniform(0.25, 4.0, g.size)
    tau = frac * M.medium_cfl(g, c2.max())
    w = rng.standard_normal(nsteps + 1)
    receivers = [int(r) for r in rng.integers(0, g.size, 3)] + [0, g.size - 1]
    observed = rng.standard_normal((nsteps // every, 5))
    return u, v, gv, c2, tau, w, receivers, observed


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- whole steps against the driver --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 10, 20])
def test_backward_steps_are_the_models_operation_by_operation(driver, tmp_path, n):
    g = grid(n)
    assert (g.xk != g.yk) == (n == 20)
    for nsteps, every in ((1, 1), (7, 3), (0, 2), (6, 2), (23, 3), (5, 7)):
        u, v, gv, c2, tau, w, receivers, _ = seeded(g, 700 + n + nsteps, nsteps, every)
        H = A.verlet_history(g, u, v, gv, c2, tau, nsteps, w)[3]
        rng = np.random.default_rng(710 + n + nsteps)
        adj = rng.standard_normal((nsteps // every, 5)) * 10.0 ** rng.integers(-3, 4, (nsteps // every, 5))
        lam, q, S = (rng.standard_normal(g.size) for _ in range(3))
        twice = [receivers[1], receivers[0], receivers[1], 0, 0]     # duplicates add in the order of the list
        for rec in (receivers, twice):
            got = run_backward(driver, tmp_path, g, tau, H, c2, adj, rec, every, lam, q, S)
            assert same(got, A.adjoint(g, H, c2, tau, adj, rec, every, lam, q, S)), (n, nsteps, every)
    # one step, written out once more without the model's loop
    u, v, gv, c2, tau, w, receivers, _ = seeded(g, 800 + n, 1, 1)
    H = A.verlet_history(g, u, v, gv, c2, tau, 1, w)[3]
    r = np.random.default_rng(801 + n).standard_normal((1, 5))
    lam, q, S = np.zeros(g.size), np.zeros(g.size), np.zeros(g.size)
    h = 0.5 * tau
    for j, node in enumerate(receivers):
        lam[node] = lam[node] + r[0, j]
    S = S + q * H[1]
    lam = lam + h * g.au(q)
    q = q + tau * (c2 * lam)
    S = S + q * H[0]
    lam = lam + h * g.au(q)
    got = run_backward(driver, tmp_path, g, tau, H, c2, r, receivers, 1, np.zeros(g.size), np.zeros(g.size), np.zeros(g.size))
    assert same(got, (lam, q, S)) and np.abs(S).max() > 0


@pytest.mark.parametrize("n", [6, 10, 20])
def test_forward_steps_with_the_history_are_the_models(driver, tmp_path, n):
    g = grid(n)
    for nsteps, every in ((1, 1), (7, 3), (0, 2), (6, 2)):
        u, v, gv, c2, tau, w, receivers, _ = seeded(g, 900 + n + nsteps, nsteps, every, frac=0.5)
        got = run_file(driver, tmp_path, [[float(g.n), tau, float(nsteps), g.A0, g.xk, g.yk, float(every), 5.0], g.image(u), gv, v, c2, w, np.asarray(receivers, dtype=np.float64)],
                       "forward")
        samples = nsteps // every
        want = A.verlet_history(g, u, v, gv, c2, tau, nsteps, w, receivers, every)
        parts = np.split(got, [g.size, 2 * g.size, 2 * g.size + samples * 5])
        assert same((parts[0], parts[1], parts[2].reshape(samples, 5), parts[3].reshape(nsteps + 1, g.size)), want), (n, nsteps)


def test_the_driver_found_no_violation(lines):
    assert not [ln for ln in lines if ln and ln[0] == "FAIL"]
    assert lines[-1] == ["ok", "0"]


# ---- the model's own properties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 20, 64])
def test_the_three_derivatives_are_central_differences_of_the_forward_models_misfit(n):
    """h S / c2, lam and q / c2 against central differences of wave_medium_reference.verlet_medium's misfit 1/2 sum (traces -
    observed)^2: 23 steps sampled every 3rd, tau at 0.77 of the bound, c2 in [0.25, 4], the five receivers; relative step 1e-5
    along one seeded direction, tolerance 1e-6 relative (measured: at most 6.6e-9)."""
    g = grid(n)
    u0, v0, gv, c2, tau, w, receivers, observed = seeded(g, 1000 + n, 23, 3)

    def misfit(c2=c2, u0=u0, v0=v0):
        r = M.verlet_medium(g, u0, v0, gv, c2, tau, 23, w, receivers, 3)[2] - observed
        return 0.5 * np.sum(r * r)

    J, gc, gu, gv0, traces = A.gradient(g, u0, v0, gv, c2, tau, 23, w, observed, receivers, 3)
    assert J == misfit() and np.array_equal(traces, M.verlet_medium(g, u0, v0, gv, c2, tau, 23, w, receivers, 3)[2])
    rng = np.random.default_rng(1001 + n)
    for name, grad, base in (("c2", gc, c2), ("u0", gu, u0), ("v0", gv0, v0)):
        d = rng.standard_normal(g.size)
        e = 1e-5 * np.linalg.norm(base) / np.linalg.norm(d)
        fd = (misfit(**{name: base + e * d}) - misfit(**{name: base - e * d})) / (2 * e)
        err = abs(fd - grad @ d) / abs(fd)
        print("N", n, name, "directional derivative", fd, "adjoint", grad @ d, "relative difference", err)
        assert err <= 1e-6, (n, name)


@pytest.mark.parametrize("n", [6, 10, 20])
def test_a_backward_run_split_at_a_multiple_of_the_cadence_is_the_whole_run(n):
    g = grid(n)
    rng = np.random.default_rng(1100 + n)
    members, nsteps, every = 4, 24, 3
    u, v = rng.standard_normal((members, g.size)), rng.standard_normal((members, g.size)) * np.sqrt(abs(g.A0))
    gv = rng.standard_normal((members, g.size)) * abs(g.A0)
    c2 = rng.uniform(0.25, 4.0, (members, g.size))
    tau = M.medium_cfl(g, c2.max(axis=-1)) * rng.uniform(0.1, 1.0, members)
    w = rng.standard_normal((members, nsteps + 1))
    receivers = [int(r) for r in rng.integers(0, g.size, 3)] + [0, g.size - 1]
    adj = rng.standard_normal((members, nsteps // every, 5))
    H = A.verlet_history(g, u, v, gv, c2, tau, nsteps, w)[3]
    whole = A.adjoint(g, H, c2, tau, adj, receivers, every)
    for cut in (3, 15, 21):                                          # the steps above the cut first
        first = A.adjoint(g, H[:, cut:], c2, tau, adj[:, cut // every:], receivers, every)
        second = A.adjoint(g, H[:, :cut + 1], c2, tau, adj[:, :cut // every], receivers, every, *first)
        assert same(second, whole), cut
    # a member alone is that member of the ensemble; one medium for all is that medium for each
    assert same(A.adjoint(g, H[2], c2[2], float(tau[2]), adj[2], receivers, every), [x[2] for x in whole])
    assert same(A.adjoint(g, H, c2[1], tau, adj, receivers, every), A.adjoint(g, H, np.stack([c2[1]] * members), tau, adj, receivers, every))
    # 23 steps: the cadence does not divide the run
    H23 = A.verlet_history(g, u, v, gv, c2, tau, 23, w[:, :24])[3]
    assert np.array_equal(H23, H[:, :24])
    a, b = A.adjoint(g, H23[:, 12:], c2, tau, adj[:, 4:7], receivers, every), A.adjoint(g, H23, c2, tau, adj[:, :7], receivers, every)
    assert same(A.adjoint(g, H23[:, :13], c2, tau, adj[:, :4], receivers, every, *a), b)


def test_no_source_and_no_state_leave_zeros_and_the_history_leaves_the_forward_run():
    g = grid(10)
    u, v, gv, c2, tau, w, receivers, _ = seeded(g, 1200, 23, 3)
    fwd = A.verlet_history(g, u, v, gv, c2, tau, 23, w, receivers, 3)
    assert same(fwd[:3], M.verlet_medium(g, u, v, gv, c2, tau, 23, w, receivers, 3))
    assert fwd[3].shape == (24, g.size) and np.array_equal(fwd[3][0], g.au(u)) and np.array_equal(fwd[3][23], g.au(fwd[0]))
    zero = A.adjoint(g, fwd[3], c2, tau, np.zeros((7, 5)), receivers, 3)
    assert not any(np.any(a) for a in zero)
    assert not any(np.any(a) for a in A.adjoint(g, fwd[3], c2, tau, np.zeros((7, 0)), (), 3))
    # no steps: the state comes back as it went in
    lam = np.arange(g.size, dtype=np.float64)
    assert same(A.adjoint(g, fwd[3][:1], c2, tau, np.zeros((0, 5)), receivers, 3, lam, lam + 1, lam + 2), (lam, lam + 1, lam + 2))


# ---- the formulas, the header, the bindings, the built kernels ----------------------------------------------------------------------
def test_byte_formulas_for_every_even_n(lines):
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    lib = _capi.load()
    cap = [int(ln[1]) for ln in lines if ln and ln[0] == "cap"][0]
    rows = {int(ln[0][2:]): ln for ln in lines if ln and ln[0].startswith("N=")}
    assert sorted(rows) == list(range(6, cap + 1, 2))
    for n, ln in rows.items():
        unknowns = int(ln[1].split("=")[1])
        assert unknowns == (n // 2 - 1) * (3 * n // 2 - 1)
        for nsys, nsteps, nbytes in (tuple(int(v) for v in e.split(":")) for e in ln[2].split("=")[1].split(",")):
            assert nbytes == 8 * nsys * (nsteps + 1) * unknowns, (n, nsys, nsteps)
            if n in (6, 10, 64, cap) or (nsys, nsteps) == (40, 7):
                out = C.c_longlong()
                assert lib.mi355cg_wave_history_bytes(n, nsys, nsteps, C.byref(out)) == _capi.OK and out.value == nbytes
                assert isa.wave_history_bytes(n, nsys, nsteps) == nbytes
        for nsys, nsteps, nrec, every, nbytes in (tuple(int(v) for v in e.split(":")) for e in ln[3].split("=")[1].split(",")):
            want = nsys * (24 * unknowns + 456) + 8 + 16 * nsys + 8 * unknowns + 4 * 64 + 16 * nsys
            assert nbytes == want == isa.wave_medium_many_workspace(n, nsys, nsteps, nrec, every), (n, nsys, nsteps, nrec, every)
            if n in (6, 10, 64, cap) or (nsys, nsteps) == (40, 7):
                out = C.c_longlong()
                assert lib.mi355cg_wave_adjoint_many_workspace(n, nsys, nsteps, nrec, every, C.byref(out)) == _capi.OK and out.value == want
                assert isa.wave_adjoint_many_workspace(n, nsys, nsteps, nrec, every) == want
    assert isa.wave_history_bytes(128, 1, 1) == 2 * 8 * 63 * 191                       # 97 KB a step at the cap
    for f, bad in ((isa.wave_history_bytes, ((cap + 2, 1, 1), (7, 1, 1), (10, 0, 1), (10, _capi.MANY_MAX + 1, 1), (10, 1, -1), (10, 1, _capi.STEPS_MANY_MAX_STEPS + 1))),
                   (isa.wave_adjoint_many_workspace, ((cap + 2, 1, 1), (7, 1, 1), (10, 0, 1), (10, 1, -1), (10, 1, 1, -1), (10, 1, 1, 65), (10, 1, 1, 1, 0)))):
        for args in bad:
            with pytest.raises(ValueError):
                f(*args)
    assert lib.mi355cg_wave_history_bytes(10, 1, 1, None) == _capi.ERR_INVALID
    assert lib.mi355cg_wave_adjoint_many_workspace(10, 1, 1, 0, 1, None) == _capi.ERR_INVALID


def test_header_ctypes_package_and_compat_agree():
    import inspect
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    text = open(os.path.join(ROOT, "include", "mi355cg.h")).read()
    lib = _capi.load()
    for name in ("mi355cg_wave_history_many", "mi355cg_wave_history_many_device", "mi355cg_wave_history_bytes", "mi355cg_wave_adjoint_many",
                 "mi355cg_wave_adjoint_many_device", "mi355cg_wave_adjoint_many_workspace"):
        assert name in _capi.EXPORTS and ("int  " + name + "(") in text
        assert hasattr(lib, name)
    assert "no reference twin" in text[text.index("The adjoint of the scheme in a medium"):text.index("int  mi355cg_wave_history_many(")]
    for name in ("wave_history_many", "wave_adjoint_many", "wave_gradient_many"):
        assert callable(getattr(isa.MatrixFreeSystem, name))
    sig = inspect.signature(isa.MatrixFreeSystem.wave_gradient_many).parameters
    assert sig["segment"].default is None and sig["c2"].default is None and sig["damping"].default is None
    assert [p for p in inspect.signature(isa.MatrixFreeSystem.wave_adjoint_many).parameters][1:5] == ["hist", "tau", "c2", "adjoint_source"]
    for name in ("wave_history_bytes", "wave_adjoint_many_workspace"):
        assert callable(getattr(isa, name)) and name in isa.__all__
    compat = open(os.path.join(ROOT, "iterative_solvers_amd", "compat", "mi355cg_compat.hpp")).read()
    assert "waveHistoryMany(" in compat and "waveAdjointMany(" in compat
    plan = open(os.path.join(ROOT, "iterative_solvers_amd", "csrc", "onchip_plan.h")).read()
    kernels = open(os.path.join(ROOT, "iterative_solvers_amd", "csrc", "onchip_kernels.h")).read()
    for fn in ("onchip_wave_au", "onchip_wave_medium_accel_of", "onchip_wave_adjoint_inject", "onchip_wave_adjoint_sens", "onchip_wave_adjoint_kick",
               "onchip_wave_adjoint_drift"):
        assert ("MI355CG_HD inline double " + fn + "(") in plan and (fn + "(") in kernels
    assert "onchip_wave_history_bytes(" in plan and "onchip_wave_adjoint_workspace_bytes(" in plan
    # the entry points refuse a null handle before they touch a GPU
    for fn in (lib.mi355cg_wave_history_many, lib.mi355cg_wave_history_many_device):
        assert fn(None, 1, 1, None, None, None, None, None, 0, None, 0, None, 0, 0, None, 1, None, 0, None, None, None) == _capi.ERR_INVALID
    for fn in (lib.mi355cg_wave_adjoint_many, lib.mi355cg_wave_adjoint_many_device):
        assert fn(None, 1, 1, None, None, 0, None, 0, 0, None, 1, None, 0, None, None, None, 0, None, None, None) == _capi.ERR_INVALID


# the three recording kernels as the parent built them: the existing calls stay the code they were
RECORD_VGPRS = {1: 30, 2: 38, 4: 50, 8: 78, 16: 134, 24: 190}
MEDIUM_VGPRS = {1: 32, 2: 42, 4: 58, 8: 94, 16: 166, 24: 238}
SPONGE_VGPRS = {1: 34, 2: 44, 4: 60, 8: 96, 16: 168, 24: 240}


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")), reason="needs the ROCm LLVM tools")
def test_the_new_kernels_are_built_without_scratch_and_the_others_are_unchanged(tmp_path):
    from iterative_solvers_amd import build as b
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", b.build(), fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={co}"])
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    names = ("k_oc_wave_history", "k_oc_wave_adjoint", "k_oc_wave_sponge", "k_oc_wave_medium", "k_oc_wave_record")
    found = {k: {} for k in names}
    for entry in notes[notes.index("amdhsa.kernels"):].split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1))
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", entry).group(1))
        m = re.search(r"\d+(" + "|".join(names) + r")ILi(\d+)E", name)
        if m:
            found[m.group(1)][int(m.group(2))] = (vgprs, scratch)
    print("k_oc_wave_history<E>: (VGPRs, scratch)", found["k_oc_wave_history"])
    print("k_oc_wave_adjoint<E>: (VGPRs, scratch)", found["k_oc_wave_adjoint"])
    for kernels in found.values():
        assert sorted(kernels) == [1, 2, 4, 8, 16, 24] and not any(s for _, s in kernels.values())
    assert all(v <= 256 for k in ("k_oc_wave_history", "k_oc_wave_adjoint") for v, _ in found[k].values())
    assert {e: v for e, (v, _) in found["k_oc_wave_record"].items()} == RECORD_VGPRS
    assert {e: v for e, (v, _) in found["k_oc_wave_medium"].items()} == MEDIUM_VGPRS
    assert {e: v for e, (v, _) in found["k_oc_wave_sponge"].items()} == SPONGE_VGPRS
