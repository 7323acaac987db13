"""Batched multigrid-PCG solves on the GPU (mi355cg_solve_batch / _device).  Every comparison is against
the sequence set_rhs / solve / solution() on the same handle -- the single-solve path -- and is an equality of bits: all of x and
the result fields iterations, converged, stop_reason, final_residual_norm, final_precision, r_norm2, initial_r_norm2."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mg_cases import batch_rhs  # noqa: E402

pytestmark = pytest.mark.gpu

DOM = (1.0, 2.0, 1.0, 2.0)
FIELDS = ("iterations", "converged", "stop_reason", "final_residual_norm", "final_precision", "r_norm2", "initial_r_norm2")
DBL_MAX = sys.float_info.max


def system(N, kind=None):
    import iterative_solvers_amd as isa
    s = isa.MatrixFreeSystem(N, N, *DOM)
    s.set_preconditioner(isa.PRECOND_MG_ANY if kind is None else kind)
    return s


def rel_params(eps=1e-8, max_iterations=1000):
    import iterative_solvers_amd as isa
    p = isa.default_params(isa.RULE_REL_2NORM)
    p.eps_rel, p.max_iterations, p.use_true_solution = eps, max_iterations, 0
    return p


def msg_params():
    import iterative_solvers_amd as isa
    p = isa.default_params(isa.RULE_MSG_MAXNORM)
    p.use_true_solution = 0
    return p


def sequential(s, p, rhs, stop_flag=None):
    """set_rhs / solve / solution() per vector on the system's own handle, which gets its b back afterwards"""
    h = s._handle
    keep = h.rhs()
    xs, res = [], []
    for v in rhs:
        h.set_rhs(v)
        res.append(h.solve(p, None, stop_flag))
        xs.append(h.solution())
    h.set_rhs(keep)
    return np.stack(xs), res


def fields(r):
    return tuple(getattr(r, f) for f in FIELDS)


def assert_same(xb, rb, xs, rs):
    assert len(rb) == len(rs) == xb.shape[0] == xs.shape[0]
    for k in range(len(rs)):
        assert fields(rb[k]) == fields(rs[k]), (k, fields(rb[k]), fields(rs[k]))
        assert rb[k].final_error_norm == DBL_MAX
        assert np.array_equal(xb[k], xs[k]), (k, np.abs(xb[k] - xs[k]).max())
    assert len({r.solve_seconds for r in rb}) == 1 and len({r.loop_seconds for r in rb}) == 1


def normals(s, nrhs, seed):
    return np.random.default_rng(seed).standard_normal((nrhs, s.size()))


# 1 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, kind", [(34, "any"), (130, "any"), (258, "any"), (1000, "any"), (256, "mg"), (16, "any")])
def test_rel_2norm_batch_has_the_bits_of_sequential_solves(N, kind):
    import iterative_solvers_amd as isa
    s = system(N, isa.PRECOND_MG if kind == "mg" else isa.PRECOND_MG_ANY)
    rhs = batch_rhs(N, s.get_rhs())
    p = rel_params()
    xs, rs = sequential(s, p, rhs)
    xb, rb = s._handle.solve_batch(p, rhs)
    its = [r.iterations for r in rs]
    print(f"N={N} {kind}: iterations {its}")
    assert len(set(its)) >= 2 and its[1] == 0, its                  # systems stopped at different iterations: the freeze path ran
    assert all(r.converged for r in rs)
    assert_same(xb, rb, xs, rs)


# 2 --------------------------------------------------------------------------------------------------------------------------
def test_msg_rule_batch_has_the_bits_of_sequential_solves():
    N = 258
    s = system(N)
    b = s.get_rhs()
    rhs = np.stack([b, np.ldexp(b, -40), np.ones(b.size), np.random.default_rng(N).standard_normal(b.size)])
    p = msg_params()
    xs, rs = sequential(s, p, rhs)
    xb, rb = s._handle.solve_batch(p, rhs)
    its = [r.iterations for r in rs]
    print(f"MSG rule N={N}: iterations {its}, reasons {[r.stop_reason for r in rs]}")
    assert its[1] == 1 and its[0] > 1, its                          # the absolute thresholds stop 2^-40 b after its first iteration
    assert_same(xb, rb, xs, rs)


# 3 --------------------------------------------------------------------------------------------------------------------------
def test_a_system_does_not_depend_on_its_place_or_its_company():
    N = 258
    s = system(N)
    rhs = batch_rhs(N, s.get_rhs())
    p = rel_params()
    xb, rb = s._handle.solve_batch(p, rhs)
    xr, rr = s._handle.solve_batch(p, np.ascontiguousarray(rhs[::-1]))
    assert_same(xr[::-1], rr[::-1], xb, rb)
    for k in range(rhs.shape[0]):
        x1, r1 = s._handle.solve_batch(p, rhs[k:k + 1].copy())
        assert_same(x1, r1, xb[k:k + 1], rb[k:k + 1])


# 4 --------------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_64_and_the_refusal_of_65():
    s = system(130)
    p = rel_params()
    rhs = normals(s, 64, 64)
    xs, rs = sequential(s, p, rhs)
    xb, rb = s._handle.solve_batch(p, rhs)
    assert_same(xb, rb, xs, rs)
    with pytest.raises(ValueError):
        s._handle.solve_batch(p, normals(s, 65, 65))
    # the library's own refusal, under the wrapper's
    res = (type(rb[0]) * 65)()
    big = normals(s, 65, 65)
    out = np.empty_like(big)
    lib = s._handle._lib
    assert lib.mi355cg_solve_batch(s._handle._h, C.byref(p), 65, big.ctypes.data, out.ctypes.data, None, res) == 1


# 5 --------------------------------------------------------------------------------------------------------------------------
def test_device_entry_point_gives_the_host_entry_points_bits():
    import torch
    N = 258
    s = system(N)
    rhs = batch_rhs(N, s.get_rhs())
    p = rel_params()
    xh, rh = s._handle.solve_batch(p, rhs)
    bt = torch.from_numpy(rhs).cuda()
    xt, rt = s._handle.solve_batch(p, bt)
    assert isinstance(xt, torch.Tensor) and xt.is_cuda and xt.dtype == torch.float64 and tuple(xt.shape) == rhs.shape
    assert_same(xt.cpu().numpy(), rt, xh, rh)
    assert np.array_equal(bt.cpu().numpy(), rhs)                    # b is read, not written
    with pytest.raises(ValueError, match="dtype"):
        s._handle.solve_batch(p, bt.float())
    with pytest.raises(ValueError, match="contiguous"):
        s._handle.solve_batch(p, bt.t().contiguous().t())
    res = (type(rh[0]) * 2)()                                       # the library's refusal of x overlapping b
    lib = s._handle._lib
    assert lib.mi355cg_solve_batch_device(s._handle._h, C.byref(p), 2, bt.data_ptr(), bt.data_ptr() + 8 * s.size(), None, res) == 1
    assert b"overlaps" in lib.mi355cg_last_error()
    assert np.array_equal(bt.cpu().numpy(), rhs)


# 6 --------------------------------------------------------------------------------------------------------------------------
def test_true_residual_of_every_system():
    from oracle.oracle import OracleGrid
    N = 258
    s = system(N)
    rhs = batch_rhs(N, s.get_rhs())
    xb, rb = s.solve_batch(rhs, eps=1e-8, max_iterations=1000)
    A = OracleGrid(N, N, *DOM)
    for k, (b, x) in enumerate(zip(rhs, xb)):
        if not b.any():
            assert not x.any()
            continue
        tr = np.linalg.norm(b - A.apply(x))
        print(f"system {k}: |b - A x| / |b| = {tr / np.linalg.norm(b):.3e}")
        assert tr <= 2e-8 * np.linalg.norm(b)


# 7 --------------------------------------------------------------------------------------------------------------------------
def test_a_batch_leaves_the_handle_as_it_was():
    N = 258
    s = system(N)
    h = s._handle
    p = rel_params()
    b0 = h.rhs()
    r1 = h.solve(p)
    x1, rr1 = h.solution(), h.recursive_residual()
    h.solve_batch(p, batch_rhs(N, b0))
    assert np.array_equal(h.solution(), x1) and np.array_equal(h.recursive_residual(), rr1)
    assert np.array_equal(h.rhs(), b0)
    r2 = h.solve(p)
    assert fields(r2) == fields(r1) and np.array_equal(h.solution(), x1)


# 8 --------------------------------------------------------------------------------------------------------------------------
def test_a_stop_flag_set_before_the_call_interrupts_every_system_that_would_iterate():
    import iterative_solvers_amd as isa
    N = 130
    s = system(N)
    rhs = batch_rhs(N, s.get_rhs())
    p = rel_params()
    flag = C.c_int(1)
    xs, rs = sequential(s, p, rhs, flag)
    xb, rb = s._handle.solve_batch(p, rhs, flag)
    assert_same(xb, rb, xs, rs)
    for k, r in enumerate(rb):
        assert r.iterations == 0 and not xb[k].any()
        if rhs[k].any():
            assert r.stop_reason == isa.StopCriterion.INTERRUPTED and not r.converged
        else:
            assert r.stop_reason == isa.StopCriterion.ITERATIONS and r.converged     # 0 <= eps * 0 before the flag is looked at


# 9 --------------------------------------------------------------------------------------------------------------------------
def test_fixed_iterations():
    N = 130
    s = system(N)
    rhs = batch_rhs(N, s.get_rhs(), scaled=False)[[0, 2, 3, 4]]     # no zero vector: 0 / 0 in alpha, and NaN bits are no contract
    p = rel_params(max_iterations=3)
    p.fixed_iterations = 1
    xs, rs = sequential(s, p, rhs)
    xb, rb = s._handle.solve_batch(p, rhs)
    assert [r.iterations for r in rb] == [3] * 4
    assert_same(xb, rb, xs, rs)


# 10 -------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    import iterative_solvers_amd as isa
    N = 130
    s = isa.MatrixFreeSystem(N, N, *DOM)
    rhs = batch_rhs(N, s.get_rhs())
    p = rel_params()

    def good():
        xs, rs = sequential(s, p, rhs)
        xb, rb = s._handle.solve_batch(p, rhs)
        assert_same(xb, rb, xs, rs)

    with pytest.raises(isa.Mi355cgError, match="no preconditioner"):
        s._handle.solve_batch(p, rhs)
    s.set_preconditioner(isa.PRECOND_MG_ANY, isa.CYCLE_F32)
    with pytest.raises(ValueError, match="CYCLE_F32"):
        s._handle.solve_batch(p, rhs)
    s.set_preconditioner(isa.PRECOND_MG_ANY)
    good()
    for name in ("use_true_solution", "diagnostics"):
        bad = rel_params()
        setattr(bad, name, 1)
        with pytest.raises(ValueError, match=name):
            s._handle.solve_batch(bad, rhs)
        good()
    bad = rel_params()
    bad.rule = 7
    with pytest.raises(ValueError, match="rule"):
        s._handle.solve_batch(bad, rhs)
    good()


# 11 -------------------------------------------------------------------------------------------------------------------------
def test_workspace_lifetime():
    import iterative_solvers_amd as isa
    N = 130
    s = system(N)
    h = s._handle
    p = rel_params()
    h.batch_release()                                               # nothing to free: OK
    rhs = np.concatenate([batch_rhs(N, s.get_rhs()), normals(s, 1, 1)])
    xs, rs = sequential(s, p, rhs)

    def check(n):
        xb, rb = h.solve_batch(p, rhs[:n].copy())
        assert_same(xb, rb, xs[:n], rs[:n])

    check(8)
    check(2)
    h.batch_release()
    check(4)
    s.set_preconditioner(isa.PRECOND_NONE)
    s.set_preconditioner(isa.PRECOND_MG_ANY)
    check(4)
    h.batch_release()
    h.batch_release()


def test_workspace_is_given_back():
    import torch
    N = 1000
    s = system(N)
    p = rel_params()
    rhs = normals(s, 16, 16)
    free = []
    for _ in range(2):
        s._handle.solve_batch(p, rhs)
        s.batch_release()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info()[0])
    vector = 8 * s._handle.layout()["padded_len"]                   # one level-0 vector, about 6 MB
    print(f"free after each release: {free}, one vector = {vector} B")
    assert free[1] >= free[0] - vector, free


# 12 -------------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_16_at_n1000_is_faster_than_16_solves():
    """Best of three wall times of one 16-system batch against the best of three sums of the 16 single solves' wall times, after
    one warm-up of each path, the repetitions alternating.  Moving the vectors is timed on neither side: set_rhs and solution()
    are outside the clock, and the batch takes its vectors from device memory (the device entry point).
    Measured (profiles/mg_batch_time_to_solution.txt, tools/mg_timing.py --batch, N = 1000, nrhs = 16): batch 8.73 ms against
    26.07 ms for the 16 solves of the commit before the feature, ratio 0.335 (0.333 against this tree's own 16 solves).  The
    bound is twice that, 0.67: boxes differ by about 5 % and sub-millisecond solves spread more."""
    import torch
    N = 1000
    s = system(N)
    h = s._handle
    p = rel_params()
    rhs = normals(s, 16, 1000)
    dev = torch.from_numpy(rhs).cuda()

    def seq():
        t = 0.0
        for v in rhs:
            h.set_rhs(v)
            t0 = time.perf_counter()
            h.solve(p)
            t += time.perf_counter() - t0
        return t

    def bat():
        t0 = time.perf_counter()
        h.solve_batch(p, dev)
        return time.perf_counter() - t0

    seq(), bat()
    ts, tb = [], []
    for _ in range(3):
        ts.append(seq())
        tb.append(bat())
    ratio = min(tb) / min(ts)
    print(f"N=1000 nrhs=16: batch {min(tb) * 1e3:.3f} ms, 16 solves {min(ts) * 1e3:.3f} ms, ratio {ratio:.3f}")
    assert ratio < 0.67, (tb, ts)


# 13 -------------------------------------------------------------------------------------------------------------------------
def test_cpp_compat_solve_batch(tmp_path):
    import subprocess
    from iterative_solvers_amd import build as b
    b.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "mg_batch_compat_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                           "-I", os.path.join(root, "iterative_solvers_amd", "compat"), os.path.join(root, "tests", "cpp", "mg_batch_compat_driver.cpp"),
                           "-L", os.path.join(root, "iterative_solvers_amd"), "-lmi355cg",
                           "-Wl,-rpath," + os.path.join(root, "iterative_solvers_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
