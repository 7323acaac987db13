"""Generic CSR path: Solver(a, b, ...) with a caller-supplied matrix.  The first three tests run on the grid
operator's own CSR (oracle-assembled in the reference's entry order), where the CPU oracle is the checker; the rest run on
matrices that are not the grid's, against the NumPy model of tests/csr_reference.py (pinned by tests/test_csr_reference_cpu.py)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csr_reference as model  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", [6, 16, 64, 130])
def test_csr_apply_bit_exact(N):
    import iterative_solvers_amd as isa
    from oracle.oracle import OracleGrid
    og = OracleGrid(N, N)
    A = isa.CrsMatrix(*og.csr())
    assert A.numRows() == og.size
    x = np.random.default_rng(5).uniform(-1, 1, og.size)
    assert np.array_equal(A.apply(x), og.apply(x))              # per-row sums in entry order = the serial CSR loop


@pytest.mark.parametrize("N", [16, 64])
def test_csr_cg_matches_oracle_both_rules(N):
    import iterative_solvers_amd as isa
    from oracle.oracle import OracleGrid
    og = OracleGrid(N, N)
    A = isa.CrsMatrix(*og.csr())
    b, u = og.rhs(), og.true_solution()
    ref = og.mf_solve(eps=1e-8, max_iterations=10 ** 5)
    sol = isa.MatrixFreeSolver(A, b, 1e-8, 10 ** 5)
    x = sol.solve()
    assert sol.getIterations() == ref.iterations
    assert np.abs(x - ref.x).max() <= 1e-9 * np.abs(ref.x).max()
    assert abs(sol.last_results.r_norm2 - ref.r_norm) / ref.initial_r_norm <= 1e-12
    refm = og.msg_solve(eps_precision=1e-9, eps_residual=1e-9, eps_exact_error=-1.0)
    m = isa.MSGSolver(A, b, 1e-9, 10000)
    m.setExactErrorEps(-1.0)
    got = []
    m.setIterationCallback(lambda *a: got.append(a))
    xm = m.solve(u)
    assert (m.getIterations(), int(m.getStopReason()), m.hasConverged()) == (refm.iterations, refm.stop_reason, refm.converged)
    assert [g[0] for g in got] == [c[0] for c in refm.callbacks]
    assert np.abs(xm - refm.x).max() <= 1e-9 * np.abs(refm.x).max()
    assert m.getFinalErrorNorm() == pytest.approx(refm.final_error_norm, rel=1e-9)
    # the stencil path and the CSR path walk the same iterates
    s = isa.GridSystem(N, N, 1.0, 2.0, 1.0, 2.0)
    ms = isa.MSGSolver(s, b, 1e-9, 10000)
    ms.setExactErrorEps(-1.0)
    assert np.array_equal(ms.solve(u), xm)


def test_csr_rejects_malformed_input_and_long_rows_work():
    import iterative_solvers_amd as isa
    with pytest.raises(ValueError):
        isa.CrsMatrix([0, 2, 1], [0, 1], [1.0, 1.0])            # row_map not monotone
    with pytest.raises(ValueError):
        isa.CrsMatrix([0, 1], [3], [1.0])                        # column out of range
    # a dense-ish SPD matrix: rows of 3000 entries cross the kernel's LDS chunk (2048 products)
    n = 3000
    rng = np.random.default_rng(11)
    M = rng.standard_normal((n, 40))
    S = M @ M.T + n * np.eye(n)
    row_map = np.arange(0, n * n + 1, n, dtype=np.int32)
    entries = np.tile(np.arange(n, dtype=np.int32), n)
    A = isa.CrsMatrix(row_map, entries, S.ravel())
    x = rng.standard_normal(n)
    y = A.apply(x)
    assert np.allclose(y, S @ x, rtol=1e-12, atol=1e-9)
    assert np.array_equal(y[:8], [float(np.cumsum(S[i] * x)[-1]) for i in range(8)])
    b = S @ np.ones(n)
    sol = isa.MatrixFreeSolver(A, b, 1e-12, 1000)
    xs = sol.solve()
    assert sol.last_results.converged and np.abs(xs - 1.0).max() < 1e-8


# ---- matrices that are not the grid's: y = A x against the model, bit for bit over the whole vector -----------------------------------
APPLY_FIXTURES = {
    "tiny_one": lambda: model.tiny(True),
    "tiny_none": lambda: model.tiny(False),
    "exact_chunk_255": lambda: model.exact_chunk(255),
    "exact_chunk_256": lambda: model.exact_chunk(256),
    "exact_chunk_257": lambda: model.exact_chunk(257),
    "boundary_between_rows": model.boundary_between_rows,
    "nine_point": model.nine_point,
    "ragged": model.ragged,
    "empty": model.empty,
    "long_chain": lambda: model.long_chain(seed=24),
}


def _same_bits(y, ref):
    return np.array_equal(y, ref) and np.array_equal(np.signbit(y), np.signbit(ref))


def _apply_into_nan(A, x):
    """A x through mi355cg_apply_device into a vector that holds NaN beforehand: a row the kernel does not write shows."""
    import torch
    from iterative_solvers_amd import _capi
    xd = torch.from_numpy(x).cuda()
    yd = torch.full_like(xd, float("nan"))
    torch.cuda.synchronize()                                                    # the library works on its own stream
    _capi.check(_capi.load().mi355cg_apply_device(A._handle._h, C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr())))
    return yd.cpu().numpy()


@pytest.mark.parametrize("name", sorted(APPLY_FIXTURES))
def test_csr_apply_equals_the_model_off_the_grid(name):
    import iterative_solvers_amd as isa
    csr = APPLY_FIXTURES[name]()
    n = len(csr[0]) - 1
    x = model.ragged_x() if name == "ragged" else np.random.default_rng(5).uniform(-1, 1, n)
    ref = model.apply(*csr, x)
    A = isa.CrsMatrix(*csr)
    assert A.numRows() == n
    y = A.apply(x)
    assert _same_bits(y, ref)
    assert _same_bits(_apply_into_nan(A, x), ref)
    empty_rows = np.diff(csr[0]) == 0
    assert not y[empty_rows].any() and not np.signbit(y[empty_rows]).any()     # +0.0, written
    if name == "ragged":                                                        # entry order, not column order
        assert tuple(y[list(model.CANCEL_ROWS)]) == model.CANCEL_Y_ENTRY_ORDER != model.CANCEL_Y_COLUMN_ORDER
    if name == "empty":
        assert empty_rows.all() and len(csr[1]) == 0
    # a second vector on the same handle: nothing of the first apply is left behind
    x2 = np.random.default_rng(6).uniform(-1, 1, n)
    assert _same_bits(A.apply(x2), model.apply(*csr, x2))


def test_csr_library_rejects_what_only_it_can_see():
    """Arrays of consistent lengths pass the wrapper's checks (tests/test_csr_reference_cpu.py); offsets that are not monotone or do
    not start at 0, columns out of range and a matrix without rows are the library's to refuse, before it creates anything."""
    import iterative_solvers_amd as isa
    for bad, what in ((([0, 2, 1], [0], [1.0]), "monotone"),
                      (([1, 1], [0], [1.0]), r"row_map\[0\]"),
                      (([0, 1, 2], [0, 2], [1.0, 1.0]), "out of range"),
                      (([0, 1, 2], [0, -1], [1.0, 1.0]), "out of range"),
                      (([0], [], []), "bad CSR arguments")):
        with pytest.raises(ValueError, match=what):
            isa.CrsMatrix(*bad)


def test_csr_create_takes_null_arrays_only_when_there_is_no_entry():
    """The C entry point itself: a caller's empty std::vector may hand over null for entries and values."""
    from iterative_solvers_amd import _capi
    L = _capi.load()
    create = C.CFUNCTYPE(C.c_int, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_void_p))(("mi355cg_create_csr", L))
    h = C.c_void_p()
    row_map = np.array([0, 1, 1], dtype=np.int32)
    assert create(2, row_map.ctypes.data, None, None, 0, C.byref(h)) == _capi.ERR_INVALID and not h
    row_map = np.zeros(301, dtype=np.int32)
    assert create(300, row_map.ctypes.data, None, None, 0, C.byref(h)) == _capi.OK and h
    try:
        y = np.full(300, np.nan)
        _capi.check(L.mi355cg_apply(h, np.random.default_rng(5).uniform(-1, 1, 300), y))
        assert not y.any() and not np.signbit(y).any()
    finally:
        L.mi355cg_destroy(h)


# ---- CG on matrices that are not the grid's -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    """(csr, b, u, the model's relative-rule run, the model's MSG run), both with high-precision inner products; computed once."""
    build, b_seed, u_seed, eps, (eps_p, eps_r) = model.CG_CASES[name]
    csr = build()
    n = len(csr[0]) - 1
    b, u = model.rhs(n, b_seed), model.far_solution(n, u_seed)
    rel = model.cg_rel(*csr, b, eps=eps, max_iterations=10 ** 5, dots=model.HIGH)
    msg = model.cg_msg(*csr, b, u, eps_p, eps_r, -1.0, 10000, dots=model.HIGH)
    for v in (b, u, rel.x, msg.x) + tuple(csr):
        v.setflags(write=False)
    return csr, b, u, rel, msg


def _msg_solver(isa, A, b, name):
    eps_p, eps_r = model.CG_CASES[name][4]
    m = isa.MSGSolver(A, b, 1e-6, 10000)
    m.setPrecisionEps(eps_p)
    m.setResidualEps(eps_r)
    m.setExactErrorEps(-1.0)
    return m


@pytest.mark.parametrize("name", sorted(model.CG_CASES))
def test_csr_cg_matches_the_model_off_the_grid(name):
    import iterative_solvers_amd as isa
    csr, b, u, ref, refm = _case(name)
    eps = model.CG_CASES[name][3]
    A = isa.CrsMatrix(*csr)
    sol = isa.MatrixFreeSolver(A, b, eps, 10 ** 5)
    x = sol.solve()
    print(f"{name} REL_2NORM: iterations {sol.getIterations()} (model {ref.iterations}), max|x - ref| / max|ref| "
          f"{np.abs(x - ref.x).max() / np.abs(ref.x).max():.2e}, true residual / eps {model.true_residual_rel(*csr, b, x) / eps:.6f}")
    assert (sol.getIterations(), bool(sol.last_results.converged)) == (ref.iterations, ref.converged)
    assert np.abs(x - ref.x).max() <= 1e-9 * np.abs(ref.x).max()
    assert abs(sol.last_results.r_norm2 - ref.r_norm) / ref.initial_r_norm <= 1e-12
    assert model.true_residual_rel(*csr, b, x) <= eps * (1 + 1e-3)             # the residual of the x that came back, not the loop's

    m = _msg_solver(isa, A, b, name)
    got = []
    m.setIterationCallback(lambda *a: got.append(a))
    xm = m.solve(u)
    print(f"{name} MSG: iterations {m.getIterations()} (model {refm.iterations}), stop {int(m.getStopReason())}, max|x - ref| / max|ref| "
          f"{np.abs(xm - refm.x).max() / np.abs(refm.x).max():.2e}, final error norm {m.getFinalErrorNorm()!r} (model {refm.final_error_norm!r})")
    assert (m.getIterations(), int(m.getStopReason()), m.hasConverged()) == (refm.iterations, refm.stop_reason, refm.converged)
    assert [g[0] for g in got] == [c[0] for c in refm.callbacks]
    assert np.abs(xm - refm.x).max() <= 1e-9 * np.abs(refm.x).max()
    assert abs(m.last_results.r_norm2 - refm.r_norm2) / refm.initial_r_norm2 <= 1e-12
    assert m.getFinalErrorNorm() == pytest.approx(refm.final_error_norm, rel=1e-9)
    if refm.stop_reason == model.STOP_RESIDUAL:                                 # max|b - A x| of the x that came back
        r_true = b.astype(model.LD) - model.apply(*csr, xm, dtype=model.LD)
        assert float(np.abs(r_true).max()) <= model.CG_CASES[name][4][1] * (1 + 1e-3)


# ---- one handle, many calls (S1) ---------------------------------------------------------------------------------------------------------
def test_csr_handle_reuse_gives_the_bits_of_fresh_handles():
    import iterative_solvers_amd as isa
    csr, b1, u, ref, refm = _case("S1")
    b2 = model.rhs(model.S1_N, 45)
    v = model.rhs(model.S1_N, 46)

    def fresh(b):
        s = isa.MatrixFreeSolver(isa.CrsMatrix(*csr), b, 1e-8, 10 ** 5)
        return s.solve(), s.getIterations()
    A = isa.CrsMatrix(*csr)
    s1 = isa.MatrixFreeSolver(A, b1, 1e-8, 10 ** 5)
    x1 = s1.solve()
    assert _same_bits(A.apply(v), model.apply(*csr, v))
    s2 = isa.MatrixFreeSolver(A, b2, 1e-8, 10 ** 5)
    x2 = s2.solve()
    f1, f2 = fresh(b1), fresh(b2)
    assert s1.getIterations() == f1[1] == ref.iterations and np.array_equal(x1, f1[0])
    assert s2.getIterations() == f2[1] and np.array_equal(x2, f2[0])
    assert not np.array_equal(x1, x2)
    # an MSG solve with a true solution and then a relative-rule solve again: the first x comes back
    _msg_solver(isa, A, b2, "S1").solve(u)
    assert np.array_equal(isa.MatrixFreeSolver(A, b1, 1e-8, 10 ** 5).solve(), x1)


def test_csr_sync_every_does_not_change_the_solve():
    import iterative_solvers_amd as isa
    csr, b, u, ref, refm = _case("S1")
    A = isa.CrsMatrix(*csr)
    runs = []
    for sync_every in (0, 1, 7):                                                # 0: the default, 200 -- the whole solve in one chunk
        s = isa.MatrixFreeSolver(A, b, 1e-8, 10 ** 5)
        runs.append((s.solve(sync_every=sync_every), s.getIterations(), s.last_results.r_norm2))
    assert ref.iterations < 200 and ref.iterations % 7 != 0                     # 7 ends inside a chunk, 1 polls every iteration
    for x, its, rn in runs:
        assert its == ref.iterations and rn == runs[0][2] and np.array_equal(x, runs[0][0])


def test_csr_apply_from_a_callback_in_mid_solve():
    import iterative_solvers_amd as isa
    csr, b, u, ref, refm = _case("S1")
    v = model.rhs(model.S1_N, 46)
    want = model.apply(*csr, v)
    A = isa.CrsMatrix(*csr)
    quiet = _msg_solver(isa, A, b, "S1")
    x_quiet = quiet.solve(u, callback_every=10)
    seen = []
    m = _msg_solver(isa, A, b, "S1")
    m.setIterationCallback(lambda it, *norms: seen.append((it, A.apply(v))))
    x = m.solve(u, callback_every=10)
    its = [it for it, _ in seen]
    assert its == [0, 1] + list(range(10, refm.iterations, 10)) + [refm.iterations] and len(its) > 4
    assert all(_same_bits(y, want) for _, y in seen)
    assert np.array_equal(x, x_quiet)
    assert (m.getIterations(), int(m.getStopReason()), m.getFinalErrorNorm(), m.getFinalPrecision(), m.getFinalResidualNorm()) == \
        (quiet.getIterations(), int(quiet.getStopReason()), quiet.getFinalErrorNorm(), quiet.getFinalPrecision(), quiet.getFinalResidualNorm())
    assert m.getIterations() == refm.iterations
