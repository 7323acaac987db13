"""Pins tests/csr_reference.py, the model tests/test_gpu_csr.py compares the generic CSR path with, and the conditions that keep
that comparison meaningful; and the argument checks of CrsMatrix, which need neither a GPU nor the library.  No GPU."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csr_reference as model  # noqa: E402

SMALL = {
    "tiny_one": lambda: model.tiny(True),
    "tiny_none": lambda: model.tiny(False),
    "exact_chunk_255": lambda: model.exact_chunk(255),
    "exact_chunk_256": lambda: model.exact_chunk(256),
    "exact_chunk_257": lambda: model.exact_chunk(257),
    "boundary_between_rows": model.boundary_between_rows,
    "nine_point": model.nine_point,
    "ragged": model.ragged,
    "empty": model.empty,
    "S1": model.S1,
}


def _x_for(name, n):
    return model.ragged_x() if name == "ragged" else np.random.default_rng(5).uniform(-1, 1, n)


@pytest.mark.parametrize("name", sorted(SMALL))
def test_apply_equals_the_plain_double_loop(name):
    A = SMALL[name]()
    row_map, entries, values = A
    n = len(row_map) - 1
    assert row_map.dtype == np.int32 and entries.dtype == np.int32 and values.dtype == np.float64
    assert row_map[0] == 0 and row_map[-1] == len(entries) == len(values) and np.all(np.diff(row_map) >= 0)
    assert entries.size == 0 or (entries.min() >= 0 and entries.max() < n)
    x = _x_for(name, n)
    y = model.apply(*A, x)
    assert np.array_equal(y, model.apply_loop(*A, x))
    assert not np.signbit(y[np.diff(row_map) == 0]).any()                      # an empty row is +0.0
    B = SMALL[name]()
    assert all(np.array_equal(a, b) for a, b in zip(A, B))                     # seeded: the same matrix every time


def test_long_chain_apply_equals_the_plain_double_loop_at_both_ends_and_is_quick():
    import time
    A = model.long_chain(seed=24)
    row_map, entries, values = A
    n = model.LONG_CHAIN_N
    assert len(row_map) == n + 1 and set(np.diff(row_map).tolist()) == {2, 3} and n == 2048 * 256 + 257
    x = np.random.default_rng(5).uniform(-1, 1, n)
    t0 = time.process_time()
    y = model.apply(*A, x)
    assert time.process_time() - t0 < 1.0                                       # 5e5 rows well under a second
    for lo, hi in ((0, 600), (n - 600, n)):
        sub = (row_map[lo:hi + 1] - row_map[lo]), entries[row_map[lo]:row_map[hi]], values[row_map[lo]:row_map[hi]]
        assert np.array_equal(y[lo:hi], model.apply_loop(*sub, x))


def test_fixtures_have_the_shapes_the_kernel_paths_need():
    B, C = model.BLOCK, model.CHUNK
    for n in (255, 256, 257):
        assert model.exact_chunk(n)[0][min(n, B)] == min(n, B) * 8 and B * 8 == C
    rm = model.boundary_between_rows()[0]
    assert rm[B] == 2 * C and C in rm[:B].tolist()                             # a chunk ends exactly at a row end
    rm = model.nine_point()[0]
    assert rm[227] < C < rm[228] and len(rm) - 1 == 777                        # the boundary falls inside row 227
    assert not np.all(np.diff(model.nine_point()[1][:9]) > 0)                  # unsorted columns
    rm, en, va = model.ragged()
    ln = np.diff(rm)
    assert len(ln) == 1029 and 1029 % B == 5
    assert not ln[256:512].any() and rm[256] == rm[512]                        # an empty block
    assert (ln[:256] == 0).any() and ln[600] == 5000 > C and ln[600] > len(ln)
    assert len(set(en[rm[600]:rm[601]].tolist())) < 5000                      # duplicate columns
    assert set(ln.tolist()) - {5000} <= {0, 1, 2, 3, 5, 8, 13, 40} and (ln == 40).any()
    rm, en, va = model.S1()
    ln = np.diff(rm)
    assert len(ln) == 3001 and ln[model.S1_HUB] == 3001 and np.delete(ln, model.S1_HUB).max() <= 13
    assert np.delete(ln, model.S1_HUB).min() == 2                              # a row with the hub and itself alone
    assert 2800 <= len(en) / (3001 / B) <= 3000                                # about 2900 products per block
    D = np.zeros((3001, 3001))
    np.add.at(D, (np.repeat(np.arange(3001), ln), en), va)
    off = np.abs(D).sum(axis=1) - np.abs(D.diagonal())
    assert np.array_equal(D, D.T) and (D.diagonal() - off).min() > 0.4         # symmetric, Gershgorin: positive definite
    assert not all(np.all(np.diff(en[rm[i]:rm[i + 1]]) > 0) for i in range(100))   # shuffled within rows
    rm, en, va = model.S2()
    assert np.all(va[rm[:-1]] >= 2.0) and np.all(np.delete(va, rm[:-1]) == -1.0)   # strictly diagonally dominant


@pytest.mark.parametrize("N", [6, 16, 64])
def test_apply_on_the_grid_csr_equals_the_oracle(N):
    from oracle.oracle import OracleGrid
    og = OracleGrid(N, N)
    x = np.random.default_rng(5).uniform(-1, 1, og.size)
    assert np.array_equal(model.apply(*og.csr(), x), og.apply(x))


@pytest.mark.parametrize("N", [16, 64])
def test_cg_with_serial_dots_reproduces_the_oracle_on_the_grid_csr(N):
    from oracle.oracle import OracleGrid
    og = OracleGrid(N, N)
    A, b, u = og.csr(), og.rhs(), og.true_solution()
    for diagnostics in (False, True):
        ref = og.mf_solve(eps=1e-8, max_iterations=10 ** 5, diagnostics=diagnostics)
        got = model.cg_rel(*A, b, u, eps=1e-8, max_iterations=10 ** 5, diagnostics=diagnostics)
        assert np.array_equal(got.x, ref.x)
        assert (got.iterations, got.converged, got.r_norm, got.initial_r_norm) == \
            (ref.iterations, ref.converged, ref.r_norm, ref.initial_r_norm)
        assert got.callbacks == ref.callbacks and bool(got.callbacks) == diagnostics
    capped = model.cg_rel(*A, b, eps=1e-8, max_iterations=7)
    ref = og.mf_solve(eps=1e-8, max_iterations=7)
    assert (capped.iterations, capped.converged) == (7, False) == (ref.iterations, ref.converged) and np.array_equal(capped.x, ref.x)
    # every stop reason of the MSG loop: precision, residual, exact error, the iteration cap; with and without a true solution
    e_final = og.msg_solve(eps_precision=1e-9, eps_residual=1e-9).final_error_norm
    reasons = set()
    for kw in (dict(eps_precision=1e-9, eps_residual=1e-9, eps_exact_error=-1.0),
               dict(eps_precision=-1.0, eps_residual=1e-6, eps_exact_error=-1.0),
               dict(eps_precision=-1.0, eps_residual=-1.0, eps_exact_error=2 * e_final),
               dict(eps_precision=1e-9, eps_residual=1e-9, eps_exact_error=-1.0, true_solution=None),
               dict(eps_precision=1e-30, eps_residual=1e-30, eps_exact_error=-1.0, max_iterations=5)):
        ref = og.msg_solve(**kw)
        kw.setdefault("true_solution", u)
        got = model.cg_msg(*A, b, **kw)
        assert np.array_equal(got.x, ref.x) and np.array_equal(got.r, ref.r)
        for f in ("iterations", "converged", "stop_reason", "final_residual_norm", "final_precision", "final_error_norm",
                  "r_norm2", "initial_r_norm2", "callbacks"):
            assert getattr(got, f) == getattr(ref, f), f
        reasons.add(got.stop_reason)
    assert reasons == {model.STOP_PRECISION, model.STOP_RESIDUAL, model.STOP_EXACT_ERROR, model.STOP_ITERATIONS}
    stopped = model.cg_msg(*A, b, u, stop_flag=[1])
    assert (stopped.iterations, stopped.converged, stopped.stop_reason) == (0, False, model.STOP_INTERRUPTED)


def test_the_model_tells_entry_order_from_column_order():
    A, x = model.ragged(), model.ragged_x()
    row_map, entries, values = A
    y = model.apply(*A, x)
    rows = list(model.CANCEL_ROWS)
    assert tuple(y[rows]) == model.CANCEL_Y_ENTRY_ORDER
    by_column = model.apply_loop(*A, x, order=model.column_sorted(entries))
    assert tuple(by_column[rows]) == model.CANCEL_Y_COLUMN_ORDER and model.CANCEL_Y_COLUMN_ORDER != model.CANCEL_Y_ENTRY_ORDER
    # the same matrix with every row's entries sorted by column is another input to the model, and gives another y
    order = np.lexsort((entries, np.repeat(np.arange(len(row_map) - 1), np.diff(row_map))))
    assert np.array_equal(model.apply(row_map, entries[order], values[order], x), by_column)


def test_high_and_exact_dots():
    rng = np.random.default_rng(3)
    a = rng.uniform(-1, 1, 4001) * 10.0 ** rng.integers(-8, 8, 4001)
    b = rng.uniform(-1, 1, 4001)
    from fractions import Fraction
    exact = sum(Fraction(float(p)) * Fraction(float(q)) for p, q in zip(a, b))
    assert model._dot_exact(a, b) == float(exact)                               # exactly rounded
    assert abs(Fraction(model._dot_high(a, b)) - exact) <= abs(exact) * Fraction(2, 2 ** 53)
    c = np.array([1e16, 1.0, -1e16])
    assert (model._dot_serial(c, np.ones(3)), model._dot_high(c, np.ones(3)), model._dot_exact(c, np.ones(3))) == (0.0, 1.0, 1.0)


# ---- the CG cases of the GPU test ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(name):
    build, b_seed, u_seed, eps, (eps_p, eps_r) = model.CG_CASES[name]
    A = build()
    n = len(A[0]) - 1
    b, u = model.rhs(n, b_seed), model.far_solution(n, u_seed)
    runs = {}
    for dots in (model.SERIAL, model.HIGH):
        runs["rel", dots] = model.cg_rel(*A, b, eps=eps, max_iterations=10 ** 5, dots=dots)
        runs["msg", dots] = model.cg_msg(*A, b, u, eps_p, eps_r, -1.0, 10000, dots=dots)
    return A, b, u, runs


@pytest.mark.parametrize("rule", ["rel", "msg"])
@pytest.mark.parametrize("name", sorted(model.CG_CASES))
def test_cg_cases_meet_the_conditions_of_the_gpu_test(name, rule):
    """What makes the GPU test's equalities meaningful: the count, the stop reason and x do not hang on how the inner products
    are summed, and no stop decision of the last two iterations is a close call."""
    A, b, u, runs = _case(name)
    eps = model.CG_CASES[name][3]
    serial, high = runs[rule, model.SERIAL], runs[rule, model.HIGH]
    gap = np.abs(serial.x - high.x).max() / np.abs(high.x).max()
    print(f"{name} {rule}: iterations {serial.iterations} / {high.iterations}, last two ratios {serial.ratios[-2:]} / "
          f"{high.ratios[-2:]}, gap {gap:.2e}, stop {getattr(high, 'stop_reason', None)}")
    assert serial.iterations == high.iterations and serial.converged and high.converged
    assert serial.iterations < 200                                              # the default sync_every: one chunk, so 1 and 7 split it
    if rule == "msg":
        assert serial.stop_reason == high.stop_reason != model.STOP_ITERATIONS
        assert [c[0] for c in serial.callbacks] == [c[0] for c in high.callbacks] == [0, 1, high.iterations]
        assert high.final_error_norm >= np.abs(high.x).max()                    # rel=1e-9 on it asks no more than 1e-9 max|x| on x
    for run in (serial, high):
        for ratios in run.ratios[-2:]:
            assert all(abs(q - 1.0) >= 0.05 for q in np.atleast_1d(ratios))
    assert gap <= 1e-10                                                         # a tenth of the GPU tolerance
    if rule == "rel":                                                           # the reference's own x meets the true-residual bound
        for run in (serial, high):
            assert model.true_residual_rel(*A, b, run.x) <= eps * (1 + 1e-3)


def test_msg_cases_stop_on_different_criteria():
    assert {_case(n)[3]["msg", model.HIGH].stop_reason for n in model.CG_CASES} == {model.STOP_PRECISION, model.STOP_RESIDUAL}


def test_long_double_dots_stand_in_for_exactly_rounded_ones_on_S1():
    A, b, u, runs = _case("S1")
    eps, (eps_p, eps_r) = model.CG_CASES["S1"][3:]
    for high, exact in ((runs["rel", model.HIGH], model.cg_rel(*A, b, eps=eps, max_iterations=10 ** 5, dots=model.EXACT)),
                        (runs["msg", model.HIGH], model.cg_msg(*A, b, u, eps_p, eps_r, -1.0, 10000, dots=model.EXACT))):
        assert high.iterations == exact.iterations
        assert np.abs(high.x - exact.x).max() <= 1e-13 * np.abs(exact.x).max()


# ---- CrsMatrix argument checks: ValueError before the library is touched ---------------------------------------------------------------
BIG = 2 ** 31
MALFORMED = {
    "entries_short": ([0, 2, 3], [0, 1], [1.0, 1.0, 1.0]),
    "entries_long": ([0, 1, 2], [0, 1, 1], [1.0, 1.0]),
    "values_short": ([0, 2, 3], [0, 1, 1], [1.0, 1.0]),
    "values_long": ([0, 1, 2], [0, 1], [1.0, 1.0, 1.0]),
    "row_map_empty": ([], [], []),
    "row_map_empty_int": (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0)),
    "row_map_2d": ([[0, 1], [1, 2]], [0, 1], [1.0, 1.0]),
    "row_map_scalar": (0, [], []),
    "entries_2d": ([0, 2], [[0], [0]], [1.0, 1.0]),
    "offset_past_int32": (np.array([0, BIG + 1], dtype=np.int64), [0], [1.0]),      # wraps to [0, -2^31 + 1] under a cast
    "offset_wraps_to_nnz": (np.array([0, 2 ** 32 + 1], dtype=np.int64), [0], [1.0]),  # wraps to [0, 1]: would look well-formed
    "offset_negative_64": (np.array([0, -BIG - 1, 1], dtype=np.int64), [0], [1.0]),
    "column_past_int32": ([0, 1], np.array([2 ** 32], dtype=np.int64), [1.0]),     # wraps to column 0
    "column_uint32": ([0, 1], np.array([BIG], dtype=np.uint32), [1.0]),
    "row_map_float": (np.array([0.0, 1.0]), [0], [1.0]),
    "row_map_bool": (np.array([False, True]), [0], [1.0]),
    "entries_float": ([0, 1], np.array([0.0]), [1.0]),
    "entries_str": ([0, 1], ["0"], [1.0]),
    "values_str": ([0, 1], [0], ["one"]),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_crs_matrix_rejects_malformed_input_before_the_library_is_called(name, monkeypatch):
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi

    def no_library():
        raise AssertionError("the library was reached with malformed CSR arrays")
    monkeypatch.setattr(_capi, "load", no_library)                              # no library: no handle can have been created
    with pytest.raises(ValueError):
        isa.CrsMatrix(*MALFORMED[name])


def test_crs_matrix_passes_well_formed_input_on_as_int32(monkeypatch):
    """The other side of the checks: lists, 64-bit and unsigned offsets that fit, and an empty matrix reach the library, once,
    as contiguous int32 / float64 arrays of the checked lengths."""
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    calls = []

    class Lib:
        def mi355cg_create_csr(self, nrows, row_map, entries, values, device, out):
            calls.append((nrows, row_map, entries, values))
            return _capi.ERR_INVALID                                            # stop here: this test has no GPU

        def mi355cg_last_error(self):
            return b"stub"
    monkeypatch.setattr(_capi, "load", lambda: Lib())
    good = [([0, 2, 3], [1, 0, 1], [1.0, 2.0, 3.0]),
            (np.array([0, 1, 1], dtype=np.uint64), np.array([1], dtype=np.int64), np.array([2], dtype=np.int32)),
            ([0, 0, 0], [], []),
            model.ragged()]
    for args in good:
        with pytest.raises(ValueError, match="stub"):
            isa.CrsMatrix(*args)
        nrows, row_map, entries, values = calls.pop()
        assert not calls and nrows == len(args[0]) - 1
        assert (row_map.dtype, entries.dtype, values.dtype) == (np.int32, np.int32, np.float64)
        assert all(a.flags.c_contiguous and a.ndim == 1 for a in (row_map, entries, values))
        assert len(entries) == len(values) == row_map[-1]
        assert np.array_equal(row_map, np.asarray(args[0])) and np.array_equal(entries, np.asarray(args[1], dtype=np.int64))
