"""The NumPy model the generic-CSR tests compare against: the kernel's stated
contract for y = A x, the two CG loops of oracle/cg_oracle.c with the operator replaced by that apply, and the seeded matrices the
tests run on.  A plain module: no test in here, nothing that needs a GPU, the package or the oracle binaries.

apply()     y[i] = sum of values[j] * x[entries[j]] for j ascending from row_map[i], from +0.0, one rounded multiply and one
            rounded add per entry (NumPy never contracts a product and a sum into an FMA): the serial CSR loop.
cg_rel()    og_mf_solve line by line (MatrixFreeSolver::solve, relative 2-norm rule).
cg_msg()    og_msg_solve line by line (MSGSolver::solve, absolute max-norm rules).
dots        SERIAL is og_dot, the ascending sum of rounded products.  HIGH carries products and sums in np.longdouble (64-bit
            significand: every product is within 2^-64 and the pairwise sum of n terms within about 2^-64 log2 n of exact, 1e-18
            relative for the squared norms at n = 5e5) and rounds once; it stands in for the library's double-double reductions.
            EXACT is the exactly rounded inner product (error-free split products through math.fsum), too slow for the 5e5-row
            chain and kept to show on S1 that HIGH is an adequate stand-in.

Measured with this module (tests/test_csr_reference_cpu.py asserts the conditions, not the figures).  "ratios" are the deciding
quantity over its threshold in the last two iterations -- ||r|| / (eps ||r0||) under the relative rule, max|r| / eps_residual and
max|dx| / eps_precision under MSG; the run goes on while a ratio is above 1.  "gap" is max|x_SERIAL - x_HIGH| / max|x_HIGH|.

  case  rule                                        iterations       last two ratios                          gap
                                                    (SERIAL = HIGH)
  S1    relative, eps 1e-8                          53               1.074, 0.748                             2.4e-16
  S1    MSG, eps_precision 1e-9, eps_residual 1e-9  61, PRECISION    max|dx| 1.23, 0.83; max|r| 2.11, 1.62    3.7e-16
  S2    relative, eps 1e-8                          30               1.408, 0.715                             8.0e-16
  S2    MSG, eps_precision 1e-9, eps_residual 1e-8  34, RESIDUAL     max|dx| 200, 73; max|r| 5.34, 0.226      8.0e-16

The ratios of the SERIAL and HIGH runs agree to 12 digits.  On S1, HIGH and EXACT give the same x bit for bit under the relative rule.
The true residual ||b - A x|| / (eps ||b||) of the model's x in long double: 0.748 (S1), 0.715 (S2).  (S1 at eps_precision =
eps_residual = 1e-8 would not qualify: max|dx| / eps is 1.023 in the last iteration but one.)
"""
import math
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
SERIAL, HIGH, EXACT = "serial", "high", "exact"
# StopCriterion / OG_STOP_*
STOP_ITERATIONS, STOP_PRECISION, STOP_RESIDUAL, STOP_EXACT_ERROR, STOP_INTERRUPTED = range(5)
DBL_MAX = float(np.finfo(np.float64).max)
BLOCK, CHUNK = 256, 2048               # rows per workgroup and products per LDS chunk of k_csr_spmv (csrc/csr_kernels.h)


# ---- y = A x ---------------------------------------------------------------------------------------------------------------------
def plan(row_map, entries, values):
    """What apply() needs of a matrix, worked out once: for step k the rows that have an entry k, with those entries' columns
    and values (rows=None: every row has one); and the few long rows that are left once at most 8 are, each with the rest of its
    entries."""
    rm = np.asarray(row_map, dtype=np.int64)
    entries = np.asarray(entries, dtype=np.int64)
    values = np.asarray(values, dtype=np.float64)
    n = len(rm) - 1
    start, length = rm[:-1], np.diff(rm)
    steps, act, k = [], np.flatnonzero(length > 0), 0
    while act.size > 8:
        j = start[act] + k
        steps.append((None if act.size == n else act, entries[j], values[j]))
        k += 1
        act = act[length[act] > k]
    tails = [(i, entries[start[i] + k:rm[i + 1]], values[start[i] + k:rm[i + 1]]) for i in act]
    return SimpleNamespace(n=n, steps=steps, tails=tails)


def apply_plan(pl, x, dtype=np.float64):
    x = np.asarray(x, dtype=np.float64).astype(dtype, copy=False)
    y = np.zeros(pl.n, dtype=dtype)                                # +0.0
    for rows, cols, vals in pl.steps:
        if rows is None:
            y = y + vals * x[cols]
        else:
            y[rows] = y[rows] + vals * x[cols]
    for i, cols, vals in pl.tails:
        y[i] = np.cumsum(np.concatenate((y[i:i + 1], vals * x[cols])))[-1]
    return y


def apply(row_map, entries, values, x, dtype=np.float64):
    """The serial CSR loop, column by column over the rows still active: step k adds entry k of every row that has one.  Once
    only a few (long) rows are left, each is finished with np.cumsum, which adds serially.  dtype=np.longdouble carries products
    and sums in long double instead (the checker of a true residual, not a model of the kernel)."""
    return apply_plan(plan(row_map, entries, values), x, dtype)


def apply_loop(row_map, entries, values, x, order=None):
    """The plain double loop in Python floats (IEEE doubles, no FMA).  order: a permutation of each row's entries applied before
    summing, e.g. sorted_order(), for the tests that must tell entry order from another order."""
    n = len(row_map) - 1
    y = np.zeros(n)
    for i in range(n):
        s = 0.0
        js = range(int(row_map[i]), int(row_map[i + 1]))
        for j in (js if order is None else order(i, js)):
            s += float(values[j]) * float(x[entries[j]])
        y[i] = s
    return y


def column_sorted(entries):
    """order= for apply_loop: each row's entries by ascending column (stable)."""
    return lambda i, js: sorted(js, key=lambda j: int(entries[j]))


def true_residual_rel(row_map, entries, values, b, x):
    """||b - A x||_2 / ||b||_2 with A x, the difference and both norms in long double."""
    r = np.asarray(b, dtype=np.float64).astype(LD) - apply(row_map, entries, values, x, dtype=LD)
    b = np.asarray(b, dtype=np.float64).astype(LD)
    return float(np.sqrt(np.sum(r * r)) / np.sqrt(np.sum(b * b)))


# ---- inner products --------------------------------------------------------------------------------------------------------------
def _dot_serial(a, b):
    return float(np.cumsum(a * b)[-1] + 0.0) if a.size else 0.0   # og_dot: result = 0.0; result += a[i] * b[i]


def _dot_high(a, b):
    assert np.finfo(LD).nmant >= 63, "np.longdouble is no wider than double here: use dots=EXACT"
    return float(np.sum(a.astype(LD) * b.astype(LD)))


def _two_product(a, b):
    """a * b = p + e exactly (Dekker, with Veltkamp's split; no overflow or underflow at the tests' magnitudes)."""
    p = a * b
    ta, tb = a * 134217729.0, b * 134217729.0
    ah, bh = ta - (ta - a), tb - (tb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _dot_exact(a, b):
    p, e = _two_product(a, b)
    return math.fsum(p.tolist() + e.tolist())


_DOTS = {SERIAL: _dot_serial, HIGH: _dot_high, EXACT: _dot_exact}


def _max_norm(a):
    return float(np.max(np.abs(a), initial=0.0))                   # og_max_norm


# ---- MatrixFreeSolver::solve (og_mf_solve) -----------------------------------------------------------------------------------------
def cg_rel(row_map, entries, values, b, true_solution=None, eps=1e-6, max_iterations=10000, diagnostics=False, dots=SERIAL):
    """og_mf_solve with og_apply replaced by apply().  Returns a namespace with the fields of oracle.MfResult (x, iterations,
    converged, r_norm, initial_r_norm, callbacks) and `ratios`: ||r|| / (eps ||r0||) after every iteration, the quantity the loop
    condition compares with 1."""
    dot = _DOTS[dots]
    norm = lambda v: math.sqrt(dot(v, v))
    pl = plan(row_map, entries, values)
    A = lambda v: apply_plan(pl, v)
    b = np.ascontiguousarray(b, dtype=np.float64)
    callbacks, ratios = [], []
    x = np.zeros_like(b)
    Ax = A(x)
    r = 1.0 * b + -1.0 * Ax
    p = r.copy()
    r_norm = norm(r)
    initial_r_norm = r_norm
    iterations = 0
    while iterations < max_iterations and r_norm > eps * initial_r_norm:
        prev_x = x.copy()
        Ap = A(p)
        p_dot_Ap = dot(p, Ap)
        r_dot_r = dot(r, r)
        alpha = r_dot_r / p_dot_Ap
        x = x + alpha * p
        r = r - alpha * Ap
        new_r_dot_r = dot(r, r)
        beta = new_r_dot_r / r_dot_r
        p = r + beta * p
        r_norm = math.sqrt(new_r_dot_r)
        ratios.append(r_norm / (eps * initial_r_norm))
        if diagnostics:
            precision = norm(x - prev_x)
            error_norm = norm(x - true_solution)
            residual_norm = norm(b - A(x))
            callbacks.append((iterations, precision, residual_norm, error_norm))
        iterations += 1
    return SimpleNamespace(x=x, iterations=iterations, converged=r_norm <= eps * initial_r_norm, r_norm=r_norm,
                           initial_r_norm=initial_r_norm, callbacks=callbacks, ratios=ratios)


# ---- MSGSolver::solve (og_msg_solve) -------------------------------------------------------------------------------------------------
def cg_msg(row_map, entries, values, b, true_solution=None, eps_precision=1e-6, eps_residual=1e-6, eps_exact_error=-1.0,
           max_iterations=10000, stop_flag=None, dots=SERIAL):
    """og_msg_solve with og_apply replaced by apply().  stop_flag: a one-element list, read at the top of every iteration.  Returns
    a namespace with the fields of oracle.MsgResult and `ratios`: per iteration, the quantity over its eps of every criterion
    that is switched on, in the order the loop tests them (each stops the loop once below 1)."""
    dot = _DOTS[dots]
    norm = lambda v: math.sqrt(dot(v, v))
    pl = plan(row_map, entries, values)
    b = np.ascontiguousarray(b, dtype=np.float64)
    u = None if true_solution is None else np.ascontiguousarray(true_solution, dtype=np.float64)
    callbacks, ratios = [], []
    converged = False
    x = np.zeros_like(b)
    r = b.copy()
    z = r.copy()
    r_norm = norm(r)
    r_max_norm = _max_norm(r)
    initial_r_norm = r_norm
    it = 0
    stop_reason = STOP_ITERATIONS
    precision_max_norm = DBL_MAX
    error_max_norm = DBL_MAX
    if u is not None:
        error_max_norm = _max_norm(x - u)
    callbacks.append((0, precision_max_norm, r_max_norm, error_max_norm))
    while it < max_iterations:
        if stop_flag is not None and stop_flag[0]:
            stop_reason = STOP_INTERRUPTED
            converged = False
            break
        x_prev = x.copy()
        A_z = apply_plan(pl, z)
        rz = dot(r, z)
        Az_z = dot(A_z, z)
        alpha = rz / Az_z
        x = x + alpha * z
        r = r - alpha * A_z
        it += 1
        r_norm = norm(r)
        r_max_norm = _max_norm(r)
        precision_max_norm = _max_norm(x - x_prev)
        if u is not None:
            error_max_norm = _max_norm(x - u)
        ratios.append([q / e for q, e, on in ((precision_max_norm, eps_precision, True), (r_max_norm, eps_residual, True),
                                              (error_max_norm, eps_exact_error, u is not None)) if on and e > 0])
        if eps_precision > 0 and precision_max_norm < eps_precision:
            converged, stop_reason = True, STOP_PRECISION
            break
        if eps_residual > 0 and r_max_norm < eps_residual:
            converged, stop_reason = True, STOP_RESIDUAL
            break
        if eps_exact_error > 0 and u is not None and error_max_norm < eps_exact_error:
            converged, stop_reason = True, STOP_EXACT_ERROR
            break
        beta = (r_norm * r_norm) / rz
        z = r + beta * z
        if it % 100 == 0 or it == 1:
            callbacks.append((it, precision_max_norm, r_max_norm, error_max_norm))
    callbacks.append((it, precision_max_norm, r_max_norm, error_max_norm))
    return SimpleNamespace(x=x, r=r, iterations=it, converged=converged, stop_reason=stop_reason,
                           final_residual_norm=r_max_norm, final_precision=precision_max_norm, final_error_norm=error_max_norm,
                           r_norm2=r_norm, initial_r_norm2=initial_r_norm, callbacks=callbacks, ratios=ratios)


# ---- fixtures: seeded, deterministic, (row_map int32, entries int32, values float64) ---------------------------------------------
def _csr(lengths, entries, values):
    row_map = np.zeros(len(lengths) + 1, dtype=np.int32)
    np.cumsum(lengths, out=row_map[1:])
    return row_map, np.asarray(entries, dtype=np.int32), np.asarray(values, dtype=np.float64)


def tiny(with_entry):
    """n = 1: one entry, or none."""
    return _csr([1], [0], [-1.75]) if with_entry else _csr([0], [], [])


def uniform_rows(n, per_row, seed):
    """per_row entries in every row, random columns (unsorted, repeats allowed), values in (-1, 1)."""
    rng = np.random.default_rng(seed)
    return _csr([per_row] * n, rng.integers(0, n, n * per_row), rng.uniform(-1, 1, n * per_row))


def exact_chunk(n):
    """8 entries per row: a full block holds BLOCK * 8 = CHUNK products, so its only chunk ends exactly at the block's end."""
    return uniform_rows(n, 8, 100 + n)


def boundary_between_rows():
    """n = 512, 16 entries per row: each block has two chunks and the first ends exactly at the end of row 127."""
    return uniform_rows(512, 16, 21)


def nine_point():
    """n = 777, 9 entries per row: the first chunk of a full block ends inside its row 227 (entries 2043..2051)."""
    return uniform_rows(777, 9, 22)


RAGGED_N, RAGGED_LONG_ROW, RAGGED_LONG_LEN = 1029, 600, 5000
RAGGED_EMPTY_ROWS = range(256, 512)                     # all of block 1
CANCEL_ROWS, CANCEL_COLS = (700, 701), (11, 13, 12)     # entry order visits column 11, 13, 12; x is 1 there (ragged_x)
CANCEL_VALUES = ([1e16, 1.0, -1e16], [1e16, -1e16, 1.0])
CANCEL_Y_ENTRY_ORDER, CANCEL_Y_COLUMN_ORDER = (0.0, 1.0), (1.0, 0.0)     # 1e16 + 1 rounds to 1e16


def ragged(seed=23):
    """n = 1029 = 4 blocks + 5 rows, not symmetric.  Row lengths from {0, 0, 1, 2, 3, 5, 8, 13, 40}; block 1 has no entry at all;
    row 600 has 5000 entries (more than a chunk, more than n: columns repeat); rows 700 and 701 are the cancellation pair."""
    rng = np.random.default_rng(seed)
    n = RAGGED_N
    lengths = rng.choice([0, 0, 1, 2, 3, 5, 8, 13, 40], n)
    lengths[RAGGED_EMPTY_ROWS.start:RAGGED_EMPTY_ROWS.stop] = 0
    lengths[RAGGED_LONG_ROW] = RAGGED_LONG_LEN
    lengths[list(CANCEL_ROWS)] = 3
    row_map, entries, values = _csr(lengths, rng.integers(0, n, lengths.sum()), rng.uniform(-1, 1, lengths.sum()))
    for row, vals in zip(CANCEL_ROWS, CANCEL_VALUES):
        entries[row_map[row]:row_map[row + 1]] = CANCEL_COLS
        values[row_map[row]:row_map[row + 1]] = vals
    return row_map, entries, values


def ragged_x(seed=5):
    x = np.random.default_rng(seed).uniform(-1, 1, RAGGED_N)
    x[list(CANCEL_COLS)] = 1.0
    return x


def empty(n=300):
    return _csr([0] * n, [], [])


LONG_CHAIN_N = 2048 * BLOCK + 257      # one more than the 2048 row blocks a launch has, and a last block of one row


def long_chain(n=LONG_CHAIN_N, seed=None):
    """Tridiagonal, entries in the order (diagonal, left, right); rows 0 and n - 1 have two.  seed=None is S2: diagonal
    2.5 + 0.5 sin i, off-diagonals -1 (symmetric, strictly diagonally dominant: positive definite).  With a seed: values in
    (-1, 1), for apply alone."""
    i = np.arange(n)
    cols = np.stack((i, i - 1, i + 1), axis=1)
    keep = (cols >= 0) & (cols < n)
    if seed is None:
        vals = np.stack((2.5 + 0.5 * np.sin(i), np.full(n, -1.0), np.full(n, -1.0)), axis=1)
    else:
        vals = np.random.default_rng(seed).uniform(-1, 1, (n, 3))
    return _csr(keep.sum(axis=1), cols[keep], vals[keep])


S1_N, S1_HUB = 3001, 1500


def S1(seed=31):
    """n = 3001, symmetric positive definite: a weighted graph Laplacian plus a diagonal in (0.5, 1.5).  Random neighbours by
    paired stubs, 0 to 11 a row and mostly 8 to 11; the hub row 1500 is joined to every other row on top of that, so it has 3001
    entries in the middle of rows of at most 13.  Entries within a row are in shuffled order, the diagonal among them."""
    rng = np.random.default_rng(seed)
    n = S1_N
    want = rng.choice(12, n, p=[.02, .01, .01, .01, .01, .02, .04, .08, .15, .25, .25, .15])
    want[S1_HUB] = 0
    stubs = rng.permutation(np.repeat(np.arange(n), want))
    stubs = stubs[:stubs.size // 2 * 2].reshape(-1, 2)
    lo, hi = stubs.min(axis=1), stubs.max(axis=1)
    pairs = np.unique(np.stack((lo, hi), axis=1)[lo != hi], axis=0)          # no self-loops, no repeated edge
    others = np.delete(np.arange(n), S1_HUB)
    ei = np.concatenate((pairs[:, 0], np.full(n - 1, S1_HUB)))
    ej = np.concatenate((pairs[:, 1], others))
    w = np.concatenate((rng.uniform(0.5, 1.5, len(pairs)), rng.uniform(0.001, 0.003, n - 1)))
    diag = rng.uniform(0.5, 1.5, n)
    np.add.at(diag, ei, w)
    np.add.at(diag, ej, w)
    rows = np.concatenate((ei, ej, np.arange(n)))
    cols = np.concatenate((ej, ei, np.arange(n)))
    vals = np.concatenate((-w, -w, diag))
    shuffle = rng.permutation(rows.size)
    order = shuffle[np.argsort(rows[shuffle], kind="stable")]
    return _csr(np.bincount(rows, minlength=n), cols[order], vals[order])


def S2():
    return long_chain()


# ---- the two CG cases of the GPU test, with the parameters chosen so that the conditions of test_csr_reference_cpu hold ----------------
def rhs(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n)


def far_solution(n, seed):
    """The "true solution" handed to the MSG runs: a vector far from x (entries in (3, 5)), so that max|x - u| is of the size of
    u and the error norm is resolved as well as x is."""
    return np.random.default_rng(seed).uniform(3, 5, n)


CG_CASES = {
    # name: (builder, rhs seed, u seed, eps of the relative rule, (eps_precision, eps_residual) of the MSG rule)
    "S1": (S1, 41, 42, 1e-8, (1e-9, 1e-9)),          # MSG stops on PRECISION
    "S2": (S2, 43, 44, 1e-8, (1e-9, 1e-8)),          # MSG stops on RESIDUAL
}
