"""csrc/solve_loop.h without a GPU: tests/cpp/solve_loop_driver.cpp prints what the header decides for tables of parameters
(built with the sanitizers, run as a program of its own) and this file checks the lines against the rules restated here
(msg_solver.cpp:75-77, 144-163, 172-183, 187-195)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = 1.7976931348623157e308
MSG, REL2 = 0, 1
ITERATIONS, PRECISION, RESIDUAL, EXACT_ERROR, INTERRUPTED = range(5)
K_HIST = 512


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("solve_loop") / "solve_loop_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "solve_loop_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr
    return [ln.split() for ln in out.stdout.splitlines()]


def test_chunk_schedules(lines):
    rows = [ln for ln in lines if ln[0] == "chunks"]
    assert len(rows) == 2 * 6 * 5 * 7 * 2
    for ln in rows:
        rule, cap, every, sync, watched, se = map(int, ln[1:7])
        a, b = ln.index(":"), len(ln) - 2
        assert ln[b] == ":"
        chunks, at_cap = [int(v) for v in ln[a + 1:b]], int(ln[b + 1])
        assert se == min(sync if sync > 0 else (100 if rule == MSG else 200), K_HIST), ln
        assert all(1 <= m <= min(se, K_HIST) for m in chunks), ln
        assert sum(chunks) == cap, ln
        ends = set()
        for m in chunks:
            ends.add(m + max(ends, default=0))
        if rule == MSG and every > 0:
            assert all(k in ends for k in range(every, cap + 1, every)), ln         # a poll on every callback iteration
        if watched:
            assert chunks[0] == 1, ln
        assert at_cap == 1, ln                                                       # never 0
        # nothing is cut shorter than the rules ask: a chunk ends at sync_every, at the cap, on the cadence or after iteration 1
        start = 0
        for i, m in enumerate(chunks):
            end = start + m
            assert m == se or end == cap or (rule == MSG and every > 0 and end % every == 0) or (watched and i == 0), ln
            start = end


def _calls(ln):
    return [tuple(float(v) if i else int(v) for i, v in enumerate(c.split(","))) for c in ln[ln.index(":") + 1:]]


def test_replayed_callbacks(lines):
    rows = [ln for ln in lines if ln[0] == "replay"]
    assert len(rows) == 5 * 4 * 2 * 2 + 1
    seen = set()
    for ln in rows:
        reason, K, every, has_u, diag, npolls = map(int, ln[1:7])
        got = _calls(ln)
        if diag:                                                # every iteration, 0-based, the roots of the 2-norm sums
            assert got == [(it - 1, 2.0 * it, 3.0 * it, 4.0 * it) for it in range(1, K + 1)]
            continue
        stopped = reason in (PRECISION, RESIDUAL, EXACT_ERROR)  # the iteration cap and an interruption are no break
        its = [it for it in range(1, K + 1) if (it == 1 or (every > 0 and it % every == 0)) and not (stopped and it == K)]
        assert got == [(it, it + 0.25, it + 0.5, it + 0.75 if has_u else DBL_MAX) for it in its], ln
        seen.add((reason, every > 0 and K % every == 0, npolls > 1))
    assert seen == {(r, on, many) for r in range(5) for on in (False, True) for many in (False, True)}
    assert ["silent", "0"] in lines


def test_msg_stop_reason_priority(lines):
    rows = [ln for ln in lines if ln[0] == "stop"]
    assert len(rows) == 8 * 8 * 2 * 2
    for ln in rows:
        holds, off, have, has_u, got = int(ln[1]), int(ln[2]), int(ln[3]), int(ln[4]), int(ln[6])
        want = 0
        if have and holds & 1 and not off & 1:
            want = PRECISION
        elif holds & 2 and not off & 2:
            want = RESIDUAL
        elif holds & 4 and not off & 4 and has_u:
            want = EXACT_ERROR
        assert got == want, ln
    assert ["stop_fixed", "0"] in lines and ["stop_rel2", "0"] in lines


def test_result_fields(lines):
    rows = {ln[1]: [float(v) for v in ln[3:]] for ln in lines if ln[0] == "results"}
    #                              it conv reason        rmax  dmax     emax     rnorm r0  solve rel outer loop
    assert rows["converged"] == [12, 1, RESIDUAL, 0.25, 0.125, 0.5, 2.0, 8.0, 0, 0, 0, 0]
    assert rows["interrupted"] == [12, 0, INTERRUPTED, 0.25, 0.125, 0.5, 2.0, 8.0, 0, 0, 0, 0]
    assert rows["no_u"] == [12, 1, RESIDUAL, 0.25, 0.125, DBL_MAX, 2.0, 16.0, 0, 0, 0, 0]
    assert rows["no_step"] == [0, 1, RESIDUAL, 0.25, DBL_MAX, 0.5, 2.0, 8.0, 0, 0, 0, 0]
    assert rows["mixed_converged"] == [40, 1, RESIDUAL, DBL_MAX, DBL_MAX, DBL_MAX, 1.0, 4.0, 0, 0.25, 3, 0]
    assert rows["mixed_interrupted"] == [40, 0, INTERRUPTED, DBL_MAX, DBL_MAX, DBL_MAX, 1.0, 0.0, 0, 0, 1, 0]
