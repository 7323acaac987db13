"""The host's decisions about an ensemble of on-chip steppers (csrc/onchip_plan.h) without a GPU:
tests/cpp/onchip_report_driver.cpp prints them over tables (built with the sanitizers, run as a program of its own) and this file
checks the lines against the contract of mi355cg_time_steps_many (include/mi355cg.h) restated here, not against the header's code."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = 1.7976931348623157e308
MSG, REL2 = 0, 1
ITERATIONS, PRECISION, RESIDUAL, EXACT_ERROR, INTERRUPTED = range(5)
BUDGET, CAP, NORM0, LAST_RMAX = 7, 50, 8.0, 0.375            # the driver's constants
# the driver's polled state: dmax, |r| (REL_2NORM does not reduce it), ||r||_2
DMAX, RNORM2 = 0.125, 2.0
RMAX = {MSG: 0.25, REL2: 0.0}


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("onchip_report") / "onchip_report_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "onchip_report_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr
    return [ln.split() for ln in out.stdout.splitlines()]


def poll_iterations(watched, sync_every, cap):
    """The iterations after which a REL_2NORM solve polls, by the rules test_solve_loop_cpu.test_chunk_schedules states: a chunk is
    sync_every iterations, cut at the cap, and a watched solve runs its first iteration on its own."""
    ends, it = set(), 0
    while it < cap:
        it += 1 if (watched and it == 0) else min(sync_every, cap - it)
        ends.add(it)
    return ends


def test_rel_solve_ends_on_a_poll(lines):
    rows = [[int(v) for v in ln[1:5]] + [int(ln[6])] for ln in lines if ln[0] == "poll"]
    assert len(rows) == 2 * 3 * (2 + 6 + 51)
    assert {(w, s, c) for w, s, c, _, _ in rows} == {(w, s, c) for w in (0, 1) for s in (1, 7, 200) for c in (1, 5, 50)}
    for watched, sync, cap, it, got in rows:
        assert got == (1 if it in poll_iterations(watched, sync, cap) else 0), (watched, sync, cap, it)     # never iteration 0
    assert any(got for *_, got in rows) and not all(got for *_, it, got in rows if it > 0)


def test_launch_cap(lines):
    rows = [[int(v) for v in ln[1:4]] + [int(ln[5])] for ln in lines if ln[0] == "cap"]
    assert len(rows) == 3 * 5 * 4
    for nsteps, cap, m, got in rows:
        units = nsteps * (max(cap, 0) + 1)                       # an iteration costs one unit, a transition one
        assert got == -(-units // m) + 1, (nsteps, cap, m)


def _reports(lines):
    for ln in lines:
        if ln[0] != "report":
            continue
        rule, polled, watched, it = map(int, ln[2:6])
        steps_done, its, conv, reason = map(int, ln[7:11])
        rmax, dmax, emax, rnorm2, r0 = map(float, ln[11:16])
        yield ln[1], rule, polled, watched, it, (steps_done, its, conv, reason, rmax, dmax, emax, rnorm2, r0), (int(ln[16]), int(ln[17]))


EMPTY = (0, 0, INTERRUPTED, 0.0, DBL_MAX, DBL_MAX, 0.0, 0.0)     # a step not begun, of a member the host stopped


def test_member_reports(lines):
    seen = set()
    for tag, rule, polled, watched, it, got, patch in _reports(lines):
        hit = PRECISION if rule == MSG else RESIDUAL
        prec = DMAX if it > 0 else DBL_MAX                       # no precision before the first step
        if tag.startswith("ended"):
            # REL_2NORM: |r| only where the single solve's own schedule polls
            rmax = RMAX[MSG] if rule == MSG else (LAST_RMAX if it in poll_iterations(watched, BUDGET, CAP) else 0.0)
            steps, conv, reason = {"ended_last": (4, 1, hit), "ended_cap": (2, 0, ITERATIONS), "ended_stop": (2, 0, INTERRUPTED)}[tag]
            assert got == (steps, it, conv, reason, rmax, prec, DBL_MAX, RNORM2, NORM0), (tag, rule, watched, it)
            assert patch[0] == -1, (tag, rule)
        elif tag == "between":                                   # the step that finished counts and keeps its count; the next was not begun
            assert got == (2,) + EMPTY and patch == (1, 9), (tag, rule)
        else:
            assert tag == "inside"
            # MSG polls the start state of a step, REL_2NORM reads no state before the step's first chunk
            begun = polled and (rule == MSG or it > 0)
            want = (it, 0, INTERRUPTED, RMAX[rule], prec, DBL_MAX, RNORM2, NORM0) if begun else EMPTY
            step = 1 if polled else 0
            assert got == (step,) + want and patch == (step, it if begun else 0), (tag, rule, polled, it)
        seen.add((tag, rule, polled, it > 0))
    for rule in (MSG, REL2):
        assert {("ended_last", rule, 1, True), ("ended_cap", rule, 1, True), ("ended_stop", rule, 1, True), ("between", rule, 1, True),
                ("inside", rule, 1, True), ("inside", rule, 1, False), ("inside", rule, 0, True)} <= seen
    # REL_2NORM: both answers occur among the ended members
    rel = [(it, got[4]) for tag, rule, _, _, it, got, _ in _reports(lines) if rule == REL2 and tag == "ended_last"]
    assert {r for _, r in rel} == {0.0, LAST_RMAX}
