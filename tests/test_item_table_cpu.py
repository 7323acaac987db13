"""csrc/item_table.h without a GPU: tests/cpp/item_table_driver.cpp (built with the sanitizers, run as a program of its own)
builds the item tables of many plans -- N from 6 to 4096, 4 / 64 / 2048 waves, 1 / 8 / 512 workgroups, item heights 1 / 3 / 49,
XCD classes on and off, queued 4- and 16-row items, whole grids, row slabs and the 2 x 2 split -- and compares every entry with
the arithmetic the kernels used to do for themselves (decode_item, item_seq), restated there: every table entry, every wave's
sequence, every item visited exactly once, every owned (row, strip) in exactly one item, the ghost-column flags."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (6, 8, 10, 16, 30, 64, 66, 130, 258, 1026, 4096)


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("item_table") / "item_table_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "item_table_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    return [ln.split() for ln in out.stdout.splitlines()]


def test_tables_match_the_restated_arithmetic(lines):
    assert not [ln for ln in lines if ln and ln[0] == "FAIL"]
    assert lines[-1] == ["ok", "0"]


def test_every_size_was_covered(lines):
    rows = [ln for ln in lines if ln[0].startswith("N=")]
    assert [int(ln[0][2:]) for ln in rows] == list(SIZES)
    plans = [int(ln[1].split("=")[1]) for ln in rows]
    items = [int(ln[2].split("=")[1]) for ln in rows]
    # per size: 7 parts (whole, 2 + 4 slabs; 11 with the 2 x 2 split from two strips on) x 27 geometries x
    # (classes off, classes on, two queue heights) + the one-row plans + the two default plans
    per_size = [plans[0]] + [b - a for a, b in zip(plans, plans[1:])]
    for n, got in zip(SIZES, per_size):
        parts = 11 if (n - 1) // 128 + 1 >= 2 else 7
        assert got == parts * (27 * 4 + 9 * 2 + 2), (n, got)
    assert items[-1] > 10_000_000            # the one-row plans of N = 4096 alone are 100 000 items each
