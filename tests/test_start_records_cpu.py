"""The start records of csrc/item_table.h without a GPU: tests/cpp/start_record_driver.cpp (built with the sanitizers, run as a
program of its own) builds the records of the plans below for both march directions and compares every wave's record, field by
field, with item_seq + decode_item + the wave-uniform part of item_addr as the kernels evaluated them before the records existed,
restated there.

    N = 6, 66     with and without MI355CG_BLOCKS=1     waves with no item (one workgroup at N = 66 gets four taller items, one per wave;
                  plus MI355CG_ITEM_ROWS=2                with 2-row items every wave has several)
    N = 258       MI355CG_BLOCKS=16                     three strips, XCD classes whose sizes are no multiple of the waves of a class
    N = 1026      MI355CG_ITEM_ROWS=3                   items that start in the bottom block, in the upper block, on the row of the re-entrant corner
    N = 514       fp32                                  256-column strips, 4-byte elements
    N = 4096      the bench's default plan
    and the upper row slab of N = 258: a part whose storage does not start at row 0."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("start_records") / "start_record_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "start_record_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    lines = [ln.split() for ln in out.stdout.splitlines()]
    assert not [ln for ln in lines if ln and ln[0] == "FAIL"]
    assert lines[-1] == ["ok", "0"]
    got = {}
    for ln in lines:
        if ln[0] == "plan":
            f = {k: int(v) for k, v in (t.split("=") for t in ln[2:])}
            got[(ln[1], f["N"])] = f
    return got


def test_every_plan_of_the_list_was_compared(plans):
    assert sorted(plans) == sorted([("default", 6), ("blocks1", 6), ("default", 66), ("blocks1", 66), ("blocks1rows2", 66), ("blocks16", 258), ("rows3", 1026),
                                    ("fp32", 514), ("default", 4096), ("slab", 258)])


def test_the_plans_cover_what_they_are_there_for(plans):
    # N = 6: 16 unknowns in two items (one per block of the L): two of the four waves of the workgroup have no item
    assert plans[("default", 6)]["items"] == 2 and plans[("default", 6)]["idle"] == 2 and plans[("blocks1", 6)]["idle"] == 2
    assert plans[("default", 66)]["idle"] == 3
    # one workgroup at N = 66: one item per wave as the plan comes; several per wave once the items are held at 2 rows
    assert plans[("blocks1", 66)]["grid"] == 1 and plans[("blocks1", 66)]["idle"] == 0
    assert plans[("blocks1rows2", 66)]["grid"] == 1 and plans[("blocks1rows2", 66)]["several"] == 4
    # N = 258 with 16 workgroups: three strips, XCD classes of sizes that 8 waves do not divide
    p = plans[("blocks16", 258)]
    assert p["grid"] == 16 and p["ncls"] == 8 and p["items"] % 64 != 0
    # N = 1026 in 3-row items: first items in the bottom block, in the upper block and on the first row above the corner
    p = plans[("rows3", 1026)]
    assert p["ty"] == 3 and p["bottom"] > 0 and p["upper"] > 0 and p["corner"] > 0
    # the bench's plan: one item per wave, 2 016 of them on 504 workgroups
    p = plans[("default", 4096)]
    assert (p["grid"], p["items"], p["several"], p["idle"]) == (504, 2016, 0, 0)
