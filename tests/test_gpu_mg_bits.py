"""The bits of the fp64 multigrid path, single and batched, are those recorded in tests/golden/mg_bits.json (tools/mg_bits.py;
the file names the commit it was recorded from).  The other multigrid suites pin batch == single and single ~ the NumPy
restatement to a tolerance; a change that moves both kernel families by one ulp passes those and fails here.  Per case: the
right-hand sides are the recorded ones (else the inputs changed, not the kernels), then apply_preconditioner, every single solve
and every system of the batch give the recorded iterations, stop_reason, r_norm2, initial_r_norm2 and x."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mg_bits  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(ROOT, "tests", "golden", "mg_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_file_records_every_case_of_the_tool():
    assert [c["name"] for c in GOLDEN["cases"]] == [c[0] for c in mg_bits.CASES]
    assert len(GOLDEN["commit"]) == 40


@pytest.mark.parametrize("case", mg_bits.CASES, ids=[c[0] for c in mg_bits.CASES])
def test_this_tree_reproduces_the_recorded_bits(case):
    want = next(c for c in GOLDEN["cases"] if c["name"] == case[0])
    got = mg_bits.compute(case)
    print(case[0], "iterations", [r["iterations"] for r in got["single"]])
    assert got["rhs_sha256"] == want["rhs_sha256"], "the right-hand sides are not the recorded ones: an input changed, not a kernel"
    for key in ("N", "kind", "rule", "rows"):
        assert got[key] == want[key], key
    assert got["precond_sha256"] == want["precond_sha256"], "apply_preconditioner"
    assert len(got["single"]) == len(want["single"]) == len(case[4])
    for k, (g, w) in enumerate(zip(got["single"], want["single"])):
        assert g == w, ("single solve", k, g, w)
    for k, (g, w) in enumerate(zip(got["batch"], want["batch"])):
        assert g == w, ("system of the batch", k, g, w)
    assert len(got["batch"]) == len(want["batch"]) == len(case[4])
