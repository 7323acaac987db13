"""The host arithmetic of the batched on-chip solves (csrc/onchip_plan.h) without a GPU.  tests/cpp/onchip_many_plan_driver.cpp,
a program of its own built with the sanitizers, checks for every even N from 6 to the cap that a workgroup's LDS bytes cover the
image of that grid and the side data, stay within 160 KiB, grow with N, and that the workspace bytes follow the documented
formula.  The header, the ctypes layer and the package must agree on the new entry points."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE = 8 * (4 + 10) * 8 + 256                        # kOnchipSideBytes


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("onchip_many") / "onchip_many_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "onchip_many_plan_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    return [ln.split() for ln in out.stdout.splitlines()]


@pytest.fixture(scope="module")
def rows(lines):
    """{N: {"lds", "cells", "unknowns", "per_cu", "ws1", "ws40"}} as the driver printed them."""
    return {int(ln[0][2:]): {k: int(v) for k, v in (f.split("=") for f in ln[1:])} for ln in lines if ln and ln[0].startswith("N=")}


def test_the_driver_found_no_violation(lines):
    assert not [ln for ln in lines if ln and ln[0] == "FAIL"]
    assert lines[-1] == ["ok", "0"]


def test_lds_follows_n_for_every_even_size(lines, rows):
    cap = [int(ln[1]) for ln in lines if ln and ln[0] == "cap"][0]
    assert sorted(rows) == list(range(6, cap + 1, 2))
    last = 0
    for n in sorted(rows):
        r = rows[n]
        assert r["cells"] == (n + 1) ** 2 and r["unknowns"] == (n // 2 - 1) * (3 * n // 2 - 1)
        assert r["cells"] * 8 + SIDE <= r["lds"] <= 160 * 1024
        assert r["lds"] > last
        last = r["lds"]
    assert rows[10]["per_cu"] >= 32 and rows[cap]["per_cu"] == 1        # small grids share a CU, the largest does not


def test_workspace_bytes_follow_the_documented_formula(rows):
    for n, r in rows.items():
        per_system = 3 * 8 * r["unknowns"] + 456
        assert r["ws1"] == per_system + 8 and r["ws40"] == 40 * per_system + 8


def test_header_ctypes_and_package_agree():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    text = open(os.path.join(ROOT, "include", "mi355cg.h")).read()
    assert "#define MI355CG_MANY_MAX 65536" in text and isa.MANY_MAX == _capi.MANY_MAX == 65536
    for name in ("mi355cg_solve_many", "mi355cg_solve_many_from", "mi355cg_solve_many_device", "mi355cg_solve_many_device_from",
                 "mi355cg_solve_many_info"):
        assert name in _capi.EXPORTS and ("int  " + name + "(") in text
    for cls in (isa.MatrixFreeSystem,):
        assert callable(cls.solve_many) and callable(cls.solve_many_info)
    compat = open(os.path.join(ROOT, "iterative_solvers_amd", "compat", "mi355cg_compat.hpp")).read()
    assert "solveMany(" in compat
