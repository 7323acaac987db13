"""The host arithmetic of the on-chip ensemble stepper (csrc/onchip_plan.h) without a GPU.
tests/cpp/onchip_steps_plan_driver.cpp, a program of its own built with the sanitizers, (1) evaluates onchip_step_rhs -- the
per-node right-hand side of a step that k_onchip_steps calls -- over a seeded image, which is compared bit for bit with the same
expression written in NumPy operation by operation, and (2) restates the workspace formula for every even N from 6 to the cap.  The
header, the ctypes layer and the package must agree on the new entry points."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("onchip_steps") / "onchip_steps_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "onchip_steps_plan_driver.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def lines(driver):
    out = subprocess.run([driver], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    return [ln.split() for ln in out.stdout.splitlines()]


def packed_cells(n):
    """The image cell of every unknown in packed order: the bottom-right block row by row, then the upper block (onchip_plan.h)."""
    half, pitch = n // 2, n + 1
    cells = [y * pitch + x for y in range(1, half + 1) for x in range(half + 1, n)]
    cells += [y * pitch + x for y in range(half + 1, n) for x in range(1, n)]
    return np.array(cells), pitch


@pytest.mark.parametrize("n", [6, 10, 20])
@pytest.mark.parametrize("theta", [1.0, 0.5])
def test_step_rhs_is_the_steppers_expression_in_its_order(driver, tmp_path, n, theta):
    rng = np.random.default_rng(100 * n + int(10 * theta))
    cells, pitch = packed_cells(n)
    assert len(cells) == (n // 2 - 1) * (3 * n // 2 - 1)
    img = rng.standard_normal((n + 1) ** 2) * 10.0 ** rng.integers(-3, 4, (n + 1) ** 2)
    g = rng.standard_normal(len(cells))
    sigma, A0, xk, yk = 1.0 / (theta * 0.037), -2.0 * (n * n + 1.7 * n * n), float(n * n), 1.7 * n * n
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([[float(n), theta, sigma, A0, xk, yk], img, g]).astype(np.float64).tofile(src)
    out = subprocess.run([driver, src, dst], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-2000:]
    got = np.fromfile(dst, dtype=np.float64)
    # k_step_rhs (step_kernels.h), one rounding per operation, in its order
    uc, left, right, down, up = img[cells], img[cells - 1], img[cells + 1], img[cells - pitch], img[cells + pitch]
    if theta < 1.0:
        b = g / theta - sigma * uc
        au = A0 * uc + xk * (left + right)
        au = au + yk * (down + up)
        b = b - ((1.0 - theta) / theta) * au
    else:
        b = g - sigma * uc
    assert got.shape == b.shape and np.array_equal(got, b)
    if theta < 1.0:                                   # the CG stencil's order (centre, left, right, up, down) gives other bits somewhere
        other = A0 * uc
        for term in (xk * left, xk * right, yk * up, yk * down):
            other = other + term
        assert not np.array_equal(g / theta - sigma * uc - ((1.0 - theta) / theta) * other, b)


def test_the_driver_found_no_violation(lines):
    assert not [ln for ln in lines if ln and ln[0] == "FAIL"]
    assert lines[-1] == ["ok", "0"]


def test_workspace_formula_header_ctypes_and_package_agree(lines):
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    import ctypes as C
    lib = _capi.load()
    cap = [int(ln[1]) for ln in lines if ln and ln[0] == "cap"][0]
    rows = {int(ln[0][2:]): ln for ln in lines if ln and ln[0].startswith("N=")}
    assert sorted(rows) == list(range(6, cap + 1, 2))
    for n, ln in rows.items():
        unknowns = int(ln[1].split("=")[1])
        assert unknowns == (n // 2 - 1) * (3 * n // 2 - 1)
        entries = [tuple(int(v) for v in e.split(":")) for e in ln[2].split("=")[1].split(",")]
        assert {e[2] for e in entries} == {0, 1} and len({e[0] for e in entries}) >= 4 and len({e[1] for e in entries}) >= 4
        for nsys, nsteps, with_counts, nbytes in entries:
            want = nsys * (24 * unknowns + 456) + 8 + 16 * nsys + 8 * unknowns + (4 * nsys * nsteps if with_counts else 0)
            assert nbytes == want, (n, nsys, nsteps, with_counts)
            if n in (6, 10, 64, cap) or (nsys, nsteps) == (40, 7):
                out = C.c_longlong()
                assert lib.mi355cg_time_steps_many_workspace(n, nsys, nsteps, with_counts, C.byref(out)) == _capi.OK and out.value == want
                assert isa.time_steps_many_workspace(n, nsys, nsteps, bool(with_counts)) == want
    # monotone in each argument
    f = isa.time_steps_many_workspace
    assert f(10, 5, 3) < f(12, 5, 3) and f(10, 5, 3) < f(10, 6, 3) and f(10, 5, 3) < f(10, 5, 4) and f(10, 5, 3, False) < f(10, 5, 3)
    assert f(10, 5, 3, False) == f(10, 5, 4, False)
    # refused above the caps
    for bad in ((cap + 2, 1, 1), (7, 1, 1), (10, 0, 1), (10, _capi.MANY_MAX + 1, 1), (10, 1, -1), (10, 1, _capi.STEPS_MANY_MAX_STEPS + 1),
                (10, 1025, 65536)):
        with pytest.raises(ValueError):
            f(*bad)
    assert f(10, 1024, 65536) > 0 and f(10, 1025, 65536, False) > 0
    assert lib.mi355cg_time_steps_many_workspace(10, 1, 1, 1, None) == _capi.ERR_INVALID


def test_header_ctypes_package_and_compat_agree():
    import iterative_solvers_amd as isa
    from iterative_solvers_amd import _capi
    text = open(os.path.join(ROOT, "include", "mi355cg.h")).read()
    assert "#define MI355CG_STEPS_MANY_MAX_STEPS 65536" in text and isa.STEPS_MANY_MAX_STEPS == _capi.STEPS_MANY_MAX_STEPS == 65536
    for name in ("mi355cg_time_steps_many", "mi355cg_time_steps_many_device", "mi355cg_time_steps_many_workspace"):
        assert name in _capi.EXPORTS and ("int  " + name + "(") in text
        assert hasattr(_capi.load(), name)
    assert callable(isa.MatrixFreeSystem.time_steps_many) and callable(isa.time_steps_many_workspace)
    compat = open(os.path.join(ROOT, "iterative_solvers_amd", "compat", "mi355cg_compat.hpp")).read()
    assert "timeStepsMany(" in compat
