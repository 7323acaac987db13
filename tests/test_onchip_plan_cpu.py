"""csrc/onchip_plan.h without a GPU.  tests/cpp/onchip_plan_driver.cpp (built with the sanitizers, run as a program of its own)
restates the ownership of the on-chip solve from node_interior for every even N from 6 to the cap and checks the plan against it:
every interior node owned by exactly one (thread, slot), no exterior node owned, every neighbour inside the LDS image, every
non-interior neighbour a halo cell nobody writes, the LDS, thread and slot limits.  mi355cg_onchip_plan (ctypes, no GPU needed)
must report the same plan."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("onchip_plan") / "onchip_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "onchip_plan_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and not out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    return [ln.split() for ln in out.stdout.splitlines()]


@pytest.fixture(scope="module")
def plans(lines):
    """{N: (threads, lds_bytes, elems, unknowns)} as the driver printed them, and the cap."""
    rows = {}
    for ln in lines:
        if ln and ln[0].startswith("N="):
            rows[int(ln[0][2:])] = tuple(int(f.split("=")[1]) for f in ln[1:])
    cap = [int(ln[1]) for ln in lines if ln and ln[0] == "cap"]
    assert len(cap) == 1
    return rows, cap[0]


def test_ownership_matches_the_restated_arithmetic(lines):
    assert not [ln for ln in lines if ln and ln[0] == "FAIL"]
    assert lines[-1] == ["ok", "0"]


def test_every_even_size_up_to_the_cap_was_covered(plans):
    rows, cap = plans
    assert cap >= 64 and cap % 2 == 0
    assert sorted(rows) == list(range(6, cap + 1, 2))
    for n, (threads, lds, elems, unknowns) in rows.items():
        assert unknowns == (n // 2 - 1) * (3 * n // 2 - 1)
        assert threads <= 1024 and threads % 64 == 0 and lds <= 160 * 1024 and threads * elems >= unknowns
    assert rows[6][0] == 64                      # 16 unknowns: one wave, not sixteen
    assert len({t for t, *_ in rows.values()}) >= 3          # the workgroup grows with the grid


def test_capi_reports_the_drivers_plan(plans):
    from iterative_solvers_amd import _capi
    import iterative_solvers_amd as isa
    lib = _capi.load()
    rows, cap = plans
    for n in (6, 10, 64, cap):
        t, lds, e = C.c_int(), C.c_int(), C.c_int()
        assert lib.mi355cg_onchip_plan(n, C.byref(t), C.byref(lds), C.byref(e)) == _capi.OK
        assert (t.value, lds.value, e.value) == rows[n][:3]
        assert isa.onchip_plan(n) == {"threads": rows[n][0], "lds_bytes": rows[n][1], "elems_per_thread": rows[n][2]}
    for n in (7, 4, cap + 2):
        assert lib.mi355cg_onchip_plan(n, None, None, None) == _capi.ERR_INVALID
        assert str(cap).encode() in lib.mi355cg_last_error()
        with pytest.raises(ValueError):
            isa.onchip_plan(n)


def test_mode_constants_are_exported():
    import iterative_solvers_amd as isa
    assert (isa.SOLVE_LAUNCHES, isa.SOLVE_ONCHIP) == (0, 1)
    text = open(os.path.join(ROOT, "include", "mi355cg.h")).read()
    assert "#define MI355CG_SOLVE_LAUNCHES 0" in text and "#define MI355CG_SOLVE_ONCHIP   1" in text
