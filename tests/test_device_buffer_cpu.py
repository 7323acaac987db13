"""Buf<T> of csrc/device_buffer.h without a GPU: tests/cpp/device_buffer_driver.cpp (built with the sanitizers, run as a program
of its own) defines the header's four allocation functions with malloc / free, counts what is live per kind and can make the k-th
allocation fail.  It checks that an empty buffer frees nothing, that reset and destruction free exactly once, that moves transfer
ownership (move assignment frees the target's old memory, self-move is harmless), that pinned memory goes back through the pinned
function, that a borrow is never freed and drops what was owned before, and the library's build-then-swap pattern: a struct of five
buffers built by a function that returns on the first error leaves nothing live for a failure at any of the five allocations, and the
object installed before is untouched."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("device_buffer") / "device_buffer_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "cpp", "device_buffer_driver.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and not out.stderr, out.stdout[-3000:] + out.stderr[-3000:]
    return [ln.split(None, 1) for ln in out.stdout.splitlines()]


def test_no_check_of_the_driver_failed(driver_lines):
    assert not [ln for ln in driver_lines if ln and ln[0] == "FAIL"]
    assert driver_lines[-1] == ["ok", "0"]


def test_the_header_includes_no_hip_header():
    # the driver above is compiled by g++ alone; this keeps the reason in sight
    with open(os.path.join(ROOT, "iterative_solvers_amd", "csrc", "device_buffer.h")) as fh:
        includes = [ln.strip() for ln in fh if ln.lstrip().startswith("#include")]
    assert includes == ["#include <cstddef>"]
