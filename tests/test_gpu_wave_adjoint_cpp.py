"""MatrixFreeSystem::waveHistoryMany and waveAdjointMany of the C++ drop-in header, reached from a C++ host
(tests/cpp/onchip_wave_adjoint_compat_driver.cpp): three members in their own media at N = 10, the forward run with its history and
the backward run, bit for bit against what the Python calls give (which tests/test_gpu_wave_adjoint.py holds to the NumPy model).
The inputs are repeated here operation by operation; the expected values go in as hex floats."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from onchip_support import system as _system  # noqa: E402
import wave_adjoint_reference as A  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "onchip_wave_adjoint_compat_driver.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "onchip_wave_adjoint_compat_driver")
HEADERS = [os.path.join(ROOT, "iterative_solvers_amd", "compat", "mi355cg_compat.hpp"), os.path.join(ROOT, "include", "mi355cg.h")]


def build_driver():
    from iterative_solvers_amd import build as b
    b.build()
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(f) for f in [SRC] + HEADERS):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                               "-I", os.path.join(ROOT, "iterative_solvers_amd", "compat"), SRC,
                               "-L", os.path.join(ROOT, "iterative_solvers_amd"), "-lmi355cg",
                               "-Wl,-rpath," + os.path.join(ROOT, "iterative_solvers_amd"), "-o", EXE])
    return EXE


def test_the_driver_compiles_warning_free():
    """Not a GPU test: waveHistoryMany and waveAdjointMany compile against the shim headers and link."""
    assert os.path.exists(build_driver())


@pytest.mark.gpu
def test_cpp_host_runs_forward_and_backward_through_the_compat_header():
    exe = build_driver()
    many = _system(10)
    e = np.zeros(many.size())
    e[0] = 1.0
    col = many.apply(e)
    grid = A.Grid(10, col[0], col[1], col[10 // 2 - 1])
    size, nsteps, every = many.size(), 7, 2
    i = np.arange(size)
    rhs = many.get_rhs()
    g = np.stack([rhs * (1.0 + 0.25 * s * (((i * 37) % 101).astype(np.float64) / 101.0)) for s in range(3)])
    u0 = np.stack([0.01 * s * (((i * 11 + s) % 53).astype(np.float64) / 53.0 - 0.5) for s in range(3)])
    v0 = np.stack([0.5 * s * (((i * 7 + s) % 31).astype(np.float64) / 31.0 - 0.5) for s in range(3)])
    c2 = np.stack([0.25 + 3.75 * (((i * 13 + s * 5) % 47).astype(np.float64) / 46.0) for s in range(3)])
    source = np.stack([((np.arange(nsteps + 1) * 5 + s * 3) % 11).astype(np.float64) / 4.0 - 1.0 for s in range(3)])
    j, r = np.meshgrid(np.arange(nsteps // every), np.arange(3), indexing="ij")
    adj = np.stack([((j * 7 + r * 3 + s * 5) % 13).astype(np.float64) / 8.0 - 0.75 for s in range(3)])
    tau = many.wave_cfl(c2) * np.array([0.25, 0.5, 1.0])
    receivers = [0, size // 2, size - 1]
    hist = many.wave_history_many(u0, v0, tau, nsteps, source, g=g, receivers=receivers, record_every=every, c2=c2)[3]
    lam, q, sens = many.wave_adjoint_many(hist, tau, c2, adj, receivers=receivers, record_every=every)
    assert np.array_equal(hist, A.verlet_history(grid, u0, v0, g, c2, tau, nsteps, source)[3]) and np.abs(sens).max() > 0
    assert all(np.array_equal(a, b) for a, b in zip((lam, q, sens), A.adjoint(grid, hist, c2, tau, adj, receivers, every)))
    args = [float(x).hex() for x in hist.reshape(-1)]
    for s in range(3):
        args += [float(x).hex() for x in lam[s]] + [float(x).hex() for x in q[s]] + [float(x).hex() for x in sens[s]]
    env = {k: val for k, val in os.environ.items() if k != "MI355CG_ONCHIP"}
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2000:]
    doc = json.loads(out.stdout)
    assert doc["forward_is_the_medium_call"] is True and doc["refused_tau"] is True and len(doc["history"]) == len(doc["adjoint"]) == 3
    for m in doc["history"]:
        assert m["same_history"] is True and (m["steps_done"], m["converged"]) == (nsteps, 1)
    for m in doc["adjoint"]:
        assert m["same_lam"] is True and m["same_q"] is True and m["same_sens"] is True and m["steps_done"] == nsteps
    many._handle.close()
