"""MatrixFreeSystem::waveSpongeMany of the C++ drop-in header, reached from a C++ host
(tests/cpp/onchip_wave_sponge_compat_driver.cpp): three members with their own media and damping fields, then one damping field in
a unit medium for all, bit for bit against the Python call (which tests/test_gpu_wave_sponge.py holds to the NumPy model).  The
inputs are repeated here operation by operation; the expected values go in as hex floats."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from onchip_support import system as _system  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "onchip_wave_sponge_compat_driver.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "onchip_wave_sponge_compat_driver")
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
    """Not a GPU test: waveSpongeMany compiles against the shim headers and links."""
    assert os.path.exists(build_driver())


@pytest.mark.gpu
def test_cpp_host_steps_a_damped_ensemble_through_the_compat_header():
    exe = build_driver()
    many = _system(12)
    size, nsteps, every = many.size(), 7, 2
    i = np.arange(size)
    rhs = many.get_rhs()
    g = np.stack([rhs * (1.0 + 0.25 * s * (((i * 37) % 101).astype(np.float64) / 101.0)) for s in range(3)])
    u0 = np.stack([0.01 * s * (((i * 11 + s) % 53).astype(np.float64) / 53.0 - 0.5) for s in range(3)])
    v0 = np.stack([0.5 * s * (((i * 7 + s) % 31).astype(np.float64) / 31.0 - 0.5) for s in range(3)])
    c2 = np.stack([0.25 + 3.75 * (((i * 13 + s * 5) % 47).astype(np.float64) / 46.0) for s in range(3)])
    source = np.stack([((np.arange(nsteps + 1) * 5 + s * 3) % 11).astype(np.float64) / 4.0 - 1.0 for s in range(3)])
    tau = many.wave_cfl(c2) * np.array([0.25, 0.5, 1.0])
    d = np.stack([((i * 17 + s * 3) % 29).astype(np.float64) / 28.0 * 0.9 / (0.25 * tau[s]) for s in range(3)])
    assert d.min() == 0.0 and 0.89 < ((0.25 * tau)[:, None] * d).max() <= 0.9 + 1e-15
    receivers = [0, size // 2, size - 1]
    ru, rv, rt, _, done = many.wave_record_many(u0, v0, tau, nsteps, source, g=g, receivers=receivers, record_every=every, c2=c2, damping=d)
    assert [int(x) for x in done] == [nsteps] * 3 and not np.array_equal(rv, many.wave_record_many(u0, v0, tau, nsteps, source, g=g, c2=c2)[1])
    half = np.full(3, 0.5 * many.wave_cfl())
    su, sv, _, _, _ = many.wave_record_many(u0, v0, half, nsteps, source[1], g=g, damping=d[2])
    args = []
    for s in range(3):
        args += [float(x).hex() for x in ru[s]] + [float(x).hex() for x in rv[s]] + [float(x).hex() for x in rt[s].reshape(-1)]
    for s in range(3):
        args += [float(x).hex() for x in su[s]] + [float(x).hex() for x in sv[s]]
    env = {k: val for k, val in os.environ.items() if k != "MI355CG_ONCHIP"}
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2000:]
    doc = json.loads(out.stdout)
    assert len(doc["damped"]) == len(doc["shared"]) == 3
    assert doc["refused_negative"] is True and doc["refused_nan"] is True and doc["refused_strong"] is True and doc["refused_size"] is True
    for m in doc["damped"]:
        assert m["same_u"] is True and m["same_v"] is True and m["same_traces"] is True and (m["steps_done"], m["converged"], m["iterations"]) == (nsteps, 1, 0)
    for m in doc["shared"]:
        assert m["same_u"] is True and m["same_v"] is True and m["no_traces"] is True and m["steps_done"] == nsteps
    many._handle.close()
