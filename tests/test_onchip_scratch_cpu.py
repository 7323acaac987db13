"""The on-chip kernels as the built library holds them: every k_onchip* instantiation is there and none uses
scratch -- a spill in the iteration or step loop is what their factoring is chosen to avoid (csrc/onchip_kernels.h: oc_chunk).  Read
from the metadata of the gfx950 code object inside libmi355cg.so; nothing is compiled and no device is needed."""
import os
import re
import shutil
import subprocess

import pytest

LLVM = os.path.join(os.path.dirname(os.path.realpath(shutil.which("hipcc") or "/opt/rocm/bin/hipcc")), "..", "lib", "llvm", "bin")
# family -> instantiations: (slots per thread) x (rule) for the chunk and step kernels, slots for Verlet, (warm) for the batch start
FAMILIES = {"k_onchip": 12, "k_onchip_many": 12, "k_onchip_many_init": 2, "k_onchip_steps": 12, "k_onchip_steps_init": 1,
            "k_onchip_wave_newmark": 12, "k_onchip_wave_newmark_init": 1, "k_onchip_wave_newmark_finish": 1, "k_onchip_wave_verlet": 6}


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")), reason="needs the ROCm LLVM tools")
def test_onchip_kernels_are_built_without_scratch(tmp_path):
    from iterative_solvers_amd import build as b
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "gfx950.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", b.build(), fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={co}"])
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    scratch = {}
    for entry in notes[notes.index("amdhsa.kernels"):].split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        if "k_onchip" in name:
            scratch[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", entry).group(1))
    for family, count in FAMILIES.items():
        mine = [n for n in scratch if re.search(rf"\d+{family}(E|I)", n)]
        assert len(mine) == count, (family, mine)
    assert len(scratch) == sum(FAMILIES.values()), sorted(scratch)
    print({n: v for n, v in scratch.items() if v})
    assert not any(scratch.values()), {n: v for n, v in scratch.items() if v}
