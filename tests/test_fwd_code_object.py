"""Code-object metadata of the compile-time-shape SP forward kernels (CPU only; the extraction
recipe is tests/test_isa.py's: the gfx950 code object is unbundled from the built librae_hip.so
with the ROCm LLVM tools and its notes are read, no GPU needed).

The fast path keeps C1 / C2 in registers from kernel entry (rae_sp.hpp sp_example_fast: 112
VGPRs at C3), in 512-thread workgroups whose waves get at most 256 VGPRs each: the C3 and C2
forward kernels must not spill -- private segment size 0, no spilled registers -- and their VGPR
counts are printed for the record."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

LLVM = "/opt/rocm/lib/llvm/bin"
LIB = os.path.join(ROOT, "relation-autoencoder_amd", "rae", "librae_hip.so")
FWD = {"C3": "_Z9k_forwardILb1EN3rae7FixDimsILi100ELi200ELi20EEEEvNS0_8StepArgsE",
       "C2": "_Z9k_forwardILb0EN3rae7FixDimsILi30ELi100ELi10EEEEvNS0_8StepArgsE"}
FIELDS = ("private_segment_fixed_size", "vgpr_count", "agpr_count", "vgpr_spill_count",
          "sgpr_spill_count", "max_flat_workgroup_size")


def _tool(name):
    p = os.path.join(LLVM, name)
    if not os.path.exists(p):
        pytest.skip(f"{p} not available")
    return p


@pytest.fixture(scope="module")
def kernels(built_lib, tmp_path_factory):
    """{kernel name: {metadata field: int}} from the code object's amdhsa.kernels note."""
    d = tmp_path_factory.mktemp("co")
    fat, co = d / "fat.bin", d / "gfx950.co"
    subprocess.run([_tool("llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", LIB,
                    str(fat)], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    notes = subprocess.run([_tool("llvm-readelf"), "--notes", str(co)], check=True,
                           capture_output=True, text=True).stdout
    # one list entry per kernel ("  - .agpr_count: ..." opens it), keys in alphabetical order
    out = {}
    for entry in re.split(r"\n\s*- (?=\.\w+:)", notes):
        name = re.search(r"^\s*\.name:\s*(\S+)\s*$", entry, re.M)
        if not name:
            continue
        vals = {}
        for f in FIELDS:
            v = re.search(rf"^\s*(?:- )?\.{f}:\s*(\d+)\s*$", entry, re.M)
            if v:
                vals[f] = int(v.group(1))
        if "private_segment_fixed_size" in vals:
            out[name.group(1)] = vals
    assert out, "no kernel metadata in the code object"
    return out


@pytest.mark.parametrize("cfg", sorted(FWD))
def test_fast_forward_has_no_scratch(kernels, cfg):
    k = kernels.get(FWD[cfg])
    assert k, f"the {cfg} forward kernel is not in the code object"
    print(f"{cfg} k_forward: {k}")
    assert k["private_segment_fixed_size"] == 0, k
    assert k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k
    # 512 threads = 8 waves, two per SIMD: 512 registers per lane between them
    assert k["max_flat_workgroup_size"] == 512, k
    assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, k
