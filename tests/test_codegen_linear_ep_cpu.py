"""Guards on the generated gfx950 code of the sixteen epilogue kernels (csrc/sqllm_linear_ep.hip: {3, 4} bits x batch tile
{1, 2, 4, 8} x {fp16, bf16}; hipcc cross-compiles without a GPU), against the bf16 linear's kernel of the same bits and batch
tile from the SAME build (csrc/sqllm_linear_bf16.hip -- the skeleton they share): no scratch, no spills, a VGPR count inside
the same occupancy step, the same LDS.  Activation and residual must cost no workgroup per CU."""
import os
import re
import shutil
import subprocess

import pytest

from squeezellm_amd import build as B

META = (".group_segment_fixed_size", ".private_segment_fixed_size", ".sgpr_spill_count", ".vgpr_count", ".vgpr_spill_count")
CASES = [(bits, bt) for bits in (3, 4) for bt in (1, 2, 4, 8)]


def _meta(hipcc, src, out):
    cmd = [hipcc, f"--offload-arch={B.ARCH}", *[f for f in B.FLAGS if f != "-fPIC"], "-S", "--cuda-device-only",
           f"-I{B.INCLUDE}", f"-I{B.CSRC}", os.path.join(B.CSRC, src), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    kernels = {}
    for block in out.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", block, re.M).group(1)
        kernels[name] = {k: int(re.search(rf"{re.escape(k)}:\s+(\d+)", block).group(1)) for k in META}
    return kernels


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("asm_ep")
    return _meta(hipcc, "sqllm_linear_ep.hip", d / "ep.s"), _meta(hipcc, "sqllm_linear_bf16.hip", d / "bf16.s")


def _ep_name(bits, bt, ot):  # ot: DF16_ = _Float16, DF16b = __bf16 (Itanium mangling)
    return f"_ZN5sqllm22sqllm_linear_ep_kernelILi{bits}ELi{bt}E{ot}EEvPKvNS_9GroupArgsEPKT1_i"


def _bf16_name(bits, bt):
    return f"_ZN5sqllm24sqllm_linear_bf16_kernelILi{bits}ELi{bt}EEEvPKvNS_9GroupArgsE"


def _occupancy_step(vgprs):
    """waves per SIMD that a VGPR count leaves room for on gfx950 (512 registers per lane, allocated in blocks of 8, at
    most 8 waves)"""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def test_the_source_is_part_of_the_product_build():
    assert "sqllm_linear_ep.hip" in B.SOURCES and B.SOURCES.index("sqllm_linear_ep.hip") < B.SOURCES.index("sqllm_capi.hip")


def test_the_sixteen_kernels_exist_and_nothing_else(kernels):
    ep, bf16 = kernels
    assert sorted(ep) == sorted(_ep_name(b, t, ot) for b, t in CASES for ot in ("DF16_", "DF16b"))
    assert sorted(bf16) == sorted(_bf16_name(b, t) for b, t in CASES)


@pytest.mark.parametrize("ot", ["DF16_", "DF16b"])
@pytest.mark.parametrize("bits,bt", CASES)
def test_no_scratch_same_occupancy_same_lds(kernels, bits, bt, ot):
    ep, bf16 = kernels
    g, ref = ep[_ep_name(bits, bt, ot)], bf16[_bf16_name(bits, bt)]
    # (SGPRs parked in VGPR lanes are inside the VGPR count checked below and touch no memory)
    assert g[".private_segment_fixed_size"] == 0 and g[".vgpr_spill_count"] == 0, g
    assert _occupancy_step(g[".vgpr_count"]) >= _occupancy_step(ref[".vgpr_count"]), (g[".vgpr_count"], ref[".vgpr_count"])
    assert g[".group_segment_fixed_size"] == ref[".group_segment_fixed_size"]
    if bt == 1:  # four 8-wave workgroups per CU
        assert g[".vgpr_count"] <= 64 and _occupancy_step(g[".vgpr_count"]) == 8
