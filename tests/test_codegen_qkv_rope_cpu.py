"""Guards on the generated gfx950 code of the sixteen q/k/v rotary kernels (csrc/sqllm_linear_qkv.hip: {3, 4} bits x batch tile
{1, 2, 4, 8} x {fp16, bf16}; hipcc cross-compiles without a GPU), against the bf16 linear's kernel of the same bits and batch
tile from the SAME build (csrc/sqllm_linear_bf16.hip -- the skeleton they share): no scratch, no spills, a VGPR count inside
the same occupancy step, the same LDS.  The rotation must cost no workgroup per CU on any tile: every tile the launcher
can pick is served by its own kernel (no tile is sent to a wider one)."""
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
        # the explicit by-value arguments, (offset, size) in order: the descriptor block, then whatever follows it
        kernels[name]["by_value"] = [(int(o), int(s)) for o, s in
                                     re.findall(r"\.offset:\s+(\d+)\n\s+\.size:\s+(\d+)\n\s+\.value_kind:\s+by_value", block)]
    return kernels


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("asm_qkv")
    return _meta(hipcc, "sqllm_linear_qkv.hip", d / "qkv.s"), _meta(hipcc, "sqllm_linear_bf16.hip", d / "bf16.s")


def _qkv_name(bits, bt, ot):  # ot: DF16_ = _Float16, DF16b = __bf16 (Itanium mangling)
    return f"_ZN5sqllm23sqllm_linear_qkv_kernelILi{bits}ELi{bt}E{ot}EEvPKvNS_9GroupArgsENS_8RopeArgsE"


def _bf16_name(bits, bt):
    return f"_ZN5sqllm24sqllm_linear_bf16_kernelILi{bits}ELi{bt}EEEvPKvNS_9GroupArgsE"


def _occupancy_step(vgprs):
    """waves per SIMD that a VGPR count leaves room for on gfx950 (512 registers per lane, allocated in blocks of 8, at
    most 8 waves)"""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def test_the_source_is_part_of_the_product_build():
    assert "sqllm_linear_qkv.hip" in B.SOURCES and B.SOURCES.index("sqllm_linear_qkv.hip") < B.SOURCES.index("sqllm_capi.hip")
    assert B.SOURCES[-1] == "sqllm_capi.hip"


def test_the_sixteen_kernels_exist_and_nothing_else(kernels):
    """the fronts' launch ladder (sqllm_fused.h: launch_front_bits) switches over batch_tile() = 1, 2, 4, 8 for both bit widths and
    both types, and the source launches its kernel through it: exactly those"""
    qkv, bf16 = kernels
    assert sorted(qkv) == sorted(_qkv_name(b, t, ot) for b, t in CASES for ot in ("DF16_", "DF16b"))
    assert sorted(bf16) == sorted(_bf16_name(b, t) for b, t in CASES)
    ladder = open(os.path.join(B.CSRC, "sqllm_fused.h")).read()
    assert [int(t) for t in re.findall(r"launch_front_inst<TAG, BITS, (\d), OT>", ladder)] == [1, 2, 4, 8]
    src = open(os.path.join(B.CSRC, "sqllm_linear_qkv.hip")).read()
    assert "return sqllm_linear_qkv_kernel<BITS, BT, OT>;" in src and "launch_front<QkvFront>(bits, a, stream, " in src


@pytest.mark.parametrize("ot", ["DF16_", "DF16b"])
@pytest.mark.parametrize("bits,bt", CASES)
def test_no_scratch_same_occupancy_same_lds(kernels, bits, bt, ot):
    qkv, bf16 = kernels
    g, ref = qkv[_qkv_name(bits, bt, ot)], bf16[_bf16_name(bits, bt)]
    # (SGPRs parked in VGPR lanes are inside the VGPR count checked below and touch no memory)
    assert g[".private_segment_fixed_size"] == 0 and g[".vgpr_spill_count"] == 0, g
    assert _occupancy_step(g[".vgpr_count"]) >= _occupancy_step(ref[".vgpr_count"]), (g[".vgpr_count"], ref[".vgpr_count"])
    assert g[".group_segment_fixed_size"] == ref[".group_segment_fixed_size"]
    if bt == 1:  # four 8-wave workgroups per CU
        assert g[".vgpr_count"] <= 64 and _occupancy_step(g[".vgpr_count"]) == 8


def test_the_rotary_arguments_sit_where_the_finisher_reads_them(kernels):
    """the finisher reads the rotary arguments from the kernel-argument segment itself, at a byte offset the source computes
    from a mirror struct (QkvKernArgs): that is the offset the compiler gave the third argument, directly behind the
    descriptor block, in every kernel -- and the loads through it exist"""
    qkv, bf16 = kernels
    (ga_off, ga_size), = {tuple(k["by_value"][0]) for k in bf16.values()}
    for name, k in qkv.items():
        assert k["by_value"] == [(ga_off, ga_size), (ga_off + ga_size, 64)], name
    src = open(os.path.join(B.CSRC, "sqllm_linear_qkv.hip")).read()
    assert "kRopeArgsOffset = offsetof(QkvKernArgs, ra)" in src
    assert "static_assert(kRopeArgsOffset == sizeof(void*) + sizeof(GroupArgs)" in src and (ga_off, ga_off + ga_size) == (8, 640)
