"""Guards on the generated gfx950 code of the thirty-two norm-front kernels (csrc/sqllm_linear_gated_norm.hip and
csrc/sqllm_linear_qkv_norm.hip: {3, 4} bits x batch tile {1, 2, 4, 8} x {fp16, bf16} each; hipcc cross-compiles without a
GPU), each beside its counterpart of the SAME build (csrc/sqllm_linear_gated.hip / sqllm_linear_qkv.hip): no scratch, no
VGPR spills, the counterpart's LDS, and room for as many 8-wave workgroups per CU as the counterpart has -- with ONE exception that DESIGN.md 4.4 names: the
4-bit 2-row tile, whose counterparts sit at 61 / 64 of 64 registers, takes the 80-register step (three workgroups per CU
instead of four).  The achieved register counts are pinned: a compiler or source change that moves one shows here."""
import os
import re
import shutil
import subprocess

import pytest

from squeezellm_amd import build as B

META = (".group_segment_fixed_size", ".private_segment_fixed_size", ".sgpr_spill_count", ".vgpr_count", ".vgpr_spill_count")
CASES = [(bits, bt) for bits in (3, 4) for bt in (1, 2, 4, 8)]
OTS = ("DF16_", "DF16b")  # _Float16, __bf16 (Itanium mangling)
FILES = {"gated_norm": "sqllm_linear_gated_norm.hip", "qkv_norm": "sqllm_linear_qkv_norm.hip", "gated": "sqllm_linear_gated.hip",
         "qkv": "sqllm_linear_qkv.hip"}
NAMES = {
    "gated_norm": "_ZN5sqllm30sqllm_linear_gated_norm_kernelILi{bits}ELi{bt}E{ot}EEvPKvNS_9GroupArgsEPyNS_8NormArgsE",
    "qkv_norm": "_ZN5sqllm28sqllm_linear_qkv_norm_kernelILi{bits}ELi{bt}E{ot}EEvPKvNS_9GroupArgsENS_8RopeArgsENS_8NormArgsE",
    "gated": "_ZN5sqllm25sqllm_linear_gated_kernelILi{bits}ELi{bt}E{ot}EEvPKvNS_9GroupArgsEPy",
    "qkv": "_ZN5sqllm23sqllm_linear_qkv_kernelILi{bits}ELi{bt}E{ot}EEvPKvNS_9GroupArgsENS_8RopeArgsE",
}
RELAXED = {(4, 2)}  # the tile class that does not hold its counterpart's step
# achieved VGPR counts, (bits, batch tile) -> (fp16, bf16)
PINNED = {
    "gated_norm": {(3, 1): (63, 63), (3, 2): (79, 79), (3, 4): (85, 85), (3, 8): (123, 123), (4, 1): (61, 61), (4, 2): (71, 71), (4, 4): (77, 77), (4, 8): (99, 99)},
    "qkv_norm": {(3, 1): (63, 63), (3, 2): (79, 79), (3, 4): (85, 85), (3, 8): (123, 123), (4, 1): (61, 61), (4, 2): (73, 73), (4, 4): (77, 77), (4, 8): (99, 99)},
}


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
    d = tmp_path_factory.mktemp("asm_norm_front")
    return {k: _meta(hipcc, src, d / f"{k}.s") for k, src in FILES.items()}


def _occupancy_step(vgprs):
    """waves per SIMD that a VGPR count leaves room for on gfx950 (512 registers per lane, allocated in blocks of 8, at
    most 8 waves)"""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def _workgroups(vgprs):
    """8-wave workgroups per CU that a VGPR count leaves room for: a workgroup puts two waves on each of the four SIMDs (71
    registers leave room for seven waves per SIMD and 79 for six: three workgroups either way -- the 3-bit 2-row tile)"""
    return _occupancy_step(vgprs) // 2


def test_the_thirty_two_kernels_exist_and_nothing_else(kernels):
    for fam in ("gated_norm", "qkv_norm"):
        assert sorted(kernels[fam]) == sorted(NAMES[fam].format(bits=b, bt=t, ot=ot) for b, t in CASES for ot in OTS)
        src = open(os.path.join(B.CSRC, FILES[fam])).read()
        # (the batch-tile ladder the fronts share, and this source's kernel on it)
        ladder = open(os.path.join(B.CSRC, "sqllm_fused.h")).read()
        assert [int(t) for t in re.findall(r"launch_front_inst<TAG, BITS, (\d), OT>", ladder)] == [1, 2, 4, 8]
        assert f"return sqllm_linear_{fam}_kernel<BITS, BT, OT>;" in src and re.search(r"launch_front<\w+NormFront>\(bits, a, stream, ", src)


@pytest.mark.parametrize("ot", OTS)
@pytest.mark.parametrize("bits,bt", CASES)
@pytest.mark.parametrize("fam", ["gated_norm", "qkv_norm"])
def test_no_scratch_no_spills_counterparts_lds_and_step(kernels, fam, bits, bt, ot):
    g = kernels[fam][NAMES[fam].format(bits=bits, bt=bt, ot=ot)]
    ref = kernels[fam[:-5]][NAMES[fam[:-5]].format(bits=bits, bt=bt, ot=ot)]
    # (SGPRs parked in VGPR lanes are inside the VGPR count checked below and touch no memory)
    assert g[".private_segment_fixed_size"] == 0 and g[".vgpr_spill_count"] == 0, g
    assert ref[".private_segment_fixed_size"] == 0 and ref[".vgpr_spill_count"] == 0, ref
    assert g[".group_segment_fixed_size"] == ref[".group_segment_fixed_size"]
    assert g[".vgpr_count"] == PINNED[fam][(bits, bt)][OTS.index(ot)], g[".vgpr_count"]
    if (bits, bt) in RELAXED:
        assert _workgroups(ref[".vgpr_count"]) == 4 and _workgroups(g[".vgpr_count"]) == 3  # three workgroups per CU, not four
    else:
        assert _workgroups(g[".vgpr_count"]) >= _workgroups(ref[".vgpr_count"]), (g[".vgpr_count"], ref[".vgpr_count"])
    if bt == 1:  # four 8-wave workgroups per CU
        assert g[".vgpr_count"] <= 64 and _occupancy_step(g[".vgpr_count"]) == 8


def test_the_relaxed_step_is_the_one_the_source_names():
    src = open(os.path.join(B.CSRC, "sqllm_norm_front.h")).read()
    assert "return (bits == 4 && bt == 2) ? 6 : fused_min_waves(bits, bt, 0);" in src
    for f in ("sqllm_linear_gated_norm.hip", "sqllm_linear_qkv_norm.hip"):
        assert "__launch_bounds__(kWaves * 64, norm_min_waves(BITS, BT))" in open(os.path.join(B.CSRC, f)).read()


def test_the_rotary_arguments_stay_where_the_finisher_reads_them():
    """the norm's arguments are the q/k/v kernel's LAST argument: the rotary block keeps its offset in the argument segment"""
    src = open(os.path.join(B.CSRC, "sqllm_linear_qkv_norm.hip")).read()
    assert "static_assert(offsetof(QkvNormKernArgs, ra) == kRopeArgsAt" in src
    assert re.search(r"struct QkvNormKernArgs \{\s*const void\* x;\s*GroupArgs ga;\s*RopeArgs ra;\s*NormArgs na;\s*\};", src)
