"""Guards on the generated gfx950 code of the attention front's cache-writing kernels (csrc/sqllm_linear_qkv_cache.hip and
csrc/sqllm_linear_qkv_norm_cache.hip: {3, 4} bits x batch tile {1, 2, 4, 8} x {fp16, bf16} each; hipcc cross-compiles without
a GPU), against the PARENT kernel of the same bits, tile and type from the SAME build (csrc/sqllm_linear_qkv.hip, resp.
csrc/sqllm_linear_qkv_norm.hip): no scratch, no spills, a VGPR count inside the parent's occupancy step, the parent's LDS.
Writing k and v a second time must cost no workgroup per CU on any tile."""
import os
import re
import shutil

import pytest

from squeezellm_amd import build as B
from tests.test_codegen_qkv_rope_cpu import CASES, _meta, _occupancy_step

OTS = ("DF16_", "DF16b")  # _Float16, __bf16 (Itanium mangling)
# (new source, its kernel, parent source, the parent's kernel, what follows GroupArgs in the signature: new / parent)
FAMILIES = {
    "plain": ("sqllm_linear_qkv_cache.hip", "29sqllm_linear_qkv_cache_kernel", "NS_8RopeArgsENS_11KvCacheArgsE",
              "sqllm_linear_qkv.hip", "23sqllm_linear_qkv_kernel", "NS_8RopeArgsE"),
    "norm": ("sqllm_linear_qkv_norm_cache.hip", "34sqllm_linear_qkv_norm_cache_kernel", "NS_8RopeArgsENS_11KvCacheArgsENS_8NormArgsE",
             "sqllm_linear_qkv_norm.hip", "28sqllm_linear_qkv_norm_kernel", "NS_8RopeArgsENS_8NormArgsE"),
}


def _name(kernel, tail, bits, bt, ot):
    return f"_ZN5sqllm{kernel}ILi{bits}ELi{bt}E{ot}EEvPKvNS_9GroupArgsE{tail}"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("asm_qkv_cache")
    return {fam: (_meta(hipcc, f[0], d / (fam + "_cache.s")), _meta(hipcc, f[3], d / (fam + "_parent.s"))) for fam, f in FAMILIES.items()}


def test_the_sources_are_part_of_the_product_build():
    for f in FAMILIES.values():
        assert f[0] in B.SOURCES and B.SOURCES.index(f[0]) < B.SOURCES.index("sqllm_capi.hip")
    assert B.SOURCES[-1] == "sqllm_capi.hip"


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_the_sixteen_kernels_exist_and_nothing_else(kernels, fam):
    """the launchers switch over batch_tile() = 1, 2, 4, 8 for both bit widths and both types: exactly those"""
    f = FAMILIES[fam]
    new, parent = kernels[fam]
    assert sorted(new) == sorted(_name(f[1], f[2], b, t, ot) for b, t in CASES for ot in OTS)
    assert sorted(parent) == sorted(_name(f[4], f[5], b, t, ot) for b, t in CASES for ot in OTS)
    src = open(os.path.join(B.CSRC, f[0])).read()
    # (the batch-tile ladder the fronts share, and this source's kernel on it)
    ladder = open(os.path.join(B.CSRC, "sqllm_fused.h")).read()
    assert [int(t) for t in re.findall(r"launch_front_inst<TAG, BITS, (\d), OT>", ladder)] == [1, 2, 4, 8]
    kernel = f[1].lstrip("0123456789")
    assert f"return {kernel}<BITS, BT, OT>;" in src and re.search(r"launch_front<Qkv(Norm)?CacheFront>\(bits, a, stream, ", src)


@pytest.mark.parametrize("ot", OTS)
@pytest.mark.parametrize("bits,bt", CASES)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_no_scratch_the_parents_occupancy_the_parents_lds(kernels, fam, bits, bt, ot):
    f = FAMILIES[fam]
    new, parent = kernels[fam]
    g, ref = new[_name(f[1], f[2], bits, bt, ot)], parent[_name(f[4], f[5], bits, bt, ot)]
    # (SGPRs parked in VGPR lanes are inside the VGPR count checked below and touch no memory)
    assert g[".private_segment_fixed_size"] == 0 and g[".vgpr_spill_count"] == 0, g
    assert _occupancy_step(g[".vgpr_count"]) >= _occupancy_step(ref[".vgpr_count"]), (g[".vgpr_count"], ref[".vgpr_count"])
    assert g[".group_segment_fixed_size"] == ref[".group_segment_fixed_size"]


def test_the_cache_arguments_sit_where_the_finisher_reads_them(kernels):
    """the finisher reads the cache's arguments from the kernel-argument segment itself, at a byte offset the source computes
    (kKvCacheArgsAt: directly behind the rotary arguments, checked against a mirror struct in either file): that is the offset
    the compiler gave the fourth argument in every kernel, with the norm's arguments LAST where there are any"""
    ga, ra = (8, 632), (640, 64)
    for name, k in kernels["plain"][0].items():
        assert k["by_value"] == [ga, ra, (704, 40)], name
    for name, k in kernels["norm"][0].items():
        assert k["by_value"] == [ga, ra, (704, 40), (744, 16)], name
    for name, k in kernels["plain"][1].items():  # (the parents: the rotary arguments where the new kernels have them)
        assert k["by_value"] == [ga, ra], name
    hdr = open(os.path.join(B.CSRC, "sqllm_cache_finish.h")).read()
    assert "kKvCacheArgsAt = kRopeArgsAt + sizeof(RopeArgs)" in hdr and "sizeof(KvCacheArgs) == 40" in hdr
    src = open(os.path.join(B.CSRC, "sqllm_linear_qkv_cache.hip")).read()
    assert "kKvCacheArgsOffset = offsetof(QkvCacheKernArgs, ca)" in src and "static_assert(kKvCacheArgsOffset == kKvCacheArgsAt" in src
    src = open(os.path.join(B.CSRC, "sqllm_linear_qkv_norm_cache.hip")).read()
    assert "static_assert(offsetof(QkvNormCacheKernArgs, ca) == kKvCacheArgsAt" in src
    assert src.index("KvCacheArgs ca;") < src.index("NormArgs na;")
