"""Guards on the generated gfx950 code of the fp8 KV cache's kernels (hipcc cross-compiles without a GPU), read from the code
objects' metadata:
  * the writers (csrc/sqllm_linear_qkv_cache_fp8.hip, csrc/sqllm_linear_qkv_norm_cache_fp8.hip: {3, 4} bits x batch tile
    {1, 2, 4, 8} x {fp16, bf16} each) against the 16-bit cache SIBLING of the same bits, tile and type from the same build: no
    scratch, no spills, a VGPR count inside the sibling's occupancy step, the sibling's LDS; the new by-value argument at the
    offset the finisher reads;
  * the reader's partials (csrc/sqllm_attn_decode_fp8.hip: head_dim {64, 128} x group class {1, 2, 4, 8} x {fp16, bf16}, and no
    combine of its own): no scratch, no spills, LDS within 64 KB, two workgroups per CU;
  * the kernel-name lists of the three sources the earlier guards pin, unchanged."""
import os
import re
import shutil

import pytest

from squeezellm_amd import build as B
from tests.test_codegen_qkv_rope_cpu import CASES, _meta, _occupancy_step

OTS = ("DF16_", "DF16b")  # _Float16, __bf16 (Itanium mangling)
# (new source, its kernel, sibling source, the sibling's kernel, what follows RopeArgs in the signature: new / sibling)
FAMILIES = {
    "plain": ("sqllm_linear_qkv_cache_fp8.hip", "33sqllm_linear_qkv_cache_fp8_kernel", "NS_14KvCacheFp8ArgsE",
              "sqllm_linear_qkv_cache.hip", "29sqllm_linear_qkv_cache_kernel", "NS_11KvCacheArgsE"),
    "norm": ("sqllm_linear_qkv_norm_cache_fp8.hip", "38sqllm_linear_qkv_norm_cache_fp8_kernel", "NS_14KvCacheFp8ArgsENS_8NormArgsE",
             "sqllm_linear_qkv_norm_cache.hip", "34sqllm_linear_qkv_norm_cache_kernel", "NS_11KvCacheArgsENS_8NormArgsE"),
}
DIMS, CLASSES = (64, 128), (1, 2, 4, 8)


def _name(kernel, tail, bits, bt, ot):
    return f"_ZN5sqllm{kernel}ILi{bits}ELi{bt}E{ot}EEvPKvNS_9GroupArgsENS_8RopeArgsE{tail}"


def _partial(d, gc, ot):
    return f"_ZN5sqllm28sqllm_attn_decode_fp8_kernelILi{d}ELi{gc}E{ot}EEvNS_8AttnArgsEf"


@pytest.fixture(scope="module")
def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        pytest.skip("hipcc not available")
    return exe


@pytest.fixture(scope="module")
def writers(hipcc, tmp_path_factory):
    d = tmp_path_factory.mktemp("asm_kv_fp8")
    return {fam: (_meta(hipcc, f[0], d / (fam + "_fp8.s")), _meta(hipcc, f[3], d / (fam + "_sibling.s"))) for fam, f in FAMILIES.items()}


@pytest.fixture(scope="module")
def reader(hipcc, tmp_path_factory):
    d = tmp_path_factory.mktemp("asm_attn_fp8")
    return _meta(hipcc, "sqllm_attn_decode_fp8.hip", d / "attn_fp8.s"), _meta(hipcc, "sqllm_attn_decode.hip", d / "attn.s")


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_the_sixteen_writers_exist_and_nothing_else_and_the_siblings_are_unchanged(writers, fam):
    f = FAMILIES[fam]
    new, sib = writers[fam]
    assert sorted(new) == sorted(_name(f[1], f[2], b, t, ot) for b, t in CASES for ot in OTS)
    assert sorted(sib) == sorted(_name(f[4], f[5], b, t, ot) for b, t in CASES for ot in OTS)  # (the pinned source: today's instances)
    src = open(os.path.join(B.CSRC, f[0])).read()
    # (the batch-tile ladder the fronts share, and this source's kernel on it)
    ladder = open(os.path.join(B.CSRC, "sqllm_fused.h")).read()
    assert [int(t) for t in re.findall(r"launch_front_inst<TAG, BITS, (\d), OT>", ladder)] == [1, 2, 4, 8]
    kernel = f[1].lstrip("0123456789")
    assert f"return {kernel}<BITS, BT, OT>;" in src and re.search(r"launch_front<Qkv(Norm)?CacheFp8Front>\(bits, a, stream, ", src)
    assert "RopeCacheFp8Finish<OT>" in src and '#include "sqllm_cache_fp8_finish.h"' in src


@pytest.mark.parametrize("ot", OTS)
@pytest.mark.parametrize("bits,bt", CASES)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_writers_no_scratch_no_spills_the_siblings_occupancy_the_siblings_lds(writers, fam, bits, bt, ot):
    f = FAMILIES[fam]
    new, sib = writers[fam]
    g, ref = new[_name(f[1], f[2], bits, bt, ot)], sib[_name(f[4], f[5], bits, bt, ot)]
    # (SGPRs parked in VGPR lanes are inside the VGPR count checked below and touch no memory)
    assert g[".private_segment_fixed_size"] == 0 and g[".vgpr_spill_count"] == 0, g
    assert _occupancy_step(g[".vgpr_count"]) >= _occupancy_step(ref[".vgpr_count"]), (g[".vgpr_count"], ref[".vgpr_count"])
    assert g[".group_segment_fixed_size"] == ref[".group_segment_fixed_size"]


def test_the_fp8_cache_arguments_sit_where_the_finisher_reads_them(writers):
    """cache_fp8_args() reads the fourth argument from the kernel-argument segment at kKvCacheFp8ArgsAt, directly behind the
    rotary arguments: the offset the compiler gave it in every kernel, 48 bytes (the 16-bit cache's 40 and the two reciprocals),
    the norm's arguments LAST where there are any"""
    ga, ra = (8, 632), (640, 64)
    for name, k in writers["plain"][0].items():
        assert k["by_value"] == [ga, ra, (704, 48)], name
    for name, k in writers["norm"][0].items():
        assert k["by_value"] == [ga, ra, (704, 48), (752, 16)], name
    for name, k in writers["plain"][1].items():  # (the siblings: theirs where it was)
        assert k["by_value"] == [ga, ra, (704, 40)], name
    hdr = open(os.path.join(B.CSRC, "sqllm_cache_fp8_finish.h")).read()
    assert "kKvCacheFp8ArgsAt = kRopeArgsAt + sizeof(RopeArgs)" in hdr and "sizeof(KvCacheFp8Args) == 48" in hdr
    assert "sizeof(KvCacheArgs) == 40" in open(os.path.join(B.CSRC, "sqllm_cache_finish.h")).read()
    src = open(os.path.join(B.CSRC, "sqllm_linear_qkv_cache_fp8.hip")).read()
    assert "kKvCacheFp8ArgsOffset = offsetof(QkvCacheFp8KernArgs, fa)" in src and "static_assert(kKvCacheFp8ArgsOffset == kKvCacheFp8ArgsAt" in src
    src = open(os.path.join(B.CSRC, "sqllm_linear_qkv_norm_cache_fp8.hip")).read()
    assert "static_assert(offsetof(QkvNormCacheFp8KernArgs, fa) == kKvCacheFp8ArgsAt" in src
    assert src.index("KvCacheFp8Args fa;") < src.index("NormArgs na;")


def test_exactly_the_expected_partials_and_the_16_bit_source_keeps_its_kernels(reader):
    new, old = reader
    assert sorted(new) == sorted(_partial(d, gc, ot) for d in DIMS for gc in CLASSES for ot in OTS)  # (no combine of its own)
    from tests import test_codegen_attn_decode_cpu as T
    assert sorted(old) == sorted([T._partial(d, gc, ot) for d in DIMS for gc in CLASSES for ot in OTS] + [T._combine(d, ot) for d in DIMS for ot in OTS])
    src = open(os.path.join(B.CSRC, "sqllm_attn_decode_fp8.hip")).read()
    # one instantiation per group class: the shared ladder's, over the kernel this file's tag names; the combine is reached through
    # the hook, and the file has no combine kernel
    ladder = open(os.path.join(B.CSRC, "sqllm_attn.h")).read()
    assert sorted(int(c) for c in re.findall(r"launch_attn_inst<TAG, D, (\d), OT>", ladder)) == list(CLASSES)
    assert "return sqllm_attn_decode_fp8_kernel<D, GC, OT>;" in src and "g_launch_attn[kAttnDecodeFp8] = launch_attn<AttnDecodeFp8Tag>" in src
    assert "struct AttnDecodeFp8Tag : AttnOneQuery" in src and "g_launch_attn_combine(k, c.head_dim, c.bf16, c.batch, stream)" in ladder
    assert "combine_kernel" not in src
    assert "16 ELEMENTS = 16 bytes per key" in src and "The cross-lane reduction this implies" in src  # the header comment's choice


@pytest.mark.parametrize("ot", OTS)
@pytest.mark.parametrize("gc", CLASSES)
@pytest.mark.parametrize("d", DIMS)
def test_partials_no_scratch_no_spills_two_workgroups_per_cu(reader, d, gc, ot):
    k = reader[0][_partial(d, gc, ot)]
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, k
    assert 0 < k[".group_segment_fixed_size"] <= 64 * 1024
    # a workgroup is 4 waves, one per SIMD: two workgroups per CU need two waves per SIMD by registers, and two LDS images
    assert _occupancy_step(k[".vgpr_count"]) >= 2, k[".vgpr_count"]
    assert 2 * k[".group_segment_fixed_size"] <= 160 * 1024
    assert k["by_value"] == [(0, 120), (120, 4)]  # AttnArgs as the combine takes it, then v_scale
