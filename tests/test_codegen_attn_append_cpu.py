"""Guards on the generated gfx950 code of the kernels behind sqllm_attn_append_* (csrc/sqllm_attn_append.hip and
csrc/sqllm_attn_append_fp8.hip; hipcc cross-compiles without a GPU), read from the code objects' metadata: exactly the template
instances the launchers switch over (head_dim {64, 128} x virtual-head class {1, 2, 4, 8} x {fp16, bf16} partials in each source,
head_dim x type combines in the 16-bit source only), no scratch, no spills, LDS within 64 KB and a register count that leaves
room for at least two workgroups per CU.  (That the instances of the two one-query sources are what they were is
tests/test_codegen_attn_decode_cpu.py's and tests/test_codegen_kv_fp8_cpu.py's.)"""
import os
import re
import shutil

import pytest

from squeezellm_amd import build as B
from tests.test_codegen_qkv_rope_cpu import _meta, _occupancy_step

DIMS, CLASSES, TYPES = (64, 128), (1, 2, 4, 8), ("DF16_", "DF16b")  # DF16_ = _Float16, DF16b = __bf16 (Itanium mangling)


def _partial(d, gc, ot):
    return f"_ZN5sqllm24sqllm_attn_append_kernelILi{d}ELi{gc}E{ot}EEvNS_14AttnAppendArgsE"


def _partial_fp8(d, gc, ot):
    return f"_ZN5sqllm28sqllm_attn_append_fp8_kernelILi{d}ELi{gc}E{ot}EEvNS_14AttnAppendArgsEf"


def _combine(d, ot):
    return f"_ZN5sqllm32sqllm_attn_append_combine_kernelILi{d}E{ot}EEvNS_14AttnAppendArgsE"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("asm_attn_append")
    return _meta(hipcc, "sqllm_attn_append.hip", d / "append.s"), _meta(hipcc, "sqllm_attn_append_fp8.hip", d / "append_fp8.s")


def test_exactly_the_expected_instances(kernels):
    k16, k8 = kernels
    assert sorted(k16) == sorted([_partial(d, gc, ot) for d in DIMS for gc in CLASSES for ot in TYPES] + [_combine(d, ot) for d in DIMS for ot in TYPES])
    assert sorted(k8) == sorted(_partial_fp8(d, gc, ot) for d in DIMS for gc in CLASSES for ot in TYPES)  # (the combine is the other source's)
    # one instantiation per virtual-head class: the shared ladder's, over the kernel each file's tag names
    ladder = open(os.path.join(B.CSRC, "sqllm_attn.h")).read()
    assert sorted(int(c) for c in re.findall(r"launch_attn_inst<TAG, D, (\d), OT>", ladder)) == list(CLASSES)
    assert "switch (TAG::heads(k))" in ladder and "return k.q_len * k.group;" in ladder
    for name, kern, tag in (("sqllm_attn_append.hip", "sqllm_attn_append_kernel", "g_launch_attn[kAttnAppend] = launch_attn<AttnAppendTag>"),
                            ("sqllm_attn_append_fp8.hip", "sqllm_attn_append_fp8_kernel", "g_launch_attn[kAttnAppendFp8] = launch_attn<AttnAppendFp8Tag>")):
        src = open(os.path.join(B.CSRC, name)).read()
        assert f"return {kern}<D, GC, OT>;" in src and tag in src
        assert "template <int D, int GC, typename OT>\n__global__" in src  # head_dim, virtual-head class and output type only


@pytest.mark.parametrize("ot", TYPES)
@pytest.mark.parametrize("gc", CLASSES)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("fp8", [False, True])
def test_partials_no_scratch_no_spills_two_workgroups_per_cu(kernels, fp8, d, gc, ot):
    k = kernels[1][_partial_fp8(d, gc, ot)] if fp8 else kernels[0][_partial(d, gc, ot)]
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, k
    assert 0 < k[".group_segment_fixed_size"] <= 64 * 1024
    # a workgroup is 4 waves, one per SIMD: two workgroups per CU need two waves per SIMD by registers, and two LDS images
    assert _occupancy_step(k[".vgpr_count"]) >= 2, k[".vgpr_count"]
    assert 2 * k[".group_segment_fixed_size"] <= 160 * 1024


@pytest.mark.parametrize("ot", TYPES)
@pytest.mark.parametrize("d", DIMS)
def test_combines_no_scratch_no_spills(kernels, d, ot):
    k = kernels[0][_combine(d, ot)]
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, k
    assert k[".group_segment_fixed_size"] == 0 and _occupancy_step(k[".vgpr_count"]) == 8
