"""Guards on the generated gfx950 code of the decode attention's kernels (csrc/sqllm_attn_decode.hip; hipcc cross-compiles
without a GPU), read from the code objects' metadata: exactly the template instances the launcher switches over (head_dim
{64, 128} x group class {1, 2, 4, 8} x {fp16, bf16} partials, head_dim x type combines), no scratch, no spills, LDS within 64 KB
and a register count that leaves room for at least two workgroups per CU."""
import os
import re
import shutil

import pytest

from squeezellm_amd import build as B
from tests.test_codegen_qkv_rope_cpu import _meta, _occupancy_step

DIMS, CLASSES, TYPES = (64, 128), (1, 2, 4, 8), ("DF16_", "DF16b")  # DF16_ = _Float16, DF16b = __bf16 (Itanium mangling)


def _partial(d, gc, ot):
    return f"_ZN5sqllm24sqllm_attn_decode_kernelILi{d}ELi{gc}E{ot}EEvNS_8AttnArgsE"


def _combine(d, ot):
    return f"_ZN5sqllm25sqllm_attn_combine_kernelILi{d}E{ot}EEvNS_8AttnArgsE"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    return _meta(hipcc, "sqllm_attn_decode.hip", tmp_path_factory.mktemp("asm_attn") / "attn.s")


def test_the_source_is_part_of_the_product_build():
    assert "sqllm_attn_decode.hip" in B.SOURCES and B.SOURCES.index("sqllm_attn_decode.hip") < B.SOURCES.index("sqllm_capi.hip")
    assert B.SOURCES[-1] == "sqllm_capi.hip"


def test_exactly_the_expected_instances(kernels):
    want = [_partial(d, gc, ot) for d in DIMS for gc in CLASSES for ot in TYPES] + [_combine(d, ot) for d in DIMS for ot in TYPES]
    assert sorted(kernels) == sorted(want)
    src = open(os.path.join(B.CSRC, "sqllm_attn_decode.hip")).read()
    # one instantiation per group class: the shared ladder's, over the kernel this file's tag names
    ladder = open(os.path.join(B.CSRC, "sqllm_attn.h")).read()
    assert sorted(int(c) for c in re.findall(r"launch_attn_inst<TAG, D, (\d), OT>", ladder)) == list(CLASSES)
    assert "return sqllm_attn_decode_kernel<D, GC, OT>;" in src and "g_launch_attn[kAttnDecode] = launch_attn<AttnDecodeTag>" in src
    assert "template <int D, int GC, typename OT>\n__global__" in src  # head_dim, group class and output type only


@pytest.mark.parametrize("ot", TYPES)
@pytest.mark.parametrize("gc", CLASSES)
@pytest.mark.parametrize("d", DIMS)
def test_partials_no_scratch_no_spills_two_workgroups_per_cu(kernels, d, gc, ot):
    k = kernels[_partial(d, gc, ot)]
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, k
    assert 0 < k[".group_segment_fixed_size"] <= 64 * 1024
    # a workgroup is 4 waves, one per SIMD: two workgroups per CU need two waves per SIMD by registers, and two LDS images
    assert _occupancy_step(k[".vgpr_count"]) >= 2, k[".vgpr_count"]
    assert 2 * k[".group_segment_fixed_size"] <= 160 * 1024


@pytest.mark.parametrize("ot", TYPES)
@pytest.mark.parametrize("d", DIMS)
def test_combines_no_scratch_no_spills(kernels, d, ot):
    k = kernels[_combine(d, ot)]
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, k
    assert k[".group_segment_fixed_size"] == 0 and _occupancy_step(k[".vgpr_count"]) == 8
