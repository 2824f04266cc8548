"""Guards on the generated gfx950 code of the sliding-window decode attention's kernels (csrc/sqllm_attn_window.hip and
csrc/sqllm_attn_window_fp8.hip; hipcc cross-compiles without a GPU), read from the code objects' metadata: exactly the template
instances the shared ladder switches over (head_dim {64, 128} x group class {1, 2, 4, 8} x {fp16, bf16} partials per file, head_dim
x type combines in the 16-bit file only), no scratch, no spills, LDS within 64 KB and a register count that leaves room for at
least two workgroups per CU -- the standards of the kernels they are copies of."""
import os
import shutil

import pytest

from squeezellm_amd import build as B
from tests.test_codegen_qkv_rope_cpu import _meta, _occupancy_step

DIMS, CLASSES, TYPES = (64, 128), (1, 2, 4, 8), ("DF16_", "DF16b")  # DF16_ = _Float16, DF16b = __bf16 (Itanium mangling)
FILES = {"16": "sqllm_attn_window.hip", "fp8": "sqllm_attn_window_fp8.hip"}


def _partial(cache, d, gc, ot):
    if cache == "fp8":
        return f"_ZN5sqllm28sqllm_attn_window_fp8_kernelILi{d}ELi{gc}E{ot}EEvNS_14AttnWindowArgsEf"
    return f"_ZN5sqllm24sqllm_attn_window_kernelILi{d}ELi{gc}E{ot}EEvNS_14AttnWindowArgsE"


def _combine(d, ot):
    return f"_ZN5sqllm32sqllm_attn_window_combine_kernelILi{d}E{ot}EEvNS_14AttnWindowArgsE"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("asm_attn_window")
    return {cache: _meta(hipcc, src, tmp / f"{cache}.s") for cache, src in FILES.items()}


def test_the_sources_are_part_of_the_product_build():
    for src in FILES.values():
        assert src in B.SOURCES and B.SOURCES.index(src) < B.SOURCES.index("sqllm_capi.hip")
    assert B.SOURCES[-1] == "sqllm_capi.hip"


def test_exactly_the_expected_instances(kernels):
    for cache in FILES:
        want = [_partial(cache, d, gc, ot) for d in DIMS for gc in CLASSES for ot in TYPES]
        if cache == "16":
            want += [_combine(d, ot) for d in DIMS for ot in TYPES]
        assert sorted(kernels[cache]) == sorted(want), cache
    src = open(os.path.join(B.CSRC, FILES["16"])).read()
    assert "g_launch_attn_window[0] = launch_attn<AttnWindowTag>" in src and "g_launch_attn_window_combine = " in src
    src8 = open(os.path.join(B.CSRC, FILES["fp8"])).read()
    assert "g_launch_attn_window[1] = launch_attn<AttnWindowFp8Tag>" in src8 and "combine_kernel" not in src8


@pytest.mark.parametrize("ot", TYPES)
@pytest.mark.parametrize("gc", CLASSES)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("cache", list(FILES))
def test_partials_no_scratch_no_spills_two_workgroups_per_cu(kernels, cache, d, gc, ot):
    k = kernels[cache][_partial(cache, d, gc, ot)]
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, k
    assert 0 < k[".group_segment_fixed_size"] <= 64 * 1024
    # a workgroup is 4 waves, one per SIMD: two workgroups per CU need two waves per SIMD by registers, and two LDS images
    assert _occupancy_step(k[".vgpr_count"]) >= 2, k[".vgpr_count"]
    assert 2 * k[".group_segment_fixed_size"] <= 160 * 1024


@pytest.mark.parametrize("ot", TYPES)
@pytest.mark.parametrize("d", DIMS)
def test_combines_no_scratch_no_spills(kernels, d, ot):
    k = kernels["16"][_combine(d, ot)]
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, k
    assert k[".group_segment_fixed_size"] == 0 and _occupancy_step(k[".vgpr_count"]) == 8
