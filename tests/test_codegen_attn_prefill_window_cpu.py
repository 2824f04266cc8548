"""Guards on the generated gfx950 code of the sliding-window prefill attention's kernels (csrc/sqllm_attn_prefill_window.hip and
csrc/sqllm_attn_prefill_window_fp8.hip; hipcc cross-compiles without a GPU), read from the code objects' metadata: exactly the
instances head_dim {64, 128} x {fp16, bf16} per file, no scratch, no spills, and registers and LDS that leave room for two
workgroups per CU -- the standards of the prefill kernels they are copies of."""
import os
import shutil

import pytest

from tests.test_codegen_qkv_rope_cpu import _meta, _occupancy_step

DIMS, TYPES = (64, 128), ("DF16_", "DF16b")  # DF16_ = _Float16, DF16b = __bf16 (Itanium mangling)
FILES = {"16": "sqllm_attn_prefill_window.hip", "fp8": "sqllm_attn_prefill_window_fp8.hip"}


def _name(cache, d, ot):
    if cache == "fp8":
        return f"_ZN5sqllm36sqllm_attn_prefill_window_fp8_kernelILi{d}E{ot}EEvNS_21AttnPrefillWindowArgsEf"
    return f"_ZN5sqllm32sqllm_attn_prefill_window_kernelILi{d}E{ot}EEvNS_21AttnPrefillWindowArgsE"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("asm_attn_prefill_window")
    return {cache: _meta(hipcc, src, tmp / f"{cache}.s") for cache, src in FILES.items()}


@pytest.mark.parametrize("cache", list(FILES))
def test_exactly_the_expected_instances(kernels, cache):
    assert sorted(kernels[cache]) == sorted(_name(cache, d, ot) for d in DIMS for ot in TYPES)


@pytest.mark.parametrize("ot", TYPES)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("cache", list(FILES))
def test_no_scratch_no_spills_two_workgroups_per_cu(kernels, cache, d, ot):
    k = kernels[cache][_name(cache, d, ot)]
    print(f"PREFILL_WINDOW_CODEGEN {cache} D={d} {ot}: vgpr {k['.vgpr_count']} lds {k['.group_segment_fixed_size']}")
    assert k[".private_segment_fixed_size"] == 0 and k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, k
    # a workgroup is 4 waves, one per SIMD: two workgroups per CU need two waves per SIMD by registers, and two LDS images
    assert _occupancy_step(k[".vgpr_count"]) >= 2, k[".vgpr_count"]
    assert 0 < 2 * k[".group_segment_fixed_size"] <= 160 * 1024
