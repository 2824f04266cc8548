"""The prefill attention over an fp8 KV cache (sqllm_attn_prefill_fp8_*) without a GPU: the ABI, the rejections in their order (fake
pointers), and the fairness of the GPU cases to an fp32 model in the kernel's structure over the bytes' exact values."""
import copy
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import attn_append_cases as A
from tests import attn_decode_cases as C
from tests import attn_prefill_cases as PC
from tests import kv_fp8_cases as F
from tests import test_attn_append_capi_cpu as TA
from tests.test_attn_prefill_cpu import model_tiles

E_SHAPE, E_NULL, E_ALIGN, E_OPTION = TA.E_SHAPE, TA.E_NULL, TA.E_ALIGN, TA.E_OPTION
ENTRIES = ("sqllm_attn_prefill_fp8_f16", "sqllm_attn_prefill_fp8_bf16")
# every case of the 16-bit entries with the power-of-two scales, and one fp16 and one bf16 case with scales that round
CASES = [(*c, F.SCALES) for c in PC.CASES] + [(*PC.CASES[3], F.ODD_SCALES), (*PC.CASES[5], F.ODD_SCALES)]


@functools.lru_cache(maxsize=None)
def reference(kind, T, D, hq, hk, dt, scales, seqs, ql):
    """(fp8 case, expansion, want, gate): the fp64 oracle over the dequantised bytes and its gate, computed once and shared"""
    fc = F.fp8_case(kind, len(seqs), D, hq, hk, dt, scales, 0, seqs)
    return (fc, A.expand(fc.case, T, ql), *C.reference_of(A.expand(fc.shadow, T, ql)))


@pytest.fixture(scope="module")
def lib():
    from squeezellm_amd import _lib
    return _lib.load()


def test_symbols_signatures_header_text_and_sources(lib):
    from squeezellm_amd import _lib
    from squeezellm_amd import build as B

    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "sqllm_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and f"int {name}(const sqllm_attn_append_fp8* a, sqllm_stream_t stream);" in header
        assert _lib.SIGNATURES[name] == [ctypes.POINTER(_lib.SqllmAttnAppendFp8), ctypes.c_void_p] and getattr(lib, name).restype is ctypes.c_int
    assert lib.sqllm_abi_version() == 1
    block = header[header.index("PREFILL attention over the fp8 KV cache"):header.index("int sqllm_attn_prefill_fp8_f16(")]
    assert header.index("int sqllm_attn_prefill_bf16(") < header.index("PREFILL attention over the fp8 KV cache")
    for text in ("float(k) = k_scale * f32(byte)", "float(v) = v_scale * f32(byte)", "count BYTES", "ONCE per element", "0x7f and 0xff are NaN",
                 "NOT THE BITS", "NO WORKSPACE", "may be NULL", "ONE kernel node", "WEAKER", "NaN BYTE of v", "LAST (SQLLM_E_OPTION)",
                 "q_len 1 to 65536; batch 1 to 65535", "hipErrorNotSupported", "a sliding window", "per-head or per-token scales"):
        assert text in block, text
    fp8, plain, capi = (B.SOURCES.index(s) for s in ("sqllm_attn_prefill_fp8.hip", "sqllm_attn_prefill.hip", "sqllm_capi.hip"))
    assert plain < fp8 < capi and B.SOURCES[-1] == "sqllm_capi.hip" and "sqllm_attn_prefill_fp8.hip" in B.NO_PACKED_FP32
    assert os.path.join(B.CSRC, "sqllm_attn_prefill.h") in B.HEADERS  # (a changed header makes the library stale)
    assert "extern AttnLauncher g_launch_attn_prefill_fp8;" in open(os.path.join(B.CSRC, "sqllm_kernels.h")).read()


@pytest.mark.parametrize("entry", ENTRIES)
def test_rejections_before_the_device_is_touched_in_order(lib, entry):
    fn, Q, nan = getattr(lib, entry), TA.Q, float("nan")
    rc = lambda **kw: fn(ctypes.byref(TA._desc(True, **kw)), None)  # noqa: E731 (nothing below may reach a launch: every call carries a defect)
    assert fn(None, None) == E_NULL
    for name in ("q", "out", "k_cache", "v_cache", "block_table", "seq_lens"):
        assert rc(**{name: None, "batch": 0, "q_len": 0, "scale": nan, "k_scale": 0.0}) == E_NULL, name  # NULL comes first
    assert rc(workspace=None, scale=nan) == E_OPTION and rc(q_lens=None, workspace=None, scale=nan) == E_OPTION  # both may be NULL
    for name in ("batch", "n_q_heads", "n_kv_heads", "head_dim", "n_slots", "block_size", "max_blocks", "table_stride", "q_len"):
        assert rc(**{name: 0, "scale": float("inf"), "out": Q, "q": Q + 1, "v_scale": nan}) == E_SHAPE, name  # shapes: before all that follows
    assert rc(slot_stride=63) == E_SHAPE and rc(head_stride=63) == E_SHAPE and rc(q_stride=255) == E_SHAPE and rc(max_blocks=5) == E_SHAPE
    # the two prefill limits stand where the append entries' stood
    for kw in (dict(q_len=65537, batch=1), dict(q_len=1, batch=65536), dict(head_dim=32, q_stride=128, out_stride=128), dict(n_q_heads=18, q_stride=18 * 64, out_stride=18 * 64)):
        assert rc(scale=nan, **kw) == E_SHAPE, kw
    for kw in (dict(q_len=17, batch=1), dict(q_len=1, batch=65), dict(q_len=65536, batch=65535), dict(block_size=5)):
        assert rc(scale=nan, workspace=None, **kw) == E_OPTION, kw  # served: the call gets as far as the scale
    assert rc(scale=float("inf"), out=Q, q=Q + 1, k_scale=0.0) == E_OPTION  # the finite scale: before the overlap and the alignment
    # overlaps name out only (4 rows of 256 elements: 2048 bytes), against extents in BYTES for the caches; an odd q stands behind them
    cache = 127 * 128 + 64 + 64
    for name, (at, size) in {"k_cache": (TA.K_CACHE, cache), "v_cache": (TA.V_CACHE, cache), "q_lens": (TA.QLENS, 8)}.items():
        assert rc(out=at, q=Q + 1) == E_SHAPE and rc(out=at + size - 2, q=Q + 1) == E_SHAPE and rc(out=at - 2046, q=Q + 1) == E_SHAPE, name
        assert rc(out=at + size + size % 2, q=Q + 1) == E_ALIGN and rc(workspace=at, q=Q + 1) == E_ALIGN, name  # adjacent; a workspace anywhere
    assert rc(q=Q + 1, k_scale=0.0) == E_ALIGN and rc(out=TA.OUT + 1, v_scale=nan) == E_ALIGN and rc(workspace=TA.WS + 1, q=Q + 1) == E_ALIGN
    # a cache at an odd address is admitted: the scales speak, last
    assert rc(k_cache=TA.K_CACHE + 1, v_cache=TA.V_CACHE + 3, k_scale=0.0, workspace=None) == E_OPTION
    for s in (0.0, -1.0, nan, float("inf"), 1e-39):
        assert rc(k_scale=s, workspace=None) == E_OPTION and rc(v_scale=s, workspace=None) == E_OPTION, s
    assert rc(scale=3e38, k_scale=16.0) == E_OPTION  # scale * k_scale overflows fp32


@pytest.mark.parametrize("kind,T,D,hq,hk,dt,scales", CASES)
def test_the_cases_are_fair_to_an_fp32_model_in_the_kernels_structure(kind, T, D, hq, hk, dt, scales):
    """a condition on the INPUTS: that model on the bytes' exact values, scale * k_scale rounded once in fp32, the result times v_scale in
    fp32, rounded once.  If a case fails here, the case changes, not the gate"""
    f = np.float32
    for seqs, ql in PC.calls(T):
        fc, case, want, gate = reference(kind, T, D, hq, hk, dt, scales, seqs, ql)
        exact = copy.copy(case)
        exact.k_buf, exact.v_buf = F.decode(fc.k_bytes), F.decode(fc.v_bytes)
        exact.scale = float(f(case.scale) * f(fc.k_scale))
        worst = C.excess(C.rounded(model_tiles(exact) * f(fc.v_scale), case.dtype), want, gate)
        print(f"PREFILL_FP8_MODEL {kind} T={T} D={D} heads={hq}/{hk} {dt} scales={scales} q_lens={ql}: {worst:.3f}")
        assert worst <= 1.0, (ql, worst)
