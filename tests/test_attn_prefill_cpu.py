"""The prefill attention (sqllm_attn_prefill_*, quant.PrefillAttention) without a GPU: the ABI, the rejections in their order (fake
pointers), the torch route against the oracle, and the fairness of the GPU cases to an fp32 model in the kernel's structure."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import attn_append_cases as A
from tests import attn_decode_cases as C
from tests import attn_prefill_cases as PC
from tests import test_attn_append_capi_cpu as TA

E_SHAPE, E_NULL, E_ALIGN, E_OPTION = TA.E_SHAPE, TA.E_NULL, TA.E_ALIGN, TA.E_OPTION
ENTRIES = ("sqllm_attn_prefill_f16", "sqllm_attn_prefill_bf16")
Q, OUT, WS, QLENS = TA.Q, TA.OUT, TA.WS, TA.QLENS


@pytest.fixture(scope="module")
def lib():
    from squeezellm_amd import _lib

    return _lib.load()


def test_symbols_signatures_header_text_and_sources(lib):
    from squeezellm_amd import _lib, quant
    from squeezellm_amd import build as B

    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "sqllm_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and f"int {name}(const sqllm_attn_append* a, sqllm_stream_t stream);" in header
        assert _lib.SIGNATURES[name] == [ctypes.POINTER(_lib.SqllmAttnAppend), ctypes.c_void_p] and getattr(lib, name).restype is ctypes.c_int
    assert lib.sqllm_abi_version() == 1
    block = header[header.index("PREFILL attention over the paged KV cache"):header.index("int sqllm_attn_prefill_f16(")]
    for text in ("L(b,t) = seq_lens[b] - (n_b - 1 - t)", "NOT\n *     THE BITS of the one-query entry", "[64 i, 64 i + 64)", "NO WORKSPACE", "may be NULL",
                 "ONE kernel node", "makes NaN only the tokens with L > p", "n_b < 0 counts as 0", "WEAKER", "NON-FINITE v[p,d]", "0 * NaN",
                 "the mask is a select", "q_len 1 to 65536; batch 1 to 65535", "hipErrorNotSupported", "fp8 caches", "a sliding window",
                 "attention sinks, ALiBi and soft-capping", "splitting one long sequence's keys", "routing sqllm_attn_decode_*"):
        assert text in block, text
    assert "sqllm_attn_prefill.hip" in B.SOURCES and B.SOURCES.index("sqllm_attn_prefill.hip") < B.SOURCES.index("sqllm_capi.hip")
    assert B.SOURCES[-1] == "sqllm_capi.hip"
    kernels_h = open(os.path.join(B.CSRC, "sqllm_kernels.h")).read()
    assert "extern AttnLauncher g_launch_attn_prefill;" in kernels_h and "kAttnAppendFp8, kAttnKinds };" in kernels_h  # a slot of its own
    assert issubclass(quant.PrefillAttention, quant.DecodeAttention) and callable(quant.fuse_prefill_attention)


@pytest.mark.parametrize("entry", ENTRIES)
def test_rejections_before_the_device_is_touched_in_order(lib, entry):
    fn = getattr(lib, entry)

    def rc(**kw):
        return fn(ctypes.byref(TA._desc(False, **kw)), None)

    # (nothing here may reach a launch: every call below carries at least one defect)
    assert fn(None, None) == E_NULL
    for name in ("q", "out", "k_cache", "v_cache", "block_table", "seq_lens"):
        assert rc(**{name: None}) == E_NULL, name
        assert rc(**{name: None, "batch": 0, "q_len": 0, "scale": float("nan")}) == E_NULL  # NULL comes first
    nan = float("nan")
    assert rc(workspace=None, scale=nan) == E_OPTION and rc(q_lens=None, workspace=None, scale=nan) == E_OPTION  # both may be NULL
    for name in ("batch", "n_q_heads", "n_kv_heads", "head_dim", "n_slots", "block_size", "max_blocks", "table_stride", "q_len"):
        for v in (0, -1):
            assert rc(**{name: v, "scale": float("inf"), "out": Q, "q": Q + 1}) == E_SHAPE, name  # before the scale, the overlap, the alignment
    assert rc(slot_stride=63) == E_SHAPE and rc(head_stride=63) == E_SHAPE and rc(q_stride=255) == E_SHAPE and rc(out_stride=255) == E_SHAPE
    assert rc(max_blocks=5) == E_SHAPE and rc(max_blocks=5, table_stride=5, scale=nan) == E_OPTION
    # what the kernel serves: the append entries' shapes with the two new limits
    for kw in (dict(head_dim=32, q_stride=128, out_stride=128), dict(n_q_heads=3, n_kv_heads=2), dict(n_q_heads=18, n_kv_heads=2, q_stride=18 * 64, out_stride=18 * 64),
               dict(q_len=65537, batch=1), dict(q_len=1, batch=65536), dict(q_len=(1 << 31) - 1, batch=(1 << 31) - 1)):
        assert rc(scale=nan, **kw) == E_SHAPE, kw
    for kw in (dict(q_len=17, batch=1), dict(q_len=16, batch=5), dict(q_len=1, batch=65), dict(q_len=65536, batch=1), dict(q_len=1, batch=65535),
               dict(q_len=65536, batch=65535), dict(n_q_heads=16, n_kv_heads=2, q_stride=1024, out_stride=1024), dict(block_size=5)):
        assert rc(scale=nan, workspace=None, **kw) == E_OPTION, kw  # served: the call gets as far as the scale
    far = dict(k_cache=0x10000000000, v_cache=0x7000000000000)
    assert rc(slot_stride=(1 << 32) - 1, scale=nan, **far) == E_OPTION and rc(slot_stride=1 << 32, scale=nan, **far) == E_SHAPE
    assert rc(q_stride=1 << 62, scale=nan) == E_SHAPE and rc(out_stride=1 << 62, scale=nan) == E_SHAPE
    for v in (nan, float("inf")):
        assert rc(scale=v, out=Q, q=Q + 1) == E_OPTION  # before the overlap and the alignment
    # overlaps name out only (4 rows of 256 elements: 2048 bytes); an unaligned q stands behind them
    cache = 2 * (127 * 128 + 64 + 64)
    for name, (at, size) in {"q": (Q, 2048), "k_cache": (TA.K_CACHE, cache), "v_cache": (TA.V_CACHE, cache), "block_table": (TA.TABLE, 32),
                             "seq_lens": (TA.LENS, 8), "q_lens": (QLENS, 8)}.items():
        q_odd = {} if name == "q" else {"q": Q + 1}
        assert rc(out=at) == E_SHAPE and rc(out=at + size - 2, **q_odd) == E_SHAPE and rc(out=at - 2046, **q_odd) == E_SHAPE, name
        if q_odd:
            assert rc(out=at + size + size % 2, **q_odd) == E_ALIGN and rc(workspace=at, **q_odd) == E_ALIGN, name  # adjacent; a workspace anywhere
    assert rc(out=WS, q=Q + 1) == E_ALIGN and rc(workspace=OUT, q=Q + 1) == E_ALIGN and rc(workspace=WS + 1, q=Q + 1) == E_ALIGN
    for name in ("q", "out", "k_cache", "v_cache"):
        assert rc(**{name: getattr(TA._desc(), name) + 1}) == E_ALIGN, name


@pytest.mark.parametrize("kind,T,D,hq,hk,dt", [PC.CASES[2], PC.CASES[4]])
def test_the_module_on_cpu_tensors_against_the_oracle(kind, T, D, hq, hk, dt):
    from squeezellm_amd import quant

    seqs, ql = PC.calls(T)[1]
    base, case, want, gate = A.reference(kind, T, D, hq, hk, dt, seqs, ql)
    att = quant.PrefillAttention(hq, hk, D, block_size=base.block_size)
    k, v = (C.cache_view(base, t) for t in (base.k_buf, base.v_buf))
    y = att(case.q_buf[:, :hq * D], k, v, torch.from_numpy(base.table).to(torch.int32), torch.from_numpy(base.lens).to(torch.int32), T,
            q_lens=torch.tensor(ql, dtype=torch.int32))
    assert att.last_route == "fallback" and y.shape == (len(seqs) * T, hq * D) and y.dtype == case.dtype
    assert C.excess(y.double().numpy(), want, gate) <= 1.0


def model_tiles(case):
    """[B, HQ * D] fp32 in the kernel's structure: key tiles of 64, online softmax, the weights as three 16-bit planes (fp16: of w * 2^15)"""
    f = np.float32
    fp16 = case.dtype == torch.float16

    def planes(w):
        if fp16:
            x = w * f(32768.0)
            h = x.astype(np.float16).astype(f)
            m = (x - h).astype(np.float16).astype(f)
            return h, m, (x - h - m).astype(np.float16).astype(f), f(32768.0)
        h = (w.view(np.uint32) & np.uint32(0xFFFF0000)).view(f)
        m = ((w - h).view(np.uint32) & np.uint32(0xFFFF0000)).view(f)
        return h, m, w - h - m, f(1.0)

    def fn(q, k, v):
        q, k, v = q.astype(f), k.astype(f), v.astype(f)
        s = f(case.scale) * (q @ k.T)
        m, l, acc = np.full(len(q), -np.inf, f), np.zeros(len(q), f), np.zeros((len(q), v.shape[1]), f)
        for i in range(0, s.shape[1], 64):
            sp = s[:, i:i + 64]
            m_new = np.maximum(m, sp.max(axis=1))
            alpha, w = np.exp(m - m_new).astype(f), np.exp(sp - m_new[:, None]).astype(f)
            h, mid, lo, c = planes(w)
            acc = acc * alpha[:, None] + ((lo @ v[i:i + 64] + mid @ v[i:i + 64]) + h @ v[i:i + 64])
            l, m = l * alpha + w.sum(axis=1, dtype=f), m_new
        return acc / (l * c)[:, None]

    return C._walk(case, fn, f)[0].reshape(case.B, -1)


@pytest.mark.parametrize("kind,T,D,hq,hk,dt", PC.CASES)
def test_the_cases_are_fair_to_an_fp32_model_in_the_kernels_structure(kind, T, D, hq, hk, dt):
    """the condition on the INPUTS: if a case fails here, the case changes, not the gate"""
    for seqs, ql in PC.calls(T):
        base, case, want, gate = A.reference(kind, T, D, hq, hk, dt, seqs, ql)
        worst = C.excess(C.rounded(model_tiles(case), case.dtype), want, gate)
        print(f"PREFILL_MODEL {kind} T={T} D={D} heads={hq}/{hk} {dt} q_lens={ql}: {worst:.3f}")
        assert worst <= 1.0, (ql, worst)
