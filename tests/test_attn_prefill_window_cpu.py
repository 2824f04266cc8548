"""The sliding-window prefill attention (sqllm_attn_prefill_window_*, quant.PrefillAttention(window=)) without a GPU: the ABI, the
rejections in their order (fake pointers), the torch route against the oracle, the fairness of the GPU cases to an fp32 model in
the kernel's structure, and ring_block_table's default.  `reference` is shared with the GPU tests."""
import copy
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import attn_append_cases as A
from tests import attn_decode_cases as C
from tests import attn_prefill_window_cases as WPC
from tests import attn_window_cases as WC
from tests import kv_fp8_cases as F
from tests import test_attn_append_capi_cpu as TA

E_SHAPE, E_NULL, E_ALIGN, E_OPTION = TA.E_SHAPE, TA.E_NULL, TA.E_ALIGN, TA.E_OPTION
ENTRIES = {False: ("sqllm_attn_prefill_window_f16", "sqllm_attn_prefill_window_bf16"),
           True: ("sqllm_attn_prefill_window_fp8_f16", "sqllm_attn_prefill_window_fp8_bf16")}
CACHES = ("16", "fp8")


def poisoned(base, T, ql, W):
    """attn_window_cases.windowed's poison per SEQUENCE: K / V of the keys below the least lo of the sequence's tokens hold the NaN
    pattern, the table entries of blocks wholly below it 1 << 30 / -7 (a deep copy: the cached case is not touched)"""
    out = copy.deepcopy(base)
    bs, cap = base.block_size, base.table.shape[1] * base.block_size
    L = A.token_lengths(base.lens, T, ql, cap).reshape(base.B, T)
    hd = np.arange(base.H)[None, :, None] * base.head_stride + np.arange(base.D)[None, None, :]
    for b in range(base.B):
        lo = min((WC.lo_of(n, W) for n in L[b] if 0 < n <= cap), default=0)
        p = np.arange(lo)
        slot = base.table[b, p // bs] * bs + p % bs
        at = torch.from_numpy((C.GUARD + slot[:, None, None] * base.slot_stride + hd).reshape(-1))
        out.k_buf[at] = out.v_buf[at] = C._poisoned(at.numel(), base.dtype, 0)
        for j in range(lo // bs):
            out.table[b, j] = -7 if j % 2 else 1 << 30
    return out


@functools.lru_cache(maxsize=None)
def reference(kind, T, D, hq, hk, dt, seq_len, W, ql, fp8=False):
    """(base, fp8 namespace or None, expansion, want, gate): the poisoned sequences, their expansion with .window, and
    attn_window_cases.reference_w over it (fp8: over the dequantised bytes) -- computed once and shared"""
    seqs = WPC.calls(T, seq_len)[0][0]
    base = poisoned(C.build(kind, len(seqs), D, hq, hk, dt, 0, seqs), T, ql, W)
    fc = F.quantise(base) if fp8 else None
    case, shadow = A.expand(base, T, ql), A.expand(fc.shadow if fp8 else base, T, ql)
    case.window = shadow.window = W
    return (base, fc, case, *WC.reference_w(shadow))


def model_tiles_w(case):
    """tests/test_attn_prefill_cpu.model_tiles over [lo, L) with ABSOLUTE tile edges (multiples of 64: the first tile is partial
    where lo is no multiple of 64): fp32, online softmax, the weights as three 16-bit planes (fp16: of w * 2^15)"""
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

    def fn(q, k, v, first):
        q, k, v = q.astype(f), k.astype(f), v.astype(f)
        s = f(case.scale) * (q @ k.T)
        n = s.shape[1]
        edges = [0] + [e - first for e in range((first // 64 + 1) * 64, first + n, 64)] + [n]
        m, l, acc = np.full(len(q), -np.inf, f), np.zeros(len(q), f), np.zeros((len(q), v.shape[1]), f)
        for i, j in zip(edges[:-1], edges[1:]):
            sp = s[:, i:j]
            m_new = np.maximum(m, sp.max(axis=1))
            alpha, w = np.exp(m - m_new).astype(f), np.exp(sp - m_new[:, None]).astype(f)
            h, mid, lo, c = planes(w)
            acc = acc * alpha[:, None] + ((lo @ v[i:j] + mid @ v[i:j]) + h @ v[i:j])
            l, m = l * alpha + w.sum(axis=1, dtype=f), m_new
        return acc / (l * c)[:, None]

    return WC._walk_w(case, fn, f)[0].reshape(case.B, -1)


@pytest.fixture(scope="module")
def lib():
    from squeezellm_amd import _lib
    return _lib.load()


def test_symbols_signatures_header_text_and_sources(lib):
    from squeezellm_amd import _lib, quant
    from squeezellm_amd import build as B

    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "sqllm_hip.h")).read()
    for fp8, names in ENTRIES.items():
        struct = _lib.SqllmAttnAppendFp8 if fp8 else _lib.SqllmAttnAppend
        for name in names:
            assert hasattr(lib, name) and f"int {name}(const {'sqllm_attn_append_fp8' if fp8 else 'sqllm_attn_append'}* a, int32_t window, sqllm_stream_t stream);" in header
            assert _lib.SIGNATURES[name] == [ctypes.POINTER(struct), ctypes.c_int32, ctypes.c_void_p] and getattr(lib, name).restype is ctypes.c_int
    assert lib.sqllm_abi_version() == 1
    start = header.index("SLIDING-WINDOW prefill attention")
    assert header.index("int sqllm_attn_prefill_fp8_bf16(") < start
    block = header[start:header.index("int sqllm_attn_prefill_window_f16(")]
    for text in ("kv_idx > q_idx - sliding_window", "lo = max(0, L - window)", "[64 i, 64 i + 64)", "BIT FOR BIT on finite caches", "L(b,t) <= window",
                 "multiple of both 64 and block_size", "q_len = 1 and seq_lens = L - lo", "NEVER READ", "EXACTLY the rows with lo(b,t) <= p < L(b,t)",
                 "WEAKER", "[64 * (lo_min / 64), lmax)", "NO WORKSPACE", "ONE kernel node", "window < 1 stands among the counts (SQLLM_E_SHAPE)",
                 "hipErrorNotSupported, never with another kernel"):
        assert text in block, text
    src16, src8, capi = (B.SOURCES.index(s) for s in ("sqllm_attn_prefill_window.hip", "sqllm_attn_prefill_window_fp8.hip", "sqllm_capi.hip"))
    assert B.SOURCES.index("sqllm_attn_prefill_fp8.hip") < src16 < src8 < capi and B.SOURCES[-1] == "sqllm_capi.hip"
    assert {"sqllm_attn_prefill_window.hip", "sqllm_attn_prefill_window_fp8.hip"} <= set(B.NO_PACKED_FP32)
    kernels_h = open(os.path.join(B.CSRC, "sqllm_kernels.h")).read()
    assert "extern AttnLauncher g_launch_attn_prefill_window[2];" in kernels_h and "kAttnAppendFp8, kAttnKinds };" in kernels_h
    assert "!c.window" in open(os.path.join(B.CSRC, "sqllm_attn_prefill.h")).read().split("inline bool prefill_served")[1].split("}")[0]
    att = quant.PrefillAttention(8, 2, 64, window=7)
    assert att.window == 7 and quant.PrefillAttention(8, 2, 64).window is None
    for bad in (0, -1, 1 << 31, 2.0, True):
        with pytest.raises(ValueError):
            quant.PrefillAttention(8, 2, 64, window=bad)


@pytest.mark.parametrize("fp8", (False, True))
@pytest.mark.parametrize("bf16", (0, 1))
def test_rejections_before_the_device_is_touched_in_order(lib, fp8, bf16):
    fn, Q, nan = getattr(lib, ENTRIES[fp8][bf16]), TA.Q, float("nan")
    rc = lambda window=4, **kw: fn(ctypes.byref(TA._desc(fp8, **kw)), window, None)  # noqa: E731 (every call below carries a defect)
    assert fn(None, 4, None) == E_NULL and fn(None, 0, None) == E_NULL
    for name in ("q", "out", "k_cache", "v_cache", "block_table", "seq_lens"):
        assert rc(0, **{name: None, "batch": 0, "scale": nan}) == E_NULL, name  # NULL comes first
    for w in (0, -1, -(1 << 31)):
        assert rc(w, scale=float("inf"), out=Q, q=Q + 1, workspace=None) == E_SHAPE, w  # a count: before the scale, the overlap, the alignment
    assert rc((1 << 31) - 1, scale=nan, workspace=None, q_lens=None) == E_OPTION  # served: the call gets as far as the scale
    for name in ("batch", "n_q_heads", "n_kv_heads", "head_dim", "n_slots", "block_size", "max_blocks", "table_stride", "q_len"):
        assert rc(**{name: 0, "scale": float("inf"), "out": Q, "q": Q + 1}) == E_SHAPE, name
    assert rc(slot_stride=63) == E_SHAPE and rc(head_stride=63) == E_SHAPE and rc(q_stride=255) == E_SHAPE and rc(max_blocks=5) == E_SHAPE
    for kw in (dict(q_len=65537, batch=1), dict(q_len=1, batch=65536), dict(head_dim=32, q_stride=128, out_stride=128), dict(n_q_heads=18, q_stride=18 * 64, out_stride=18 * 64)):
        assert rc(scale=nan, **kw) == E_SHAPE, kw
    for kw in (dict(q_len=17, batch=1), dict(q_len=1, batch=65), dict(q_len=65536, batch=65535), dict(block_size=5)):
        assert rc(scale=nan, workspace=None, **kw) == E_OPTION, kw  # the prefill limits, not the append entries'
    assert rc(scale=float("inf"), out=Q, q=Q + 1) == E_OPTION  # the finite scale: before the overlap and the alignment
    assert rc(out=TA.K_CACHE, q=Q + 1) == E_SHAPE and rc(out=TA.QLENS, q=Q + 1) == E_SHAPE  # overlaps name out only
    assert rc(workspace=TA.K_CACHE, q=Q + 1) == E_ALIGN and rc(workspace=TA.WS + 1, q=Q + 1) == E_ALIGN and rc(out=TA.OUT + 1) == E_ALIGN
    if fp8:  # a cache at an odd address is admitted: the scales speak, last
        assert rc(k_cache=TA.K_CACHE + 1, k_scale=0.0, workspace=None) == E_OPTION and rc(v_scale=nan) == E_OPTION
    else:
        assert rc(k_cache=TA.K_CACHE + 1) == E_ALIGN and rc(v_cache=TA.V_CACHE + 1) == E_ALIGN


@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("kind,T,D,hq,hk,dt,seq_len,W", [WPC.CASES[0], WPC.CASES[3]])
def test_the_module_on_cpu_tensors_against_the_oracle(kind, T, D, hq, hk, dt, seq_len, W, cache):
    from squeezellm_amd import quant

    seqs, ql = WPC.calls(T, seq_len)[1]
    base, fc, case, want, gate = reference(kind, T, D, hq, hk, dt, seq_len, W, ql, cache == "fp8")
    att = quant.PrefillAttention(hq, hk, D, block_size=base.block_size, window=W)
    k, v = ((F.cache_view(fc, t) for t in (fc.k_bytes, fc.v_bytes)) if fc else (C.cache_view(base, t) for t in (base.k_buf, base.v_buf)))
    kw = dict(k_scale=fc.k_scale, v_scale=fc.v_scale) if fc else {}
    y = att(case.q_buf[:, :hq * D], k, v, torch.from_numpy(base.table).to(torch.int32), torch.from_numpy(base.lens).to(torch.int32), T,
            q_lens=torch.tensor(ql, dtype=torch.int32), **kw)
    assert att.last_route == "fallback" and y.shape == (len(seqs) * T, hq * D) and y.dtype == case.dtype
    assert C.excess(y.double().numpy(), want, gate) <= 1.0


@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("kind,T,D,hq,hk,dt,seq_len,W", WPC.CASES)
def test_the_cases_are_fair_to_an_fp32_model_in_the_kernels_structure(kind, T, D, hq, hk, dt, seq_len, W, cache):
    """the condition on the INPUTS (fp8: the model on the bytes' exact values, scale * k_scale rounded once, the result times v_scale in
    fp32, as tests/test_attn_prefill_fp8_cpu.py): if a case fails here, the case changes, not the gate"""
    f = np.float32
    for seqs, ql in WPC.calls(T, seq_len):
        base, fc, case, want, gate = reference(kind, T, D, hq, hk, dt, seq_len, W, ql, cache == "fp8")
        exact, post = case, f(1.0)
        if fc:
            exact, post = copy.copy(case), f(fc.v_scale)
            exact.k_buf, exact.v_buf, exact.scale = F.decode(fc.k_bytes), F.decode(fc.v_bytes), float(f(case.scale) * f(fc.k_scale))
        worst = C.excess(C.rounded(model_tiles_w(exact) * post, case.dtype), want, gate)
        print(f"PREFILL_WINDOW_MODEL {kind} T={T} D={D} heads={hq}/{hk} {dt} seq={seq_len} W={W} {cache} q_lens={ql}: {worst:.3f}")
        assert worst <= 1.0, (ql, worst)


def test_ring_block_table_default_q_len_is_todays_table_and_fuse_passes_the_window():
    from squeezellm_amd import quant

    for W, bs in ((40, 16), (7, 5), (1, 4)):
        R = -(-W // bs) + 1
        t = quant.ring_block_table(2, W, bs, 3 * R * bs)
        assert torch.equal(t, quant.ring_block_table(2, W, bs, 3 * R * bs, None, 1)) and int(t.max()) == 2 * R - 1
        assert int(quant.ring_block_table(1, W, bs, 400, q_len=33).max()) == -(-(W + 32) // bs)
    with pytest.raises(ValueError):
        quant.ring_block_table(1, 4, 4, 4, q_len=0)
    front = quant.QuantQKVRopeFused.__new__(quant.QuantQKVRopeFused)
    torch.nn.Module.__init__(front)
    front.__dict__.update(head_dim=64, q=type("M", (), {"outfeatures": 512})(), k=type("M", (), {"outfeatures": 128})())
    holder = torch.nn.Module()
    holder.__dict__["qkv_rope"] = front
    assert quant.fuse_prefill_attention(holder, window=4096) == 1 and holder.attend_prefill.window == 4096
    assert quant.fuse_prefill_attention(holder) == 1 and holder.attend_prefill.window is None
