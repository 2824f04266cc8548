"""The prefill attention over an fp8 KV cache on the GPU (quant.PrefillAttention(..., k_scale=, v_scale=), sqllm_attn_prefill_fp8_*):
tests/attn_prefill_cases.py quantised by tests/kv_fp8_cases.py, against the fp64 oracle over the dequantised bytes under the gate."""
import copy
import ctypes
import types

import numpy as np
import pytest

from tests import attn_append_cases as A
from tests import attn_decode_cases as C
from tests import attn_prefill_cases as PC
from tests import kv_fp8_cases as F
from tests.test_attn_prefill_fp8_cpu import CASES, reference
from tests.test_gpu_attn_append import Dev
from tests.test_gpu_attn_decode import _bits, _f64, _node_types, _poison_lds
from tests.test_gpu_attn_prefill import _module


def _prefill(d, att=None, seqs=slice(None), out=None):
    att = att or _module(d.base)
    b0, b1, _ = seqs.indices(d.base.B)
    ql = None if d.q_lens is None else d.q_lens[seqs]
    y = att(d.q[b0 * d.T:b1 * d.T], d.k, d.v, d.table[seqs], d.seq[seqs], d.T, q_lens=ql, out=out, **d.kw)
    assert att.last_route == "attn_prefill"
    return y


def _dev(gpu, kind, T, D, hq, hk, dt, seqs, ql, poison=0):
    fc = F.fp8_case(kind, len(seqs), D, hq, hk, dt, F.SCALES, poison, seqs)
    return Dev(gpu, fc.case, A.expand(fc.case, T, ql, poison), fc)


def _c_entry(d):
    """the same call through the C entry directly, with a NULL workspace"""
    import torch
    from squeezellm_amd import _lib
    base, W = d.base, d.base.HQ * d.base.D
    out = torch.full((base.B * d.T, W), 7.0, dtype=base.dtype, device=d.q.device)
    a = _lib.SqllmAttnAppendFp8()
    a.q, a.out, a.k_cache, a.v_cache, a.workspace = d.q.data_ptr(), out.data_ptr(), d.k.data_ptr(), d.v.data_ptr(), None
    a.block_table, a.seq_lens, a.q_lens = d.table.data_ptr(), d.seq.data_ptr(), (None if d.q_lens is None else d.q_lens.data_ptr())
    a.batch, a.n_q_heads, a.n_kv_heads, a.head_dim, a.q_len = base.B, base.HQ, base.H, base.D, d.T
    a.n_slots, a.block_size, a.max_blocks, a.table_stride = base.n_slots, base.block_size, base.table.shape[1], base.table.shape[1]
    a.slot_stride, a.head_stride, a.q_stride, a.out_stride = base.slot_stride, base.head_stride, base.q_stride, W  # (cache strides: bytes)
    a.scale, a.k_scale, a.v_scale = base.scale, d.fc.k_scale, d.fc.v_scale
    fn = getattr(_lib.load(), "sqllm_attn_prefill_fp8_bf16" if base.dtype == torch.bfloat16 else "sqllm_attn_prefill_fp8_f16")
    assert fn(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind,T,D,hq,hk,dt,scales", CASES)
def test_parity_with_the_oracle_through_the_module_and_the_c_entry(gpu, kind, T, D, hq, hk, dt, scales):
    for seqs, ql in PC.calls(T):
        fc, case, want, gate = reference(kind, T, D, hq, hk, dt, scales, seqs, ql)
        d = Dev(gpu, fc.case, case, fc)
        _poison_lds()
        y = _prefill(d)
        worst = C.excess(_f64(y), want, gate)
        print(f"PREFILL_FP8_GATE {kind} T={T} D={D} heads={hq}/{hk} {dt} scales={scales} q_lens={ql}: {worst:.3f}")
        assert y.shape == (len(seqs) * T, hq * D) and worst <= 1.0, (ql, worst)
        assert np.array_equal(_bits(_c_entry(d)), _bits(y)), ql  # one kernel: the same bits, with no workspace at all


@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("D,H", [(128, 2), (64, 4)])
def test_every_byte_through_the_conversion(gpu, D, H, dt):
    """one key, so its weight is 1 and the row is v itself: the 256 bytes of key 0 are 0 .. 255, v_scale a power of two"""
    import torch
    from squeezellm_amd.quant import PrefillAttention
    dtype, v_scale = C.DTYPES[dt], 0.03125
    k, v = (torch.full((16, H, D), b, dtype=torch.uint8) for b in F.NAN_BYTES)
    k[0], v[0] = 0x38, torch.arange(256, dtype=torch.uint8).reshape(H, D)  # (0x38: 1.0)
    att = PrefillAttention(H, H, D, block_size=16)
    y = att(torch.ones((1, H * D), dtype=dtype, device=gpu), k.to(gpu).view(torch.float8_e4m3fn), v.to(gpu).view(torch.float8_e4m3fn),
            torch.zeros((1, 1), dtype=torch.int32, device=gpu), torch.ones(1, dtype=torch.int32, device=gpu), 1, k_scale=0.5, v_scale=v_scale)
    assert att.last_route == "attn_prefill"
    want = (F.decode(v[0].reshape(-1)) * v_scale).to(dtype)
    assert torch.isnan(want).nonzero().reshape(-1).tolist() == [0x7F, 0xFF]
    torch.testing.assert_close(y.cpu().reshape(-1), want, rtol=0, atol=0, equal_nan=True)


@pytest.mark.gpu
def test_corner_rows_in_one_call(gpu):
    """+0: padding, L <= 0; NaN: n_b > T, L beyond the table, a table entry outside the cache between the tokens of a sequence"""
    T, seqs, ql = 17, (14, 82, 40, 30, 20), (17, 17, 5, 18, 17)
    fc0 = F.fp8_case("paged", len(seqs), 128, 8, 2, "fp16", F.SCALES, 0, seqs)
    sides = []
    for base0 in (fc0.case, fc0.shadow):
        base = copy.copy(base0)
        base.table, base.lens = base0.table.copy(), base0.lens.copy()
        base.table[1, 5] = base.n_slots // base.block_size  # keys 80 .. 95 of sequence 1: the first block id outside the cache
        base.lens[4] = 10 ** 6
        sides.append(base)
    base, case = sides[0], A.expand(sides[0], T, ql)
    want, gate = C.reference_of(A.expand(sides[1], T, ql))
    L = case.lens.reshape(len(seqs), T)
    assert L[0, :3].tolist() == [0, 0, 0] and L[0, 3] == 1 and L[1, -3:].tolist() == [80, 81, 82] and (L[2, 5:] == 0).all()
    nan = np.isnan(want).all(axis=1).reshape(len(seqs), T)
    assert not nan[:3, :-2].any() and nan[1, -2:].all() and nan[3:].all() and np.isfinite(want[~nan.reshape(-1)]).all()
    y = _prefill(Dev(gpu, base, case, types.SimpleNamespace(**{**vars(fc0), "case": base})))
    assert C.excess(_f64(y), want, gate) <= 1.0
    assert not _bits(y)[case.lens == 0].any()  # +0, not -0


@pytest.mark.gpu
def test_independence_of_the_batch_the_poison_run_to_run_bits_and_the_writes(gpu):
    import torch
    kind, T, D, hq, hk, dt = PC.CASES[4]
    seqs, ql = PC.calls(T)[1]
    d = _dev(gpu, kind, T, D, hq, hk, dt, seqs, ql)
    att, W, rows = _module(d.base), hq * D, len(seqs) * T
    buf = torch.full((rows + 2, W + 6), 7.0, dtype=d.base.dtype, device=gpu)  # a guard row on either side, padding behind every row
    k0, v0 = d.k_buf.clone(), d.v_buf.clone()
    y = _bits(_prefill(d, att, out=buf[1:-1, :W]))
    assert bool((buf[0] == 7).all() and (buf[-1] == 7).all() and (buf[:, W:] == 7).all())
    assert torch.equal(d.k_buf, k0) and torch.equal(d.v_buf, v0)
    _poison_lds()
    assert np.array_equal(_bits(_prefill(d, att)), y)  # run to run
    for b in range(len(seqs)):  # a sequence alone
        assert np.array_equal(_bits(_prefill(d, att, slice(b, b + 1))), y[b * T:(b + 1) * T]), b
    other = _dev(gpu, kind, T, D, hq, hk, dt, seqs, ql, poison=1)  # the other NaN byte wherever nothing is addressed
    assert not torch.equal(other.k_buf, d.k_buf) and np.array_equal(_bits(_prefill(other)), y)


@pytest.mark.gpu
def test_a_captured_call_is_one_kernel_node_and_follows_lengths_updated_in_place(gpu):
    import torch
    T = 33
    d = _dev(gpu, "paged", T, 128, 8, 2, "bf16", (2 * PC.P + 3, 70, 40), (33, 33, 33))
    att = _module(d.base)
    out = torch.empty((3 * T, 8 * 128), dtype=d.base.dtype, device=gpu)
    run = lambda: _prefill(d, att, out=out)  # noqa: E731
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        run()
    assert _node_types(g) == [0]  # hipGraphNodeTypeKernel
    g.instantiate()
    for seq, ql in (((2 * PC.P + 1, 64, 40), (33, 20, 1)), ((200, 70, 33), (7, 33, 33)), ((2 * PC.P + 3, 65, 3), (33, 0, 33))):
        d.seq.copy_(torch.tensor(seq, dtype=torch.int32))  # in place: the graph holds the addresses
        d.q_lens.copy_(torch.tensor(ql, dtype=torch.int32))
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        replayed = _bits(out)
        assert np.array_equal(replayed, _bits(_prefill(d, att))), (seq, ql)  # a fresh eager call
