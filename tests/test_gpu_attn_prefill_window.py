"""The sliding-window prefill attention on the GPU (quant.PrefillAttention(window=W), sqllm_attn_prefill_window_*) on the cases of
tests/attn_prefill_window_cases.py over 16-bit and fp8 caches, against tests/attn_window_cases.reference_w under its gate.  The
caches are poisoned per sequence (tests/test_attn_prefill_window_cpu.poisoned): whoever looks behind the earliest window gets NaN."""
import copy
import ctypes

import numpy as np
import pytest

from tests import attn_append_cases as A
from tests import attn_decode_cases as C
from tests import attn_prefill_window_cases as WPC
from tests import attn_window_cases as WC
from tests import kv_fp8_cases as F
from tests.test_attn_prefill_window_cpu import CACHES, ENTRIES, reference
from tests.test_gpu_attn_append import Dev
from tests.test_gpu_attn_decode import _bits, _f64, _node_types, _poison_lds


def _module(base, W):
    from squeezellm_amd.quant import PrefillAttention
    return PrefillAttention(base.HQ, base.H, base.D, block_size=base.block_size, window=W)


def _prefill(d, W, att=None, out=None):
    att = att or _module(d.base, W)
    y = att(d.q, d.k, d.v, d.table, d.seq, d.T, q_lens=d.q_lens, out=out, **d.kw)
    assert att.last_route == ("attn_prefill" if W is None else "attn_prefill_window")
    return y


def _c_entry(d, W):
    """the same call through the C entry directly, with a NULL workspace"""
    import torch
    from squeezellm_amd import _lib
    base, width = d.base, d.base.HQ * d.base.D
    out = torch.full((base.B * d.T, width), 7.0, dtype=base.dtype, device=d.q.device)
    a = _lib.SqllmAttnAppendFp8() if d.fc else _lib.SqllmAttnAppend()
    a.q, a.out, a.k_cache, a.v_cache, a.workspace = d.q.data_ptr(), out.data_ptr(), d.k.data_ptr(), d.v.data_ptr(), None
    a.block_table, a.seq_lens, a.q_lens = d.table.data_ptr(), d.seq.data_ptr(), (None if d.q_lens is None else d.q_lens.data_ptr())
    a.batch, a.n_q_heads, a.n_kv_heads, a.head_dim, a.q_len = base.B, base.HQ, base.H, base.D, d.T
    a.n_slots, a.block_size, a.max_blocks, a.table_stride = base.n_slots, base.block_size, base.table.shape[1], base.table.shape[1]
    a.slot_stride, a.head_stride, a.q_stride, a.out_stride, a.scale = base.slot_stride, base.head_stride, base.q_stride, width, base.scale
    if d.fc:
        a.k_scale, a.v_scale = d.fc.k_scale, d.fc.v_scale
    fn = getattr(_lib.load(), ENTRIES[bool(d.fc)][base.dtype == torch.bfloat16])
    assert fn(ctypes.byref(a), W, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("kind,T,D,hq,hk,dt,seq_len,W", WPC.CASES)
def test_parity_with_the_oracle_through_the_module_and_the_c_entry(gpu, kind, T, D, hq, hk, dt, seq_len, W, cache):
    for seqs, ql in WPC.calls(T, seq_len):
        base, fc, case, want, gate = reference(kind, T, D, hq, hk, dt, seq_len, W, ql, cache == "fp8")
        d = Dev(gpu, base, case, fc)
        _poison_lds()
        y = _prefill(d, W)
        worst = C.excess(_f64(y), want, gate)
        print(f"PREFILL_WINDOW_GATE {kind} T={T} D={D} heads={hq}/{hk} {dt} seq={seq_len} W={W} {cache} q_lens={ql}: {worst:.3f}")
        assert y.shape == (len(seqs) * T, hq * D) and worst <= 1.0, (ql, worst)
        assert np.array_equal(_bits(_c_entry(d, W)), _bits(y)), ql  # one kernel: the same bits, with no workspace at all
        assert np.array_equal(_bits(_prefill(d, W)), _bits(y))  # run to run


@pytest.mark.gpu
@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("kind,T,D,hq,hk,dt,seq_len,W", WPC.CASES)
def test_bit_identities_with_the_entry_without_a_window(gpu, kind, T, D, hq, hk, dt, seq_len, W, cache):
    """(a) rows with L <= W: the bits of PrefillAttention() in the same call; (b) rows whose lo is a multiple of 64 and of block_size:
    the bits PrefillAttention() gives the query alone, q_len = 1, seq_lens = L - lo, over the table row advanced by lo / block_size"""
    import torch
    base, fc, case, want, gate = reference(kind, T, D, hq, hk, dt, seq_len, W, None, cache == "fp8")
    d = Dev(gpu, base, case, fc)
    y, bs, L = _bits(_prefill(d, W)), base.block_size, case.lens
    a = (L > 0) & (L <= W)  # (a sequence with such a row has lo = 0 somewhere: nothing of it is poisoned)
    assert a.any() and np.isfinite(want[a]).all() and np.array_equal(y[a], _bits(_prefill(d, None))[a])
    lo = np.maximum(L - W, 0)
    rows = np.nonzero((lo > 0) & (lo % 64 == 0) & (lo % bs == 0))[0]
    assert len(rows) or (kind, W) not in (("paged", 40), ("paged", 64))
    if len(rows):
        table = np.zeros((len(rows), base.table.shape[1]), dtype=np.int64)
        for i, r in enumerate(rows):
            table[i, :base.table.shape[1] - lo[r] // bs] = base.table[r // T, lo[r] // bs:]
        i32 = lambda x: torch.from_numpy(np.asarray(x)).to(torch.int32).to(gpu)  # noqa: E731
        one = _module(base, None)(d.q[torch.from_numpy(rows).to(gpu)], d.k, d.v, i32(table), i32(L[rows] - lo[rows]), 1, **d.kw)
        assert np.isfinite(want[rows]).all() and np.array_equal(_bits(one), y[rows])


@pytest.mark.gpu
@pytest.mark.parametrize("cache", CACHES)
def test_corner_rows_in_one_call(gpu, cache):
    """+0: padding, L <= 0; NaN: n_b > T, L beyond the table, and a table entry outside the cache for exactly the tokens that attend
    its keys -- tokens 14 and 15 of the same query tile have left them behind and hold oracle values"""
    T, W, seqs, ql = 17, 2, (14, 84, 40, 30, 20), (17, 17, 5, 18, 17)
    base = copy.copy(A.build("paged", T, 128, 8, 2, "fp16", seqs, ql)[0])
    base.table, base.lens = base.table.copy(), base.lens.copy()
    base.table[1, 4] = base.n_slots // base.block_size  # keys 64 .. 79 of sequence 1: the first block id outside the cache
    base.lens[4] = 10 ** 6
    fc = F.quantise(base) if cache == "fp8" else None
    case, shadow = A.expand(base, T, ql), A.expand(fc.shadow if fc else base, T, ql)
    shadow.window = W
    want, gate = WC.reference_w(shadow)
    L = case.lens.reshape(len(seqs), T)
    assert L[0, :3].tolist() == [0, 0, 0] and L[1].tolist() == list(range(68, 85)) and (L[2, 5:] == 0).all()
    nan = np.isnan(want).all(axis=1).reshape(len(seqs), T)
    assert nan[1, :14].all() and not nan[1, 14:].any() and not nan[[0, 2]].any() and nan[3:].all() and np.isfinite(want[~nan.reshape(-1)]).all()
    y = _prefill(Dev(gpu, base, case, fc), W)
    assert C.excess(_f64(y), want, gate) <= 1.0
    assert not _bits(y)[case.lens == 0].any()  # +0, not -0


@pytest.mark.gpu
@pytest.mark.parametrize("cache", CACHES)
def test_a_captured_call_is_one_kernel_node_and_follows_lengths_updated_in_place(gpu, cache):
    import torch
    T, W, seqs, ql = 33, 20, (2 * WPC.P + 3, 70, 40), (33, 33, 33)
    base = A.build("paged", T, 128, 8, 2, "bf16", seqs, ql)[0]
    d = Dev(gpu, base, A.expand(base, T, ql), F.quantise(base) if cache == "fp8" else None)
    att = _module(base, W)
    out = torch.empty((3 * T, 8 * 128), dtype=base.dtype, device=gpu)
    run = lambda: _prefill(d, W, att, out=out)  # noqa: E731
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
    for seq, n in (((2 * WPC.P + 1, 64, 40), (33, 20, 1)), ((200, 70, 33), (7, 33, 33)), ((2 * WPC.P + 3, 65, 3), (33, 0, 33))):
        d.seq.copy_(torch.tensor(seq, dtype=torch.int32))  # in place: the graph holds the addresses
        d.q_lens.copy_(torch.tensor(n, dtype=torch.int32))
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        replayed = _bits(out)
        assert np.array_equal(replayed, _bits(_prefill(d, W, att))), (seq, n)  # a fresh eager call


@pytest.mark.gpu
def test_two_chunks_through_a_ring_equal_the_flat_table(gpu):
    """quant.ring_block_table(q_len=33) with W = 8 and blocks of 16: R = 4, 64 slots.  Two chunks of 33 tokens are written where the
    ring's table says (the second overwrites keys 0 and 1) and attended: the bits of the same chunks over the flat table"""
    import torch
    from squeezellm_amd import quant
    W, bs, T, n = 8, 16, 33, 66
    lin = C.build("paged", 1, 64, 8, 2, "fp16", 0, (n,))
    d = Dev(gpu, lin, A.expand(lin, n))
    att = _module(lin, W)
    ring_table = quant.ring_block_table(1, W, bs, n, gpu, q_len=T)
    assert ring_table.shape == (1, 5) and int(ring_table.max()) == 3
    ring_k, ring_v = (torch.full((4 * bs, 2, 64), float("nan"), dtype=lin.dtype, device=gpu) for _ in range(2))
    lin_slot = torch.from_numpy(C.key_slots(lin, 0, n)).to(gpu)
    ring_slot = ring_table[0].long()[torch.arange(n, device=gpu) // bs] * bs + torch.arange(n, device=gpu) % bs
    assert int(ring_slot[64]) == int(ring_slot[0]) == 0
    for c in range(2):
        p = torch.arange(c * T, (c + 1) * T, device=gpu)
        ring_k.index_copy_(0, ring_slot[p], d.k[lin_slot[p]])
        ring_v.index_copy_(0, ring_slot[p], d.v[lin_slot[p]])
        lens = torch.tensor([(c + 1) * T], dtype=torch.int32, device=gpu)
        y = att(d.q[p], ring_k, ring_v, ring_table, lens, T)
        assert att.last_route == "attn_prefill_window" and np.isfinite(_f64(y)).all()
        assert np.array_equal(_bits(y), _bits(att(d.q[p], d.k, d.v, d.table, lens, T))), c
