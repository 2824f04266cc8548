"""The prefill attention on the GPU (quant.PrefillAttention, sqllm_attn_prefill_*) on the cases of tests/attn_prefill_cases.py,
against the fp64 oracle under the gate of tests/attn_decode_cases.py."""
import copy
import ctypes

import numpy as np
import pytest

from tests import attn_append_cases as A
from tests import attn_decode_cases as C
from tests import attn_prefill_cases as PC
from tests.test_gpu_attn_append import Dev
from tests.test_gpu_attn_decode import _bits, _f64, _node_types, _poison_lds

gpu_test = pytest.mark.gpu


def _module(base):
    from squeezellm_amd.quant import PrefillAttention

    return PrefillAttention(base.HQ, base.H, base.D, block_size=base.block_size)


def _prefill(d, att=None, seqs=slice(None), out=None):
    att = att or _module(d.base)
    b0, b1, _ = seqs.indices(d.base.B)
    ql = None if d.q_lens is None else d.q_lens[seqs]
    y = att(d.q[b0 * d.T:b1 * d.T], d.k, d.v, d.table[seqs], d.seq[seqs], d.T, q_lens=ql, out=out)
    assert att.last_route == "attn_prefill"
    return y


def _c_entry(d):
    """the same call through the C entry directly, with a NULL workspace"""
    import torch
    from squeezellm_amd import _lib
    base, W = d.base, d.base.HQ * d.base.D
    out = torch.full((base.B * d.T, W), 7.0, dtype=base.dtype, device=d.q.device)
    a = _lib.SqllmAttnAppend()
    a.q, a.out, a.k_cache, a.v_cache = d.q.data_ptr(), out.data_ptr(), d.k.data_ptr(), d.v.data_ptr()
    a.block_table, a.seq_lens, a.q_lens, a.workspace = d.table.data_ptr(), d.seq.data_ptr(), (None if d.q_lens is None else d.q_lens.data_ptr()), None
    a.batch, a.n_q_heads, a.n_kv_heads, a.head_dim, a.q_len = base.B, base.HQ, base.H, base.D, d.T
    a.n_slots, a.block_size, a.max_blocks, a.table_stride = base.n_slots, base.block_size, base.table.shape[1], base.table.shape[1]
    a.slot_stride, a.head_stride, a.q_stride, a.out_stride, a.scale = base.slot_stride, base.head_stride, base.q_stride, W, base.scale
    fn = getattr(_lib.load(), "sqllm_attn_prefill_bf16" if base.dtype == torch.bfloat16 else "sqllm_attn_prefill_f16")
    assert fn(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    return out


@gpu_test
@pytest.mark.parametrize("kind,T,D,hq,hk,dt", PC.CASES)
def test_parity_with_the_oracle_through_the_module_and_the_c_entry(gpu, kind, T, D, hq, hk, dt):
    for seqs, ql in PC.calls(T):
        base, case, want, gate = A.reference(kind, T, D, hq, hk, dt, seqs, ql)
        d = Dev(gpu, base, case)
        _poison_lds()
        y = _prefill(d)
        worst = C.excess(_f64(y), want, gate)
        print(f"PREFILL_GATE {kind} T={T} D={D} heads={hq}/{hk} {dt} q_lens={ql}: {worst:.3f}")
        assert y.shape == (len(seqs) * T, hq * D) and worst <= 1.0, (ql, worst)
        assert np.array_equal(_bits(_c_entry(d)), _bits(y)), ql  # one kernel: the same bits, with no workspace at all


@gpu_test
@pytest.mark.parametrize("D,hq,dt", [(128, 8, "fp16"), (64, 8, "bf16"), (64, 2, "fp16")])
def test_causality_against_the_one_query_entry_and_under_changed_later_keys(gpu, D, hq, dt):
    """each side is inside one gate of the oracle: two between them; other FINITE values at the last token's own key change its row alone"""
    import torch

    T, seqs = 33, (33 + 64,)  # (33 rows: the one-query entry serves 64)
    base, case, want, gate = A.reference("paged", T, D, hq, 2, dt, seqs, None)
    d = Dev(gpu, base, case)
    y = _prefill(d)
    one = d.decode()
    assert C.excess(_f64(y), _f64(one), gate) <= 2.0
    for b, n in enumerate(seqs):
        at = torch.from_numpy(C.GUARD + C.key_slots(base, b, n)[-1:, None, None] * base.slot_stride + np.arange(base.H)[None, :, None] * base.head_stride
                              + np.arange(D)[None, None, :]).reshape(-1).to(gpu)
        d.k_buf[at] = -d.k_buf[at] + 0.5
        d.v_buf[at] = d.v_buf[at] * 3.0 + 1.0
    y2 = _bits(_prefill(d)).reshape(len(seqs), T, -1)
    y1 = _bits(y).reshape(len(seqs), T, -1)
    assert np.array_equal(y2[:, :-1], y1[:, :-1]) and not np.array_equal(y2[:, -1], y1[:, -1])


@gpu_test
def test_corner_rows_in_one_call(gpu):
    """+0: padding, L <= 0; NaN: n_b > T, L beyond the table, a table entry outside the cache between the tokens of a sequence"""
    T, seqs, ql = 17, (14, 82, 40, 30, 20), (17, 17, 5, 18, 17)
    base0 = A.build("paged", T, 128, 8, 2, "fp16", seqs, ql)[0]
    base = copy.copy(base0)
    base.table, base.lens = base0.table.copy(), base0.lens.copy()
    base.table[1, 5] = base.n_slots // base.block_size  # keys 80 .. 95 of sequence 1: the first block id outside the cache
    base.lens[4] = 10 ** 6
    case = A.expand(base, T, ql)
    want, gate = C.reference_of(case)
    L = case.lens.reshape(len(seqs), T)
    assert L[0, :3].tolist() == [0, 0, 0] and L[0, 3] == 1 and L[1, -3:].tolist() == [80, 81, 82] and (L[2, 5:] == 0).all()
    nan = np.isnan(want).all(axis=1).reshape(len(seqs), T)
    assert not nan[:3, :-2].any() and nan[1, -2:].all() and nan[3:].all() and np.isfinite(want[~nan.reshape(-1)]).all()
    y = _prefill(Dev(gpu, base, case))
    assert C.excess(_f64(y), want, gate) <= 1.0
    assert not _bits(y)[case.lens == 0].any()  # +0, not -0


@gpu_test
def test_independence_of_the_batch_run_to_run_bits_and_the_writes(gpu):
    import torch

    kind, T, D, hq, hk, dt = PC.CASES[4]
    seqs, ql = PC.calls(T)[1]
    base, case = A.build(kind, T, D, hq, hk, dt, seqs, ql)
    d = Dev(gpu, base, case)
    att, W, rows = _module(base), hq * D, len(seqs) * T
    buf = torch.full((rows + 2, W + 6), 7.0, dtype=base.dtype, device=gpu)  # a guard row on either side, padding behind every row
    k0, v0 = d.k_buf.clone(), d.v_buf.clone()
    y = _bits(_prefill(d, att, out=buf[1:-1, :W]))
    assert bool((buf[0] == 7).all() and (buf[-1] == 7).all() and (buf[:, W:] == 7).all())
    assert torch.equal(d.k_buf.view(torch.int16), k0.view(torch.int16)) and torch.equal(d.v_buf.view(torch.int16), v0.view(torch.int16))
    _poison_lds()
    assert np.array_equal(_bits(_prefill(d, att)), y)  # run to run
    for b in range(len(seqs)):  # a sequence alone
        assert np.array_equal(_bits(_prefill(d, att, slice(b, b + 1))), y[b * T:(b + 1) * T]), b


@gpu_test
def test_a_captured_call_is_one_kernel_node_and_follows_lengths_updated_in_place(gpu):
    import torch

    T = 33
    base, case = A.build("paged", T, 128, 8, 2, "bf16", (2 * PC.P + 3, 70, 40), (33, 33, 33))
    d = Dev(gpu, base, case)
    att = _module(base)
    out = torch.empty((3 * T, 8 * 128), dtype=base.dtype, device=gpu)
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
