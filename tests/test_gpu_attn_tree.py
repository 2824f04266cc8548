"""The tree-masked decode attention on the GPU (sqllm_attn_tree_f16 / _bf16 / _fp8_f16 / _fp8_bf16 behind
quant.DecodeAttention(..., q_len=, tree_mask=); include/sqllm_hip.h, sqllm_attn_tree) on the cases of tests/attn_tree_cases.py:
the chain's words give the BITS of the append entries wherever the context is not negative (there the append entry serves the
last tokens and the tree entry's contract says NaN), and trees pass the fp64 oracle under the gate of tests/attn_decode_cases.py."""
import ctypes

import numpy as np
import pytest

from tests import attn_append_cases as A
from tests import attn_decode_cases as C
from tests import attn_tree_cases as K
from tests import kv_fp8_cases as F
from tests.test_gpu_attn_append import Dev, _dev
from tests.test_gpu_attn_decode import _bits, _f64, _node_types

gpu_test = pytest.mark.gpu
P = C.P
# T x head ratio x cache; head_dim and the type alternate so that each occurs with each of them
IDENTITY = [(T, (64, 128)[(i + j) % 2], hq, hk, ("fp16", "bf16")[(i + j // 2) % 2], fp8)
            for i, T in enumerate((1, 2, 3, 5, 16)) for j, (hq, hk) in enumerate(((2, 2), (6, 2), (16, 2))) for fp8 in (False, True)]
ORACLE = [(tree, T, ("paged", "padded")[(i + j) % 2], (64, 128)[(i // 2 + j) % 2], *((8, 2), (6, 2))[(i + j) % 2], ("fp16", "bf16")[i % 2])
          for i, tree in enumerate(K.TREES) for j, T in enumerate((5, 16))]


def _mask(gpu, name, T, n_seqs):
    import torch

    return torch.tensor([K.words(name, T)] * n_seqs, dtype=torch.int32, device=gpu)


def _tree(d, mask, att=None, out=None):
    """the call under test"""
    att = att or d.module()
    y = att(d.q, d.k, d.v, d.table, d.seq, out=out, q_len=d.T, q_lens=d.q_lens, tree_mask=mask, **d.kw)
    assert att.last_route == "attn_tree"
    return y


@gpu_test
@pytest.mark.parametrize("T,D,hq,hk,dt,fp8", IDENTITY)
def test_the_chain_words_give_the_bits_of_the_append_entries(gpu, T, D, hq, hk, dt, fp8):
    """every batch of seq_lens_for(T), q_lens NULL and ragged"""
    import torch

    for seqs, ragged in A.ragged_batches(T, "paged"):
        for ql in (None, ragged):
            d = _dev(gpu, "paged", T, D, hq, hk, dt, seqs, ql, fp8)
            att = d.module()
            got, want = _tree(d, _mask(gpu, "chain", T, len(seqs)), att), d.append(att)
            negative = [0 < n <= T and s < n for s, n in zip(seqs, ql or (T,) * len(seqs))]  # the contract's NaN: no chain there
            keep = torch.tensor(np.repeat(~np.array(negative), T), device=gpu)
            assert got.dtype == want.dtype and torch.equal(got.view(torch.int16)[keep], want.view(torch.int16)[keep]), (seqs, ql)
            assert bool(torch.isnan(got[~keep]).all()) and (ql is not None or bool(keep[-T:].all()))  # (the longest sequence is compared)


@gpu_test
@pytest.mark.parametrize("tree,T,kind,D,hq,hk,dt", ORACLE)
def test_trees_against_the_fp64_oracle(gpu, tree, T, kind, D, hq, hk, dt):
    import torch

    for seqs in K.context_batches(T):
        base, case = K.build(kind, T, D, hq, hk, dt, seqs)
        d, words = Dev(gpu, base, case), [K.words(tree, T)] * len(seqs)
        got = _tree(d, _mask(gpu, tree, T, len(seqs)))
        want, gate = C.reference_of(K.as_decode_case(base, case, words))
        worst = C.excess(_f64(got), want, gate)
        print(f"TREE_GATE {tree} {kind} T={T} D={D} heads={hq}/{hk} {dt} seqs={seqs}: {worst:.3f}")
        assert np.isfinite(want).all() and worst <= 1.0, worst
        if tree == "star":  # (the gate cannot be met by ignoring the mask)
            assert not torch.equal(got, _tree(d, _mask(gpu, "chain", T, len(seqs))))
    if T == 5:  # ... and once per tree over the dequantised bytes of an fp8 cache (base, case: the last call's)
        fc = F.quantise(base)
        want, gate = C.reference_of(K.as_decode_case(fc.shadow, case, words))
        worst = C.excess(_f64(_tree(Dev(gpu, base, case, fc), _mask(gpu, tree, T, len(seqs)))), want, gate)
        print(f"TREE_GATE fp8 {tree} {kind} T={T} D={D} heads={hq}/{hk} {dt}: {worst:.3f}")
        assert worst <= 1.0, worst


@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("node", [1, 2])
def test_a_nan_at_a_sibling_node(gpu, node, fp8):
    """a star of 5 nodes behind P - 2 keys (node 1 ends the first partition, node 2 begins the second).  One NaN in k, then in v, at
    that node: its own row follows the sibling's NaN rule, every other row is finite and bit-identical to the run without it"""
    import torch

    T = 5
    d = _dev(gpu, "paged", T, 64, 8, 2, "fp16", (9, P - 2 + T, 7), None, fp8)
    m = _mask(gpu, "star", T, 3)
    plain = _bits(_tree(d, m)).reshape(3, T, 8, 64)
    pos = P - 2 + node
    slot = int(d.base.table[1, pos // 16]) * 16 + pos % 16
    for which, (h, col) in ((d.k, (1, 5)), (d.v, (0, 9))):
        cache = which.view(torch.uint8) if fp8 else which  # (through the bytes: torch has no indexing for float8)
        keep = cache[slot, h, col].clone()
        cache[slot, h, col] = 0x7F if fp8 else float("nan")
        y = _tree(d, m)
        got, same = _f64(y).reshape(3, T, 8, 64), np.ones((3, T, 8, 64), bool)
        hit = (1, node, slice(4, 8)) if which is d.k else (1, node, slice(0, 4), 9)  # kv head 1's query heads; column 9 of kv head 0's
        assert np.isnan(got[hit]).all()
        same[hit] = False
        assert np.isfinite(got[same]).all() and np.array_equal(_bits(y).reshape(3, T, 8, 64)[same], plain[same])
        cache[slot, h, col] = keep


@gpu_test
@pytest.mark.parametrize("dt,fp8", [("fp16", False), ("bf16", True)])
def test_corner_rows(gpu, dt, fp8):
    """the contract's corner rows; nothing out of range is read: the kernel judges the table's values before it touches the caches"""
    import torch

    T, long_ = 5, 2 * P + 3
    d = _dev(gpu, "paged", T, 64, 8, 2, dt, (20, long_, 40, T), (5, 5, 3, 5), fp8)
    m = _mask(gpu, "star", T, 4)
    m[3, 1] = 0  # sequence 3 has no context: this row attends nothing
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=gpu)  # noqa: E731
    run = lambda mask=m: _tree(d, mask)  # noqa: E731
    y = run()
    got, plain = _f64(y).reshape(4, T, -1), _bits(y).reshape(4, T, -1)
    zero = np.zeros((4, T), bool)
    zero[2, 3:] = zero[3, 1] = True  # padding rows, and C == 0 with m == 0
    assert (got[zero] == 0).all() and not np.signbit(got[zero]).any() and np.isfinite(got[~zero]).all()
    assert np.array_equal(_bits(run(m | i32([[-1 << n] for n in (5, 5, 3, 5)]))).reshape(4, T, -1), plain)  # bits at and above n_b
    d.q_lens.copy_(i32([6, 0, 3, 5]))  # n_b > q_len: NaN; n_b = 0: +0; the neighbours are what they were
    y = run()
    got = _f64(y).reshape(4, T, -1)
    assert np.isnan(got[0]).all() and (got[1] == 0).all() and not np.signbit(got[1]).any()
    assert np.array_equal(_bits(y).reshape(4, T, -1)[2:], plain[2:])
    d.q_lens.copy_(i32([5, 5, 3, 5]))
    d.seq[0] = 4  # a negative context
    y = run()
    assert np.isnan(_f64(y).reshape(4, T, -1)[0]).all() and np.array_equal(_bits(y).reshape(4, T, -1)[1:], plain[1:])
    d.seq[0] = 20
    cap = d.base.table.shape[1] * 16
    chain = m.clone()
    chain[1] = i32(K.words("chain", T))
    d.seq[1] = cap + 2  # Leff = cap - 2 + t: beyond the capacity for the last two rows
    y = run(chain)
    assert np.isnan(_f64(y).reshape(4, T, -1)[1, 3:]).all() and np.array_equal(_bits(y).reshape(4, T, -1)[[0, 2, 3]], plain[[0, 2, 3]])
    d.seq[1] = long_
    # a bad entry at the block of the last nodes only (keys 512 ..; the star's rows end at 511, 512, 513, 514, 515)
    blk = (long_ - 1) // 16
    for entry in (-1, d.base.n_slots // 16, -(1 << 31)):
        keep = d.table[1, blk].clone()
        d.table[1, blk] = entry
        y = run()
        assert np.isnan(_f64(y).reshape(4, T, -1)[1, 2:]).all()
        assert np.array_equal(_bits(y).reshape(4, T, -1)[1, :2], plain[1, :2]) and np.array_equal(_bits(y).reshape(4, T, -1)[[0, 2, 3]], plain[[0, 2, 3]])
        d.table[1, blk] = keep
    assert np.array_equal(_bits(run()).reshape(4, T, -1), plain)


@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("kind,nodes", [("paged", 2), ("paged_single", 1)])
def test_a_captured_call_follows_the_mask_and_the_lengths_updated_in_place(gpu, kind, nodes, fp8):
    import torch

    T = 3
    top = P + 2 if kind == "paged" else P
    d = _dev(gpu, kind, T, 128, 8, 2, "bf16", (top, 9, 40), (3, 3, 3), fp8)
    att, m = d.module(), _mask(gpu, "star", T, 3)
    out = torch.empty((3 * T, 8 * 128), dtype=d.case.dtype, device=gpu)
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        _tree(d, m, att, out)
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        _tree(d, m, att, out)
    assert _node_types(g) == [0] * nodes  # hipGraphNodeTypeKernel
    g.instantiate()
    for seq, ql, tree in (((top - 2, 7, 40), (3, 2, 1), "heap"), ((top, 9, 39), (2, 3, 0), "chain"), ((top - 1, 8, 40), (3, 3, 3), "no_tree")):
        d.seq.copy_(torch.tensor(seq, dtype=torch.int32))  # in place: the graph holds the addresses
        d.q_lens.copy_(torch.tensor(ql, dtype=torch.int32))
        m.copy_(_mask(gpu, tree, T, 3))
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out), _bits(_tree(d, m))), (seq, ql, tree)  # a fresh eager call


@gpu_test
@pytest.mark.parametrize("kind,dt,fp8", [("padded", "fp16", False), ("padded", "bf16", True), ("paged_single", "bf16", False), ("paged_single", "fp16", True)])
def test_c_abi_directly(gpu, kind, dt, fp8):
    """by hand: mask rows wider than q_len, a workspace of exactly the documented size full of 0xFF with a guard behind it"""
    import torch

    from squeezellm_amd import _lib, quant_cuda

    T, seqs = 3, ((P + 2, 9, 40) if kind == "padded" else (P, 9, 40))
    d = _dev(gpu, kind, T, 128, 8, 2, dt, seqs, (3, 2, 3), fp8)
    base, rows, W = d.base, 3 * T, 8 * 128
    wide = torch.full((3, T + 3), -1, dtype=torch.int32, device=gpu)
    wide[:, :T] = _mask(gpu, "heap", T, 3)
    out = torch.full((rows, W + 4), 7.0, dtype=base.dtype, device=gpu)
    need = _lib.attn_decode_workspace_bytes(rows, base.HQ, base.D, base.table.shape[1], base.block_size)
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=gpu)
    ws[need:] = 0xA5
    a = _lib.SqllmAttnTreeFp8() if fp8 else _lib.SqllmAttnTree()
    celem = 1 if fp8 else 2
    a.q, a.out = d.q_buf.data_ptr(), out.data_ptr()
    a.k_cache, a.v_cache = d.k_buf.data_ptr() + celem * C.GUARD, d.v_buf.data_ptr() + celem * C.GUARD
    a.block_table, a.seq_lens, a.q_lens, a.q_len = d.table.data_ptr(), d.seq.data_ptr(), d.q_lens.data_ptr(), T
    a.tree_mask, a.mask_stride = wide.data_ptr(), T + 3
    a.batch, a.n_q_heads, a.n_kv_heads, a.head_dim = 3, base.HQ, base.H, base.D
    a.n_slots, a.block_size, a.max_blocks, a.table_stride = base.n_slots, base.block_size, base.table.shape[1], base.table.shape[1]
    a.slot_stride, a.head_stride, a.q_stride, a.out_stride = base.slot_stride, base.head_stride, base.q_stride, W + 4
    a.scale, a.workspace = base.scale, ws.data_ptr()
    if fp8:
        a.k_scale, a.v_scale = d.fc.k_scale, d.fc.v_scale
    fn = getattr(_lib.load(), "sqllm_attn_tree_" + ("fp8_" if fp8 else "") + ("f16" if dt == "fp16" else "bf16"))
    assert fn(ctypes.byref(a), quant_cuda._raw_stream(gpu.index)) == 0
    torch.cuda.synchronize()
    assert bool((out[:, W:] == 7.0).all()) and bool((ws[need:] == 0xA5).all())
    y = _tree(d, wide[:, :T])  # (rows T + 3 apart: used without a copy)
    assert bool(torch.isfinite(y).all()) == bool(torch.isfinite(out[:, :W]).all()) and np.array_equal(_bits(out[:, :W]), _bits(y))
