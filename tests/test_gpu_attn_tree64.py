"""Tree verification up to 64 nodes on the GPU (sqllm_attn_tree64_f16 / _bf16 / _fp8_f16 / _fp8_bf16 behind
quant.PrefillAttention(..., q_len=, tree_mask=); include/sqllm_hip.h, sqllm_attn_tree64): trees against the fp64 oracle under the
gate of tests/attn_decode_cases.py, in tables of 2 P + 3 + 64 keys.  The contexts put the nodes inside one key tile (0, 1), across a
tile edge (62 with T > 2), across a partition edge (P - 2), on one (P) and behind a combine of three (2 P + 3)."""
import numpy as np
import pytest

from tests import attn_decode_cases as C
from tests import attn_tree_cases as K
from tests import kv_fp8_cases as F
from tests.test_attn_tree64_cpu import P, build, mask_of
from tests.test_gpu_attn_append import Dev
from tests.test_gpu_attn_decode import _bits, _f64

gpu_test = pytest.mark.gpu
CONTEXTS = (0, 1, 62, P - 2, P, 2 * P + 3)
# tree x T, the geometry, head_dim, the head ratio (1, 3, 4, 8; 3: 64 is no multiple of it, a token's heads straddle tiles) and the
# type interleaved so that each occurs with each of the others
ORACLE = [(tree, T, ("paged", "padded")[(i + j) % 2], (64, 128)[(i // 2 + j) % 2], *((2, 2), (6, 2), (8, 2), (16, 2))[(i + j) % 4], ("fp16", "bf16")[i % 2])
          for i, tree in enumerate(K.TREES) for j, T in enumerate((5, 17, 33, 64))]


def _module(base):
    from squeezellm_amd.quant import PrefillAttention

    return PrefillAttention(base.HQ, base.H, base.D, block_size=base.block_size)


def _tree(d, mask, seqs=slice(None), att=None):
    """the call under test, over the sequences `seqs` (a slice)"""
    att = att or _module(d.base)
    b0, b1, _ = seqs.indices(d.base.B)
    ql = None if d.q_lens is None else d.q_lens[seqs]
    y = att(d.q[b0 * d.T:b1 * d.T], d.k, d.v, d.table[seqs], d.seq[seqs], d.T, q_lens=ql, tree_mask=mask, **d.kw)
    assert att.last_route == "attn_tree64"
    return y


def _gate(base, case, words, got, tag):
    want, gate = C.reference_of(K.as_decode_case(base, case, words))
    worst = C.excess(_f64(got), want, gate)
    print(f"TREE64_GATE {tag}: {worst:.3f}")
    assert np.isfinite(want).all() and worst <= 1.0, worst


@gpu_test
@pytest.mark.parametrize("tree,T,kind,D,hq,hk,dt", ORACLE)
def test_trees_against_the_fp64_oracle(gpu, tree, T, kind, D, hq, hk, dt):
    import torch

    base, case = build(kind, T, D, hq, hk, dt, CONTEXTS)
    d, words = Dev(gpu, base, case), [K.words(tree, T)] * len(CONTEXTS)
    got = _tree(d, mask_of(words, gpu))
    _gate(base, case, words, got, f"{tree} {kind} T={T} D={D} heads={hq}/{hk} {dt}")
    if tree == "star":  # (the gate cannot be met by ignoring the mask)
        assert not torch.equal(got, _tree(d, mask_of([K.words("chain", T)] * len(CONTEXTS), gpu)))
    if T == 17:  # ... and once per tree over the dequantised bytes of an fp8 cache
        fc = F.quantise(base)
        got = _tree(Dev(gpu, base, case, fc), mask_of(words, gpu))
        _gate(fc.shadow, case, words, got, f"fp8 {tree} {kind} T={T} D={D} heads={hq}/{hk} {dt}")


@gpu_test
def test_a_bit_in_the_high_word_only(gpu):
    """row 40 of 64 attends nodes 0 and 40: its bit 40 lies in the second int32 word of the pair"""
    T = 64
    base, case = build("paged", T, 64, 6, 2, "fp16", (P - 2, 3))
    words = [[1 | (1 << t) for t in range(T)]] * 2
    assert words[0][40] >> 32 == 1 << 8 and words[0][40] & 0xFFFFFFFF == 1
    d = Dev(gpu, base, case)
    _gate(base, case, words, _tree(d, mask_of(words, gpu)), "high word")


@gpu_test
@pytest.mark.parametrize("dt,fp8", [("fp16", False), ("bf16", True)])
def test_a_sequence_has_its_own_bits_alone_and_in_a_batch(gpu, dt, fp8):
    import torch

    T = 33
    base, case = build("paged", T, 128, 8, 2, dt, (9, P - 2, 2 * P + 3))
    d = Dev(gpu, base, case, F.quantise(base) if fp8 else None)
    m = mask_of([K.words("heap", T), K.words("two_chains", T), K.words("star", T)], gpu)
    y = _tree(d, m)
    alone = _tree(d, m[1:2], slice(1, 2))
    assert bool(torch.isfinite(y).all()) and np.array_equal(_bits(y)[T:2 * T], _bits(alone))


@gpu_test
@pytest.mark.parametrize("dt,fp8", [("bf16", False), ("fp16", True)])
def test_a_table_of_one_partition_takes_one_kernel_node(gpu, dt, fp8):
    """capacity P: the partial kernel finishes the rows itself"""
    import torch

    T = 17
    contexts = (P - T, 23, 0)
    base, case = build("paged_single", T, 128, 6, 2, dt, contexts, None)
    assert base.table.shape[1] * base.block_size == P
    words = [K.words("two_chains", T)] * 3
    if fp8:
        fc = F.quantise(base)
        got = _tree(Dev(gpu, base, case, fc), mask_of(words, gpu))
        _gate(fc.shadow, case, words, got, f"one node fp8 {dt}")
    else:
        got = _tree(Dev(gpu, base, case), mask_of(words, gpu))
        _gate(base, case, words, got, f"one node {dt}")
    assert bool(torch.isfinite(got).all())


@gpu_test
@pytest.mark.parametrize("dt,fp8", [("fp16", False), ("bf16", True)])
def test_corner_rows(gpu, dt, fp8):
    """the contract's corner rows, as test_corner_rows of tests/test_gpu_attn_tree.py; nothing out of range is read: the kernel
    judges the table's values before it touches the caches"""
    import torch

    T, long_ = 33, 2 * P + 3
    base, case = build("paged", T, 64, 8, 2, dt, (20, long_, 40, 0))
    d = Dev(gpu, base, case, F.quantise(base) if fp8 else None)
    d.q_lens = torch.tensor([T, T, 30, T], dtype=torch.int32, device=gpu)
    d.seq[2] = 40 + 30
    m = mask_of([K.words("star", T)] * 4, gpu)
    m[3, 1] = 0  # sequence 3 has no context: this row attends nothing
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=gpu)  # noqa: E731
    run = lambda mask=m: _tree(d, mask)  # noqa: E731
    y = run()
    got, plain = _f64(y).reshape(4, T, -1), _bits(y).reshape(4, T, -1)
    zero = np.zeros((4, T), bool)
    zero[2, 30:] = zero[3, 1] = True  # padding rows, and C == 0 with m == 0
    assert (got[zero] == 0).all() and not np.signbit(got[zero]).any() and np.isfinite(got[~zero]).all()
    above = torch.tensor([[-1 << n] for n in (T, T, 30, T)], dtype=torch.int64, device=gpu)
    assert np.array_equal(_bits(run(m | above)).reshape(4, T, -1), plain)  # bits at and above n_b
    d.q_lens.copy_(i32([T + 1, 0, 30, T]))  # n_b > q_len: NaN; n_b = 0: +0; the neighbours are what they were
    y = run()
    got = _f64(y).reshape(4, T, -1)
    assert np.isnan(got[0]).all() and (got[1] == 0).all() and not np.signbit(got[1]).any()
    assert np.array_equal(_bits(y).reshape(4, T, -1)[2:], plain[2:])
    d.q_lens.copy_(i32([T, T, 30, T]))
    d.seq[0] = T - 1  # a negative context
    y = run()
    assert np.isnan(_f64(y).reshape(4, T, -1)[0]).all() and np.array_equal(_bits(y).reshape(4, T, -1)[1:], plain[1:])
    d.seq[0] = 20 + T
    cap = base.table.shape[1] * 16
    chain = m.clone()
    chain[1] = mask_of([K.words("chain", T)], gpu)[0]
    d.seq[1] = cap + 2  # Leff = cap + 2 - T + t + 1: beyond the capacity for the last two rows
    y = run(chain)
    assert np.isnan(_f64(y).reshape(4, T, -1)[1, T - 2:]).all() and np.array_equal(_bits(y).reshape(4, T, -1)[[0, 2, 3]], plain[[0, 2, 3]])
    d.seq[1] = long_ + T
    # a bad entry at the block of the last nodes only (keys 544 ..; the star's rows end at 516, 517, ..., 548: rows 29 .. 32 reach it)
    blk = (long_ + T - 1) // 16
    for entry in (-1, base.n_slots // 16, -(1 << 31)):
        keep = d.table[1, blk].clone()
        d.table[1, blk] = entry
        y = run()
        assert np.isnan(_f64(y).reshape(4, T, -1)[1, 29:]).all()
        assert np.array_equal(_bits(y).reshape(4, T, -1)[1, :29], plain[1, :29]) and np.array_equal(_bits(y).reshape(4, T, -1)[[0, 2, 3]], plain[[0, 2, 3]])
        d.table[1, blk] = keep
    assert np.array_equal(_bits(run()).reshape(4, T, -1), plain)
