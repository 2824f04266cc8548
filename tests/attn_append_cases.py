"""Cases of the decode attention for several new tokens per sequence (include/sqllm_hip.h, sqllm_attn_append), built on
tests/attn_decode_cases.py (imported, untouched) and shared by the CPU and the GPU tests.  No GPU and no library needed here.

The entry is DEFINED by reduction: row (b, t) holds the bits the one-query entry writes for table row b and length
L(b, t) = seq_lens[b] - (n_b - 1 - t).  So a case here is a one-query case of SEQUENCES (`base`: attn_decode_cases.build with
one row per sequence, whose cache holds the keys 0 .. seq_lens[b]-1 and NaN patterns everywhere else) and its EXPANSION
(`expand`): a one-query case of batch * T rows -- the table rows repeated, the per-token lengths, a q of its own -- over the
same guarded cache buffers.  The oracle, the fp32 model, the gate, the poisons and the guards are attn_decode_cases', applied
to the expansion.

The choices, each with its reason:
  * Q_LENS     T = 1 (the entry must be the sibling), 2 and 3 (speculation's small ends; 3 is odd), 5 (does not divide the 8
               virtual heads of a workgroup), 16 (the largest served).
  * HEADS      (2,2), (8,2), (6,2), (16,2): groups of 1, 4, 3 and 8, so that T * group takes 1, 8, 9 (one past a workgroup's 8),
               15, 20 and 128 among others: every group class, chunks that end inside a token, many chunks.
  * seq_lens_for(T)   {1, 2, T-1, P-1, P, P+1, P+2, 2P+3}: every T > 1 has a sequence whose tokens straddle the partition length
               P (some tokens reach the second partition, others do not; P+2 for T = 2, where P+1 leaves token 0 at exactly P),
               one shorter than its tokens (seq_lens < T: the first tokens have L <= 0), one of three partitions.
  * q_lens_for(T, n)  per sequence 0, 1, T-1, T, T+1 (beyond T: NaN rows), -3 (as 0), cycling, against NULL: padding rows in
               front of, among and behind real ones.  ragged_batches(T) carries the cycle on from call to call (a call has 4
               sequences at the most): the calls of a T meet every class between them.
  * GEOMETRIES attn_decode_cases' three and "paged_single" (a table of exactly P keys: one kernel node).
"""
import copy
import functools

import numpy as np
import torch

from tests import attn_decode_cases as C

P = C.P
Q_LENS = (1, 2, 3, 5, 16)
HEADS = ((2, 2), (8, 2), (6, 2), (16, 2))
GEOMETRIES = C.GEOMETRIES + ("paged_single",)
MAX_ROWS = 64  # batch * T the entry serves


def seq_lens_for(T, kind="paged"):
    """the sequences' lengths for T new tokens each, ascending; "paged_single" holds P keys at most"""
    if kind == "paged_single":
        want = {1, 2, T - 1, 17, P - 2, P - 1, P}
    else:
        want = {1, 2, T - 1, P - 1, P, P + 1, P + 2, 2 * P + 3}
    return tuple(sorted(n for n in want if n >= 1))


def q_lens_for(T, n, start=0):
    """ragged real-token counts for n sequences: the classes of the contract, cycling from class `start`"""
    return tuple((0, 1, T - 1, T, T + 1, -3)[(start + i) % 6] for i in range(n))


def ragged_batches(T, kind="paged"):
    """((seqs, q_lens), ...) over batches(T, kind): the cycle of q_lens_for goes on from batch to batch, so that the calls of a T
    meet EVERY class between them (a call has 4 sequences at the most, the cycle 6 classes) -- T + 1 and -3 in the second call"""
    out, at = [], 0
    for seqs in batches(T, kind):
        out.append((seqs, q_lens_for(T, len(seqs), at)))
        at += len(seqs)
    return tuple(out)


def batches(T, kind="paged"):
    """seq_lens_for(T) cut into calls of at most MAX_ROWS rows (and at most 4 sequences: the cases stay small)"""
    seqs = seq_lens_for(T, kind)
    step = max(1, min(4, MAX_ROWS // T))
    return tuple(seqs[i:i + step] for i in range(0, len(seqs), step))


def token_lengths(seq_lens, T, q_lens, capacity):
    """int64 [B * T]: L(b, t) as the one-query entry is to see it -- 0 for the +0 rows (padding, L <= 0), capacity + 1 for the
    NaN rows (L > capacity, n_b > T)"""
    seq = np.asarray(seq_lens, dtype=np.int64)
    n = np.full_like(seq, T) if q_lens is None else np.asarray(q_lens, dtype=np.int64)
    t = np.arange(T, dtype=np.int64)[None, :]
    nb = np.maximum(n, 0)[:, None]
    L = np.clip(seq[:, None] - (nb - 1 - t), 0, capacity + 1)
    L = np.where(t < nb, L, 0)
    L = np.where((n > T)[:, None], capacity + 1, L)
    return L.reshape(-1)


def expand(base, T, q_lens=None, poison=0):
    """the one-query case of base.B * T rows that an append call over `base` is defined by: row b * T + t has table row b and
    L(b, t); q is new ([B * T, HQ * D] inside rows 6 elements wider, the padding NaN), the caches are base's buffers"""
    B, W = base.B, base.HQ * base.D
    case = copy.copy(base)
    case.B = B * T
    case.table = np.repeat(base.table, T, axis=0)
    case.lens = token_lengths(base.lens, T, q_lens, base.table.shape[1] * base.block_size)
    case.seed = base.seed + [T, 0 if q_lens is None else 1]
    rng = np.random.default_rng(case.seed + [5])
    case.q_buf = C._poisoned(B * T * base.q_stride, base.dtype, poison).reshape(B * T, base.q_stride)
    case.q_buf[:, :W] = torch.from_numpy(rng.standard_normal((B * T, W))).to(base.dtype)
    case.base, case.T = base, T
    case.q_lens = None if q_lens is None else np.asarray(q_lens, dtype=np.int64)
    return case


@functools.lru_cache(maxsize=None)
def build(kind, T, D, HQ, H, dtype_name, seqs, q_lens=None, poison=0):
    """(base, expansion) of `seqs` sequences with T new tokens each; q_lens: None or a tuple per sequence"""
    base = C.build(kind, len(seqs), D, HQ, H, dtype_name, poison, tuple(seqs))
    return base, expand(base, T, q_lens, poison)


@functools.lru_cache(maxsize=None)
def reference(kind, T, D, HQ, H, dtype_name, seqs, q_lens=None):
    """(base, expansion, want, gate): the fp64 oracle and the gate of attn_decode_cases on the expansion, computed once"""
    base, case = build(kind, T, D, HQ, H, dtype_name, seqs, q_lens)
    return (base, case, *C.reference_of(case))


# ---- sharp softmax (attn_decode_cases.sharpen) under several new tokens ----

# A token that attends two or three keys -- or whose two or three top keys carry the row -- at scores beyond +-100 has a result
# whose last bits follow from the ORDER of the fp32 dot products (a unit in the last place of such a score is 1.5e-5; an fp16
# output near zero is finer).  The gate's yardstick for that is ONE draw, model32's own rounding of that (row, head); 16 new tokens
# behind sequences of 7 and 2P + 3 keys hold a hundred such (row, head)s, and on 21 of the 648 (case, cache, T) of the sharp-softmax
# tests the fp32 model in the kernels' own structure (attn_decode_cases.model_parts) exceeds the gate on the first draw of the
# new tokens' q: those cases are unfair to any fp32 implementation of that structure, and take the next draw on which the model is
# inside (tests/test_attn_ranges_cpu.py asserts all of it: every draw below the listed one is outside, the used ones inside, the
# unlisted cases inside on their first draw -- on the CPU, from the model alone).  All 21 are fp16 outputs; all but one T = 16.
# Key: (geometry, head_dim, query heads, type, profile, fp8 cache?, T).
SHARP_DRAWS = {
    ("paged", 64, 8, "fp16", "ramp_up", True, 16): 1, ("paged", 64, 8, "fp16", "all_low", True, 16): 1, ("paged", 64, 8, "fp16", "all_high", True, 16): 1,
    ("paged", 128, 4, "fp16", "all_low", True, 16): 1, ("paged", 128, 4, "fp16", "all_high", True, 16): 1,
    ("paged", 64, 16, "fp16", "all_low", False, 16): 3, ("paged", 64, 16, "fp16", "all_low", True, 16): 3,
    ("paged", 64, 16, "fp16", "all_high", False, 16): 3, ("paged", 64, 16, "fp16", "all_high", True, 16): 3,
    ("padded", 64, 8, "fp16", "ramp_up", True, 2): 1, ("padded", 64, 8, "fp16", "all_low", True, 16): 1, ("padded", 64, 8, "fp16", "all_high", True, 16): 1,
    ("padded", 128, 4, "fp16", "ramp_up", False, 16): 1,
    ("padded", 64, 16, "fp16", "all_low", False, 16): 1, ("padded", 64, 16, "fp16", "all_low", True, 16): 2,
    ("padded", 64, 16, "fp16", "all_high", False, 16): 1, ("padded", 64, 16, "fp16", "all_high", True, 16): 2,
    ("bhsd", 64, 8, "fp16", "all_low", False, 16): 1, ("bhsd", 64, 8, "fp16", "all_high", False, 16): 1,
    ("bhsd", 128, 4, "fp16", "ramp_up", True, 16): 1, ("bhsd", 64, 16, "fp16", "ramp_up", True, 16): 1,
}


def sharp_expand(base, T, fp8=False, draw=None):
    """the expansion of a sharpened case (or of its fp8 shadow) for T new tokens per sequence, q sharpened the same way; `draw`:
    which draw of the new tokens' q (None: the one SHARP_DRAWS lists for the case, else the first)"""
    if draw is None:
        dt = {v: k for k, v in C.DTYPES.items()}[base.dtype]
        draw = SHARP_DRAWS.get((base.kind, base.D, base.HQ, dt, base.profile, bool(fp8), T), 0)
    if draw:
        base = copy.copy(base)
        base.seed = base.seed + [1000 + draw]
    return C.sharpen_q(expand(base, T), base.sharp_c)
