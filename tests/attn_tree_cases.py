"""Cases of the tree-masked decode attention (include/sqllm_hip.h, sqllm_attn_tree), built on tests/attn_decode_cases.py and
tests/attn_append_cases.py (imported, untouched) and shared by the CPU and the GPU tests.  No GPU and no library needed here.

The reference needs no oracle of its own: a copy of the case with block_size = 1, the slots of the keys row (b, t) attends as
its table row and their number as its length IS a one-query case of attn_decode_cases' fp64 oracle, its fp32 model and its gate.

TREES: a star, a heap, two chains from one root, and "no_tree", words that are no ancestor closure (a bit j > t, the own bit
missing).  CONTEXTS: the nodes in one partition, straddling an edge, starting on an edge, behind a combine of three."""
import copy

import numpy as np

from tests import attn_append_cases as A
from tests import attn_decode_cases as C

P = C.P
TREES = ("star", "heap", "two_chains", "no_tree")
CONTEXTS = (0, 1, P - 2, P, 2 * P + 3)
CAPACITY = 2 * P + 3 + 16  # keys a table row must hold


def parents(name, T):
    """the parent of each of T nodes (-1: a root); a parent stands in front of its children"""
    if name == "star":
        return [-1] + [0] * (T - 1)
    if name == "heap":
        return [(t - 1) // 2 if t else -1 for t in range(T)]
    if name == "two_chains":  # 0 <- 1 <- 3 <- 5 ... and 0 <- 2 <- 4 <- 6 ...
        return [-1 if t == 0 else max(t - 2, 0) for t in range(T)]
    raise ValueError(name)


def words(name, T):
    """the T mask words of a tree: the ancestor closure with the own bit; "chain": the append entry's causal rows"""
    if name == "chain":
        return [(2 << t) - 1 for t in range(T)]
    if name == "no_tree":  # every earlier node but not the own one, and on even rows the node two behind
        return [((1 << t) - 1) | ((1 << (t + 2)) if t % 2 == 0 and t + 2 < T else 0) or 1 for t in range(T)]
    out = []
    for t, p in enumerate(parents(name, T)):
        out.append((1 << t) | (out[p] if p >= 0 else 0))
    return out


def context_batches(T):
    """CONTEXTS as seq_lens, cut into calls of at most 64 rows"""
    step = min(len(CONTEXTS), A.MAX_ROWS // T)
    return tuple(tuple(c + T for c in CONTEXTS[i:i + step]) for i in range(0, len(CONTEXTS), step))


def build(kind, T, D, HQ, H, dtype_name, seqs):
    """(base, case): the sequences' one-query case, with tables of CAPACITY keys, and its expansion into T rows each (for q)"""
    base = C.build(kind, len(seqs), D, HQ, H, dtype_name, 0, tuple(seqs), CAPACITY)
    return base, A.expand(base, T)


def as_decode_case(base, case, mask):
    """the one-query case at block size 1 that the tree call (mask: [B, T] words, every node real) is defined by; `base` may be an
    fp8 shadow of the sequences' case: its buffers are the ones read"""
    T, bs = case.T, base.block_size
    rows, lens = [], []
    for b in range(base.B):
        ctx = int(base.lens[b]) - T
        assert ctx >= 0
        for t in range(T):
            keys = list(range(ctx)) + [ctx + j for j in range(T) if mask[b][t] >> j & 1]
            rows.append([int(base.table[b, p // bs]) * bs + p % bs for p in keys])
            lens.append(len(keys))
    out = copy.copy(case)
    out.k_buf, out.v_buf, out.block_size, out.lens = base.k_buf, base.v_buf, 1, np.asarray(lens, dtype=np.int64)
    out.table = np.zeros((len(rows), max(max(lens), 1)), dtype=np.int64)
    for i, r in enumerate(rows):
        out.table[i, :len(r)] = r
    return out
