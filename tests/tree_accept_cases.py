"""Cases and loop references of sqllm_tree_accept and sqllm_kv_compact (include/sqllm_hip.h), shared by the CPU and the GPU tests.
Plain Python over numpy copies, written from the header's semantics; integers and bytes only, so every comparison is exact."""
import numpy as np

from tests import attn_tree_cases as TC

TREES = tuple(t for t in TC.TREES if t != "no_tree")
SIZES = (1, 5, 17, 33, 64)


def _closure(par, t):
    out = []
    while t >= 0:
        out.append(t)
        t = par[t]
    return out


def accept_batch(tree, T):
    """(parents, words, draft, target, q_lens) as nested lists, one sequence per property: only the root matches; the deepest
    leaf's whole path; everything matches (equal-depth leaves: the lowest wins); a mismatch in the middle of the deepest path;
    the path to node T - 1 (beyond bit 31 from T = 33 on); padding nodes whose tokens would match; no node at all"""
    par, words = TC.parents(tree, T), TC.words(tree, T)
    deepest = max(range(T), key=lambda t: (len(_closure(par, t)), -t))
    deep = _closure(par, deepest)
    matching = [{0}, set(deep), set(range(T)), set(deep) - {deep[len(deep) // 2]} | {0}, set(_closure(par, T - 1)), set(range(T)), set(range(T))]
    q_lens = [T, T, T, T, T, (T + 1) // 2, 0]
    draft, target = [], []
    for b, ok in enumerate(matching):
        tgt = [1000 + 7 * t + b for t in range(T)]
        draft.append([5 if par[t] < 0 else tgt[par[t]] + (t not in ok) for t in range(T)])
        target.append(tgt)
    return [par] * len(matching), [words] * len(matching), draft, target, q_lens


def accept_ref(par, words, draft, target, q_lens, T, seq=None):
    """(accept_len, path, next_token, seq_out) by the header's formulas, a loop per sequence and node"""
    alen, path, nxt, out = [], [], [], []
    for b in range(len(par)):
        n = T if q_lens is None else q_lens[b]
        best, W = -1, 0
        if 0 < n <= T:
            w = [(words[b][t] | 1 << t) & ((1 << n) - 1) for t in range(n)]
            M = sum(1 << t for t in range(n) if par[b][t] < 0 or (par[b][t] < t and draft[b][t] == target[b][par[b][t]]))
            for t in range(n):
                if w[t] & ~M == 0 and bin(w[t]).count("1") > bin(W).count("1"):
                    best, W = t, w[t]
        nodes = [j for j in range(64) if W >> j & 1]
        alen.append(len(nodes))
        path.append(nodes + [-1] * (T - len(nodes)))
        nxt.append(target[b][best] if best >= 0 else -1)
        if seq is not None:
            out.append(seq[b] if n > T else seq[b] - max(n, 0) + len(nodes))
    return alen, path, nxt, out


def geometry(kind, B, H, D, keys):
    """(block_size, table [B, max_blocks], n_slots, slot_stride, head_stride) for `keys` keys per sequence: block size 16 and shuffled
    blocks, slot-major -- "paged" dense, "padded" with head_stride = D + 3, "pad4" with D + 4 --, or the head-major static "bhsd" """
    if kind == "bhsd":
        return keys, (np.arange(B, dtype=np.int64) * H).reshape(B, 1), (B - 1) * H * keys + keys, D, keys * D
    pad = {"paged": 0, "padded": 3, "pad4": 4}[kind]
    blocks = (keys + 15) // 16
    ids = np.random.default_rng(B * 131 + D).permutation(B * blocks + 3)[:B * blocks]
    return 16, ids.reshape(B, blocks).astype(np.int64), (B * blocks + 3) * 16, H * (D + pad) + (5 if pad == 3 else pad), D + pad


def pattern(n, cache, elem_bytes):
    """n elements of a cache buffer as raw integers (int16 or uint8): a function of (cache, index) in which neighbouring rows, slots and
    caches differ and every bit pattern of the element occurs, NaN and inf among them"""
    i = np.arange(n, dtype=np.int64)
    v = i * (40503 if elem_bytes == 2 else 167) + (i >> 8) * 101 + (i >> 16) * 7919 + cache * 977
    return (v & 0xFFFF).astype(np.uint16).view(np.int16) if elem_bytes == 2 else (v & 0xFF).astype(np.uint8)


def compact_batch(T=64):
    """(contexts, q_lens, accept_len, path [B, T]) of one batch: the shift chain (the read-before-write hazard); a sparse path; a prefix
    (nothing moves); a = 0; a > n_b (untouched); an entry below its index (skipped); a sequence for a bad table entry (BAD_KEY)"""
    paths = [list(range(1, T)), [0, 5, T - 1], [0, 1, 2, 3], [3, 4], list(range(1, 12)), [2, 0, 5], [1, 40, T - 1]]
    alen = [T - 1, 3, 4, 0, 11, 3, 3]
    path = np.full((len(paths), T), -1, dtype=np.int32)
    for b, p in enumerate(paths):
        path[b, :len(p)] = p
    return [14, 255, 0, 14, 0, 255, 14], [T, T, T, T, 10, T, T], alen, path


BAD_KEY = (6, 14 + 40)  # (sequence, key): its table entry leads outside the cache in the GPU test


def compact_ref(bufs, base, geo, H, D, seq, q_lens, T, path, alen):
    """sqllm_kv_compact on numpy element buffers (one per cache, the cache beginning at element `base`), in place: per sequence every
    source row is copied out before a destination is written"""
    bs, table, n_slots, ss, hs = geo
    cap = table.shape[1] * bs

    def slot(b, p):
        if p >= cap:
            return None
        s = int(table[b, p // bs]) * bs + p % bs
        return s if 0 <= s < n_slots else None

    for b in range(len(seq)):
        n, a = (T if q_lens is None else q_lens[b]), alen[b]
        ctx = seq[b] - n
        if n <= 0 or n > T or ctx < 0 or a <= 0 or a > n:
            continue
        moves = []
        for j in range(a):
            s = int(path[b, j])
            if s <= j or s >= n:
                continue
            src, dst = slot(b, ctx + s), slot(b, ctx + j)
            if src is not None and dst is not None:
                moves.append((src, dst))
        for buf in bufs:
            old = [[buf[base + src * ss + h * hs:base + src * ss + h * hs + D].copy() for h in range(H)] for src, _ in moves]
            for rows, (_, dst) in zip(old, moves):
                for h in range(H):
                    buf[base + dst * ss + h * hs:base + dst * ss + h * hs + D] = rows[h]
