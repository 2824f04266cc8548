"""Cases, oracle and gate of the sliding-window decode attention (include/sqllm_hip.h, sqllm_attn_decode_window_*), built on
tests/attn_decode_cases.py by import only and shared by the CPU and the GPU tests.  No GPU and no library needed here.

A row of length L attends the keys [lo, L), lo = max(0, L - W).

  * `windowed(case, W)` -- a deep copy of a `build(...)` case (the cached original is not touched) in which, additionally, the K
                   and V elements of every key below each row's lo hold the case's NaN pattern, and the table entries of every
                   block wholly below lo hold the far-outside values `build` gives unused entries (1 << 30, -7): whoever looks
                   behind the window gets a NaN row.  `.window` is W, `.base` the original.
  * `oracle_w`  -- the contract in fp64 over [lo, L); `mutant` (MUTANTS_W): "one_below" attends lo - 1 too, "one_short" starts at
                   lo + 1, "no_window" attends [0, L) -- the keys behind the window read from `.base`, where they are values.
  * `model32_w` -- the same formulas in sequential fp32, the yardstick of the gate.
  * `reference_w` -- (want, gate): the gate of attn_decode_cases, unchanged: half an ulp of the output type + 4 x the largest
                   |fp32 model - oracle| of that (row, head) + 2^-24 x max|attended v|.  Pass: excess <= 1.
  * `model_parts_w` -- attn_decode_cases.model_parts with ABSOLUTE partition edges and a partial first partition: fp32 in the
                   kernels' structure.
  * `win_parts` -- the header's formula.
"""
import copy
import functools

import numpy as np
import torch

from tests import attn_decode_cases as AC

P = AC.P
INT32_MAX = (1 << 31) - 1
# (L, W): the smallest pairs at which the kernels can still go wrong
PAIRS = ((200, 50),           # the window inside partition 0
         (300, 100),          # lo in partition 0, the end in partition 1
         (P + 40, 40),        # lo = 256: the first partition skipped whole
         (P + 40, 41),        # lo = 255: one key in partition 0
         (P + 1, 1),          # a single key, the first of partition 1
         (P, 1),              # a single key, the last of partition 0
         (2 * P + 3, 2),      # a two-key window
         (2 * P + 3, P + 3),  # lo = 256, aligned: the shift identity
         (2 * P + 3, P + 100),  # three partitions = win_parts
         (3, P + 7))          # a row shorter than the window
SECOND_ROW = 7  # every pair's case has a second row of 7 keys: another first partition, and mostly a row inside the window
LONG_WINDOWS = (P + 7, 4 * P)  # on the LONG table: win_parts 3 and 5 of 18
MUTANTS_W = ("one_below", "one_short", "no_window")


def win_parts(max_blocks, block_size, window):
    n_parts = (min(max_blocks * block_size, INT32_MAX) + P - 1) // P
    return min(n_parts, (window - 1 + P - 1) // P + 1)


def lo_of(L, W):
    return max(0, int(L) - int(W))


def _served(case, b):
    L = int(case.lens[b])
    return 0 < L <= case.table.shape[1] * case.block_size


def windowed(case, W, poison=0):
    out = copy.deepcopy(case)
    out.base, out.window = case, int(W)
    bs = case.block_size
    hd = np.arange(case.H)[None, :, None] * case.head_stride + np.arange(case.D)[None, None, :]
    for b in range(case.B):
        if not _served(case, b):
            continue
        lo = lo_of(case.lens[b], W)
        if lo == 0:
            continue
        p = np.arange(lo)
        slot = case.table[b, p // bs] * bs + p % bs
        assert ((slot >= 0) & (slot < case.n_slots)).all()
        at = torch.from_numpy((AC.GUARD + slot[:, None, None] * case.slot_stride + hd).reshape(-1))
        nan = AC._poisoned(at.numel(), case.dtype, poison)
        out.k_buf[at] = nan
        out.v_buf[at] = nan
        for j in range(lo // bs):  # the blocks wholly below lo
            out.table[b, j] = -7 if j % 2 else 1 << 30
    assert not torch.equal(out.k_buf.view(torch.int16), case.k_buf.view(torch.int16)) or all(
        lo_of(case.lens[b], W) == 0 for b in range(case.B) if _served(case, b))
    return out


@functools.lru_cache(maxsize=None)
def pair_case(kind, L, W, D, HQ, H, dtype_name, poison=0):
    """the windowed two-row case of a pair (computed once, shared, left unchanged)"""
    return windowed(AC.build(kind, 2, D, HQ, H, dtype_name, poison, (L, SECOND_ROW)), W, poison)


@functools.lru_cache(maxsize=None)
def long_case(kind, W, D, HQ, H, dtype_name):
    return windowed(AC.build(kind, len(AC.LONG_LENS), D, HQ, H, dtype_name, 0, AC.LONG_LENS, AC.LONG), W)


def _rows_kv_w(case, b, first, L, k64, v64):
    """(k, v) [L - first, H, D] of keys first .. L-1 of row b, or None when the table leads outside the cache"""
    bs = case.block_size
    p = np.arange(first, L)
    slot = case.table[b, p // bs] * bs + p % bs
    if ((slot < 0) | (slot >= case.n_slots)).any():
        return None
    at = slot[:, None, None] * case.slot_stride + np.arange(case.H)[None, :, None] * case.head_stride + np.arange(case.D)[None, None, :]
    return k64[at], v64[at]


def _walk_w(case, fn, out_dtype, mutant=None):
    """out [B, HQ, D]: fn(q [G, D], k [n, D], v [n, D], first) per (row, kv head) over the attended keys first .. L-1, with the
    contract's corner rows; None where a mutant is not defined on the case (no row it changes)"""
    src = case.base if mutant in ("one_below", "no_window") else case  # (the keys behind the window, as values)
    G, W = case.HQ // case.H, case.window
    k64, v64 = (t[AC.GUARD:AC.GUARD + case.extent].double().numpy() for t in (src.k_buf, src.v_buf))
    q64 = case.q_buf[:, :case.HQ * case.D].double().numpy().reshape(case.B, case.H, G, case.D)
    out = np.zeros((case.B, case.HQ, case.D), dtype=out_dtype)
    vmax = np.zeros((case.B, case.HQ))
    changed = mutant is None
    for b in range(case.B):
        L = int(case.lens[b])
        if L <= 0:
            continue  # +0
        if L > case.table.shape[1] * case.block_size:
            out[b] = np.nan
            continue
        first = lo_of(L, W)
        if mutant == "one_below" and first >= 1:
            first, changed = first - 1, True
        elif mutant == "one_short" and first + 1 < L and L > W:
            first, changed = first + 1, True
        elif mutant == "no_window" and first > 0:
            first, changed = 0, True
        kv = _rows_kv_w(src, b, first, L, k64, v64)
        if kv is None:
            out[b] = np.nan
            continue
        k, v = kv
        for h in range(case.H):
            vmax[b, h * G:(h + 1) * G] = np.abs(v[:, h]).max()
            out[b, h * G:(h + 1) * G] = fn(q64[b, h], k[:, h], v[:, h], first)
    return (out, vmax) if changed else (None, None)


def oracle_w(case, mutant=None):
    """(want [B, HQ * D] fp64, max|attended v| [B, HQ]); (None, None) where `mutant` changes no row of the case"""
    def fn(q, k, v, first):
        s = case.scale * (q @ k.T)
        w = np.exp(s - s.max(axis=1, keepdims=True))
        return (w @ v) / w.sum(axis=1, keepdims=True)

    out, vmax = _walk_w(case, fn, np.float64, mutant)
    return (None, None) if out is None else (out.reshape(case.B, -1), vmax)


def model32_w(case):
    f = np.float32

    def fn(q, k, v, first):
        q, k, v = q.astype(f), k.astype(f), v.astype(f)
        s = f(case.scale) * np.cumsum(q[:, None, :] * k[None, :, :], axis=2, dtype=f)[:, :, -1]
        w = np.exp(s - s.max(axis=1, keepdims=True)).astype(f)
        acc = np.cumsum(w[:, :, None] * v[None, :, :], axis=1, dtype=f)[:, -1]
        return acc / np.cumsum(w, axis=1, dtype=f)[:, -1:]

    return _walk_w(case, fn, f)[0].reshape(case.B, -1)


def reference_w(case):
    """(want, gate) [B, HQ * D] of a windowed case: attn_decode_cases' gate, unchanged"""
    D = case.D
    want, vmax = oracle_w(case)
    m32 = model32_w(case).astype(np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(m32 - want).reshape(case.B, case.HQ, D)
    err = np.where(np.isnan(err), 0.0, err).max(axis=2, keepdims=True)
    g = AC.half_ulp(want, case.dtype).reshape(case.B, case.HQ, D) + 4.0 * err + 2.0 ** -24 * vmax[:, :, None]
    return want, g.reshape(case.B, -1)


@functools.lru_cache(maxsize=None)
def pair_reference(kind, L, W, D, HQ, H, dtype_name):
    case = pair_case(kind, L, W, D, HQ, H, dtype_name)
    return (case, *reference_w(case))


@functools.lru_cache(maxsize=None)
def long_reference(kind, W, D, HQ, H, dtype_name):
    case = long_case(kind, W, D, HQ, H, dtype_name)
    return (case, *reference_w(case))


def model_parts_w(case):
    """[B, HQ * D] fp32: attn_decode_cases.model_parts over the attended keys, cut at the ABSOLUTE partition edges (multiples of P:
    the first partition is partial where lo is no multiple of P), folded in ascending order"""
    f = np.float32
    per_lane = 16 if case.k_buf.dtype == torch.float64 else 8

    def fn(q, k, v, first):
        q, k, v = q.astype(f), k.astype(f), v.astype(f)
        x = np.cumsum((q[:, None, :] * k[None, :, :]).reshape(len(q), len(k), -1, per_lane), axis=3, dtype=f)[..., -1]
        while x.shape[2] > 1:
            x = (x[:, :, 0::2] + x[:, :, 1::2]).astype(f)
        s = f(case.scale) * x[:, :, 0]
        n = s.shape[1]
        edges = [0] + [e - first for e in range((first // P + 1) * P, first + n, P)] + [n]
        ms, ls, accs = [], [], []
        for i, j in zip(edges[:-1], edges[1:]):
            sp = s[:, i:j]
            m = sp.max(axis=1, keepdims=True)
            w = np.exp(sp - m).astype(f)
            ms.append(m)
            ls.append(w.sum(axis=1, keepdims=True, dtype=f))
            accs.append(w @ v[i:j])
        top = np.max(ms, axis=0)
        lsum, t = np.zeros((len(q), 1), f), np.zeros((len(q), v.shape[1]), f)
        for m, l, acc in zip(ms, ls, accs):
            wgt = np.exp(m - top).astype(f)
            lsum = (lsum + wgt * l).astype(f)
            t = (t + wgt * acc).astype(f)
        return t / lsum

    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return _walk_w(case, fn, f)[0].reshape(case.B, -1)
