"""Cases, oracle and tolerance of the decode attention (include/sqllm_hip.h, sqllm_attn_decode), shared by the CPU and the GPU
tests.  No GPU and no library needed here.

  * `oracle`   -- the contract in fp64 numpy: the table walk, the zero row, the NaN rows, max-subtracted softmax.
  * `model32`  -- the same formulas in plain fp32 numpy, one pass over ascending keys (every sum a sequential np.cumsum): what
                  a straightforward fp32 implementation loses against the oracle, the yardstick of the gate.
  * `build`    -- a case: caches inside guard-padded allocations in which EVERY unaddressed slot (beyond seq_lens, unused blocks,
                  the padding between strided heads and slots) and the guards hold NaN bit patterns; shuffled, non-monotonic
                  block tables whose unused entries lead far outside the cache; rows of different lengths; q strided, its
                  padding NaN.  The values do not depend on `poison`, only the NaN patterns do.
  * `gate`     -- per element: half a unit in the last place of the output type at |want| (the one rounding) + 4 x the largest
                  |fp32 model - fp64 oracle| of that (row, head) + 2^-24 x max|attended v| of that (row, kv head).
"""
import functools
import types

import numpy as np
import torch

from squeezellm_amd._lib import ATTN_PARTITION as P

LENGTHS = (1, 2, P - 1, P, P + 1, 2 * P + 3)
# rows -> per-row lengths: all six lengths occur, no case consists of length-1 rows alone (one key: every weight is 1 and
# neither the scale nor the precision of a score can show)
ROW_LENGTHS = {1: (2 * P + 3,), 3: (1, P, P + 1), 5: (2, P - 1, 1, 2 * P + 3, P)}
SINGLE_ROW_LENGTHS = {1: (P,), 3: (1, P - 1, 2), 5: (2, P - 1, 1, P, 17)}  # for the one-partition geometry (capacity P)
HEADS = ((2, 2), (8, 2), (6, 2))
GEOMETRIES = ("paged", "bhsd", "padded")
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}
NAN_BITS = {torch.float16: (0x7E01, 0xFE55), torch.bfloat16: (0x7FC1, 0xFFD5)}  # two different poisons per type
GUARD = 4096  # elements in front of and behind every cache
MUTANTS = ("drop_last", "extra_key", "neighbour_group", "no_scale", "fp16_scores")


def _poisoned(n, dtype, poison):
    bits = NAN_BITS[dtype][poison]
    t = torch.full((n,), bits - (1 << 16) if bits >= (1 << 15) else bits, dtype=torch.int16).view(dtype)
    assert bool(torch.isnan(t).all())
    return t


def _geometry(kind, B, H, D, lens, rng):
    """(block_size, table [B, max_blocks] int64, n_slots, slot_stride, head_stride)"""
    longest = 2 * P + 3
    if kind == "bhsd":  # head-major static [B, H, S, D] through kv_cache_view(cache, "bhsd") and static_cache_blocks
        S = longest
        table = (np.arange(B, dtype=np.int64) * H).reshape(B, 1)
        return S, table, (B - 1) * H * S + S, D, S * D
    if kind in ("paged", "paged_single"):  # [blocks, 16, H, D], slot-major
        bs, ss, hs = 16, H * D, D
        max_blocks = (longest + bs - 1) // bs if kind == "paged" else P // bs
    elif kind == "padded":  # slot-major with padding between heads and slots; 5 keys per block: blocks straddle partitions
        bs, ss, hs = 5, H * (D + 3) + 5, D + 3
        max_blocks = (longest + bs - 1) // bs + 2
    else:
        raise ValueError(kind)
    need = [(int(n) + bs - 1) // bs for n in lens]
    n_blocks = sum(need) + 3  # three blocks nobody uses
    ids = rng.permutation(n_blocks)[: sum(need)]  # shuffled, non-monotonic
    table = np.full((B, max_blocks), 1 << 30, dtype=np.int64)  # unused entries lead far outside the cache
    table[:, 1::2] = -7
    at = 0
    for b, n in enumerate(need):
        table[b, :n] = ids[at:at + n]
        at += n
    return bs, table, n_blocks * bs, ss, hs


@functools.lru_cache(maxsize=None)
def build(kind, rows, D, HQ, H, dtype_name, poison=0, lens=None):
    dtype = DTYPES[dtype_name]
    if lens is None:
        lens = (SINGLE_ROW_LENGTHS if kind == "paged_single" else ROW_LENGTHS)[rows]
    lens = np.asarray(lens, dtype=np.int64)
    B = len(lens)
    seed = [GEOMETRIES.index(kind) if kind in GEOMETRIES else 7, rows, D, HQ, H, len(dtype_name), *[int(n) for n in lens]]
    rng = np.random.default_rng(seed)
    bs, table, n_slots, ss, hs = _geometry(kind, B, H, D, lens, rng)
    extent = (n_slots - 1) * ss + (H - 1) * hs + D
    k_buf, v_buf = (_poisoned(GUARD + extent + GUARD, dtype, poison) for _ in range(2))
    W = HQ * D
    q_stride = W + 6
    q_buf = _poisoned(B * q_stride, dtype, poison).reshape(B, q_stride)
    q_buf[:, :W] = torch.from_numpy(rng.standard_normal((B, W))).to(dtype)
    d = np.arange(D)
    for b in range(B):
        p = np.arange(max(int(lens[b]), 0))
        p = p[p < table.shape[1] * bs]
        slot = table[b, p // bs] * bs + p % bs
        slot = slot[(slot >= 0) & (slot < n_slots)]
        at = torch.from_numpy((GUARD + slot[:, None, None] * ss + np.arange(H)[None, :, None] * hs + d[None, None, :]).reshape(-1))
        k_buf[at] = torch.from_numpy(rng.standard_normal(at.numel())).to(dtype)
        v_buf[at] = torch.from_numpy(rng.standard_normal(at.numel())).to(dtype)
    return types.SimpleNamespace(kind=kind, dtype=dtype, B=B, D=D, HQ=HQ, H=H, block_size=bs, table=table, lens=lens, n_slots=n_slots,
                                 slot_stride=ss, head_stride=hs, extent=extent, k_buf=k_buf, v_buf=v_buf, q_buf=q_buf, q_stride=q_stride,
                                 scale=float(D) ** -0.5, seed=seed)


def cache_view(case, buf):
    """the [n_slots, H, D] view of a case's cache inside its guarded buffer (on whatever device `buf` lives)"""
    return buf.as_strided((case.n_slots, case.H, case.D), (case.slot_stride, case.head_stride, 1), GUARD)


def bhsd_cache(case, buf):
    """the contiguous [B, H, S, D] tensor a "bhsd" case's buffer holds"""
    S = case.block_size
    return buf[GUARD:GUARD + case.B * case.H * S * case.D].view(case.B, case.H, S, case.D)


def _rows_kv(case, b, n, k64, v64):
    """(k, v) [n, H, D] of the first n keys of row b, or None when the table leads outside the cache"""
    bs = case.block_size
    p = np.arange(n)
    slot = case.table[b, p // bs] * bs + p % bs
    if ((slot < 0) | (slot >= case.n_slots)).any():
        return None
    at = slot[:, None, None] * case.slot_stride + np.arange(case.H)[None, :, None] * case.head_stride + np.arange(case.D)[None, None, :]
    return k64[at], v64[at]


def _walk(case, fn, out_dtype, mutant=None):
    """out [B, HQ, D]: fn(q [G, D], k [n, D], v [n, D]) per (row, kv head), with the contract's corner rows"""
    G = case.HQ // case.H
    k64, v64 = (t[GUARD:GUARD + case.extent].double().numpy() for t in (case.k_buf, case.v_buf))
    q64 = case.q_buf[:, :case.HQ * case.D].double().numpy().reshape(case.B, case.H, G, case.D)
    out = np.zeros((case.B, case.HQ, case.D), dtype=out_dtype)
    vmax = np.zeros((case.B, case.HQ))
    rng = np.random.default_rng(case.seed + [99])
    for b in range(case.B):
        n = int(case.lens[b])
        if n <= 0:
            continue  # +0
        if n > case.table.shape[1] * case.block_size:
            out[b] = np.nan
            continue
        kv = _rows_kv(case, b, n, k64, v64)
        if kv is None:
            out[b] = np.nan
            continue
        k, v = kv
        extra = rng.standard_normal((2, case.H, case.D))
        if mutant == "drop_last":
            k, v = k[:-1], v[:-1]
        elif mutant == "extra_key":  # one key of an unattended slot, finite values substituted for its poison
            k, v = np.concatenate((k, extra[:1]), 0), np.concatenate((v, extra[1:]), 0)
        for h in range(case.H):
            hk = (h + 1) % case.H if mutant == "neighbour_group" else h
            vmax[b, h * G:(h + 1) * G] = np.abs(v[:, hk]).max() if len(v) else 0.0
            if len(k):
                out[b, h * G:(h + 1) * G] = fn(q64[b, h], k[:, hk], v[:, hk])
    return out, vmax


def oracle(case, mutant=None):
    """(want [B, HQ * D] fp64, max|attended v| [B, HQ]) -- the contract; `mutant`: one of MUTANTS, a deliberately wrong oracle"""
    scale = 1.0 if mutant == "no_scale" else case.scale

    def fn(q, k, v):
        s = scale * (q @ k.T)  # [G, n]
        if mutant == "fp16_scores":
            s = s.astype(np.float16).astype(np.float64)
        w = np.exp(s - s.max(axis=1, keepdims=True))
        return (w @ v) / w.sum(axis=1, keepdims=True)

    out, vmax = _walk(case, fn, np.float64, mutant)
    return out.reshape(case.B, -1), vmax


def model32(case):
    """[B, HQ * D] fp32: the same formulas in plain fp32, one pass, ascending keys and ascending d, every sum sequential"""
    f = np.float32

    def fn(q, k, v):
        q, k, v = q.astype(f), k.astype(f), v.astype(f)
        s = f(case.scale) * np.cumsum(q[:, None, :] * k[None, :, :], axis=2, dtype=f)[:, :, -1]  # [G, n]
        w = np.exp(s - s.max(axis=1, keepdims=True)).astype(f)
        acc = np.cumsum(w[:, :, None] * v[None, :, :], axis=1, dtype=f)[:, -1]  # [G, D]
        return acc / np.cumsum(w, axis=1, dtype=f)[:, -1:]

    return _walk(case, fn, f)[0].reshape(case.B, -1)


def half_ulp(x, dtype):
    """half a unit in the last place of `dtype` at |x| (fp64 array)"""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    a = np.abs(np.where(np.isfinite(x), x, 1.0))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** emin)))
    return 0.5 * 2.0 ** (e - mant)


@functools.lru_cache(maxsize=None)
def reference(kind, rows, D, HQ, H, dtype_name, lens=None):
    """(case, want, gate) -- computed once per case and shared"""
    case = build(kind, rows, D, HQ, H, dtype_name, 0, lens)
    return (case, *reference_of(case))


def reference_of(case):
    """(want, gate) of a case: the oracle and the docstring's gate, [B, HQ * D]"""
    D = case.D
    want, vmax = oracle(case)
    m32 = model32(case).astype(np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(m32 - want).reshape(case.B, case.HQ, D)
    err = np.where(np.isnan(err), 0.0, err).max(axis=2, keepdims=True)
    g = half_ulp(want, case.dtype).reshape(case.B, case.HQ, D) + 4.0 * err + 2.0 ** -24 * vmax[:, :, None]
    return want, g.reshape(case.B, -1)


def excess(got, want, gate_):
    """max over elements of |got - want| / gate (0 where both are NaN; inf where only one is, or where a zero row is not +0)"""
    got = np.asarray(got, dtype=np.float64)
    nan_w, nan_g = np.isnan(want), np.isnan(got)
    if (nan_w != nan_g).any():
        return float("inf")
    with np.errstate(invalid="ignore"):
        r = np.abs(got - want) / gate_
    return float(np.where(nan_w, 0.0, r).max())
