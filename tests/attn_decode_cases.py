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

For tests/test_attn_ranges_cpu.py and tests/test_gpu_attn_ranges.py (all additive: the cases above keep their seeds and bits):
  * `build(..., capacity=)` -- tables for more than 2P + 3 keys (LONG: 18 partitions); ALL_HEADS: every group ratio 1 .. 8.
  * `sharpen`  -- a case whose scores leave N(0, 1) by a profile of PROFILES; `profile_conditions` asserts on the oracle's own
                  scores what the profile is there for.
  * `model_parts` -- fp32 in the kernels' structure (lane-wise dot products, partitions of P keys, an ascending combine) and
                  three wrong variants of it: the evidence that the gate is fair on a case, and that it sees the structure.
"""
import copy
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
# ---- the ranges of tests/test_attn_ranges_cpu.py and tests/test_gpu_attn_ranges.py ----
ALL_HEADS = tuple((2 * g, 2) for g in range(1, 9))  # every query / kv ratio the kernels serve; two kv heads: a neighbour's read shows
GROUP_MUTANTS = ("rotate_in_group",)  # wrong only inside a group: the identity at ratio 1, so not among MUTANTS ("at every shape")
PROFILES = ("ramp_up", "ramp_down", "all_low", "all_high", "spike", "tie")  # `sharpen`
SHARP_LENS = (2 * P + 3, P + 1, 7)
LONG = 17 * P + 5  # keys: 18 partitions
LONG_LENS = (LONG, 9 * P, 3, 16 * P + 1, 0)  # full; ends on an edge in the middle; 17 partitions unwritten; one key in the last; +0
FAR_LENS = (P + 1, 40, 2 * P + 3)  # the compact case behind the far offsets
PART_VARIANTS = ("no_max", "first_max", "no_rescale")  # `model_parts`


def _poisoned(n, dtype, poison):
    bits = NAN_BITS[dtype][poison]
    t = torch.full((n,), bits - (1 << 16) if bits >= (1 << 15) else bits, dtype=torch.int16).view(dtype)
    assert bool(torch.isnan(t).all())
    return t


def _geometry(kind, B, H, D, lens, rng, capacity=None):
    """(block_size, table [B, max_blocks] int64, n_slots, slot_stride, head_stride); `capacity`: the keys a table row must hold
    (2P + 3 where None)"""
    longest = 2 * P + 3 if capacity is None else int(capacity)
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
def build(kind, rows, D, HQ, H, dtype_name, poison=0, lens=None, capacity=None):
    dtype = DTYPES[dtype_name]
    if lens is None:
        lens = (SINGLE_ROW_LENGTHS if kind == "paged_single" else ROW_LENGTHS)[rows]
    lens = np.asarray(lens, dtype=np.int64)
    B = len(lens)
    seed = [GEOMETRIES.index(kind) if kind in GEOMETRIES else 7, rows, D, HQ, H, len(dtype_name), *[int(n) for n in lens]]
    if capacity is not None:  # (the cases without one keep their seeds)
        seed.append(int(capacity))
    rng = np.random.default_rng(seed)
    bs, table, n_slots, ss, hs = _geometry(kind, B, H, D, lens, rng, capacity)
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
                res = fn(q64[b, h], k[:, hk], v[:, hk])
                out[b, h * G:(h + 1) * G] = np.roll(res, -1, axis=0) if mutant == "rotate_in_group" else res  # head j: head (j+1) % G's
    return out, vmax


def oracle(case, mutant=None):
    """(want [B, HQ * D] fp64, max|attended v| [B, HQ]) -- the contract; `mutant`: one of MUTANTS or GROUP_MUTANTS, a deliberately wrong oracle"""
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


# ---- sharp softmax: scores far from N(0, 1), so that the max subtraction and the combine's rescale carry the result ----

def key_slots(case, b, n):
    """the slots of keys 0 .. n-1 of row b (a row the table serves)"""
    p = np.arange(n)
    slot = case.table[b, p // case.block_size] * case.block_size + p % case.block_size
    assert ((slot >= 0) & (slot < case.n_slots)).all()
    return slot


def profile_offsets(profile, n):
    """[n] fp64: what `profile` adds to the score of key p of a row of n keys"""
    p = np.arange(n)
    o = np.zeros(n)
    if profile == "ramp_up":
        o = 60.0 * (p // P)
    elif profile == "ramp_down":
        o = -60.0 * (p // P)
    elif profile == "all_low":
        o[:] = -150.0
    elif profile == "all_high":
        o[:] = 150.0
    elif profile == "spike":
        o[min(2 * P - 1, n - 1)] = 100.0
    elif profile == "tie":
        assert n >= 5
        o[3] = o[n - 1] = 100.0
    else:
        raise ValueError(profile)
    return o


def sharpen_q(case, c):
    """a copy of `case` whose q has the constant c in coordinate 0 of every query head (c exact in the case's type)"""
    out = copy.copy(case)
    out.q_buf = case.q_buf.clone()
    out.q_buf[:, 0:case.HQ * case.D:case.D] = c
    assert bool((out.q_buf[:, 0:case.HQ * case.D:case.D].double() == c).all())
    return out


def sharpen(case, profile, c=8.0):
    """A copy of a built case in which coordinate 0 of every query head is the constant c and coordinate 0 of key p of every kv
    head is profile_offsets(p) / (scale * c), rounded to the cache's type: every head's score becomes the offset plus the old
    N(0, 1) score (less its old first term).  "tie": the last key's whole k vector is a copy of key 3's first, so that the two
    top scores are the same fp64 number.  The oracle reads the stored values: the rounding of the offsets does not matter, and
    `profile_conditions` asserts on the oracle's own scores what the profile is there for."""
    out = sharpen_q(case, c)
    out.k_buf = case.k_buf.clone()
    out.profile, out.sharp_c = profile, float(c)
    hd = (np.arange(case.H)[None, :, None] * case.head_stride + np.arange(case.D)[None, None, :])
    for b in range(case.B):
        n = int(case.lens[b])
        if n <= 0:
            continue
        slot = key_slots(case, b, n)
        if profile == "tie":
            src, dst = (torch.from_numpy((GUARD + slot[i] * case.slot_stride + hd).reshape(-1)) for i in (3, n - 1))
            out.k_buf[dst] = out.k_buf[src]
        at = torch.from_numpy((GUARD + slot[:, None] * case.slot_stride + np.arange(case.H)[None, :] * case.head_stride).reshape(-1))
        vals = np.repeat(profile_offsets(profile, n) / (case.scale * c), case.H)
        out.k_buf[at] = torch.from_numpy(vals).to(case.dtype)
    return out


def scores64(case):
    """per row (None for a row without keys): the oracle's own fp64 scores [HQ, n]"""
    G = case.HQ // case.H
    k64 = case.k_buf[GUARD:GUARD + case.extent].double().numpy()
    q64 = case.q_buf[:, :case.HQ * case.D].double().numpy().reshape(case.B, case.H, G, case.D)
    out = []
    for b in range(case.B):
        n = int(case.lens[b])
        if n <= 0:
            out.append(None)
            continue
        k = _rows_kv(case, b, n, k64, k64)[0]  # [n, H, D]
        out.append(case.scale * np.einsum("hgd,nhd->hgn", q64[b], k).reshape(case.HQ, n))
    return out


def profile_conditions(case, profile, want):
    """what a profile is there for, asserted per (row, head) on the oracle's own fp64 scores of a case `sharpen` made; the bounds
    between partitions hold where a row HAS those partitions (consecutive maxima: two or more; first against last, 120 apart by
    construction: three or more), and every case must hold a row of three"""
    assert np.isfinite(want).all()
    three = False
    for s in scores64(case):
        if s is None:
            continue
        n = s.shape[1]
        top = np.sort(s, axis=1)
        if profile in ("ramp_up", "ramp_down"):
            m = np.stack([s[:, i:i + P].max(axis=1) for i in range(0, n, P)], axis=1)  # [HQ, parts]
            step = np.diff(m, axis=1) * (1.0 if profile == "ramp_up" else -1.0)
            assert (step > 50.0).all()
            if m.shape[1] >= 3:
                three = True
                assert (np.abs(m[:, -1] - m[:, 0]) > 89.0).all()
        elif profile == "all_low":
            assert (s < -100.0).all()
        elif profile == "all_high":
            assert (s > 100.0).all()
        elif profile == "spike":
            assert n == 1 or (top[:, -1] - top[:, -2] > 80.0).all()
        elif profile == "tie":
            assert (top[:, -1] == top[:, -2]).all() and (top[:, -1] - top[:, -3] > 80.0).all()
            assert (s[:, 3] == top[:, -1]).all() and (s[:, n - 1] == top[:, -1]).all()
    assert three or profile not in ("ramp_up", "ramp_down")


@functools.lru_cache(maxsize=None)
def sharp_reference(kind, D, HQ, H, dtype_name, profile, lens=SHARP_LENS):
    """(sharpened case, want, gate), its profile's conditions asserted -- computed once per case and shared"""
    case = sharpen(build(kind, len(lens), D, HQ, H, dtype_name, 0, lens), profile)
    want, gate = reference_of(case)
    profile_conditions(case, profile, want)
    return case, want, gate


# ---- the kernels' structure in fp32: partitions of P keys, then an ascending combine ----

def model_parts(case, variant=None):
    """[B, HQ * D] fp32: per partition of P keys the maximum, w = exp(s - m_part), the sum of w and w @ v; then m = the largest
    m_part and an ascending fold with exp(m_part - m) -- fp32 throughout.  `variant` (PART_VARIANTS) breaks it on purpose:
    "no_max" subtracts nothing anywhere, "first_max" takes m from partition 0, "no_rescale" folds with weights of 1."""
    f = np.float32
    per_lane = 16 if case.k_buf.dtype == torch.float64 else 8  # (a shadow of kv_fp8_cases: dequantised bytes)

    def fn(q, k, v):
        q, k, v = q.astype(f), k.astype(f), v.astype(f)
        # [G, n]; every dot product in the kernels' order: `per_lane` consecutive coordinates summed in turn (8 16-bit elements, 16
        # bytes: a lane's load), the lanes of a key then pairwise.  Equal keys have equal scores (a BLAS product does not promise
        # that, and "tie" would show it); and where two or three keys carry a row at scores beyond +-100, the order of a dot
        # product decides the result's last bits -- the model is to stand for the kernels there, not for model32
        x = np.cumsum((q[:, None, :] * k[None, :, :]).reshape(len(q), len(k), -1, per_lane), axis=3, dtype=f)[..., -1]
        while x.shape[2] > 1:
            x = (x[:, :, 0::2] + x[:, :, 1::2]).astype(f)
        s = f(case.scale) * x[:, :, 0]
        ms, ls, accs = [], [], []
        for i in range(0, s.shape[1], P):
            sp = s[:, i:i + P]
            m = np.zeros((len(q), 1), f) if variant == "no_max" else sp.max(axis=1, keepdims=True)
            w = np.exp(sp - m).astype(f)
            ms.append(m)
            ls.append(w.sum(axis=1, keepdims=True, dtype=f))
            accs.append(w @ v[i:i + P])
        top = ms[0] if variant == "first_max" else np.max(ms, axis=0)
        lsum, t = np.zeros((len(q), 1), f), np.zeros((len(q), v.shape[1]), f)
        for m, l, acc in zip(ms, ls, accs):
            wgt = np.ones_like(m) if variant == "no_rescale" else np.exp(m - top).astype(f)
            lsum = (lsum + wgt * l).astype(f)
            t = (t + wgt * acc).astype(f)
        return t / lsum

    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        return _walk(case, fn, f)[0].reshape(case.B, -1)


def rounded(x, dtype):
    """fp64 values of x rounded once to `dtype`"""
    return torch.from_numpy(np.asarray(x, dtype=np.float64)).to(dtype).double().numpy()


# ---- long tables and the served maximum of rows ----

MAX_ROWS = 64


@functools.lru_cache(maxsize=None)
def long_reference(kind, D, HQ, H, dtype_name):
    """(case, want, gate) of LONG_LENS in tables of LONG keys"""
    case = build(kind, len(LONG_LENS), D, HQ, H, dtype_name, 0, LONG_LENS, LONG)
    return (case, *reference_of(case))


def batch64_lens():
    return tuple(LENGTHS[i % len(LENGTHS)] for i in range(MAX_ROWS))
