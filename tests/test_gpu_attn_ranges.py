"""The four decode-attention entries on the GPU (sqllm_attn_decode_* / _fp8_* / sqllm_attn_append_* / _fp8_* behind
quant.DecodeAttention) in four regions the neighbouring files do not enter, on cases of tests/attn_decode_cases.py,
tests/kv_fp8_cases.py and tests/attn_append_cases.py, with their fp64 oracle and their gate unchanged (excess <= 1.0).
tests/test_attn_ranges_cpu.py shows that the gate is fair on these inputs and which wrong implementations it fails there.

  A. group ratios: n_heads / n_kv_heads = 1 .. 8 on the one-query entries (every group class of the launch ladder; 5, 6 and 7
     run the second round of the key-lane exchange with heads missing), two launches and one, both cache types; one NaN in
     the q of a group's last head reaches that head alone.
  B. sharp softmax (attn_decode_cases.sharpen): partitions whose maxima lie 60 and 120 apart, every score below -100 or above
     +100, one dominating key, two equal maxima in different partitions -- the max subtraction and the combine's rescale carry
     the result; the append entries on the same caches, bit for bit against the one-query entries and against the oracle.
  C. tables of 18 partitions with rows that use 18, 9, 1, 17 and none of them (most workgroups of the short row return without
     writing: the combine must not read their partials), and the served maximum of 64 rows.
  D. slots whose element (byte) offsets lie at and beyond 2^31 and 2^32, in one allocation of 2^32 + 2^20 elements that holds k
     and v interleaved: the bits of the same call over a compact cache; and the attention front writing such slots.
     The front takes no caches whose extents overlap (include/sqllm_hip.h, sqllm_kv_cache), so there k and v are the two halves of
     one allocation of twice the size.

In B, 21 of the 432 expansions (all fp16, 20 of them T = 16) use another draw of the new tokens' q than the first:
attn_append_cases.SHARP_DRAWS says why, and tests/test_attn_ranges_cpu.py derives the list from the fp32 model alone.  That model
(attn_decode_cases.model_parts) gave, on the CPU, the very figures the kernels then gave on those first draws (1.006 .. 2.613).

Observed on an MI355X, the largest excess per part in units of the gate (each case passes <= 1.0; the half-unit term alone
admits up to 1, and among several hundred outputs one nearly always sits next to a rounding boundary), 16-bit / e4m3 cache:
  A  fp16 0.998 / 0.999, bf16 1.000 / 1.000 to three places (64 cases each type)
  B  one query: 1.000 to three places for both types and caches (108 each); append T = 2 and 16: the same (216 each)
  C  18 partitions: fp16 0.998 / 0.998, bf16 0.999 / 0.999; 64 rows: inside those
  D  far slots: fp16 0.987 / 0.993, bf16 0.998 / 0.999; append T = 2: fp16 0.992 / 0.994, bf16 0.999 / 0.999;
     behind the front: fp16 0.984 / 0.991, bf16 0.998 / 0.996
All 312 tests ran, none skipped; no part found a defect in a kernel or in the host layer."""
import types

import numpy as np
import pytest

from tests import attn_append_cases as A
from tests import attn_decode_cases as C
from tests import kv_fp8_cases as F
from tests.test_gpu_attn_append import Dev as DevAppend
from tests.test_gpu_attn_decode import Dev as Dev16
from tests.test_gpu_attn_decode import _bits, _f64, _node_types, _poison_lds, _poison_workspaces
from tests.test_gpu_kv_fp8 import Dev as Dev8

gpu_test = pytest.mark.gpu
P = C.P
RATIOS = [(kind, D, hq, hk, dt) for kind in ("paged", "paged_single") for D in (64, 128) for hq, hk in C.ALL_HEADS for dt in C.DTYPES]
SHARP_SHAPES = ((64, 8, 2), (128, 4, 2), (64, 16, 2))
SHARP = [(kind, D, hq, hk, dt, prof) for kind in ("paged", "padded", "bhsd") for D, hq, hk in SHARP_SHAPES for dt in C.DTYPES
         for prof in C.PROFILES]
LONG = [(kind, D, hq, hk, dt) for kind in ("paged", "padded") for D, hq, hk in ((64, 8, 2), (128, 2, 2)) for dt in C.DTYPES]


def _one_query(gpu, fp8, ref16, ref8, *key):
    """(device operands, want, gate) of a one-query case over a 16-bit or an e4m3 cache"""
    if fp8:
        fc, want, gate = ref8(*key)
        return Dev8(gpu, fc), want, gate
    case, want, gate = ref16(*key)
    return Dev16(gpu, case), want, gate


def _checked(tag, y, want, gate):
    worst = C.excess(_f64(y), want, gate)
    print(f"ATTN_GATE ranges {tag}: {worst:.3f}")
    assert worst <= 1.0, worst


def _poisoned_rerun(d, att, y):
    _poison_workspaces(att)
    _poison_lds()
    assert np.array_equal(_bits(d.run(att)), _bits(y))


# ---- A. group ratios ----

@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("kind,D,hq,hk,dt", RATIOS)
def test_group_ratios_against_the_oracle(gpu, kind, D, hq, hk, dt, fp8):
    d, want, gate = _one_query(gpu, fp8, C.reference, F.reference, kind, 3, D, hq, hk, dt)
    att = d.module()
    y = d.run(att)
    assert y.shape == (3, hq * D)
    _checked(f"A {kind} D={D} heads={hq}/{hk} {dt} fp8={fp8}", y, want, gate)
    _poisoned_rerun(d, att, y)


@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("kind", ["paged", "paged_single"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("g", [2, 5, 8])
def test_a_nan_in_the_q_of_a_groups_last_head_reaches_that_head_alone(gpu, g, D, kind, dt, fp8):
    """head hk * g + g - 1 of either kv head (for g = 5 and 8 in the second round of the key-lane exchange): exactly its D
    outputs of one row become NaN, every other element keeps its bits"""
    hq = 2 * g
    d, _, _ = _one_query(gpu, fp8, C.reference, F.reference, kind, 3, D, hq, 2, dt)
    plain = _bits(d.run()).reshape(3, hq, D)
    for hk in (0, 1):
        head, row = hk * g + g - 1, (2 if kind == "paged" else 1)  # P + 1 keys: two partitions and the combine; P - 1: one launch
        keep = d.q[row, head * D + 7].clone()
        d.q[row, head * D + 7] = float("nan")
        y = d.run()
        got = _f64(y).reshape(3, hq, D)
        same = np.ones((3, hq, D), bool)
        same[row, head] = False
        assert np.isnan(got[row, head]).all() and np.isfinite(got[same]).all()
        assert np.array_equal(_bits(y).reshape(3, hq, D)[same], plain[same])
        d.q[row, head * D + 7] = keep
    assert np.array_equal(_bits(d.run()).reshape(3, hq, D), plain)


# ---- B. sharp softmax ----

@gpu_test
@pytest.mark.parametrize("kind,D,hq,hk,dt,prof", SHARP)
def test_sharp_softmax_on_the_four_entries(gpu, kind, D, hq, hk, dt, prof):
    """the one-query entries against the oracle of the sharpened case; the append entries (T = 2 and 16, forced to the kernels) on
    the same caches with q sharpened the same way: the one-query entries' bits on the expansion, and the oracle's values"""
    import torch

    for fp8 in (False, True):
        d, want, gate = _one_query(gpu, fp8, C.sharp_reference, F.sharp_reference, kind, D, hq, hk, dt, prof)
        _checked(f"B {prof} {kind} D={D} heads={hq}/{hk} {dt} fp8={fp8}", d.run(), want, gate)
        fc = d.fc if fp8 else None
        base = d.case  # (the sharpened 16-bit case; over bytes its q, and the geometry)
        assert base.sharp_c == (F.SHARP_C if fp8 else 8.0)
        for T in (2, 16):
            case = A.sharp_expand(base, T, fp8)  # (the first draw of the new tokens' q on all but the 21 cases of A.SHARP_DRAWS)
            shadow = A.sharp_expand(fc.shadow, T, fp8) if fp8 else case
            assert torch.equal(shadow.q_buf.view(torch.int16), case.q_buf.view(torch.int16))
            want_x, gate_x = C.reference_of(shadow)
            assert np.isfinite(want_x).all()
            da = DevAppend(gpu, base, case, fc)
            att = da.module()
            got = da.append(att)
            assert torch.equal(got.view(torch.int16), da.decode(att).view(torch.int16)), (fp8, T)
            _checked(f"B append T={T} {prof} {kind} D={D} heads={hq}/{hk} {dt} fp8={fp8}", got, want_x, gate_x)


# ---- C. long tables, short rows in long tables, 64 rows ----

@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("kind,D,hq,hk,dt", LONG)
def test_long_tables(gpu, kind, D, hq, hk, dt, fp8):
    import torch

    from squeezellm_amd import _lib

    d, want, gate = _one_query(gpu, fp8, C.long_reference, F.long_reference, kind, D, hq, hk, dt)
    case = d.case
    max_blocks, bs = case.table.shape[1], case.block_size
    assert case.B == 5 and (max_blocks * bs + P - 1) // P == 18
    att = d.module()
    y = d.run(att)
    _checked(f"C {kind} D={D} heads={hq}/{hk} {dt} fp8={fp8}", y, want, gate)
    got = _f64(y)
    assert (got[4] == 0).all() and not np.signbit(got[4]).any()
    _poisoned_rerun(d, att, y)  # (0xFF in every partial nobody wrote: the short rows' upper partitions)
    for b in range(case.B):  # a 1-row call: another batch size, the same row
        assert np.array_equal(_bits(d.run(rows=slice(b, b + 1))), _bits(y)[b:b + 1]), b
    assert _lib.attn_decode_workspace_bytes(case.B, hq, D, max_blocks, bs) == case.B * hq * 18 * (D + 2) * 4
    # captured: two kernel nodes (partials, combine), and the eager call's bits
    out = torch.empty((case.B, hq * D), dtype=case.dtype, device=gpu)
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        d.run(att, out=out)
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        d.run(att, out=out)
    assert _node_types(g) == [0, 0]  # hipGraphNodeTypeKernel
    g.instantiate()
    out.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out), _bits(y))
    # four new tokens per sequence over the same cache: the one-query entry's bits on the expansion
    fc = d.fc if fp8 else None
    da = DevAppend(gpu, case, A.expand(case, 4), fc)
    att4 = da.module()
    assert torch.equal(da.append(att4).view(torch.int16), da.decode(att4).view(torch.int16))


@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_sixty_four_rows(gpu, dt, fp8):
    lens = C.batch64_lens()
    if fp8:
        ref16, ref8, key = None, F.reference, ("paged", 64, 64, 8, 2, dt, F.SCALES, lens)
    else:
        ref16, ref8, key = C.reference, None, ("paged", 64, 64, 8, 2, dt, lens)
    d, want, gate = _one_query(gpu, fp8, ref16, ref8, *key)
    assert d.case.B == C.MAX_ROWS == 64
    att = d.module()
    y = d.run(att)
    _checked(f"C rows=64 {dt} fp8={fp8}", y, want, gate)
    for b in (0, 31, 63):
        assert np.array_equal(_bits(d.run(rows=slice(b, b + 1))), _bits(y)[b:b + 1]), b


# ---- D. offsets beyond 2^31 and 2^32 ----

FAR_ELEMS = (1 << 32) + (1 << 20)
FAR_H, FAR_D = 2, 64
FAR_SS = 2 * FAR_H * FAR_D  # k and v interleaved per slot: v's base lies H * D elements behind k's
FAR_SLOTS = FAR_ELEMS // FAR_SS
FAR_LENS = C.FAR_LENS


def _far_buffer(gpu, fp8, dtype, halves=False):
    """(buffer, k view, v view) as integers (int16 / uint8: torch indexes no float8) -- 2^32 + 2^20 elements on the GPU, never copied to
    the host, every element the NaN poison of attn_decode_cases / kv_fp8_cases; k and v interleaved slot by slot.  `halves`: twice
    as many elements in the one allocation, k's cache the first half and v's the second, each of tight slots of H * D -- for the
    attention front, which rejects caches whose extents overlap (include/sqllm_hip.h, sqllm_kv_cache)"""
    import torch

    free, _ = torch.cuda.mem_get_info(gpu)
    if free < 24 << 30:
        pytest.skip(f"offsets beyond 2^32 need an allocation of {FAR_ELEMS * (1 if fp8 else 2) >> 20} MiB: less than 24 GiB free")
    buf = torch.empty(FAR_ELEMS * (2 if halves else 1), dtype=torch.uint8 if fp8 else torch.int16, device=gpu)
    buf.fill_(F.NAN_BYTES[0] if fp8 else C.NAN_BITS[dtype][0])
    if halves:
        k, v = (buf[off:off + FAR_ELEMS].view(-1, FAR_H, FAR_D) for off in (0, FAR_ELEMS))
        return buf, k, v
    k, v = (buf.as_strided((FAR_SLOTS, FAR_H, FAR_D), (FAR_SS, FAR_D, 1), off) for off in (0, FAR_H * FAR_D))
    assert (FAR_SLOTS - 1) * FAR_SS + FAR_H * FAR_D + (FAR_H - 1) * FAR_D + FAR_D == FAR_ELEMS  # the last slot's v ends the allocation
    return buf, k, v


def _as_cache(view, fp8, dtype):
    import torch

    return view.view(torch.float8_e4m3fn if fp8 else dtype)


def _far_table(case):
    """the compact table with every used block id replaced: each row's blocks alternate between the three regions the two
    thresholds cut (element / byte offset 2^31 = block 2^19, 2^32 = block 2^20, blocks of 16 slots of 256), and block 0, the
    blocks on either side of each threshold and the very last block the buffer holds are all in use"""
    bs = case.block_size
    assert bs == 16 and bs * FAR_SS == 4096
    n_blocks, t1, t2 = FAR_SLOTS // bs, (1 << 31) // 4096, (1 << 32) // 4096
    rng = np.random.default_rng(2031)
    pools = [[lo, hi - 1] + sorted(rng.choice(np.arange(lo + 1, hi - 1), 24, replace=False).tolist(), reverse=True)
             for lo, hi in ((0, t1), (t1, t2), (t2, n_blocks))]
    table, pairs = case.table.copy(), []
    for b in range(case.B):
        for i in range((int(case.lens[b]) + bs - 1) // bs):
            far = pools[(i + b) % 3].pop(0)
            pairs.append((int(case.table[b, i]), far))
            table[b, i] = far
    used = {f for _, f in pairs}
    assert {0, t1 - 1, t1, t2 - 1, t2, n_blocks - 1} <= used and len(used) == len(pairs)
    for b in range(case.B):  # each row on both sides of both thresholds
        row = table[b, :(int(case.lens[b]) + bs - 1) // bs]
        assert (row < t1).any() and ((row >= t1) & (row < t2)).any() and (row >= t2).any()
    return table, pairs


def _scatter(pairs, far, compact, bs=16):
    import torch

    src = torch.tensor([c * bs + j for c, _ in pairs for j in range(bs)], device=far.device)
    dst = torch.tensor([f * bs + j for _, f in pairs for j in range(bs)], device=far.device)
    far[dst] = compact[src]


def _released(body, *args):
    """one far buffer at a time: the body's locals die with its frame, then the allocator gives the memory back"""
    import torch

    try:
        body(*args)
    finally:
        torch.cuda.empty_cache()


@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_slots_at_and_beyond_two_to_the_31_and_32(gpu, dt, fp8):
    _released(_far_attention, gpu, dt, fp8)


def _far_attention(gpu, dt, fp8):
    """the one-query and the append entry (T = 2) over the far cache: the oracle's values (it runs on the compact case) and the
    bits of the same kernels over the compact cache, on the first run and on a second.  Every slot used lies inside [0, n_slots)
    and inside the allocation."""
    import torch

    T = 2
    key = ("paged", 3, 64, 8, 2, dt) + ((F.SCALES,) if fp8 else ()) + (FAR_LENS,)
    d, want, gate = _one_query(gpu, fp8, C.reference, F.reference, *key)
    case = d.case
    assert (case.H, case.D, case.slot_stride, case.head_stride) == (FAR_H, FAR_D, FAR_H * FAR_D, FAR_D)
    fc = d.fc if fp8 else None
    kw = dict(k_scale=fc.k_scale, v_scale=fc.v_scale) if fp8 else {}
    x = A.expand(case, T)
    want_x, gate_x = C.reference_of(A.expand(fc.shadow, T) if fp8 else x)
    da = DevAppend(gpu, case, x, fc)
    att = da.module()
    near = d.run(att), da.append(att)
    table, pairs = _far_table(case)
    buf, k, v = _far_buffer(gpu, fp8, case.dtype)
    ints = torch.uint8 if fp8 else torch.int16
    _scatter(pairs, k, d.k.view(ints))
    _scatter(pairs, v, d.v.view(ints))
    c_last, f_last = max(pairs, key=lambda p: p[1])  # the last block of the buffer, read back flat: the scatter went where it should
    flat = buf[f_last * 4096:(f_last + 1) * 4096].view(16, 2, FAR_H * FAR_D)
    assert torch.equal(flat[:, 0].reshape(16, FAR_H, FAR_D), d.k.view(ints)[c_last * 16:(c_last + 1) * 16])
    assert torch.equal(flat[:, 1].reshape(16, FAR_H, FAR_D), d.v.view(ints)[c_last * 16:(c_last + 1) * 16])
    fk, fv = _as_cache(k, fp8, case.dtype), _as_cache(v, fp8, case.dtype)
    assert fk.shape[0] == FAR_SLOTS and int(table.max()) > FAR_SLOTS  # (the unused entries still lead outside)
    t_far = torch.from_numpy(table).to(torch.int32).to(gpu)
    for run in (1, 2):
        y = att(d.q, fk, fv, t_far, d.lens, **kw)
        assert att.last_route == "attn_decode"
        ya = att(da.q, fk, fv, t_far, da.seq, q_len=T, **kw)
        assert att.last_route == "attn_append"
        assert torch.equal(y.view(torch.int16), near[0].view(torch.int16)), run
        assert torch.equal(ya.view(torch.int16), near[1].view(torch.int16)), run
    _checked(f"D {dt} fp8={fp8}", y, want, gate)
    _checked(f"D append T={T} {dt} fp8={fp8}", ya, want_x, gate_x)


def _count_not(buf, value, chunk=1 << 28):
    """how many elements of `buf` differ from `value`, in chunks: no temporary approaches the buffer's size"""
    return sum(int((buf[a:a + chunk] != value).sum()) for a in range(0, buf.numel(), chunk))


@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_the_front_writes_two_tokens_beyond_two_to_the_32(gpu, dt, fp8):
    _released(_far_front, gpu, dt, fp8)


def _far_front(gpu, dt, fp8):
    """QuantQKVRopeFused (the K = 1024 operands of tests/test_gpu_qkv_rope.py, as test_three_decode_steps_behind_the_front) writes
    positions 0 and 1 of one sequence into the first slot wholly beyond element (byte) offset 2^32 and into the last slot of
    either cache (the two halves of one allocation: the front takes no caches that overlap): exactly those 2 x H x D elements of each of k and v differ from the poison afterwards, and the attention over them
    (blocks of one slot; rows of 1 and 2 keys) meets the oracle formed from what the cache holds"""
    import torch

    from squeezellm_amd import quant
    from tests import test_gpu_qkv_rope as TQ

    rows, (Nq, Nk, Nv, D) = 2, TQ.SHAPES["d64"]
    HQ, H = Nq // D, Nk // D
    assert (H, D) == (FAR_H, FAR_D)
    dtype = C.DTYPES[dt]
    front = TQ._module(TQ._members(gpu, 4, "hybrid", "d64"), D, "half", fused_members=True)
    att = quant.DecodeAttention(HQ, H, D, block_size=1)
    cos, sin = TQ._tables(D)
    x = TQ._x(gpu, rows, str(dtype).split(".")[1])
    ks, vs = float(torch.tensor(0.0421, dtype=torch.float32)), float(torch.tensor(0.0173, dtype=torch.float32))
    kw = dict(k_scale=ks, v_scale=vs) if fp8 else {}
    ss = H * D
    slots = [(1 << 32) // ss + 1, FAR_ELEMS // ss - 1]
    buf, k, v = _far_buffer(gpu, fp8, dtype, halves=True)
    assert slots[0] * ss > (1 << 32) and slots[0] < slots[1] < k.shape[0] == v.shape[0] and k.stride() == v.stride() == (ss, D, 1)
    poison = F.NAN_BYTES[0] if fp8 else C.NAN_BITS[dtype][0]
    assert _count_not(buf, poison) == 0
    fk, fv = _as_cache(k, fp8, dtype), _as_cache(v, fp8, dtype)
    tp, tc, ts = TQ._dev(gpu, [0, 1], cos, sin)
    q = front(x, tp, tc, ts, k_cache=fk, v_cache=fv, slots=torch.tensor(slots, dtype=torch.int32, device=gpu), **kw)[0]
    assert front.last_route == "qkv_rope"
    torch.cuda.synchronize()
    got_k, got_v = k[slots].cpu(), v[slots].cpu()  # [2, H, D] integers
    for got in (got_k, got_v):
        live = (got & 0x7F) != 0x7F if fp8 else torch.isfinite(got.view(dtype))
        assert bool(live.all())
    for half in (buf[:FAR_ELEMS], buf[FAR_ELEMS:]):  # ... and nothing else was written, in k's cache or in v's
        assert _count_not(half, poison) == rows * H * D
    table = torch.tensor([slots, slots], dtype=torch.int32, device=gpu)
    lens = torch.tensor([1, 2], dtype=torch.int32, device=gpu)
    y = att(q, fk, fv, table, lens, **kw)
    assert att.last_route == "attn_decode"
    host = types.SimpleNamespace(kind="far", dtype=dtype, B=rows, D=D, HQ=HQ, H=H, block_size=1, table=np.array([[0, 1], [0, 1]], dtype=np.int64),
                                 n_slots=2, slot_stride=ss, head_stride=D, extent=2 * ss, scale=float(D) ** -0.5, seed=[13, rows, D],
                                 q_buf=q.cpu(), q_stride=HQ * D, lens=np.array([1, 2]))
    bufs = []
    for got, scale in ((got_k, ks), (got_v, vs)):
        vals = F.decode(got.reshape(-1)).double() * scale if fp8 else got.reshape(-1).view(dtype)
        b = torch.full((2 * C.GUARD + 2 * ss,), float("nan"), dtype=vals.dtype)
        b[C.GUARD:C.GUARD + 2 * ss] = vals
        bufs.append(b)
    host.k_buf, host.v_buf = bufs
    want, gate = C.reference_of(host)
    assert np.isfinite(want).all()
    _checked(f"D front {dt} fp8={fp8}", y, want, gate)
    TQ._clean(front)
