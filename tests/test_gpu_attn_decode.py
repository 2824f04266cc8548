"""The decode attention on the GPU (sqllm_attn_decode_f16 / _bf16 behind quant.DecodeAttention; include/sqllm_hip.h,
sqllm_attn_decode), against the fp64 oracle of tests/attn_decode_cases.py on that file's cases: caches inside guard-padded
allocations whose every unaddressed slot holds NaN bit patterns, shuffled block tables whose unused entries lead far outside
the cache, rows of different lengths around the kernel's partition length P (imported, not retyped), a strided q.

Geometries: "paged" (blocks of 16, shuffled), "bhsd" (head-major static, S = 2P + 3, through kv_cache_view and
static_cache_blocks), "padded" (slot-major, both strides beyond their minimum and no multiple of 16 bytes, blocks of 5 keys: they
straddle partitions and the divide is no shift), and "paged_single" (a table of exactly P keys: the one-kernel path).

The gate is that file's, per element: half a unit in the last place of the output type at |want| + 4 x the largest
|fp32 model - fp64 oracle| of that (row, head) + 2^-24 x max|attended v|.  tests/test_attn_decode_cpu.py shows that five wrong
oracles fail it on these inputs at every shape.  Observed maximum on an MI355X, in units of the gate: 0.998 (fp16), 1.000 to
three places (bf16); test_parity_with_the_oracle's docstring."""
import copy
import ctypes
import types

import numpy as np
import pytest

from tests import attn_decode_cases as C

gpu_test = pytest.mark.gpu
P = C.P
PARITY = [(kind, rows, D, hq, hk, dt) for kind in C.GEOMETRIES + ("paged_single",) for rows in (1, 3, 5) for D in (64, 128)
          for hq, hk in C.HEADS for dt in C.DTYPES]
FIVE = [(kind, 5, D, hq, hk, dt) for kind in C.GEOMETRIES + ("paged_single",) for D, hq, hk in ((128, 8, 2), (64, 6, 2)) for dt in C.DTYPES]


class Dev:
    """a case's operands on the GPU: the guarded cache buffers and their views, q (strided), table and lengths as int32"""

    def __init__(self, gpu, case):
        import torch

        from squeezellm_amd import quant

        self.case = case
        self.k_buf, self.v_buf, self.q_buf = case.k_buf.to(gpu), case.v_buf.to(gpu), case.q_buf.to(gpu)
        if case.kind == "bhsd":  # the library's own view of the static cache, and its own table
            self.k, self.v = (quant.kv_cache_view(C.bhsd_cache(case, t), "bhsd") for t in (self.k_buf, self.v_buf))
            self.table = quant.static_cache_blocks(case.B, case.H, gpu)
            assert np.array_equal(self.table.cpu().numpy(), case.table)
            assert self.k.shape[0] == case.n_slots and self.k.stride() == (case.slot_stride, case.head_stride, 1)
        else:
            self.k, self.v = (C.cache_view(case, t) for t in (self.k_buf, self.v_buf))
            self.table = torch.from_numpy(case.table).to(torch.int32).to(gpu)
        self.q = self.q_buf[:, :case.HQ * case.D]
        self.lens = torch.from_numpy(case.lens).to(torch.int32).to(gpu)

    def module(self):
        from squeezellm_amd.quant import DecodeAttention

        c = self.case
        return DecodeAttention(c.HQ, c.H, c.D, block_size=c.block_size)

    def run(self, att=None, rows=slice(None), out=None):
        att = att or self.module()
        y = att(self.q[rows], self.k, self.v, self.table[rows], self.lens[rows], out=out)
        assert att.last_route == "attn_decode"
        return y


def _bits(t):
    import torch

    return t.contiguous().view(torch.int16).cpu().numpy()


def _f64(t):
    return t.double().cpu().numpy()


def _node_types(g):
    hip = ctypes.CDLL("libamdhip64.so")
    raw = ctypes.c_void_p(g.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) == 0
    out = []
    for nd in nodes:
        ty = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(nd), ctypes.byref(ty)) == 0
        out.append(ty.value)
    return out


def _poison_lds():
    """the LDS of every CU filled with a pattern (tests/native/lds_poison.hip through tests/conftest.py), in front of a launch"""
    import torch

    from tests.conftest import POISON_PATTERNS, _lds_poison_lib

    lds = _lds_poison_lib()
    if lds:
        sink = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        assert lds.lds_poison(torch.cuda.current_stream().cuda_stream, POISON_PATTERNS[0], sink.data_ptr()) == 0
        torch.cuda.synchronize()
        assert int(sink[0]) == 0


def _poison_workspaces(att):
    """the header says the workspace's contents are irrelevant: every buffer the module holds is filled with NaN patterns"""
    import torch

    for ws in att.__dict__.get("_ws", {}).values():
        if isinstance(ws, torch.Tensor):
            ws.fill_(0xFF)


# ---- 1. parity ----

@gpu_test
@pytest.mark.parametrize("kind,rows,D,hq,hk,dt", PARITY)
def test_parity_with_the_oracle(gpu, kind, rows, D, hq, hk, dt):
    """Observed on an MI355X over all cases of this test: the largest |got - want| is 0.998 of the gate for fp16 and 1.000 to
    three places for bf16 (each case passes <= 1; the half-unit term alone admits up to 1, and among several hundred outputs
    one nearly always sits next to a rounding boundary); the smallest per-case maximum is 0.95.  The first run, a run on
    poisoned workspaces and LDS, and a third run give the same bits."""
    import torch

    case, want, gate = C.reference(kind, rows, D, hq, hk, dt)
    d = Dev(gpu, case)
    att = d.module()
    y = d.run(att)
    torch.cuda.synchronize()
    assert y.dtype == case.dtype and y.shape == (case.B, hq * D)
    worst = C.excess(_f64(y), want, gate)
    print(f"ATTN_GATE {kind} rows={rows} D={D} heads={hq}/{hk} {dt}: {worst:.3f}")
    assert worst <= 1.0, worst
    _poison_workspaces(att)
    _poison_lds()
    y2 = d.run(att)
    assert np.array_equal(_bits(y2), _bits(y))
    assert len(att.__dict__["_ws"]) >= 1 and np.array_equal(_bits(d.run(att)), _bits(y))


# ---- 2. isolation ----

@gpu_test
@pytest.mark.parametrize("kind,rows,D,hq,hk,dt", FIVE)
def test_rows_alone_other_poison_and_a_second_run_give_the_same_bits(gpu, kind, rows, D, hq, hk, dt):
    import torch

    case = C.build(kind, rows, D, hq, hk, dt)
    d = Dev(gpu, case)
    y = _bits(d.run())
    for b in range(case.B):  # a 1-row call: another batch size, the same row
        assert np.array_equal(_bits(d.run(rows=slice(b, b + 1))), y[b:b + 1]), b
    other = C.build(kind, rows, D, hq, hk, dt, 1)
    assert not torch.equal(other.k_buf.view(torch.int16), case.k_buf.view(torch.int16))
    assert not torch.equal(other.q_buf.view(torch.int16), case.q_buf.view(torch.int16))
    assert np.array_equal(_bits(Dev(gpu, other).run()), y)
    assert np.array_equal(_bits(d.run()), y)


# ---- 3. writes ----

@gpu_test
@pytest.mark.parametrize("kind,rows,D,hq,hk,dt", FIVE)
def test_nothing_but_the_addressed_elements_of_out_is_written(gpu, kind, rows, D, hq, hk, dt):
    """out: rows 11 elements wider than they need be, inside a guarded allocation with a per-element distinct pattern; q is
    strided too (its padding NaN); the inputs are left as they were"""
    import torch

    case, want, gate = C.reference(kind, rows, D, hq, hk, dt)
    d = Dev(gpu, case)
    W, stride, guard = hq * D, hq * D + 11, 512
    total = guard + case.B * stride + guard
    pattern = (torch.arange(total, dtype=torch.int32) * 7 + 3).to(torch.int16).to(gpu)
    backing = pattern.clone().view(case.dtype)
    out = backing[guard:guard + case.B * stride].view(case.B, stride)[:, :W]
    assert d.q.stride(0) > W and out.stride(0) > W
    before = [t.clone() for t in (d.k_buf, d.v_buf, d.q_buf, d.table, d.lens)]
    y = d.run(out=out)
    torch.cuda.synchronize()
    assert y is out and C.excess(_f64(out), want, gate) <= 1.0
    touched = torch.zeros(total, dtype=torch.bool, device=gpu)
    touched[guard:guard + case.B * stride].view(case.B, stride)[:, :W] = True
    assert torch.equal(backing.view(torch.int16)[~touched], pattern[~touched])
    for t, b in zip((d.k_buf, d.v_buf, d.q_buf), before):
        assert torch.equal(t.view(torch.int16), b.view(torch.int16))
    assert torch.equal(d.table, before[3]) and torch.equal(d.lens, before[4])
    assert np.array_equal(_bits(out), _bits(d.run()))  # the strides change no bit


# ---- 4. corners ----

@gpu_test
@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("kind", ["paged", "padded", "paged_single"])
def test_zero_rows_nan_rows_and_their_neighbours(gpu, kind, dt):
    """seq_lens of 0 -> +0; a length beyond the table's capacity -> NaN; a table entry that leads outside the cache -> NaN (above
    and below); the neighbours are what they are without them, bit for bit.  Nothing out of range is read: the contract, not a
    provocation -- the kernel decides on the table's values before it touches the caches."""
    import torch

    long_ = P if kind == "paged_single" else 2 * P + 3
    lens = (0, 5, 40, long_, 3)
    base, want0, gate0 = C.reference(kind, 5, 64, 8, 2, dt, lens)
    d = Dev(gpu, base)
    plain = _bits(d.run())
    assert C.excess(_f64(d.run()), want0, gate0) <= 1.0
    bs, cap = base.block_size, base.table.shape[1] * base.block_size
    for entry in (base.n_slots // bs, -1, (1 << 31) - 1, -(1 << 31)):  # the first block outside, below, and where 32 bits would wrap
        case = copy.copy(base)
        case.lens = np.array([0, 5, cap + 1, long_, 3])
        case.table = base.table.copy()
        case.table[3, 7] = entry
        d.lens.copy_(torch.from_numpy(case.lens).to(torch.int32))
        d.table[3, 7] = entry
        want, _ = C.oracle(case)
        y = d.run()
        got = _f64(y)
        assert (got[0] == 0).all() and not np.signbit(got[0]).any()
        assert np.isnan(got[2]).all() and np.isnan(got[3]).all() and np.isnan(want[[2, 3]]).all()
        assert np.array_equal(_bits(y)[[1, 4]], plain[[1, 4]])
    d.lens[2] = (1 << 31) - 1
    assert np.isnan(_f64(d.run())[2]).all()
    d.lens[2] = -5
    got = _f64(d.run())
    assert (got[2] == 0).all() and not np.signbit(got[2]).any()


@gpu_test
@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_the_static_cache_at_and_beyond_its_capacity(gpu, dt):
    """"bhsd": a row of exactly S keys is served, S + 1 is NaN and reads nothing of the next row's slots"""
    import torch

    S = 2 * P + 3
    case, want, gate = C.reference("bhsd", 3, 128, 8, 2, dt, (S, 7, S))
    d = Dev(gpu, case)
    assert C.excess(_f64(d.run()), want, gate) <= 1.0
    plain = _bits(d.run())
    d.lens[0] = S + 1
    y = d.run()
    assert np.isnan(_f64(y)[0]).all() and np.array_equal(_bits(y)[1:], plain[1:])


@gpu_test
@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("kind", ["paged", "paged_single"])
def test_one_nan_in_an_attended_k_and_one_in_an_attended_v(gpu, kind, dt):
    """k: the outputs of the query heads of that kv head; v: that column of those heads; nothing else"""
    long_ = P if kind == "paged_single" else 2 * P + 3
    case, want, gate = C.reference(kind, 5, 64, 8, 2, dt, (0, 5, 40, long_, 3))
    d = Dev(gpu, case)
    plain = _bits(d.run()).reshape(5, 8, 64)
    last = long_ - 1  # the last key of the long row: its last partition
    d.k[int(case.table[3, last // 16]) * 16 + last % 16, 1, 5] = float("nan")
    d.v[int(case.table[4, 0]) * 16 + 1, 0, 9] = float("nan")
    y = d.run()
    got = _f64(y).reshape(5, 8, 64)
    assert np.isnan(got[3, 4:]).all() and np.isnan(got[4, :4, 9]).all()
    keep = np.ones((5, 8, 64), bool)
    keep[3, 4:] = False
    keep[4, :4, 9] = False
    assert np.array_equal(_bits(y).reshape(5, 8, 64)[keep], plain[keep])


# ---- 5. capture ----

@gpu_test
@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("kind,nodes", [("paged", 2), ("paged_single", 1)])
def test_a_captured_call_follows_lengths_updated_in_place(gpu, kind, nodes, dt):
    """two kernel nodes (partials, combine), one where the table fits one partition; between replays seq_lens advances in place
    across a partition boundary (P-1 -> P -> P+1; P-2 -> P-1 -> P on the one-partition path) and the new slots are filled"""
    import torch

    top = P + 1 if kind == "paged" else P
    full = C.build(kind, 3, 128, 8, 2, dt, 0, (top, 9, 40))
    d = Dev(gpu, copy.copy(full))
    slot = lambda b, p: int(full.table[b, p // 16]) * 16 + p % 16  # noqa: E731
    k_full, v_full = d.k.clone(), d.v.clone()
    for p in (top - 3, top - 2, top - 1):  # not there yet: poison, as every other unaddressed slot
        d.k[slot(0, p)] = float("nan")
        d.v[slot(0, p)] = float("nan")
    d.v[slot(1, 8)] = float("nan")
    d.lens.copy_(torch.tensor([top - 3, 8, 40], dtype=torch.int32))
    att = d.module()
    out = torch.empty((3, 8 * 128), dtype=full.dtype, device=gpu)
    run = lambda: att(d.q, d.k, d.v, d.table, d.lens, out=out)  # noqa: E731
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        run()
    assert _node_types(g) == [0] * nodes  # hipGraphNodeTypeKernel
    g.instantiate()
    for step in range(3):
        n0 = top - 2 + step
        d.k[slot(0, n0 - 1)] = k_full[slot(0, n0 - 1)]  # the new token's slot, as the front would fill it
        d.v[slot(0, n0 - 1)] = v_full[slot(0, n0 - 1)]
        if step == 1:
            d.v[slot(1, 8)] = v_full[slot(1, 8)]
        d.lens.copy_(torch.tensor([n0, 9 if step else 8, 40], dtype=torch.int32))  # in place: the graph holds the address
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        case = copy.copy(full)
        case.lens = np.array([n0, 9 if step else 8, 40])
        want, gate = C.reference_of(case)
        assert C.excess(_f64(out), want, gate) <= 1.0, step
        assert np.array_equal(_bits(out), _bits(d.run())), step  # ... and the eager call's bits


# ---- 6. end to end behind the attention front ----

@gpu_test
@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_three_decode_steps_behind_the_front(gpu, dt):
    """QuantQKVRopeFused(..., k_cache, v_cache, slots, return_kv=True) then DecodeAttention, three steps over a paged cache with
    blocks of 2 (the K = 1024 operands of tests/test_gpu_qkv_rope.py): the result against the oracle applied to the k / v rows the
    front RETURNED, and the cache holds exactly those rows"""
    import torch

    from squeezellm_amd import quant
    from tests import test_gpu_qkv_rope as TQ

    rows, (Nq, Nk, Nv, D) = 2, TQ.SHAPES["d64"]
    HQ, H, bs = Nq // D, Nk // D, 2
    dtype = C.DTYPES[dt]
    members = TQ._members(gpu, 4, "hybrid", "d64")
    front = TQ._module(members, D, "half", fused_members=True)
    att = quant.DecodeAttention(HQ, H, D, block_size=bs)
    cos, sin = TQ._tables(D)
    x0 = TQ._x(gpu, rows, str(dtype).split(".")[1])
    table = np.array([[5, 2], [0, 7]], dtype=np.int64)
    n_slots, ss, hs = 16, H * D, D
    extent = n_slots * ss
    # the oracle's view of these three steps: a case refilled from what the front returns
    host = types.SimpleNamespace(kind="e2e", dtype=dtype, B=rows, D=D, HQ=HQ, H=H, block_size=bs, table=table, n_slots=n_slots, slot_stride=ss,
                                 head_stride=hs, extent=extent, scale=float(D) ** -0.5, seed=[11, rows, D])
    host.k_buf, host.v_buf = (C._poisoned(2 * C.GUARD + extent, dtype, 0) for _ in range(2))
    k_buf, v_buf = host.k_buf.to(gpu), host.v_buf.to(gpu)
    k, v = C.cache_view(host, k_buf), C.cache_view(host, v_buf)
    t_table = torch.from_numpy(table).to(torch.int32).to(gpu)
    for step in range(3):
        pos = [step, step]
        slots = [int(table[b, p // bs]) * bs + p % bs for b, p in enumerate(pos)]
        tp, tc, ts = TQ._dev(gpu, pos, cos, sin)
        x = x0.roll(17 * step, dims=1)
        q, rk, rv = front(x, tp, tc, ts, k_cache=k, v_cache=v, slots=torch.tensor(slots, dtype=torch.int32, device=gpu), return_kv=True)
        lens = tp + 1
        y = att(q, k, v, t_table, lens)
        assert front.last_route == "qkv_rope" and att.last_route == "attn_decode"
        for b, s in enumerate(slots):  # the rows the front returned, where the oracle will look for them
            at = C.GUARD + s * ss
            host.k_buf[at:at + ss] = rk[b].cpu()
            host.v_buf[at:at + ss] = rv[b].cpu()
        assert torch.equal(k_buf.cpu().view(torch.int16), host.k_buf.view(torch.int16))  # the cache holds them, and nothing else
        assert torch.equal(v_buf.cpu().view(torch.int16), host.v_buf.view(torch.int16))
        host.q_buf, host.q_stride, host.lens = q.cpu(), HQ * D, np.array(pos) + 1
        want, gate = C.reference_of(host)
        worst = C.excess(_f64(y), want, gate)
        print(f"ATTN_GATE e2e step={step} {dt}: {worst:.3f}")
        assert np.isfinite(want).all() and worst <= 1.0, step


# ---- 7. the C ABI, directly ----

@gpu_test
@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("kind", ["padded", "bhsd", "paged_single"])
def test_c_abi_directly(gpu, kind, dt):
    """the descriptor filled in by hand, a workspace full of NaN patterns with a guard behind it, the LDS poisoned in front of the
    launch: the oracle's values, the module's bits, the guard intact"""
    import torch

    from squeezellm_amd import _lib, quant_cuda

    case, want, gate = C.reference(kind, 5, 128, 8, 2, dt)
    d = Dev(gpu, case)
    W = case.HQ * case.D
    out = torch.full((case.B, W + 4), 7.0, dtype=case.dtype, device=gpu)
    need = _lib.attn_decode_workspace_bytes(case.B, case.HQ, case.D, case.table.shape[1], case.block_size)
    assert need == case.B * case.HQ * ((case.table.shape[1] * case.block_size + P - 1) // P) * (case.D + 2) * 4
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=gpu)
    ws[need:] = 0xA5
    a = _lib.SqllmAttnDecode()
    a.q, a.out = d.q_buf.data_ptr(), out.data_ptr()
    a.k_cache, a.v_cache = d.k_buf.data_ptr() + 2 * C.GUARD, d.v_buf.data_ptr() + 2 * C.GUARD
    a.block_table, a.seq_lens = d.table.data_ptr(), d.lens.data_ptr()
    a.batch, a.n_q_heads, a.n_kv_heads, a.head_dim = case.B, case.HQ, case.H, case.D
    a.n_slots, a.block_size, a.max_blocks, a.table_stride = case.n_slots, case.block_size, case.table.shape[1], case.table.shape[1]
    a.slot_stride, a.head_stride, a.q_stride, a.out_stride = case.slot_stride, case.head_stride, case.q_stride, W + 4
    a.scale, a.workspace = case.scale, ws.data_ptr()
    stream = quant_cuda._raw_stream(gpu.index)
    _poison_lds()
    fn = getattr(_lib.load(), "sqllm_attn_decode_" + ("f16" if dt == "fp16" else "bf16"))
    assert fn(ctypes.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert C.excess(_f64(out[:, :W]), want, gate) <= 1.0
    assert bool((out[:, W:] == 7.0).all()) and bool((ws[need:] == 0xA5).all())
    assert np.array_equal(_bits(out[:, :W]), _bits(d.run()))


# ---- 8. the module's surface ----

@gpu_test
def test_module_surface(gpu):
    """int64 tables and lengths, leading dimensions, fp32 and an unserved head_dim on the fallback"""
    import torch

    from squeezellm_amd.quant import DecodeAttention

    case, want, gate = C.reference("paged", 3, 64, 8, 2, "fp16")
    d = Dev(gpu, case)
    att = d.module()
    y = _bits(d.run(att))
    assert np.array_equal(_bits(att(d.q, d.k, d.v, d.table.long(), d.lens.long())), y)
    y3 = att(d.q.contiguous().reshape(3, 1, -1), d.k, d.v, d.table, d.lens)
    assert y3.shape == (3, 1, 8 * 64) and np.array_equal(_bits(y3).reshape(3, -1), y)
    f32 = att(d.q.float(), d.k.float(), d.v.float(), d.table, d.lens)
    assert att.last_route == "fallback" and f32.dtype == torch.float32
    assert C.excess(_f64(f32.to(case.dtype)), want, gate) <= 1.0
    odd = DecodeAttention(16, 4, 32, block_size=16)  # head_dim 32: not served by the kernel
    yo = odd(d.q, d.k.reshape(-1, 4, 32)[: case.n_slots], d.v.reshape(-1, 4, 32)[: case.n_slots], d.table, torch.ones_like(d.lens))
    assert odd.last_route == "fallback" and yo.shape == (3, 512)
