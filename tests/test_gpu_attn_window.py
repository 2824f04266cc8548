"""The sliding-window decode attention on the GPU (sqllm_attn_decode_window_f16 / _bf16 / _fp8_f16 / _fp8_bf16 behind
quant.DecodeAttention(window=); include/sqllm_hip.h, sliding-window decode attention), against the fp64 oracle of
tests/attn_window_cases.py on that file's cases: the cases of tests/attn_decode_cases.py in which, additionally, every key behind
a row's window holds NaN patterns and every table entry of a block wholly behind it leads far outside the cache -- a kernel that
looks behind the window shows as a NaN row.  The byte caches are the same cases through tests/kv_fp8_cases.quantise.

The gate is attn_decode_cases', unchanged; tests/test_attn_window_cpu.py shows that three wrong windows fail it on these inputs.
The two identities of the contract -- a row inside the window, and a window that starts on a partition and block edge -- are
checked bit for bit against the entries without a window."""
import copy
import ctypes

import numpy as np
import pytest

from tests import attn_decode_cases as AC
from tests import attn_window_cases as WC
from tests import kv_fp8_cases as F
from tests import test_gpu_attn_decode as TG

gpu_test = pytest.mark.gpu
P = WC.P
INT32_MAX = WC.INT32_MAX
ALL_SHAPES = [(D, hq, hk) for D in (64, 128) for hq, hk in AC.HEADS]
TWO_SHAPES = [(128, 8, 2), (64, 6, 2)]
PARITY = ([("paged", L, W, *s, dt) for L, W in WC.PAIRS for s in ALL_SHAPES for dt in AC.DTYPES]
          + [(kind, L, W, *s, dt) for kind in ("padded", "bhsd") for L, W in WC.PAIRS for s in TWO_SHAPES for dt in AC.DTYPES]
          + [("paged_single", L, W, *s, dt) for L, W in WC.PAIRS if L <= P for s in TWO_SHAPES for dt in AC.DTYPES])
CACHES = ("16", "fp8")


class Dev:
    """a case's operands on the GPU, for either cache type: the guarded cache buffers and their views, q (strided), table and
    lengths as int32; `window`: the module's (the case's where it has one)"""

    def __init__(self, gpu, case, cache="16", poison=0):
        import torch

        from squeezellm_amd import quant

        self.case, self.fp8, self.gpu = case, cache == "fp8", gpu
        self.window = getattr(case, "window", None)
        if self.fp8:
            self.fc = F.quantise(case, poison=poison)
            self.k_buf, self.v_buf = self.fc.k_bytes.to(gpu), self.fc.v_bytes.to(gpu)
            self.scales = dict(k_scale=self.fc.k_scale, v_scale=self.fc.v_scale)
            typed = lambda t: t.view(torch.float8_e4m3fn)  # noqa: E731
        else:
            self.k_buf, self.v_buf = case.k_buf.to(gpu), case.v_buf.to(gpu)
            self.scales = {}
            typed = lambda t: t  # noqa: E731
        self.q_buf = case.q_buf.to(gpu)
        if case.kind == "bhsd":  # the library's own view of the static cache, and its own table
            S = case.block_size
            self.k, self.v = (quant.kv_cache_view(typed(t)[AC.GUARD:AC.GUARD + case.B * case.H * S * case.D].view(case.B, case.H, S, case.D), "bhsd")
                              for t in (self.k_buf, self.v_buf))
            self.table = quant.static_cache_blocks(case.B, case.H, gpu)
            assert self.k.shape[0] == case.n_slots and self.k.stride() == (case.slot_stride, case.head_stride, 1)
        else:
            self.k, self.v = (typed(t).as_strided((case.n_slots, case.H, case.D), (case.slot_stride, case.head_stride, 1), AC.GUARD)
                              for t in (self.k_buf, self.v_buf))
            self.table = torch.from_numpy(case.table).to(torch.int32).to(gpu)
        self.q = self.q_buf[:, :case.HQ * case.D]
        self.lens = torch.from_numpy(np.asarray(case.lens)).to(torch.int32).to(gpu)

    def module(self, window="case"):
        from squeezellm_amd.quant import DecodeAttention

        c = self.case
        return DecodeAttention(c.HQ, c.H, c.D, block_size=c.block_size, window=self.window if window == "case" else window)

    def run(self, att=None, rows=slice(None), out=None, table=None, lens=None):
        att = att or self.module()
        y = att(self.q[rows], self.k, self.v, self.table[rows] if table is None else table, self.lens[rows] if lens is None else lens,
                out=out, **self.scales)
        assert att.last_route == ("attn_decode" if att.window is None else "attn_window")
        return y

    def want(self):
        """(want, gate) of the case this Dev holds: over the dequantised bytes for a byte cache"""
        return WC.reference_w(self.fc.shadow if self.fp8 else self.case)


_bits, _f64 = TG._bits, TG._f64


def _want(case, fp8):
    """(want, gate) of a windowed case, over the dequantised bytes for a byte cache"""
    return WC.reference_w(F.quantise(case).shadow if fp8 else case)


def _check(d, att=None, what=""):
    import torch

    want, gate = d.want()
    att = att or d.module()
    y = d.run(att)
    torch.cuda.synchronize()
    assert y.dtype == d.case.dtype and y.shape == (d.case.B, d.case.HQ * d.case.D)
    worst = AC.excess(_f64(y), want, gate)
    print(f"ATTN_WINDOW_GATE {what} {'fp8' if d.fp8 else '16'}: {worst:.3f}")
    assert worst <= 1.0, (what, d.fp8, worst)
    return y


# ---- 1. parity ----

@gpu_test
@pytest.mark.parametrize("kind,L,W,D,hq,hk,dt", PARITY)
def test_parity_with_the_oracle(gpu, kind, L, W, D, hq, hk, dt):
    """both cache types; the first run, a run on poisoned workspaces and LDS, and a third run give the same bits"""
    case = WC.pair_case(kind, L, W, D, hq, hk, dt)
    for cache in CACHES:
        d = Dev(gpu, case, cache)
        att = d.module()
        y = _check(d, att, f"{kind} L={L} W={W} D={D} heads={hq}/{hk} {dt}")
        TG._poison_workspaces(att)
        TG._poison_lds()
        assert np.array_equal(_bits(d.run(att)), _bits(y))
        assert len(att.__dict__["_ws"]) >= 1 and np.array_equal(_bits(d.run(att)), _bits(y))


@gpu_test
@pytest.mark.parametrize("dt", list(AC.DTYPES))
@pytest.mark.parametrize("D,hq,hk", TWO_SHAPES)
@pytest.mark.parametrize("W", WC.LONG_WINDOWS)
@pytest.mark.parametrize("kind", ["paged", "padded"])
def test_parity_on_the_long_table(gpu, kind, W, D, hq, hk, dt):
    """18 partitions, 3 resp. 5 of them per row: every row its own first partition, a row shorter than the window, a +0 row"""
    from squeezellm_amd import _lib

    case = WC.long_case(kind, W, D, hq, hk, dt)
    mb, bs = case.table.shape[1], case.block_size
    assert WC.win_parts(mb, bs, W) == {P + 7: 3, 4 * P: 5}[W] and (mb * bs + P - 1) // P >= 18
    assert _lib.attn_window_workspace_bytes(case.B, hq, D, mb, bs, W) * ((mb * bs + P - 1) // P) == \
        _lib.attn_decode_workspace_bytes(case.B, hq, D, mb, bs) * WC.win_parts(mb, bs, W)
    for cache in CACHES:
        y = _check(Dev(gpu, case, cache), what=f"long {kind} W={W} D={D} heads={hq}/{hk} {dt}")
        got = _f64(y)
        assert (got[4] == 0).all() and not np.signbit(got[4]).any()


# ---- 2. the two identities ----

@gpu_test
@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("dt", list(AC.DTYPES))
@pytest.mark.parametrize("kind,D,hq,hk", [("paged", 128, 8, 2), ("padded", 64, 6, 2), ("bhsd", 64, 2, 2), ("paged_single", 128, 6, 2)])
def test_a_row_inside_the_window_holds_the_bits_of_the_entry_without_one(gpu, kind, D, hq, hk, dt, cache):
    case = AC.build(kind, 5, D, hq, hk, dt)  # (2, P-1, 1, 2P+3, P); one partition: (2, P-1, 1, P, 17) -- not poisoned behind any window
    d = Dev(gpu, case, cache)
    plain = _bits(d.run(d.module(None)))
    for W in (2 * P + 3, P + 1, INT32_MAX):
        y = _bits(d.run(d.module(W)))
        inside = np.asarray(case.lens) <= W
        assert inside.sum() >= 4 and np.array_equal(y[inside], plain[inside]), W
        assert inside.all() or not np.array_equal(y[~inside], plain[~inside])  # (the long row is another result: the window is on)


@gpu_test
@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("dt", list(AC.DTYPES))
@pytest.mark.parametrize("L,W", [(2 * P + 3, P + 3), (P + 77, 77)])
@pytest.mark.parametrize("D,hq,hk", TWO_SHAPES)
def test_a_window_on_a_partition_and_block_edge_is_the_shorter_row_over_the_advanced_table(gpu, D, hq, hk, L, W, dt, cache):
    case = WC.pair_case("paged", L, W, D, hq, hk, dt)
    lo = L - W
    assert lo % P == 0 and lo % case.block_size == 0
    d = Dev(gpu, case, cache)
    y = d.run(rows=slice(0, 1))
    table = d.table[0:1, lo // case.block_size:]  # the offset pointer, the same row stride
    assert table.data_ptr() == d.table.data_ptr() + 4 * (lo // case.block_size)
    shifted = d.run(d.module(None), rows=slice(0, 1), table=table, lens=d.lens[0:1] - lo)
    assert np.array_equal(_bits(y), _bits(shifted))
    assert np.array_equal(_bits(y), _bits(d.run())[0:1])


# ---- 3. isolation and writes ----

@gpu_test
@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("dt", list(AC.DTYPES))
@pytest.mark.parametrize("kind,D,hq,hk", [("paged", 128, 8, 2), ("padded", 64, 6, 2), ("bhsd", 128, 8, 2)])
def test_rows_alone_other_poison_a_second_run_and_a_guarded_out(gpu, kind, D, hq, hk, dt, cache):
    import torch

    W = P + 7
    case = WC.long_case(kind, W, D, hq, hk, dt) if kind != "bhsd" else WC.pair_case(kind, 2 * P + 3, P + 100, D, hq, hk, dt)
    d = Dev(gpu, case, cache)
    y = _bits(d.run())
    for b in range(case.B):  # a 1-row call: another batch size, the same row
        assert np.array_equal(_bits(d.run(rows=slice(b, b + 1))), y[b:b + 1]), b
    if kind == "bhsd":
        other = WC.pair_case(kind, 2 * P + 3, P + 100, D, hq, hk, dt, 1)
    else:
        other = WC.windowed(AC.build(kind, len(AC.LONG_LENS), D, hq, hk, dt, 1, AC.LONG_LENS, AC.LONG), W, 1)
    assert not torch.equal(other.k_buf.view(torch.int16), case.k_buf.view(torch.int16))
    assert np.array_equal(_bits(Dev(gpu, other, cache, poison=1).run()), y)
    # out: rows 11 elements wider than they need be, inside a guarded allocation with a per-element distinct pattern
    Wd, stride, guard = hq * D, hq * D + 11, 512
    total = guard + case.B * stride + guard
    pattern = (torch.arange(total, dtype=torch.int32) * 7 + 3).to(torch.int16).to(gpu)
    backing = pattern.clone().view(case.dtype)
    out = backing[guard:guard + case.B * stride].view(case.B, stride)[:, :Wd]
    before = [t.clone() for t in (d.k_buf, d.v_buf, d.q_buf, d.table, d.lens)]
    assert d.run(out=out) is out
    torch.cuda.synchronize()
    touched = torch.zeros(total, dtype=torch.bool, device=gpu)
    touched[guard:guard + case.B * stride].view(case.B, stride)[:, :Wd] = True
    assert torch.equal(backing.view(torch.int16)[~touched], pattern[~touched]) and np.array_equal(_bits(out), y)
    for t, b in zip((d.k_buf, d.v_buf, d.q_buf, d.table, d.lens), before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))


# ---- 4. the window's edges, bad entries and corner rows ----

@gpu_test
@pytest.mark.parametrize("dt", list(AC.DTYPES))
@pytest.mark.parametrize("kind", ["paged", "padded"])
def test_nan_at_the_first_attended_key_and_just_behind_the_window(gpu, kind, dt):
    """k at key lo: the outputs of the query heads of that kv head are NaN; k and v at key lo - 1: no bit changes"""
    L, W = 2 * P + 3, P + 100
    lo, bs = L - W, AC.build(kind, 2, 64, 8, 2, dt, 0, (L, WC.SECOND_ROW)).block_size
    case = AC.build(kind, 2, 64, 8, 2, dt, 0, (L, WC.SECOND_ROW))  # values behind the window, not poison: only the edge may show
    d = Dev(gpu, case)
    att = d.module(W)
    plain = _bits(d.run(att)).reshape(2, 8, 64)
    slot = lambda p: int(case.table[0, p // bs]) * bs + p % bs  # noqa: E731
    d.k[slot(lo - 1)] = float("nan")
    d.v[slot(lo - 1)] = float("nan")
    assert np.array_equal(_bits(d.run(att)).reshape(2, 8, 64), plain)
    d.k[slot(lo), 1, 5] = float("nan")
    y = d.run(att)
    got = _f64(y).reshape(2, 8, 64)
    assert np.isnan(got[0, 4:]).all()
    keep = np.ones((2, 8, 64), bool)
    keep[0, 4:] = False
    assert np.array_equal(_bits(y).reshape(2, 8, 64)[keep], plain[keep])


@gpu_test
@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("dt", list(AC.DTYPES))
@pytest.mark.parametrize("kind", ["paged", "padded", "paged_single"])
def test_bad_entries_zero_rows_and_rows_beyond_the_capacity(gpu, kind, dt, cache):
    """a USED table entry that leads outside the cache -> NaN, the neighbours untouched; an entry behind the window may hold
    anything; seq_lens <= 0 -> +0; a length beyond the capacity -> NaN.  Nothing out of range is read: the contract, not a
    provocation -- the kernel decides on the table's values before it touches the caches."""
    import torch

    long_ = P if kind == "paged_single" else 2 * P + 3
    W = 100
    lens = (0, 5, 40, long_, 3)
    base = WC.windowed(AC.build(kind, 5, 64, 8, 2, dt, 0, lens), W)
    d = Dev(gpu, base, cache)
    plain = _bits(_check(d, what=f"corners {kind} {dt}"))
    bs, cap = base.block_size, base.table.shape[1] * base.block_size
    used, behind = (long_ - 1) // bs, (long_ - W) // bs - 1  # the last attended block; the last block wholly behind the window
    for entry in (base.n_slots // bs, -1, INT32_MAX, -INT32_MAX - 1):
        d.table[3, behind] = entry
        assert np.array_equal(_bits(d.run()), plain), entry  # behind the window: anything
        d.table[3, used] = entry
        d.lens.copy_(torch.tensor([0, 5, cap + 1, long_, 3], dtype=torch.int32))
        y = d.run()
        got = _f64(y)
        assert (got[0] == 0).all() and not np.signbit(got[0]).any()
        assert np.isnan(got[2]).all() and np.isnan(got[3]).all()
        assert np.array_equal(_bits(y)[[1, 4]], plain[[1, 4]])
        d.table[3, used] = int(base.table[3, used])
        d.lens.copy_(torch.tensor(lens, dtype=torch.int32))
        assert np.array_equal(_bits(d.run()), plain)
    d.lens[2] = INT32_MAX
    assert np.isnan(_f64(d.run())[2]).all()
    d.lens[2] = -5
    got = _f64(d.run())
    assert (got[2] == 0).all() and not np.signbit(got[2]).any()


# ---- 5. capture ----

@gpu_test
@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("dt", list(AC.DTYPES))
@pytest.mark.parametrize("kind,nodes,top", [("paged", 2, P + 41), ("paged_single", 1, 102)])
def test_a_captured_call_follows_lengths_across_a_partition_edge(gpu, kind, nodes, top, dt, cache):
    """W = 40: between replays seq_lens advances in place so that lo goes 255 -> 256 -> 257 and the row's first partition changes
    (60 -> 61 -> 62 on the one-partition table); two kernel nodes, one where the table fits one partition"""
    import torch

    W = 40
    full = AC.build(kind, 3, 128, 8, 2, dt, 0, (top, 9, 45))
    d = Dev(gpu, full, cache)
    att = d.module(W)
    out = torch.empty((3, 8 * 128), dtype=full.dtype, device=gpu)
    d.lens.copy_(torch.tensor([top - 3, 8, 45], dtype=torch.int32))
    run = lambda: d.run(att, out=out)  # noqa: E731
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        run()
    assert TG._node_types(g) == [0] * nodes  # hipGraphNodeTypeKernel
    g.instantiate()
    for step in range(3):
        n0 = top - 2 + step
        d.lens.copy_(torch.tensor([n0, 9 if step else 8, 45], dtype=torch.int32))  # in place: the graph holds the address
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        case = copy.copy(full)
        case.lens = np.array([n0, 9 if step else 8, 45])
        want, gate = _want(WC.windowed(case, W), d.fp8)
        assert AC.excess(_f64(out), want, gate) <= 1.0, step
        assert np.array_equal(_bits(out), _bits(d.run(att))), step  # ... and the eager call's bits


@gpu_test
def test_the_module_without_a_window_is_unchanged(gpu):
    import torch

    case, want, gate = AC.reference("paged", 3, 64, 8, 2, "fp16")
    d = Dev(gpu, case)
    att = d.module(None)
    out = torch.empty((3, 8 * 64), dtype=case.dtype, device=gpu)
    d.run(att, out=out)
    torch.cuda.synchronize()
    assert att.last_route == "attn_decode" and AC.excess(_f64(out), want, gate) <= 1.0
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        d.run(att, out=out)
    assert TG._node_types(g) == [0, 0]
    assert np.array_equal(_bits(out), _bits(TG.Dev(gpu, case).run()))


# ---- 6. the rolling buffer ----

@gpu_test
@pytest.mark.parametrize("dt", list(AC.DTYPES))
def test_a_ring_of_four_blocks_serves_a_sequence_of_two_hundred_keys(gpu, dt):
    """quant.ring_block_table with W = 40 and blocks of 16: R = 4, 64 slots.  The sequence grows key by key, each written where the
    ring's table says (index_copy_, as a front would); at 12 lengths, the first overwrite and each wrap among them, the output
    equals bit for bit the windowed call over the linear table of a cache nothing was recycled in, and lies inside the gate"""
    import torch

    from squeezellm_amd import quant

    W, bs, n = 40, 16, 200
    lin = AC.build("paged", 1, 64, 8, 2, dt, 0, (n,))
    d = Dev(gpu, lin)
    att = d.module(W)
    ring_table = quant.ring_block_table(1, W, bs, n, gpu)
    R = 4
    assert ring_table.shape == (1, 13) and int(ring_table.max()) == R - 1
    ring_k, ring_v = (torch.full((R * bs, 2, 64), float("nan"), dtype=lin.dtype, device=gpu) for _ in range(2))
    lin_slot = torch.from_numpy(AC.key_slots(lin, 0, n)).to(gpu)
    ring_slot = (ring_table[0].long()[torch.arange(n, device=gpu) // bs] * bs + torch.arange(n, device=gpu) % bs)
    assert int(ring_slot[64]) == int(ring_slot[0]) == 0  # key 64 overwrites key 0
    checks = (1, 40, 41, 64, 65, 80, 105, 128, 129, 192, 193, 200)
    for L in range(1, n + 1):
        p = torch.tensor([L - 1], device=gpu)
        ring_k.index_copy_(0, ring_slot[p], d.k[lin_slot[p]])
        ring_v.index_copy_(0, ring_slot[p], d.v[lin_slot[p]])
        if L not in checks:
            continue
        lens = torch.tensor([L], dtype=torch.int32, device=gpu)
        y = att(d.q, ring_k, ring_v, ring_table, lens)
        assert att.last_route == "attn_window"
        assert np.array_equal(_bits(y), _bits(d.run(att, lens=lens))), L
        case = copy.copy(lin)
        case.lens = np.array([L])
        want, gate = WC.reference_w(WC.windowed(case, W))
        assert AC.excess(_f64(y), want, gate) <= 1.0, L


# ---- 7. several new tokens per sequence on a windowed module ----

@gpu_test
@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("dt", list(AC.DTYPES))
def test_q_len_on_a_windowed_module_is_the_expansion_on_the_window_kernels(gpu, dt, cache):
    import torch

    from squeezellm_amd import quant

    W = 50
    base = AC.build("paged", 2, 64, 8, 2, dt, 0, (300, 47))
    d = Dev(gpu, base, cache)
    att = d.module(W)
    q = torch.from_numpy(np.random.default_rng(3).standard_normal((6, 8 * 64))).to(base.dtype).to(gpu)
    q_lens = torch.tensor([3, 2], dtype=torch.int32, device=gpu)
    for route in ("auto", "kernel", "emulate"):  # ignored with a window
        att.append_route = route
        y = att(q, d.k, d.v, d.table, d.lens, q_len=3, q_lens=q_lens, **d.scales)
        assert att.last_route == "attn_window", route
        table, lens = quant.append_as_decode_rows(d.table, d.lens, 3, q_lens, 16)
        assert lens.tolist() == [298, 299, 300, 46, 47, 0]
        for r in range(6):  # the per-row windowed one-query calls
            one = att(q[r:r + 1], d.k, d.v, table[r:r + 1], lens[r:r + 1], **d.scales)
            assert np.array_equal(_bits(one), _bits(y[r:r + 1])), (route, r)
    rows = copy.copy(d.fc.shadow if d.fp8 else base)  # the oracle's view: six rows over the two sequences' tables, values behind the window
    rows.B, rows.table, rows.lens = 6, np.repeat(base.table, 3, axis=0), np.array([298, 299, 300, 46, 47, 0])
    rows.q_buf, rows.window, rows.base = q.cpu(), W, None
    want, gate = WC.reference_w(rows)
    assert AC.excess(_f64(y), want, gate) <= 1.0


# ---- 8. the C ABI, directly ----

@gpu_test
@pytest.mark.parametrize("cache", CACHES)
@pytest.mark.parametrize("dt", list(AC.DTYPES))
@pytest.mark.parametrize("kind,L,W", [("padded", 2 * P + 3, P + 100), ("bhsd", 300, 100), ("paged_single", 200, 50), ("paged", 2 * P + 3, 1)])
def test_c_abi_directly(gpu, kind, L, W, dt, cache):
    """the descriptor filled in by hand, a workspace of the new size function full of NaN patterns with a guard behind it, the LDS
    poisoned in front of the launch: the oracle's values, the module's bits, the guard intact"""
    import torch

    from squeezellm_amd import _lib, quant_cuda

    case = WC.pair_case(kind, L, W, 128, 8, 2, dt)
    d = Dev(gpu, case, cache)
    want, gate = d.want()
    Wd, mb = case.HQ * case.D, case.table.shape[1]
    out = torch.full((case.B, Wd + 4), 7.0, dtype=case.dtype, device=gpu)
    need = _lib.attn_window_workspace_bytes(case.B, case.HQ, case.D, mb, case.block_size, W)
    assert need == case.B * case.HQ * WC.win_parts(mb, case.block_size, W) * (case.D + 2) * 4
    assert need <= _lib.attn_decode_workspace_bytes(case.B, case.HQ, case.D, mb, case.block_size)
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=gpu)
    ws[need:] = 0xA5
    a = _lib.SqllmAttnDecodeFp8() if d.fp8 else _lib.SqllmAttnDecode()
    elem = 1 if d.fp8 else 2
    a.q, a.out = d.q_buf.data_ptr(), out.data_ptr()
    a.k_cache, a.v_cache = d.k_buf.data_ptr() + elem * AC.GUARD, d.v_buf.data_ptr() + elem * AC.GUARD
    a.block_table, a.seq_lens = d.table.data_ptr(), d.lens.data_ptr()
    a.batch, a.n_q_heads, a.n_kv_heads, a.head_dim = case.B, case.HQ, case.H, case.D
    a.n_slots, a.block_size, a.max_blocks, a.table_stride = case.n_slots, case.block_size, mb, mb
    a.slot_stride, a.head_stride, a.q_stride, a.out_stride = case.slot_stride, case.head_stride, case.q_stride, Wd + 4
    a.scale, a.workspace = case.scale, ws.data_ptr()
    if d.fp8:
        a.k_scale, a.v_scale = d.fc.k_scale, d.fc.v_scale
    stream = quant_cuda._raw_stream(gpu.index)
    TG._poison_lds()
    fn = getattr(_lib.load(), "sqllm_attn_decode_window_" + ("fp8_" if d.fp8 else "") + ("f16" if dt == "fp16" else "bf16"))
    assert fn(ctypes.byref(a), W, stream) == 0
    torch.cuda.synchronize()
    assert AC.excess(_f64(out[:, :Wd]), want, gate) <= 1.0
    assert bool((out[:, Wd:] == 7.0).all()) and bool((ws[need:] == 0xA5).all())
    assert np.array_equal(_bits(out[:, :Wd]), _bits(d.run()))
    assert fn(ctypes.byref(a), 0, stream) == -2  # SQLLM_E_SHAPE, before the device is touched
