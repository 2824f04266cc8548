"""The fp8 KV cache on the GPU (include/sqllm_hip.h, sqllm_kv_cache_fp8 / sqllm_attn_decode_fp8): the attention front writing
e4m3fn bytes (sqllm_qkv_rope_cache_fp8_* / sqllm_qkv_rope_norm_cache_fp8_* behind quant.QuantQKVRopeFused's k_scale / v_scale) and
the decode attention reading them (sqllm_attn_decode_fp8_* behind quant.DecodeAttention's).

The writer.  Operands, shapes, geometries and slots are those of tests/test_gpu_qkv_cache.py (K = 1024; the rotation's two
layouts, 3 and 4 bits, batch tiles 1 / 2 / 4 / 8, fp16 and bf16, with and without the norm, the three cache geometries), by import.
The fp64 sums and `tol32`, the tolerance tests/test_gpu_qkv_rope.py gives the fp32 value BEFORE its rounding (_rotated / _plain
with "float32"), bound every live byte: in the sign-magnitude order of the encoding it lies between enc((exact - tol32) * inv)
and enc((exact + tol32) * inv) inclusive -- bit-exactness where the two coincide, either neighbour where they differ, no
element left out.  With return_kv=True every byte is also inside the encodings of the rounding interval of the 16-bit element
the call returned.  One geometry per configuration runs with a scale small enough that elements saturate at +-448 and one with
a scale large enough that elements land in e4m3's subnormals, each asserted on the reference side first.

The reader.  The cases of tests/kv_fp8_cases.py (tests/attn_decode_cases.py's, quantised; every unaddressed byte 0x7f or 0xff),
the oracle and the gate of tests/attn_decode_cases.py over the dequantised bytes: excess <= 1.  tests/test_kv_fp8_cpu.py shows
that seven wrong oracles fail that gate at every shape used here."""
import copy
import ctypes
import types

import numpy as np
import pytest

from tests import attn_decode_cases as AC
from tests import kv_fp8_cases as F
from tests import test_gpu_qkv_cache as TK
from tests import test_gpu_qkv_rope as TQ
from tests.test_gpu_attn_decode import _bits, _f64, _node_types, _poison_lds, _poison_workspaces
from tests.test_gpu_qkv_rope import K, N_POS

gpu_test = pytest.mark.gpu
P = AC.P
PARITY = [(kind, rows, D, hq, hk, dt) for kind in AC.GEOMETRIES + ("paged_single",) for rows in (1, 3, 5) for D in (64, 128)
          for hq, hk in AC.HEADS for dt in AC.DTYPES]
FIVE = [(kind, 5, D, hq, hk, dt) for kind in AC.GEOMETRIES + ("paged_single",) for D, hq, hk in ((128, 8, 2), (64, 6, 2)) for dt in AC.DTYPES]


# =============================================================================================================== the writer

class ByteCache:
    """TK.Cache's geometry and slots over uint8 allocations whose every byte is one of the two NaN bytes"""

    def __init__(self, gpu, geom, rows, N, D):
        import torch

        from squeezellm_amd import quant

        g = TK.Cache(gpu, geom, rows, N, D, "float16")
        self.g, self.H, self.D, self.rows, self.n_slots, self.ss, self.hs, self.off = g, g.H, D, rows, g.n_slots, g.ss, g.hs, g.off
        self.slots, self.t_slots = g.slots, g.t_slots
        total = g.backing[0].numel()
        i = torch.arange(total)
        self.pattern = [torch.where((i * m) % 3 == 0, 0xFF, 0x7F).to(torch.uint8) for m in (1, 2)]
        self.backing = [p.clone().to(gpu) for p in self.pattern]
        self.views = []
        for b in self.backing:
            f8 = b.view(torch.float8_e4m3fn)
            if geom == "bhsd":
                v = quant.kv_cache_view(f8[TK.GUARD:total - TK.GUARD].view(rows, g.H, TK.S, D), "bhsd")
            else:
                v = f8.as_strided((g.n_slots, g.H, D), (g.ss, g.hs, 1), g.off)
            assert tuple(v.shape) == (g.n_slots, g.H, D) and v.stride() == (g.ss, g.hs, 1) and v.storage_offset() == g.off
            self.views.append(v)

    def reset(self):
        for b, p in zip(self.backing, self.pattern):
            b.copy_(p)

    def got(self, which):
        return self.backing[which].cpu().numpy()

    def split(self, which, slots=None):
        """(bytes of the live rows [live, N], which rows are live, whether everything else still holds its pattern)"""
        at, live = self.g.index(slots)
        got = self.got(which)
        rest = np.ones(got.size, bool)
        rest[at.reshape(-1)] = False
        return got[at], live, bool((got[rest] == self.pattern[which].numpy()[rest]).all())


def _enc(x64, scale, outward):
    """bytes of fp64 values by the contract's formula, the fp32 operand rounded AWAY from the interval's inside (`outward` -1: down,
    +1: up), so that the bound holds for every fp32 value inside the fp64 interval"""
    import torch

    x32 = x64.astype(np.float32)
    wrong = (x32.astype(np.float64) > x64) if outward < 0 else (x32.astype(np.float64) < x64)
    x32 = np.where(wrong, np.nextafter(x32, np.float32(outward) * np.float32(np.inf)), x32)
    return F.encode(torch.from_numpy(x32), scale).numpy()


def _between(got, lo64, hi64, scale, what):
    """every byte of `got` lies, in the encoding's order, between enc(lo) and enc(hi) inclusive; returns how many had no choice"""
    lo, hi = F.byte_order(_enc(lo64, scale, -1)), F.byte_order(_enc(hi64, scale, +1))
    assert ((got & 0x7F) != 0x7F).all(), f"{what}: NaN bytes among finite values"
    o = F.byte_order(got)
    bad = (o < lo) | (o > hi)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} bytes outside their bounds, first at {np.argwhere(bad)[0]}: " \
                          f"got {got[bad][0]:#x}, bounds {lo[bad][0]}..{hi[bad][0]} (ordered)"
    return int((lo == hi).sum())


def _interval16(t16):
    """(lo, hi) fp64: the reals that round to each 16-bit element (to its neighbours' midpoints, inclusive)"""
    import torch

    bits = t16.contiguous().view(torch.int16).cpu().numpy().astype(np.int64) & 0xFFFF
    o = np.where(bits >= 0x8000, -(bits & 0x7FFF), bits)

    def val(o):
        b = np.where(o < 0, 0x8000 | -o, o).astype(np.uint16).astype(np.int16)
        return torch.from_numpy(b).view(t16.dtype).double().numpy()

    v = val(o)
    with np.errstate(invalid="ignore", over="ignore"):
        return (v + val(o - 1)) / 2, (v + val(o + 1)) / 2


def _scales(exact, mode):
    """a scale for values `exact`: "fit" -- the largest magnitude lands at 448 x 0.83 (no power of two); "saturate" -- an eighth of
    that: the upper three binades of the values clamp; "subnormal" -- the largest magnitude lands at 2^-4, a good part of the rest
    below 2^-6, the smallest normal"""
    import torch

    top = float(np.abs(exact).max())
    s = {"fit": top / (448.0 * 0.83), "saturate": top / (448.0 * 0.83) / 8.0, "subnormal": top * 16.0}[mode]
    s = float(torch.tensor(s, dtype=torch.float32))
    y = np.abs(exact) * float(1.0 / torch.tensor(s, dtype=torch.float32))
    if mode == "saturate":
        assert (y > 480.0).sum() >= 2, "the reference side: no element saturates"
    elif mode == "subnormal":
        assert ((y > 2.0 ** -10) & (y < 2.0 ** -6)).sum() >= exact.size // 8, "the reference side: too few subnormals"
    else:
        assert y.max() < 448.0
    return s


MODES = ("fit", "saturate", "subnormal")


@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 2, 4, 5])
@pytest.mark.parametrize("kind", ["dense", "hybrid"])
@pytest.mark.parametrize("bits", [3, 4])
def test_writer_bytes_against_the_oracle_and_against_its_own_outputs(gpu, bits, kind, rows, dtype):
    """every configuration (shape class x layout) x every geometry, each geometry with another scale mode (in turn); the norm
    entry on one geometry per configuration, its bytes against its own returned outputs.  Checked per call: the bounds from
    the fp64 oracle (plain entry), the bounds from the returned 16-bit elements (both entries), out_q / out_k / out_v equal to the
    16-bit cache-less parent's, everything outside the addressed bytes untouched (rows with out-of-range slots wrote nothing), a
    call with NULL out_k / out_v and a second run leaving identical bytes."""
    import torch

    x = TQ._x(gpu, rows, dtype)
    pos = TQ._positions(rows)
    g = TK._norm_weight(gpu, dtype)
    exact_count = 0
    for ci, (shape, layout) in enumerate(TK.CONFIGS):
        Nq, Nk, Nv, D = TK.SHAPES[shape]
        members = TK._members(gpu, bits, kind, shape)
        TQ._in_range(members, x)
        sums = TQ._sums(members, x, rows, dtype)
        cos, sin = TQ._tables(D)
        bounds = (TQ._rotated(sums[1], pos, cos, sin, D, layout, "float32"), TQ._plain(sums[2], "float32"))
        mod = TQ._module(members, D, layout)
        tp, tc, ts = TQ._dev(gpu, pos, cos, sin)
        xin = x if rows > 1 else x.reshape(1, 1, K)
        parent = mod(xin, tp, tc, ts)
        for gi, geom in enumerate(TK.GEOMS):
            mode = MODES[(gi + ci) % 3]
            ks, vs = _scales(bounds[0][0], mode), _scales(bounds[1][0], MODES[(gi + ci + 1) % 3])
            c = ByteCache(gpu, geom, rows, Nk, D)
            for norm in ((False, True) if gi == ci % 3 else (False,)):
                kw = dict(norm_weight=g, norm_eps=1e-5) if norm else {}
                what = f"{shape} {layout} {geom} {mode} norm={norm}"
                c.reset()
                outs = mod(xin, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=c.t_slots, k_scale=ks, v_scale=vs, **kw)
                assert mod.last_route == ("qkv_rope_norm" if norm else "qkv_rope")
                if norm:  # (the 16-bit outputs are the cache-less norm entry's, bit for bit)
                    assert all(TK._eq16(o, p) for o, p in zip(outs, mod(xin, tp, tc, ts, **kw)))
                first = []
                for which, scale in ((0, ks), (1, vs)):
                    got, live, untouched = c.split(which)
                    assert untouched, f"{what}: bytes outside the addressed ones were written ({'kv'[which]})"
                    assert live.sum() == (rows - 2 if rows >= 3 else rows)
                    if not norm:  # (the norm entry's sums are other sums: its own outputs bound it below)
                        exact, tol = bounds[which]
                        exact_count += _between(got, (exact - tol)[live], (exact + tol)[live], scale, what + " oracle " + "kv"[which])
                        assert TK._eq16(outs[1 + which], parent[1 + which]) and TK._eq16(outs[0], parent[0])
                    lo, hi = _interval16(outs[1 + which].reshape(rows, -1))
                    _between(got, lo[live], hi[live], scale, what + " own output " + "kv"[which])
                    first.append(c.got(which))
                for return_kv in (False, True):  # NULL outputs, and a second run with them: identical bytes
                    c.reset()
                    again = mod(xin, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=c.t_slots, k_scale=ks, v_scale=vs, return_kv=return_kv, **kw)
                    torch.cuda.synchronize()
                    assert TK._eq16(again[0], outs[0]) and (return_kv or (again[1] is None and again[2] is None))
                    assert np.array_equal(c.got(0), first[0]) and np.array_equal(c.got(1), first[1]), what
        TQ._clean(mod)
    assert exact_count > 0  # (where the two ends coincide the test is bit-exact: that happens)


@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("layout", ["half", "interleaved"])
def test_a_position_outside_the_tables_puts_nan_bytes_into_k_cache_only(gpu, layout, dtype):
    """positions -1 and n_pos with VALID slots: k_cache receives NaN bytes where the output receives its NaN rows, v_cache's bytes
    are finite; a valid position with an out-of-range slot writes nothing"""
    import torch

    rows, shape = 5, "d8"
    Nq, Nk, Nv, D = TK.SHAPES[shape]
    members = TK._members(gpu, 4, "mixed", shape)
    x = TQ._x(gpu, rows, dtype)
    mod = TQ._module(members, D, layout)
    tp, tc, ts = TQ._dev(gpu, [3, -1, 0, N_POS, N_POS - 1], *TQ._tables(D))
    c = ByteCache(gpu, "nhd", rows, Nk, D)
    slots = [TK.N_SLOTS - 1, 4, -1, 0, 9]
    t_slots = torch.tensor(slots, dtype=torch.int32, device=gpu)
    outs = mod(x, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=t_slots, k_scale=0.05, v_scale=0.03)
    assert torch.isnan(outs[1][1].float()).all() and torch.isnan(outs[1][3].float()).all() and torch.isfinite(outs[1][[0, 2, 4]].float()).all()
    kb, live, untouched_k = c.split(0, slots)
    vb, _, untouched_v = c.split(1, slots)
    assert untouched_k and untouched_v and list(live) == [True, True, False, True, True]
    nan = (kb & 0x7F) == 0x7F  # rows of the live slots, in the order of the rows: 0, 1, 3, 4
    assert nan[1].all() and nan[2].all() and not nan[0].any() and not nan[3].any()
    assert not ((vb & 0x7F) == 0x7F).any()
    TQ._clean(mod)


@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_a_captured_writer_call_is_one_kernel_node_and_follows_slots_and_positions(gpu, dtype):
    import torch

    rows, shape, layout = 2, "d64", "half"
    Nq, Nk, Nv, D = TK.SHAPES[shape]
    members = TK._members(gpu, 4, "hybrid", shape)
    mod = TQ._module(members, D, layout, fused_members=True)
    x = TQ._x(gpu, rows, dtype)
    cos, sin = TQ._tables(D)
    pos, slots = [4, 9], [6, 17]
    tp, tc, ts = TQ._dev(gpu, pos, cos, sin)
    c = ByteCache(gpu, "nhd", rows, Nk, D)
    t_slots = torch.tensor(slots, dtype=torch.int32, device=gpu)
    ks, vs = 0.031, 0.017
    eager = []
    for step in range(3):  # what eager calls leave at the three steps
        c.reset()
        mod(x, torch.tensor([p + step for p in pos], dtype=torch.int32, device=gpu), tc, ts, k_cache=c.views[0], v_cache=c.views[1],
            slots=torch.tensor([s + step for s in slots], dtype=torch.int32, device=gpu), k_scale=ks, v_scale=vs, return_kv=False)
        eager.append([c.split(w, [s + step for s in slots])[0] for w in (0, 1)])
    assert not np.array_equal(eager[0][0], eager[1][0])
    run = lambda: mod(x, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=t_slots, k_scale=ks, v_scale=vs, return_kv=False)  # noqa: E731
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side), torch.no_grad():
        run()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g), torch.no_grad():
        run()
    assert _node_types(g) == [0]  # hipGraphNodeTypeKernel: the q/k/v kernel and nothing else
    g.instantiate()
    c.reset()
    for step in range(3):
        if step:
            t_slots.add_(1)  # in place: the graph holds the tensors' addresses
            tp.add_(1)
        g.replay()
        torch.cuda.synchronize()
        for w in (0, 1):
            for earlier in range(step + 1):  # (the earlier steps' slots keep their bytes)
                assert np.array_equal(c.split(w, [s + earlier for s in slots])[0], eager[earlier][w]), (step, earlier, w)
    TQ._clean(mod)


@gpu_test
@pytest.mark.parametrize("route", ["fallback", "dense"])
def test_the_torch_routes_make_the_same_writes_by_the_same_formula(gpu, route):
    """fp32 activations (fallback) and dense_min_rows (dense): bytes inside the oracle's bounds widened by that route's own
    tolerance (tests/test_gpu_qkv_cache.py), inside the rounding interval of what the call returns, nothing else written"""
    import torch

    shape, layout, rows, dtype = "d24", "half", 5, "float16"
    Nq, Nk, Nv, D = TK.SHAPES[shape]
    members = TK._members(gpu, 4, "mixed", shape)
    mod = TQ._module(members, D, layout, fused_members=route == "dense")
    x = TQ._x(gpu, rows, dtype)
    if route == "dense":
        mod.q.dense_min_rows = 4
        sums = TQ._sums(members, x, rows, dtype)
    else:
        x = x.float()
        sums = [TQ.BF._exact(npl, x, k) for _, npl, _, k in members]
    cos, sin = TQ._tables(D)
    pos = TQ._positions(rows)
    tp, tc, ts = TQ._dev(gpu, pos, cos, sin)
    for geom in TK.GEOMS:
        c = ByteCache(gpu, geom, rows, Nk, D)
        bounds = []
        for i in (1, 2):
            exact, tol = TQ._rotated(sums[i], pos, cos, sin, D, layout, "float32") if i == 1 else TQ._plain(sums[i], "float32")
            if route == "dense":  # the parent route's tolerance (tests/test_gpu_qkv_rope.py: test_dense_route_from_dense_min_rows)
                _, npl, mag, _ = members[i]
                gemm = K * 2.0 ** -24 * TQ.BF._abs_sum(npl, mag, x)
                if i == 1:
                    lo, hi = TQ._split(gemm, D, layout)
                    cc, sn = np.abs(TQ._at(cos, pos)).astype(np.float64), np.abs(TQ._at(sin, pos)).astype(np.float64)
                    gemm = TQ._merge(lo * cc + hi * sn, hi * cc + lo * sn, layout)
                tol = tol + gemm
            bounds.append((exact, tol))
        ks, vs = _scales(bounds[0][0], "fit"), _scales(bounds[1][0], "subnormal")
        outs = mod(x, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=c.t_slots, k_scale=ks, v_scale=vs)
        assert mod.last_route == route
        for which, scale in ((0, ks), (1, vs)):
            got, live, untouched = c.split(which)
            assert untouched and live.sum() == rows - 2
            exact, tol = bounds[which]
            _between(got, (exact - tol)[live], (exact + tol)[live], scale, f"{route} {geom} " + "kv"[which])
            if route == "dense":
                lo, hi = _interval16(outs[1 + which])
                _between(got, lo[live], hi[live], scale, f"{route} {geom} own output " + "kv"[which])


# =============================================================================================================== the reader

class Dev:
    """an fp8 case's operands on the GPU: the guarded byte buffers and their float8 views, q (strided), table and lengths"""

    def __init__(self, gpu, fc):
        import torch

        from squeezellm_amd import quant

        case = fc.case
        self.fc, self.case = fc, case
        self.k_buf, self.v_buf, self.q_buf = fc.k_bytes.to(gpu), fc.v_bytes.to(gpu), case.q_buf.to(gpu)
        if case.kind == "bhsd":  # the library's own view of the static cache, and its own table
            S = case.block_size
            self.k, self.v = (quant.kv_cache_view(t.view(torch.float8_e4m3fn)[AC.GUARD:AC.GUARD + case.B * case.H * S * case.D]
                                                  .view(case.B, case.H, S, case.D), "bhsd") for t in (self.k_buf, self.v_buf))
            self.table = quant.static_cache_blocks(case.B, case.H, gpu)
            assert self.k.shape[0] == case.n_slots and self.k.stride() == (case.slot_stride, case.head_stride, 1)
        else:
            self.k, self.v = (F.cache_view(fc, t) for t in (self.k_buf, self.v_buf))
            self.table = torch.from_numpy(case.table).to(torch.int32).to(gpu)
        self.q = self.q_buf[:, :case.HQ * case.D]
        self.lens = torch.from_numpy(case.lens).to(torch.int32).to(gpu)

    def module(self):
        from squeezellm_amd.quant import DecodeAttention

        c = self.case
        return DecodeAttention(c.HQ, c.H, c.D, block_size=c.block_size)

    def run(self, att=None, rows=slice(None), out=None):
        att = att or self.module()
        y = att(self.q[rows], self.k, self.v, self.table[rows], self.lens[rows], out=out, k_scale=self.fc.k_scale, v_scale=self.fc.v_scale)
        assert att.last_route == "attn_decode"
        return y


@gpu_test
@pytest.mark.parametrize("kind,rows,D,hq,hk,dt", PARITY)
def test_reader_parity_with_the_oracle_over_the_dequantised_bytes(gpu, kind, rows, D, hq, hk, dt):
    """excess <= 1 in units of tests/attn_decode_cases.py's gate; the first run, a run on poisoned workspaces and LDS, and a third
    run give the same bits.  Observed maximum on an MI355X: DESIGN.md 4.4."""
    import torch

    fc, want, gate = F.reference(kind, rows, D, hq, hk, dt)
    d = Dev(gpu, fc)
    att = d.module()
    y = d.run(att)
    torch.cuda.synchronize()
    assert y.dtype == fc.case.dtype and y.shape == (fc.case.B, hq * D)
    worst = AC.excess(_f64(y), want, gate)
    print(f"FP8_GATE {kind} rows={rows} D={D} heads={hq}/{hk} {dt}: {worst:.3f}")
    assert worst <= 1.0, worst
    _poison_workspaces(att)
    _poison_lds()
    assert np.array_equal(_bits(d.run(att)), _bits(y)) and np.array_equal(_bits(d.run(att)), _bits(y))


@gpu_test
@pytest.mark.parametrize("dt", list(AC.DTYPES))
@pytest.mark.parametrize("kind,D,hq,hk", [("padded", 128, 6, 2), ("paged", 64, 8, 2), ("paged_single", 128, 2, 2)])
def test_reader_parity_with_scales_that_are_no_powers_of_two(gpu, kind, D, hq, hk, dt):
    fc, want, gate = F.reference(kind, 3, D, hq, hk, dt, F.ODD_SCALES)
    worst = AC.excess(_f64(Dev(gpu, fc).run()), want, gate)
    print(f"FP8_GATE odd scales {kind} D={D} heads={hq}/{hk} {dt}: {worst:.3f}")
    assert worst <= 1.0, worst


@gpu_test
@pytest.mark.parametrize("kind,rows,D,hq,hk,dt", FIVE)
def test_reader_rows_alone_the_other_poison_and_a_second_run_give_the_same_bits(gpu, kind, rows, D, hq, hk, dt):
    import torch

    fc = F.fp8_case(kind, rows, D, hq, hk, dt)
    d = Dev(gpu, fc)
    y = _bits(d.run())
    for b in range(fc.case.B):  # a 1-row call: another batch size and another row index, the same row
        assert np.array_equal(_bits(d.run(rows=slice(b, b + 1))), y[b:b + 1]), b
    other = F.fp8_case(kind, rows, D, hq, hk, dt, poison=1)
    assert not torch.equal(other.k_bytes, fc.k_bytes) and not torch.equal(other.v_bytes, fc.v_bytes)
    assert np.array_equal(_bits(Dev(gpu, other).run()), y)
    assert np.array_equal(_bits(d.run()), y)


@gpu_test
@pytest.mark.parametrize("dt", list(AC.DTYPES))
@pytest.mark.parametrize("kind", ["paged", "padded", "paged_single"])
def test_reader_zero_rows_nan_rows_and_nan_bytes(gpu, kind, dt):
    """seq_lens of 0 -> +0; a length beyond the table's capacity -> NaN; a table entry that leads outside the cache -> NaN (the
    kernel decides on the table's values before it touches the caches: nothing out of range is read); the neighbours keep their
    bits.  Then one NaN byte in an attended k (the outputs of that kv head's query heads) and one in an attended v (that column)."""
    import torch

    long_ = P if kind == "paged_single" else 2 * P + 3
    fc, want0, gate0 = F.reference(kind, 5, 64, 8, 2, dt, F.SCALES, (0, 5, 40, long_, 3))
    base = fc.case
    d = Dev(gpu, fc)
    y0 = d.run()
    plain = _bits(y0)
    got0 = _f64(y0)
    assert AC.excess(got0, want0, gate0) <= 1.0 and (got0[0] == 0).all() and not np.signbit(got0[0]).any()
    bs, cap = base.block_size, base.table.shape[1] * base.block_size
    for entry in (base.n_slots // bs, -1, (1 << 31) - 1, -(1 << 31)):
        d.lens.copy_(torch.tensor([0, 5, cap + 1, long_, 3], dtype=torch.int32))
        d.table[3, 7 if long_ > 7 * bs else 0] = entry
        y = d.run()
        got = _f64(y)
        assert (got[0] == 0).all() and not np.signbit(got[0]).any()
        assert np.isnan(got[2]).all() and np.isnan(got[3]).all()
        assert np.array_equal(_bits(y)[[1, 4]], plain[[1, 4]])
    d.table.copy_(torch.from_numpy(base.table).to(torch.int32))
    d.lens.copy_(torch.from_numpy(base.lens).to(torch.int32))
    assert np.array_equal(_bits(d.run()), plain)
    last = long_ - 1  # the last key of the long row: its last partition
    slot = lambda b, p: int(base.table[b, p // bs]) * bs + p % bs  # noqa: E731
    d.k.view(torch.uint8)[slot(3, last), 1, 5] = 0xFF
    d.v.view(torch.uint8)[slot(4, 1), 0, 9] = 0x7F
    y = d.run()
    got = _f64(y).reshape(5, 8, 64)
    assert np.isnan(got[3, 4:]).all() and np.isnan(got[4, :4, 9]).all()
    keep = np.ones((5, 8, 64), bool)
    keep[3, 4:] = False
    keep[4, :4, 9] = False
    assert np.array_equal(_bits(y).reshape(5, 8, 64)[keep], plain.reshape(5, 8, 64)[keep])


@gpu_test
@pytest.mark.parametrize("dt", list(AC.DTYPES))
@pytest.mark.parametrize("kind,nodes", [("paged", 2), ("paged_single", 1)])
def test_a_captured_reader_call_follows_lengths_and_tables_updated_in_place(gpu, kind, nodes, dt):
    """two kernel nodes (partials, the 16-bit kernel's combine), one where the table fits one partition; between replays seq_lens
    advances in place across a partition boundary and two rows' table rows are swapped in place"""
    import torch

    top = P + 1 if kind == "paged" else P
    fc = F.fp8_case(kind, 3, 128, 8, 2, dt, F.SCALES, 0, (top, 9, 40))
    d = Dev(gpu, fc)
    att = d.module()
    out = torch.empty((3, 8 * 128), dtype=fc.case.dtype, device=gpu)
    d.lens.copy_(torch.tensor([top - 2, 9, 40], dtype=torch.int32))
    run = lambda: att(d.q, d.k, d.v, d.table, d.lens, out=out, k_scale=fc.k_scale, v_scale=fc.v_scale)  # noqa: E731
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
    for step, (lens, swap) in enumerate((((top - 2, 9, 40), False), ((top - 1, 9, 40), False), ((top, 9, 40), False), ((9, top, 40), True))):
        table = fc.case.table.copy()
        if swap:  # rows 0 and 1 trade their blocks (and their lengths): q stays, so the outputs are new ones
            table[[0, 1]] = table[[1, 0]]
        d.table.copy_(torch.from_numpy(table).to(torch.int32))  # in place: the graph holds the addresses
        d.lens.copy_(torch.tensor(lens, dtype=torch.int32))
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        shadow = copy.copy(fc.shadow)
        shadow.lens, shadow.table = np.array(lens), table
        want, gate = AC.reference_of(shadow)
        assert AC.excess(_f64(out), want, gate) <= 1.0, step
        assert np.array_equal(_bits(out), _bits(d.run())), step  # ... and the eager call's bits


# ============================================================================================================ the round trip

@gpu_test
@pytest.mark.parametrize("dt", list(AC.DTYPES))
def test_three_decode_steps_the_front_writes_the_attention_reads(gpu, dt):
    """QuantQKVRopeFused with an fp8 cache, then DecodeAttention over it, three steps over a paged cache with blocks of 2: the
    oracle is formed from the BYTES READ BACK from the cache (dequantised in fp64), every other byte keeps its poison, and the
    C ABI called directly gives the module's bits"""
    import torch

    from squeezellm_amd import _lib, quant, quant_cuda

    rows, (Nq, Nk, Nv, D) = 2, TQ.SHAPES["d64"]
    HQ, H, bs = Nq // D, Nk // D, 2
    dtype = AC.DTYPES[dt]
    members = TQ._members(gpu, 4, "hybrid", "d64")
    front = TQ._module(members, D, "half", fused_members=True)
    att = quant.DecodeAttention(HQ, H, D, block_size=bs)
    cos, sin = TQ._tables(D)
    x0 = TQ._x(gpu, rows, str(dtype).split(".")[1])
    table = np.array([[5, 2], [0, 7]], dtype=np.int64)
    n_slots, ss, hs = 16, H * D, D
    extent = n_slots * ss
    ks, vs = float(torch.tensor(0.0421, dtype=torch.float32)), float(torch.tensor(0.0173, dtype=torch.float32))
    host = types.SimpleNamespace(kind="e2e", dtype=dtype, B=rows, D=D, HQ=HQ, H=H, block_size=bs, table=table, n_slots=n_slots, slot_stride=ss,
                                 head_stride=hs, extent=extent, scale=float(D) ** -0.5, seed=[11, rows, D])
    total = 2 * AC.GUARD + extent
    k_buf, v_buf = (torch.full((total,), b, dtype=torch.uint8, device=gpu) for b in F.NAN_BYTES)
    fcs = types.SimpleNamespace(case=host)
    k, v = F.cache_view(fcs, k_buf), F.cache_view(fcs, v_buf)
    t_table = torch.from_numpy(table).to(torch.int32).to(gpu)
    written = np.zeros(total, bool)
    for step in range(3):
        pos = [step, step]
        slots = [int(table[b, p // bs]) * bs + p % bs for b, p in enumerate(pos)]
        tp, tc, ts = TQ._dev(gpu, pos, cos, sin)
        x = x0.roll(17 * step, dims=1)
        q, rk, rv = front(x, tp, tc, ts, k_cache=k, v_cache=v, slots=torch.tensor(slots, dtype=torch.int32, device=gpu), k_scale=ks, v_scale=vs)
        lens = tp + 1
        y = att(q, k, v, t_table, lens, k_scale=ks, v_scale=vs)
        assert front.last_route == "qkv_rope" and att.last_route == "attn_decode"
        for s in slots:
            written[AC.GUARD + s * ss:AC.GUARD + (s + 1) * ss] = True
        kb, vb = k_buf.cpu(), v_buf.cpu()
        for b, poison in ((kb, F.NAN_BYTES[0]), (vb, F.NAN_BYTES[1])):  # the addressed bytes are finite, the others keep their poison
            assert ((b.numpy()[written] & 0x7F) != 0x7F).all() and (b.numpy()[~written] == poison).all()
        host.k_buf, host.v_buf = F.decode(kb).double() * ks, F.decode(vb).double() * vs
        host.q_buf, host.q_stride, host.lens = q.cpu(), HQ * D, np.array(pos) + 1
        want, gate = AC.reference_of(host)
        worst = AC.excess(_f64(y), want, gate)
        print(f"FP8_GATE e2e step={step} {dt}: {worst:.3f}")
        assert np.isfinite(want).all() and worst <= 1.0, step
        # the C ABI, directly, on a workspace full of NaN patterns
        need = _lib.attn_decode_workspace_bytes(rows, HQ, D, 2, bs)
        ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=gpu)
        ws[need:] = 0xA5
        out = torch.full((rows, HQ * D), 7.0, dtype=dtype, device=gpu)
        a = _lib.SqllmAttnDecodeFp8()
        a.q, a.out, a.k_cache, a.v_cache = q.data_ptr(), out.data_ptr(), k_buf.data_ptr() + AC.GUARD, v_buf.data_ptr() + AC.GUARD
        a.block_table, a.seq_lens = t_table.data_ptr(), lens.data_ptr()
        a.batch, a.n_q_heads, a.n_kv_heads, a.head_dim = rows, HQ, H, D
        a.n_slots, a.block_size, a.max_blocks, a.table_stride = n_slots, bs, 2, 2
        a.slot_stride, a.head_stride, a.q_stride, a.out_stride = ss, hs, HQ * D, HQ * D
        a.scale, a.k_scale, a.v_scale, a.workspace = host.scale, ks, vs, ws.data_ptr()
        fn = getattr(_lib.load(), "sqllm_attn_decode_fp8_" + ("f16" if dt == "fp16" else "bf16"))
        assert fn(ctypes.byref(a), quant_cuda._raw_stream(gpu.index)) == 0
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out), _bits(y)) and bool((ws[need:] == 0xA5).all())
    TQ._clean(front)
