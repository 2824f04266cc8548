"""The decode attention for several new tokens per sequence on the GPU (sqllm_attn_append_f16 / _bf16 / _fp8_f16 / _fp8_bf16
behind quant.DecodeAttention(..., q_len=, q_lens=); include/sqllm_hip.h, sqllm_attn_append), on the cases of
tests/attn_append_cases.py: a one-query case of sequences and its expansion into batch * T one-query rows.

The main gate is BIT IDENTITY with the same library's one-query entries on the expansion (torch.equal on the raw 16-bit words):
that is the entry's definition, and what makes verifying T tokens at once yield what T decode steps would.  Identity to a sibling
does not hide a bug shared with it, so a subset also passes the fp64 oracle under the gate of tests/attn_decode_cases.py
(excess <= 1; tests/test_attn_append_cpu.py shows the five wrong oracles fail it on these expanded cases).  The three hazards
of the design each have a test: a later token's NaN, sequences whose tokens straddle a partition (in every T > 1 case, and
per token under the oracle), and seq_lens < n_b (the first tokens are +0 rows while the last ones attend 1, 2, ... keys)."""
import copy
import ctypes
import types

import numpy as np
import pytest

from tests import attn_append_cases as A
from tests import attn_decode_cases as C
from tests import kv_fp8_cases as F
from tests.test_gpu_attn_decode import _bits, _f64, _node_types, _poison_lds, _poison_workspaces

gpu_test = pytest.mark.gpu
P = C.P
# every geometry x T x head ratio; head_dim and the type alternate so that each occurs with each of them
IDENTITY = [(kind, T, (64, 128)[(i + j) % 2], hq, hk, ("fp16", "bf16")[(i + j // 2 + g) % 2])
            for g, kind in enumerate(A.GEOMETRIES) for i, T in enumerate(A.Q_LENS) for j, (hq, hk) in enumerate(A.HEADS)]
SUBSET = [("paged", 2, 128, 8, 2, "fp16"), ("padded", 3, 64, 6, 2, "bf16"), ("bhsd", 5, 128, 16, 2, "bf16"), ("paged_single", 16, 64, 2, 2, "fp16"),
          ("padded", 16, 128, 8, 2, "fp16"), ("paged", 5, 64, 6, 2, "bf16")]


class Dev:
    """a case's operands on the GPU: the guarded caches (16-bit, or e4m3 bytes with their scales) and their views, q of all
    batch * T rows, the sequences' table / lengths / q_lens and the expansion's table / lengths as int32"""

    def __init__(self, gpu, base, case, fc=None):
        import torch

        self.base, self.case, self.fc, self.T = base, case, fc, case.T
        i32 = lambda a: torch.from_numpy(np.asarray(a)).to(torch.int32).to(gpu)  # noqa: E731
        if fc is None:
            self.k_buf, self.v_buf = base.k_buf.to(gpu), base.v_buf.to(gpu)
            self.k, self.v = (C.cache_view(base, t) for t in (self.k_buf, self.v_buf))
            self.kw = {}
        else:
            self.k_buf, self.v_buf = fc.k_bytes.to(gpu), fc.v_bytes.to(gpu)
            self.k, self.v = (F.cache_view(fc, t) for t in (self.k_buf, self.v_buf))
            self.kw = dict(k_scale=fc.k_scale, v_scale=fc.v_scale)
        self.q_buf = case.q_buf.to(gpu)
        self.q = self.q_buf[:, :case.HQ * case.D]
        self.table, self.seq = i32(base.table), i32(base.lens)
        self.q_lens = None if case.q_lens is None else i32(case.q_lens)
        self.table_x, self.lens_x = i32(case.table), i32(case.lens)

    def module(self):
        from squeezellm_amd.quant import DecodeAttention

        c = self.base
        att = DecodeAttention(c.HQ, c.H, c.D, block_size=c.block_size)
        att.append_route = "kernel"  # the kernels under test, whatever the measured routing would pick for the shape
        return att

    def append(self, att=None, seqs=slice(None), out=None):
        """the call under test, over the sequences `seqs` (a slice)"""
        att = att or self.module()
        b0, b1, _ = seqs.indices(self.base.B)
        ql = None if self.q_lens is None else self.q_lens[seqs]
        y = att(self.q[b0 * self.T:b1 * self.T], self.k, self.v, self.table[seqs], self.seq[seqs], out=out, q_len=self.T, q_lens=ql, **self.kw)
        assert att.last_route == "attn_append"
        return y

    def decode(self, att=None):
        """the one-query entry on the expansion: what the call under test is defined by"""
        att = att or self.module()
        y = att(self.q, self.k, self.v, self.table_x, self.lens_x, **self.kw)
        assert att.last_route == "attn_decode"
        return y


def _dev(gpu, kind, T, D, hq, hk, dt, seqs, q_lens=None, fp8=False, poison=0):
    base, case = A.build(kind, T, D, hq, hk, dt, tuple(seqs), q_lens, poison)
    fc = F.fp8_case(kind, len(seqs), D, hq, hk, dt, F.SCALES, poison, tuple(seqs)) if fp8 else None
    if fc is not None and poison == 0:
        assert fc.case is base
    return Dev(gpu, base, case, fc)


# ---- 1. bit identity with the one-query entries: the main gate ----

@gpu_test
@pytest.mark.parametrize("kind,T,D,hq,hk,dt", IDENTITY)
def test_bit_identity_with_the_decode_entries_on_the_expanded_case(gpu, kind, T, D, hq, hk, dt):
    """every batch of seq_lens_for(T), q_lens NULL and ragged, a 16-bit and an fp8 cache"""
    import torch

    for seqs, ragged in A.ragged_batches(T, kind):  # (between them the calls meet every class of q_lens, T + 1 and -3 included)
        for ql in (None, ragged):
            for fp8 in (False, True):
                d = _dev(gpu, kind, T, D, hq, hk, dt, seqs, ql, fp8)
                att = d.module()
                got, want = d.append(att), d.decode(att)
                assert got.shape == want.shape == (len(seqs) * T, hq * D) and got.dtype == want.dtype
                assert torch.equal(got.view(torch.int16), want.view(torch.int16)), (seqs, ql, fp8)
                live = (d.case.lens > 0) & (d.case.lens <= d.base.table.shape[1] * d.base.block_size)
                assert bool(torch.isfinite(got[torch.from_numpy(live).to(gpu)]).all())


# ---- 2. parity with the fp64 oracle ----

@gpu_test
@pytest.mark.parametrize("kind,T,D,hq,hk,dt", SUBSET)
def test_parity_with_the_oracle(gpu, kind, T, D, hq, hk, dt):
    for seqs, ragged in A.ragged_batches(T, kind)[-2:]:
        for ql in (None, ragged):
            base, case, want, gate = A.reference(kind, T, D, hq, hk, dt, tuple(seqs), ql)
            d = Dev(gpu, base, case)
            worst = C.excess(_f64(d.append()), want, gate)
            print(f"APPEND_GATE {kind} T={T} D={D} heads={hq}/{hk} {dt} seqs={seqs} q_lens={ql}: {worst:.3f}")
            assert worst <= 1.0, worst
    # ... and over the dequantised bytes of an fp8 cache
    seqs = A.batches(T, kind)[-1]
    fc = F.fp8_case(kind, len(seqs), D, hq, hk, dt, F.SCALES, 0, tuple(seqs))
    case = A.expand(fc.case, T)
    want, gate = C.reference_of(A.expand(fc.shadow, T))
    worst = C.excess(_f64(Dev(gpu, fc.case, case, fc).append()), want, gate)
    print(f"APPEND_GATE fp8 {kind} T={T} D={D} heads={hq}/{hk} {dt}: {worst:.3f}")
    assert worst <= 1.0, worst


# ---- 3. a later token's NaN ----

@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("T,seq", [(3, 40), (5, P + 2), (16, 2 * P + 3)])
def test_a_nan_at_a_key_only_the_last_token_attends(gpu, T, seq, dt, fp8):
    """one NaN in k, then one in v, at key seq - 1: the earlier tokens' rows stay finite and bit-identical to the run without it
    (their weight for that key is a select, never a factor 0); the last token's row follows the sibling's NaN rule"""
    import torch

    d = _dev(gpu, "paged", T, 64, 8, 2, dt, (9, seq, 3), None, fp8)
    plain = _bits(d.append()).reshape(3, T, 8, 64)
    slot = int(d.base.table[1, (seq - 1) // 16]) * 16 + (seq - 1) % 16
    nan = 0x7F if fp8 else float("nan")
    for which, (h, col) in ((d.k, (1, 5)), (d.v, (0, 9))):
        cache = which.view(torch.uint8) if fp8 else which  # (through the bytes: torch has no indexing for float8)
        keep = cache[slot, h, col].clone()
        cache[slot, h, col] = nan
        y = d.append()
        assert torch.equal(y.view(torch.int16), d.decode().view(torch.int16))
        got = _f64(y).reshape(3, T, 8, 64)
        same = np.ones((3, T, 8, 64), bool)
        if which is d.k:  # the query heads of kv head 1, every column
            assert np.isnan(got[1, T - 1, 4:]).all()
            same[1, T - 1, 4:] = False
        else:  # column 9 of the query heads of kv head 0
            assert np.isnan(got[1, T - 1, :4, 9]).all()
            same[1, T - 1, :4, 9] = False
        assert np.isfinite(got[same]).all() and np.array_equal(_bits(y).reshape(3, T, 8, 64)[same], plain[same])
        cache[slot, h, col] = keep


# ---- 4. isolation and writes ----

@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("kind,T,D,hq,hk,dt", SUBSET[:4])
def test_sequences_alone_the_other_poison_a_second_run_and_nothing_else_written(gpu, kind, T, D, hq, hk, dt, fp8):
    import torch

    seqs, ql = A.ragged_batches(T, kind)[-1]  # (the last call's q_lens hold T + 1 and -3)
    d = _dev(gpu, kind, T, D, hq, hk, dt, seqs, ql, fp8)
    att = d.module()
    y = _bits(d.append(att))
    for b in range(len(seqs)):  # a call of one sequence: another batch size, the same rows
        assert np.array_equal(_bits(d.append(seqs=slice(b, b + 1))), y[b * T:(b + 1) * T]), b
    other = _dev(gpu, kind, T, D, hq, hk, dt, seqs, ql, fp8, poison=1)
    assert not torch.equal(other.k_buf.view(torch.uint8), d.k_buf.view(torch.uint8))
    assert np.array_equal(_bits(other.append()), y)
    _poison_workspaces(att)
    _poison_lds()
    assert np.array_equal(_bits(d.append(att)), y)
    # out: more rows than needed and rows wider than needed, NaN-filled, inside a guarded allocation
    rows, W, stride, guard = len(seqs) * T, hq * D, hq * D + 11, 512
    backing = C._poisoned(guard + (rows + 2) * stride + guard, d.case.dtype, 1).to(gpu)
    pattern = backing.view(torch.int16).clone()
    out = backing[guard:guard + rows * stride].view(rows, stride)[:, :W]
    before = [t.clone() for t in (d.k_buf, d.v_buf, d.q_buf, d.table, d.seq, d.q_lens)]
    assert d.append(att, out=out) is out and np.array_equal(_bits(out), y)
    touched = torch.zeros(backing.numel(), dtype=torch.bool, device=gpu)
    touched[guard:guard + rows * stride].view(rows, stride)[:, :W] = True
    assert torch.equal(backing.view(torch.int16)[~touched], pattern[~touched])
    for t, b in zip((d.k_buf, d.v_buf, d.q_buf, d.table, d.seq, d.q_lens), before):
        assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))


# ---- 5. corner rows ----

@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("kind", ["paged", "paged_single"])
def test_padding_rows_zero_rows_nan_rows_and_a_bad_table_entry(gpu, kind, dt, fp8):
    """nothing out of range is read: the contract, not a provocation -- the kernel decides on the table's values before it touches
    the caches, and a bad key's stand-in slot is an attended one"""
    import torch

    T = 5
    long_ = P if kind == "paged_single" else 2 * P + 3
    seqs = (3, long_, 40, 2)  # 3 < T and 2 < T: their first tokens have L <= 0
    d = _dev(gpu, kind, T, 64, 8, 2, dt, seqs, (5, 5, 3, 2), fp8)
    y = d.append()
    assert torch.equal(y.view(torch.int16), d.decode().view(torch.int16))
    got = _f64(y).reshape(4, T, -1)
    L = d.case.lens.reshape(4, T)
    assert L[0].tolist() == [0, 0, 1, 2, 3] and L[2].tolist() == [38, 39, 40, 0, 0] and L[3].tolist() == [1, 2, 0, 0, 0]
    zero = got[L == 0]
    assert (zero == 0).all() and not np.signbit(zero).any() and np.isfinite(got[L > 0]).all()
    plain = _bits(y).reshape(4, T, -1)
    cap = d.base.table.shape[1] * d.base.block_size
    # q_lens beyond T: all T rows of that sequence NaN; negative: all +0; the neighbours are what they were
    d.q_lens.copy_(torch.tensor([6, -3, 3, 2], dtype=torch.int32))
    got = _f64(d.append()).reshape(4, T, -1)
    assert np.isnan(got[0]).all() and (got[1] == 0).all() and not np.signbit(got[1]).any()
    assert np.array_equal(_bits(d.append()).reshape(4, T, -1)[2:], plain[2:])
    d.q_lens.copy_(torch.tensor([5, 5, 3, 2], dtype=torch.int32))
    # a length beyond the capacity, per token: seq_lens = capacity + 2 makes the last two tokens NaN, the others are served
    d.seq[1] = cap + 2
    y = d.append()
    got = _f64(y).reshape(4, T, -1)
    assert np.isnan(got[1, 3:]).all() and np.array_equal(_bits(y).reshape(4, T, -1)[[0, 2, 3]], plain[[0, 2, 3]])
    if kind == "paged_single":  # (where the keys up to the capacity are all there: the tokens below it are finite, and the decode entry's)
        assert np.isfinite(got[1, :3]).all()
        x = copy.copy(d.case)
        x.lens = A.token_lengths((3, cap + 2, 40, 2), T, (5, 5, 3, 2), cap)
        d.lens_x.copy_(torch.from_numpy(x.lens).to(torch.int32))
        assert torch.equal(y.view(torch.int16), d.decode().view(torch.int16))
        d.lens_x.copy_(torch.from_numpy(d.case.lens).to(torch.int32))
    d.seq[1] = long_
    # a bad table entry in the middle of sequence 2 (block 2: keys 32 .. 47; tokens with L 38, 39, 40 all use it) and at the end
    # of sequence 1's walk (the block of its last key only): the tokens below stay exact, the tokens above are NaN
    for entry in (d.base.n_slots // d.base.block_size, -1, (1 << 31) - 1, -(1 << 31)):
        last_blk = (long_ - 1) // 16
        keep = d.table[1, last_blk].clone(), d.table[2, 2].clone()
        d.table[1, last_blk] = entry
        d.table[2, 2] = entry
        y = d.append()
        got = _f64(y).reshape(4, T, -1)
        first_bad = last_blk * 16  # tokens of sequence 1 with L > first_bad are NaN
        L1 = L[1]
        assert np.isnan(got[1, L1 > first_bad]).all() and (L1 > first_bad).any()
        assert np.array_equal(_bits(y).reshape(4, T, -1)[1, L1 <= first_bad], plain[1, L1 <= first_bad])
        assert np.isnan(got[2, :3]).all() and (got[2, 3:] == 0).all()
        assert np.array_equal(_bits(y).reshape(4, T, -1)[[0, 3]], plain[[0, 3]])
        d.table_x.copy_(torch.from_numpy(d.case.table).to(torch.int32))
        d.table_x[T:2 * T, last_blk] = entry
        d.table_x[2 * T:3 * T, 2] = entry
        assert torch.equal(y.view(torch.int16), d.decode().view(torch.int16))
        d.table_x.copy_(torch.from_numpy(d.case.table).to(torch.int32))
        d.table[1, last_blk], d.table[2, 2] = keep
    assert np.array_equal(_bits(d.append()).reshape(4, T, -1), plain)


@gpu_test
@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_a_bad_entry_between_the_tokens_of_one_sequence(gpu, dt):
    """blocks of 5 keys ("padded"): with seq_lens = P + 2 and T = 5 the tokens end at P-2 .. P+2; a bad entry at the block of keys
    P .. P+4 (P = 256 is no multiple of 5: the block 255 .. 259) makes NaN exactly the tokens with L > 255"""
    import torch

    T, seq = 5, P + 2
    d = _dev(gpu, "padded", T, 128, 6, 2, dt, (seq, 7), None)
    plain = _bits(d.append()).reshape(2, T, -1)
    blk = 255 // 5
    d.table[0, blk] = -1
    y = d.append()
    got = _f64(y).reshape(2, T, -1)
    L = d.case.lens.reshape(2, T)[0]
    assert L.tolist() == [P - 2, P - 1, P, P + 1, P + 2]
    assert np.isnan(got[0, L > 255]).all() and np.array_equal(_bits(y).reshape(2, T, -1)[0, L <= 255], plain[0, L <= 255])
    assert np.array_equal(_bits(y).reshape(2, T, -1)[1], plain[1])


# ---- 6. capture ----

@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("kind,nodes", [("paged", 2), ("paged_single", 1)])
def test_a_captured_call_follows_seq_lens_and_q_lens_updated_in_place(gpu, kind, nodes, fp8):
    import torch

    T = 3
    top = P + 2 if kind == "paged" else P
    d = _dev(gpu, kind, T, 128, 8, 2, "bf16", (top, 9, 40), (3, 3, 3), fp8)
    att = d.module()
    out = torch.empty((3 * T, 8 * 128), dtype=d.case.dtype, device=gpu)
    d.seq.copy_(torch.tensor([top - 4, 5, 40], dtype=torch.int32))
    run = lambda: d.append(att, out=out)  # noqa: E731
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
    for seq, ql in (((top - 2, 7, 40), (3, 2, 1)), ((top, 9, 39), (2, 3, 0)), ((top - 1, 8, 40), (3, 3, 3))):
        d.seq.copy_(torch.tensor(seq, dtype=torch.int32))  # in place: the graph holds the addresses
        d.q_lens.copy_(torch.tensor(ql, dtype=torch.int32))
        out.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        replayed = _bits(out)
        assert np.array_equal(replayed, _bits(d.append())), (seq, ql)  # a fresh eager call
        cap = d.base.table.shape[1] * d.base.block_size
        d.lens_x.copy_(torch.from_numpy(A.token_lengths(seq, T, ql, cap)).to(torch.int32))
        assert np.array_equal(replayed, _bits(d.decode())), (seq, ql)


# ---- 7. behind the attention front ----

@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dt", list(C.DTYPES))
def test_one_front_call_writes_t_tokens_the_append_entry_reads_them(gpu, dt, fp8):
    """one QuantQKVRopeFused call with T rows of ONE sequence (positions 3 .. 3+T-1 behind three earlier tokens) writes the cache;
    the append entry on that q and cache equals the expanded decode call, and passes the oracle formed from the cache's contents"""
    import torch

    from squeezellm_amd import quant
    from tests import test_gpu_qkv_rope as TQ

    T, first, (Nq, Nk, Nv, D) = 4, 3, TQ.SHAPES["d64"]
    HQ, H, bs = Nq // D, Nk // D, 2
    dtype = C.DTYPES[dt]
    front = TQ._module(TQ._members(gpu, 4, "hybrid", "d64"), D, "half", fused_members=True)
    att = quant.DecodeAttention(HQ, H, D, block_size=bs)
    att.append_route = "kernel"
    cos, sin = TQ._tables(D)
    table = np.array([[5, 2, 0, 7]], dtype=np.int64)
    n_slots, ss, hs = 16, H * D, D
    extent = n_slots * ss
    host = types.SimpleNamespace(kind="e2e", dtype=dtype, B=1, D=D, HQ=HQ, H=H, block_size=bs, table=table, n_slots=n_slots, slot_stride=ss,
                                 head_stride=hs, extent=extent, scale=float(D) ** -0.5, seed=[12, T, D], q_stride=HQ * D)
    ks, vs = float(torch.tensor(0.0421, dtype=torch.float32)), float(torch.tensor(0.0173, dtype=torch.float32))
    kw = dict(k_scale=ks, v_scale=vs) if fp8 else {}
    if fp8:
        k_buf, v_buf = (torch.full((2 * C.GUARD + extent,), b, dtype=torch.uint8, device=gpu) for b in F.NAN_BYTES)
        k, v = (F.cache_view(types.SimpleNamespace(case=host), t) for t in (k_buf, v_buf))
    else:
        k_buf, v_buf = (C._poisoned(2 * C.GUARD + extent, dtype, 0).to(gpu) for _ in range(2))
        k, v = C.cache_view(host, k_buf), C.cache_view(host, v_buf)
    t_table = torch.from_numpy(table).to(torch.int32).to(gpu)
    slot = lambda p: int(table[0, p // bs]) * bs + p % bs  # noqa: E731
    for pos in ([0, 1, 2], list(range(first, first + T))):  # three tokens before, then the step under test: T rows of one sequence
        tp, tc, ts = TQ._dev(gpu, pos, cos, sin)
        x = TQ._x(gpu, len(pos), str(dtype).split(".")[1]).roll(7 * len(pos), dims=1)
        q = front(x, tp, tc, ts, k_cache=k, v_cache=v, slots=torch.tensor([slot(p) for p in pos], dtype=torch.int32, device=gpu), **kw)[0]
    assert front.last_route == "qkv_rope"
    seq_lens = torch.tensor([first + T], dtype=torch.int32, device=gpu)
    y = att(q, k, v, t_table, seq_lens, q_len=T, **kw)
    assert att.last_route == "attn_append" and y.shape == (T, HQ * D)
    lens_x = (tp + 1).to(torch.int32)  # position + 1 per token: the emulation
    one = att(q, k, v, t_table.expand(T, -1).contiguous(), lens_x, **kw)
    assert att.last_route == "attn_decode" and torch.equal(y.view(torch.int16), one.view(torch.int16))
    if fp8:
        host.k_buf, host.v_buf = F.decode(k_buf.cpu()).double() * ks, F.decode(v_buf.cpu()).double() * vs
    else:
        host.k_buf, host.v_buf = k_buf.cpu(), v_buf.cpu()
    host.lens = np.array([first + T])
    case = A.expand(host, T)
    case.q_buf = q.cpu()
    want, gate = C.reference_of(case)
    worst = C.excess(_f64(y), want, gate)
    print(f"APPEND_GATE e2e {dt} fp8={fp8}: {worst:.3f}")
    assert np.isfinite(want).all() and worst <= 1.0


# ---- 8. the C ABI directly, and the module's surface ----

@gpu_test
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dt", list(C.DTYPES))
@pytest.mark.parametrize("kind", ["padded", "bhsd", "paged_single"])
def test_c_abi_directly(gpu, kind, dt, fp8):
    """the descriptor filled in by hand, a workspace of exactly the documented size full of NaN patterns with a guard behind it,
    the LDS poisoned in front of the launch: the module's bits (which are the decode entry's), the guards intact"""
    import torch

    from squeezellm_amd import _lib, quant_cuda

    T = 3
    seqs, ql = A.ragged_batches(T, kind)[-1]  # (the last call's q_lens hold T + 1 and -3)
    d = _dev(gpu, kind, T, 128, 8, 2, dt, seqs, ql, fp8)
    base, rows, W = d.base, len(seqs) * T, 8 * 128
    out = torch.full((rows, W + 4), 7.0, dtype=base.dtype, device=gpu)
    need = _lib.attn_decode_workspace_bytes(rows, base.HQ, base.D, base.table.shape[1], base.block_size)
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=gpu)
    ws[need:] = 0xA5
    a = _lib.SqllmAttnAppendFp8() if fp8 else _lib.SqllmAttnAppend()
    celem = 1 if fp8 else 2
    a.q, a.out = d.q_buf.data_ptr(), out.data_ptr()
    a.k_cache, a.v_cache = d.k_buf.data_ptr() + celem * C.GUARD, d.v_buf.data_ptr() + celem * C.GUARD
    a.block_table, a.seq_lens, a.q_lens, a.q_len = d.table.data_ptr(), d.seq.data_ptr(), d.q_lens.data_ptr(), T
    a.batch, a.n_q_heads, a.n_kv_heads, a.head_dim = len(seqs), base.HQ, base.H, base.D
    a.n_slots, a.block_size, a.max_blocks, a.table_stride = base.n_slots, base.block_size, base.table.shape[1], base.table.shape[1]
    a.slot_stride, a.head_stride, a.q_stride, a.out_stride = base.slot_stride, base.head_stride, base.q_stride, W + 4
    a.scale, a.workspace = base.scale, ws.data_ptr()
    if fp8:
        a.k_scale, a.v_scale = d.fc.k_scale, d.fc.v_scale
    stream = quant_cuda._raw_stream(gpu.index)
    _poison_lds()
    fn = getattr(_lib.load(), "sqllm_attn_append_" + ("fp8_" if fp8 else "") + ("f16" if dt == "fp16" else "bf16"))
    assert fn(ctypes.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert bool((out[:, W:] == 7.0).all()) and bool((ws[need:] == 0xA5).all())
    assert np.array_equal(_bits(out[:, :W]), _bits(d.append())) and np.array_equal(_bits(out[:, :W]), _bits(d.decode()))
    a.q_lens = None  # NULL: q_len real tokens everywhere
    assert fn(ctypes.byref(a), stream) == 0
    torch.cuda.synchronize()
    d.q_lens = None
    assert np.array_equal(_bits(out[:, :W]), _bits(d.append()))


@gpu_test
def test_module_surface(gpu):
    """routes, [batch, q_len, W], int64 operands, out=, the fallback for what the kernels do not serve; the defaults keep today's call"""
    import torch

    from squeezellm_amd.quant import DecodeAttention

    T, seqs = 3, (2 * P + 3, 9, P + 1)
    ql = (3, 1, 2)
    base, case, want, gate = A.reference("paged", T, 64, 8, 2, "fp16", seqs, ql)
    d = Dev(gpu, base, case)
    att = d.module()
    y = _bits(d.append(att))
    assert C.excess(_f64(d.append(att)), want, gate) <= 1.0
    y3 = att(d.q.contiguous().reshape(3, T, -1), d.k, d.v, d.table.long(), d.seq.long(), q_len=T, q_lens=d.q_lens.long())
    assert att.last_route == "attn_append" and y3.shape == (3, T, 8 * 64) and np.array_equal(_bits(y3).reshape(3 * T, -1), y)
    out = torch.empty((3 * T, 8 * 64), dtype=case.dtype, device=gpu)
    assert att(d.q, d.k, d.v, d.table, d.seq, out=out, q_len=T, q_lens=d.q_lens) is out and np.array_equal(_bits(out), y)
    f32 = att(d.q.float(), d.k.float(), d.v.float(), d.table, d.seq, q_len=T, q_lens=d.q_lens)
    assert att.last_route == "fallback" and f32.dtype == torch.float32 and C.excess(_f64(f32.to(case.dtype)), want, gate) <= 1.0
    # q_len beyond 16 is the fallback's: one sequence of 17 rows
    q17 = d.q[:1].expand(17, -1).contiguous()
    y17 = att(q17, d.k, d.v, d.table[:1], d.seq[:1], q_len=17)
    assert att.last_route == "fallback" and y17.shape == (17, 8 * 64) and bool(torch.isfinite(y17).all())
    # without the new arguments the call is today's
    assert np.array_equal(_bits(att(d.q, d.k, d.v, d.table_x, d.lens_x)), y) and att.last_route == "attn_decode"
    # routing by measurement is invisible but for last_route: "auto" takes the append kernels, but for an fp8 cache at 64 rows,
    # which takes the expansion on the one-query kernels; "emulate" and "kernel" force either way
    auto = DecodeAttention(8, 2, 64, block_size=base.block_size)
    assert auto.append_route == "auto"
    assert np.array_equal(_bits(auto(d.q, d.k, d.v, d.table, d.seq, q_len=T, q_lens=d.q_lens)), y) and auto.last_route == "attn_append"
    auto.append_route = "emulate"
    assert np.array_equal(_bits(auto(d.q, d.k, d.v, d.table, d.seq, q_len=T, q_lens=d.q_lens)), y) and auto.last_route == "attn_decode"
    auto.append_route = "auto"
    d8 = _dev(gpu, "paged", 16, 64, 2, 2, "fp16", (P + 2, 9, 2 * P + 3, 40), None, True)  # fp8, 4 x 16 = 64 rows
    y8 = _bits(d8.append())
    one = DecodeAttention(2, 2, 64, block_size=base.block_size)
    assert np.array_equal(_bits(one(d8.q, d8.k, d8.v, d8.table, d8.seq, q_len=16, **d8.kw)), y8) and one.last_route == "attn_decode"
    assert np.array_equal(_bits(one(d8.q[:48], d8.k, d8.v, d8.table[:3], d8.seq[:3], q_len=16, **d8.kw)), y8[:48]) and one.last_route == "attn_append"
    d1 = d8
    one.append_route = "sideways"
    with pytest.raises(ValueError):
        one(d1.q, d1.k, d1.v, d1.table, d1.seq, q_len=16, **d1.kw)


@gpu_test
def test_one_instance_serves_the_four_kinds_in_turn_from_one_descriptor_cache(gpu):
    """one-query 16-bit, one-query fp8, append 16-bit, append fp8, twice round on one instance and one stream: each call fills the
    descriptor of its own kind, so every output is what a fresh instance gives for the same call.  2 sequences of 2 new tokens
    (300 keys: two partitions and the combine; 17 keys: one partition), 4 query heads over 2 kv heads of 64, blocks of 16"""
    import torch

    d16 = _dev(gpu, "paged", 2, 64, 4, 2, "fp16", (300, 17))
    d8 = _dev(gpu, "paged", 2, 64, 4, 2, "fp16", (300, 17), None, True)
    assert d16.base.block_size == 16 and d16.table.shape[1] * 16 > P  # (more than one partition: the workspace and the combine are in use)
    calls = [(d16, Dev.decode), (d8, Dev.decode), (d16, Dev.append), (d8, Dev.append)]
    want = [call(d, d.module()) for d, call in calls]
    assert all(bool(torch.isfinite(y).all()) for y in want) and not torch.equal(want[0], want[1])  # (the fp8 cache is other data)
    att = d16.module()
    for _ in range(2):
        for (d, call), y in zip(calls, want):
            assert torch.equal(call(d, att), y)
    assert sorted(k[0] for k in att._desc) == [0, 1, 2, 3]  # one descriptor per kind
