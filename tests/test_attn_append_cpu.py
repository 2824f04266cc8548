"""The decode attention for several new tokens per sequence without a GPU (include/sqllm_hip.h, sqllm_attn_append;
quant.DecodeAttention(..., q_len=, q_lens=)): the expansion into one-query rows against a brute-force loop, the module's torch
fallback against the existing fallback on the expanded case bit for bit, and the proof that the gate of
tests/attn_decode_cases.py still fails its five wrong oracles on the expanded cases the GPU test compares under it."""
import numpy as np
import pytest
import torch

from tests import attn_append_cases as A
from tests import attn_decode_cases as C
from tests import kv_fp8_cases as F

P = C.P
# (kind, T, D, heads, dtype): every geometry, every T, every head ratio, both widths and types among them
SMALL = [("paged", 2, 64, (8, 2), "fp16"), ("padded", 3, 128, (6, 2), "bf16"), ("bhsd", 5, 64, (16, 2), "fp16"),
         ("paged_single", 16, 128, (2, 2), "bf16"), ("paged", 1, 64, (6, 2), "bf16"), ("padded", 16, 64, (8, 2), "fp16")]


def _brute(seq_lens, T, q_lens, capacity):
    out = []
    for b, seq in enumerate(seq_lens):
        n = T if q_lens is None else q_lens[b]
        for t in range(T):
            if n > T:
                out.append(capacity + 1)  # NaN
            elif t >= n:
                out.append(0)  # padding (n < 0 included)
            else:
                L = seq - (n - 1 - t)
                out.append(0 if L <= 0 else capacity + 1 if L > capacity else L)
    return out


@pytest.mark.parametrize("T", A.Q_LENS)
def test_the_expansion_against_a_brute_force_loop(T):
    from squeezellm_amd.quant import append_as_decode_rows

    for kind in ("paged", "paged_single"):
        seqs = A.seq_lens_for(T, kind) + (0, -4, (1 << 31) - 1, -(1 << 31))
        cap = P if kind == "paged_single" else 2 * P + 16
        for ql in (None, A.q_lens_for(T, len(seqs)), A.q_lens_for(T, len(seqs) + 3)[3:]):
            want = _brute(seqs, T, ql, cap)
            assert A.token_lengths(seqs, T, ql, cap).tolist() == want
            # ... and the library's own expansion, for int32 and int64 operands
            table = torch.arange(len(seqs) * (cap // 16), dtype=torch.int32).reshape(len(seqs), -1)
            for dt in (torch.int32, torch.int64):
                tq = None if ql is None else torch.tensor(ql, dtype=dt)
                tab, lens = append_as_decode_rows(table, torch.tensor(seqs, dtype=dt), T, tq, 16)
                assert lens.dtype == dt and lens.tolist() == want
                assert tab.shape == (len(seqs) * T, cap // 16) and torch.equal(tab, table.repeat_interleave(T, dim=0))
    # the choices hold what their reasons say
    if T > 1:
        seqs = A.seq_lens_for(T)
        L = A.token_lengths(seqs, T, None, 2 * P + 16).reshape(len(seqs), T)
        assert any(row.min() <= P < row.max() for row in L), "a sequence whose tokens straddle the partition"
        assert any(row.min() == 0 and row.max() >= 1 for row in L), "a sequence shorter than its tokens"
    assert all(len(b) * T <= A.MAX_ROWS for b in A.batches(T))
    assert sorted({T * hq // hk for T in A.Q_LENS for hq, hk in A.HEADS} & {1, 8, 9, 15, 20, 128}) == [1, 8, 9, 15, 20, 128]


def _args(base, case):
    k, v = (C.cache_view(base, t) for t in (base.k_buf, base.v_buf))
    q = case.q_buf[:, :case.HQ * case.D]
    i32 = lambda a: torch.from_numpy(np.asarray(a)).to(torch.int32)  # noqa: E731
    return q, k, v, i32(base.table), i32(base.lens), i32(case.table), i32(case.lens)


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("kind,T,D,heads,dt", SMALL)
def test_the_fallback_is_the_existing_fallback_on_the_expanded_case(kind, T, D, heads, dt, ragged):
    from squeezellm_amd.quant import DecodeAttention

    hq, hk = heads
    for seqs, ql in A.ragged_batches(T, kind) if ragged else [(A.batches(T, kind)[-1], None)]:
        _fallback_on(kind, T, D, hq, hk, dt, seqs, ql)


def _fallback_on(kind, T, D, hq, hk, dt, seqs, ql):
    from squeezellm_amd.quant import DecodeAttention

    base, case, want, gate = A.reference(kind, T, D, hq, hk, dt, seqs, ql)
    att = DecodeAttention(hq, hk, D, block_size=base.block_size)
    q, k, v, table, seq_lens, table_x, lens_x = _args(base, case)
    tq = None if ql is None else torch.tensor(ql, dtype=torch.int32)
    got = att(q, k, v, table, seq_lens, q_len=T, q_lens=tq)
    assert att.last_route == "fallback" and got.dtype == case.dtype and got.shape == (len(seqs) * T, hq * D)
    one = att(q, k, v, table_x, lens_x)  # today's call, on the expansion
    assert torch.equal(got.view(torch.int16), one.view(torch.int16))
    assert C.excess(got.double().numpy(), want, gate) <= 1.0
    # [batch, q_len, W], int64 operands, out=
    got3 = att(q.contiguous().reshape(len(seqs), T, -1), k, v, table.long(), seq_lens.long(), q_len=T, q_lens=None if tq is None else tq.long())
    assert got3.shape == (len(seqs), T, hq * D) and torch.equal(got3.reshape(len(seqs) * T, -1).view(torch.int16), one.view(torch.int16))
    out = torch.full((len(seqs) * T, hq * D + 3), 7.0, dtype=case.dtype)[:, :hq * D]
    assert att(q, k, v, table, seq_lens, out=out, q_len=T, q_lens=tq) is out and torch.equal(out.view(torch.int16), one.view(torch.int16))
    # the corner rows are where the contract puts them
    lens = case.lens.reshape(len(seqs), T)
    g = got.double().numpy().reshape(len(seqs), T, -1)
    assert (g[lens == 0] == 0).all() and not np.signbit(g[lens == 0]).any()
    assert np.isnan(g[lens > base.table.shape[1] * base.block_size]).all()
    assert np.isfinite(g[(lens > 0) & (lens <= base.table.shape[1] * base.block_size)]).all()


@pytest.mark.parametrize("kind,T,D,heads,dt", SMALL[:3])
def test_the_fallback_over_an_fp8_cache(kind, T, D, heads, dt):
    from squeezellm_amd.quant import DecodeAttention

    hq, hk = heads
    seqs, ql = A.ragged_batches(T, kind)[-1]
    fc = F.fp8_case(kind, len(seqs), D, hq, hk, dt, F.SCALES, 0, tuple(seqs))
    case = A.expand(fc.case, T, ql)
    att = DecodeAttention(hq, hk, D, block_size=fc.case.block_size)
    q, _, _, table, seq_lens, table_x, lens_x = _args(fc.case, case)
    k, v = F.cache_view(fc, fc.k_bytes), F.cache_view(fc, fc.v_bytes)
    kw = dict(k_scale=fc.k_scale, v_scale=fc.v_scale)
    got = att(q, k, v, table, seq_lens, q_len=T, q_lens=torch.tensor(ql, dtype=torch.int32), **kw)
    assert att.last_route == "fallback"
    assert torch.equal(got.view(torch.int16), att(q, k, v, table_x, lens_x, **kw).view(torch.int16))


def test_the_module_rejects_what_it_cannot_take():
    from squeezellm_amd.quant import DecodeAttention

    base, case = A.build("paged", 2, 64, 8, 2, "fp16", (5, 40, 3))
    att = DecodeAttention(8, 2, 64, block_size=16)
    q, k, v, table, seq_lens, table_x, lens_x = _args(base, case)
    ql = torch.tensor([2, 1, 0], dtype=torch.int32)
    att(q, k, v, table, seq_lens, q_len=2, q_lens=ql)
    for bad in (dict(q_len=0), dict(q_len=-1), dict(q_len=4), dict(q_lens=ql), dict(q_len=2, q_lens=ql[:2]), dict(q_len=2, q_lens=ql.float()),
                dict(q_len=3)):
        with pytest.raises(ValueError):
            att(q, k, v, table, seq_lens, **bad)
    with pytest.raises(ValueError):
        att(q, k, v, table_x, seq_lens, q_len=2)  # one table row per SEQUENCE
    with pytest.raises(ValueError):
        att(q.contiguous().reshape(2, 3, -1), k, v, table, seq_lens, q_len=2)  # [batch, q_len, W] or nothing
    # without the new arguments the call is today's: one row per table row
    assert att(q, k, v, table_x, lens_x).shape == (6, 512) and att.last_route == "fallback"


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("kind,T,D,heads,dt", SMALL)
def test_the_gate_fails_every_mutant_on_the_expanded_cases(kind, T, D, heads, dt, ragged):
    hq, hk = heads
    # (ragged: the first call, whose classes 0, 1, T - 1, T leave rows of many keys; the last call's T + 1 and -3 leave none)
    seqs, ql = A.ragged_batches(T, kind)[0] if ragged else (A.batches(T, kind)[-1], None)
    base, case, want, gate = A.reference(kind, T, D, hq, hk, dt, seqs, ql)
    rounded = torch.from_numpy(want).to(case.dtype).double().numpy()
    assert C.excess(rounded, want, gate) <= 1.0
    for mutant in C.MUTANTS:
        wrong = torch.from_numpy(C.oracle(case, mutant)[0]).to(case.dtype).double().numpy()
        assert C.excess(wrong, want, gate) > 1.0, mutant
