"""The decode attention without a GPU: the fp64 oracle of tests/attn_decode_cases.py against torch SDPA, the module's torch
fallback against the oracle, the static cache's three helpers against each other, fuse_decode_attention, and the proof that
the GPU test's gate, on the GPU test's own inputs, is tight enough to fail five wrong oracles at every shape."""
import copy

import numpy as np
import pytest
import torch

from tests import attn_decode_cases as C

P = C.P
ALL = [(kind, rows, D, hq, hk, dt) for kind in C.GEOMETRIES + ("paged_single",) for rows in (1, 3, 5) for D in (64, 128)
       for hq, hk in C.HEADS for dt in C.DTYPES]
SMALL = [("paged", 3, 64, 8, 2, "fp16"), ("bhsd", 5, 64, 6, 2, "bf16"), ("padded", 5, 128, 2, 2, "fp16"), ("paged_single", 5, 64, 8, 2, "bf16")]


def _module_args(case, device="cpu"):
    k, v = (C.cache_view(case, t.to(device)) for t in (case.k_buf, case.v_buf))
    q = case.q_buf.to(device)[:, :case.HQ * case.D]
    return q, k, v, torch.from_numpy(case.table).to(torch.int32).to(device), torch.from_numpy(case.lens).to(torch.int32).to(device)


def test_the_partition_is_the_librarys():
    from squeezellm_amd import _lib, quant

    header = open(_lib.HERE + "/../include/sqllm_hip.h").read()
    assert f"#define SQLLM_ATTN_PARTITION {P}\n" in header and quant.ATTN_PARTITION == P == 256
    assert sorted({n for ls in C.ROW_LENGTHS.values() for n in ls}) == sorted(C.LENGTHS)  # every length of the issue occurs


@pytest.mark.parametrize("kind,rows,D,hq,hk,dt", SMALL)
def test_oracle_against_torch_sdpa_in_fp64(kind, rows, D, hq, hk, dt):
    case, want, _ = C.reference(kind, rows, D, hq, hk, dt)
    G = hq // hk
    k64, v64 = (C.cache_view(case, t).double() for t in (case.k_buf, case.v_buf))
    for b in range(case.B):
        n = int(case.lens[b])
        p = torch.arange(n)
        slot = torch.from_numpy(case.table)[b, p // case.block_size] * case.block_size + p % case.block_size
        k = k64[slot].permute(1, 0, 2).repeat_interleave(G, dim=0)  # [hq, n, D]
        v = v64[slot].permute(1, 0, 2).repeat_interleave(G, dim=0)
        q = case.q_buf[b, :hq * D].double().reshape(hq, 1, D)
        ref = torch.nn.functional.scaled_dot_product_attention(q[None], k[None], v[None], scale=case.scale)[0, :, 0].reshape(-1)
        np.testing.assert_allclose(want[b], ref.numpy(), rtol=1e-12, atol=1e-13)


def test_oracle_corner_rows():
    """a zero row, a row beyond the table's capacity, a row whose table leads outside the cache: +0, NaN, NaN; neighbours intact"""
    lens = (0, 5, 40, 2 * P + 3, 3)
    base, want0, _ = C.reference("paged", 5, 64, 8, 2, "fp16", lens)
    case = copy.copy(base)
    case.lens = np.array([0, 5, 16 * case.table.shape[1] + 1, 2 * P + 3, 3])
    case.table = case.table.copy()
    case.table[3, 7] = case.n_slots // 16  # the first block outside
    want, _ = C.oracle(case)
    assert (want[0] == 0).all() and not np.signbit(want[0]).any()
    assert np.isnan(want[2]).all() and np.isnan(want[3]).all()
    assert np.array_equal(want[[1, 4]], want0[[1, 4]]) and np.isfinite(want[[1, 4]]).all()
    case.table[3, 7] = -1
    assert np.isnan(C.oracle(case)[0][3]).all()


@pytest.mark.parametrize("kind,rows,D,hq,hk,dt", SMALL)
def test_fallback_against_the_oracle(kind, rows, D, hq, hk, dt):
    from squeezellm_amd.quant import DecodeAttention

    case, want, gate = C.reference(kind, rows, D, hq, hk, dt)
    att = DecodeAttention(hq, hk, D, block_size=case.block_size)
    got = att(*_module_args(case))
    assert att.last_route == "fallback" and got.dtype == case.dtype and got.shape == (case.B, hq * D)
    assert C.excess(got.double().numpy(), want, gate) <= 1.0
    # the other poison in every unaddressed slot: the same bits
    other = C.build(kind, rows, D, hq, hk, dt, 1)
    assert not torch.equal(other.k_buf.view(torch.int16), case.k_buf.view(torch.int16))
    assert torch.equal(att(*_module_args(other)).view(torch.int16), got.view(torch.int16))
    # int64 tables and lengths, block_size per call, out=
    q, k, v, bt, sl = _module_args(case)
    out = torch.full((case.B, hq * D + 3), 7.0, dtype=case.dtype)[:, :hq * D]
    att2 = DecodeAttention(hq, hk, D)
    assert att2(q, k, v, bt.long(), sl.long(), out=out, block_size=case.block_size) is out
    assert torch.equal(out.view(torch.int16), got.view(torch.int16))
    with pytest.raises(ValueError):
        att2(q, k, v, bt, sl)  # no block size anywhere


def test_fallback_corner_rows_and_nans():
    from squeezellm_amd.quant import DecodeAttention

    lens = (0, 5, 40, 2 * P + 3, 3)
    base, want0, gate = C.reference("paged", 5, 64, 8, 2, "fp16", lens)
    att = DecodeAttention(8, 2, 64, block_size=16)
    q, k, v, bt, sl = _module_args(base)
    sl[2] = 16 * bt.shape[1] + 1
    bt[3, 7] = base.n_slots // 16
    got = att(q, k, v, bt, sl).double().numpy()
    assert (got[0] == 0).all() and not np.signbit(got[0]).any()
    assert np.isnan(got[2]).all() and np.isnan(got[3]).all()
    assert C.excess(got[[1, 4]], want0[[1, 4]], gate[[1, 4]]) <= 1.0
    # one NaN in an attended k: that head group's... that kv head's query heads; one in an attended v: that column of the group
    q, k, v, bt, sl = _module_args(base)
    k, v = k.clone(), v.clone()
    k[int(bt[1, 0]) * 16 + 2, 1, 5] = float("nan")
    v[int(bt[4, 0]) * 16 + 1, 0, 9] = float("nan")
    got = att(q, k, v, bt, sl).double().numpy().reshape(5, 8, 64)
    assert np.isnan(got[1, 4:]).all() and np.isfinite(got[1, :4]).all()
    assert np.isnan(got[4, :4, 9]).all() and np.isnan(got[4]).sum() == 4
    assert np.isfinite(got[[2, 3]]).all()


def test_static_cache_helpers_address_the_same_elements():
    from squeezellm_amd.quant import kv_cache_view, static_cache_blocks, static_cache_slots

    B, H, S, D = 3, 2, 7, 4
    cache = torch.arange(B * H * S * D, dtype=torch.float32).reshape(B, H, S, D)
    view = kv_cache_view(cache, "bhsd")
    table = static_cache_blocks(B, H)
    assert table.dtype == torch.int32 and table.shape == (B, 1) and table[:, 0].tolist() == [0, H, 2 * H]
    for p in range(S):
        slots = static_cache_slots(torch.full((B,), p, dtype=torch.int32), H, S)
        walked = table[:, p // S].long() * S + p % S  # the decode attention's formula with block_size = S
        assert torch.equal(walked, slots.long())
        for b in range(B):
            assert torch.equal(view[int(walked[b])], cache[b, :, p])  # [H, D]: the same elements


def test_fuse_decode_attention_attaches_by_reference():
    from squeezellm_amd import quant

    class Attn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.q_proj = quant.QuantLinearLUT(4, 128, 256, False)
            self.k_proj = quant.QuantLinearLUT(4, 128, 128, False)
            self.v_proj = quant.QuantLinearLUT(4, 128, 128, False)
            self.head_dim = 64

    class Layer(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.self_attn, self.other = Attn(), torch.nn.Linear(4, 4)

    model = Layer()
    keys, mods, fwd = list(model.state_dict()), [n for n, _ in model.named_modules()], model.self_attn.forward
    assert quant.fuse_decode_attention(model) == 0  # no front yet
    assert quant.fuse_qkv_rope(model) == 1 and quant.fuse_decode_attention(model) == 1
    att = model.self_attn.attend_decode
    assert isinstance(att, quant.DecodeAttention) and (att.n_heads, att.n_kv_heads, att.head_dim) == (4, 2, 64)
    assert att.scale == 64 ** -0.5 and "attend_decode" in model.self_attn.__dict__
    assert list(model.state_dict()) == keys and [n for n, _ in model.named_modules()] == mods
    assert model.self_attn.forward == fwd and not hasattr(model.other, "attend_decode")
    assert list(att.state_dict()) == [] and list(att.parameters()) == []


def test_module_rejects_what_it_cannot_take():
    from squeezellm_amd.quant import DecodeAttention

    with pytest.raises(ValueError):
        DecodeAttention(6, 4, 64)
    with pytest.raises(ValueError):
        DecodeAttention(4, 2, 64, scale=float("inf"))
    case = C.build("paged", 3, 64, 8, 2, "fp16")
    att = DecodeAttention(8, 2, 64, block_size=16)
    q, k, v, bt, sl = _module_args(case)
    for bad in ((q[:, :-1], k, v, bt, sl), (q, k.float(), v, bt, sl), (q, k, v[:, :1], bt, sl), (q, k, v, bt[:2], sl), (q, k, v, bt, sl[:2]),
                (q, k, v, bt.float(), sl)):
        with pytest.raises(ValueError):
            att(*bad)


@pytest.mark.parametrize("kind,rows,D,hq,hk,dt", ALL)
def test_the_gate_fails_every_mutant_at_every_shape(kind, rows, D, hq, hk, dt):
    """the oracle itself passes with nothing to spare for a wrong one: each mutant exceeds the gate on this case's inputs"""
    case, want, gate = C.reference(kind, rows, D, hq, hk, dt)
    assert np.isfinite(want).all() and C.excess(want, want, gate) == 0.0
    rounded = torch.from_numpy(want).to(case.dtype).double().numpy()  # the best any implementation can do: inside the gate
    assert C.excess(rounded, want, gate) <= 1.0
    for mutant in C.MUTANTS:
        wrong = torch.from_numpy(C.oracle(case, mutant)[0]).to(case.dtype).double().numpy()
        assert C.excess(wrong, want, gate) > 1.0, mutant
