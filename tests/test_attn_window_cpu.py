"""The sliding-window decode attention without a GPU (include/sqllm_hip.h, sqllm_attn_decode_window_*): the cases, the oracle and
the gate of tests/attn_window_cases.py judged by three wrong oracles and by an fp32 model in the kernels' structure; the
partitions a window can touch, by brute force; quant.DecodeAttention(window=) on CPU tensors (the torch fallback);
quant.ring_block_table over a simulated growth; quant.fuse_decode_attention(window=)."""
import numpy as np
import pytest
import torch

from tests import attn_decode_cases as AC
from tests import attn_window_cases as WC

P = WC.P
SHAPES = ((64, 2, 2, "fp16"), (128, 8, 2, "bf16"), (64, 6, 2, "bf16"), (128, 2, 2, "fp16"))
GEOMS = ("paged", "padded", "bhsd")


def _excess(got, want, gate):
    return AC.excess(got, want, gate)


@pytest.mark.parametrize("L,W", WC.PAIRS)
@pytest.mark.parametrize("kind", GEOMS)
def test_the_gate_admits_the_structured_model_and_rejects_three_wrong_windows(kind, L, W):
    for D, hq, hk, dt in SHAPES:
        case, want, gate = WC.pair_reference(kind, L, W, D, hq, hk, dt)
        assert case.window == W and np.isfinite(want).all()
        worst = _excess(AC.rounded(WC.model_parts_w(case), case.dtype), want, gate)
        assert worst <= 1.0, (D, hq, hk, dt, worst)
        defined = 0
        for mutant in WC.MUTANTS_W:
            wrong, _ = WC.oracle_w(case, mutant)
            if wrong is None:
                continue
            defined += 1
            off = _excess(AC.rounded(wrong, case.dtype), want, gate)
            assert off > 1.0, (mutant, D, hq, hk, dt, off)
        assert defined >= (0 if L <= W and WC.SECOND_ROW <= W else 2)


@pytest.mark.parametrize("W", WC.LONG_WINDOWS)
def test_the_long_table(W):
    case, want, gate = WC.long_reference("paged", W, 64, 8, 2, "fp16")
    assert WC.win_parts(case.table.shape[1], case.block_size, W) == {P + 7: 3, 4 * P: 5}[W]
    firsts = [WC.lo_of(n, W) // P for n in case.lens if n > 0]
    assert len(set(firsts)) == len(firsts) == 4  # every row has its own first partition
    assert (want[4] == 0).all() and min(case.lens[case.lens > 0]) <= W
    assert _excess(AC.rounded(WC.model_parts_w(case), case.dtype), want, gate) <= 1.0
    for mutant in WC.MUTANTS_W:
        assert _excess(AC.rounded(WC.oracle_w(case, mutant)[0], case.dtype), want, gate) > 1.0, mutant


def test_windowed_leaves_the_cached_case_alone_and_poisons_what_lies_behind_the_window():
    base = AC.build("paged", 2, 64, 8, 2, "fp16", 0, (2 * P + 3, WC.SECOND_ROW))
    k0, t0 = base.k_buf.clone(), base.table.copy()
    case = WC.windowed(base, P + 100)
    assert torch.equal(base.k_buf.view(torch.int16), k0.view(torch.int16)) and np.array_equal(base.table, t0)
    lo = 2 * P + 3 - (P + 100)
    assert (case.table[0, :lo // 16] != t0[0, :lo // 16]).all() and np.array_equal(case.table[0, lo // 16:], t0[0, lo // 16:])
    assert set(case.table[0, :lo // 16]) == {1 << 30, -7} and np.array_equal(case.table[1], t0[1])
    k = AC.cache_view(case, case.k_buf)
    for p in range(2 * P + 3):
        slot = int(t0[0, p // 16]) * 16 + p % 16
        assert bool(torch.isnan(k[slot]).all()) == (p < lo), p
    # the unwindowed oracle on the windowed case: a NaN row -- whoever looks behind the window shows
    assert np.isnan(AC.oracle(case)[0][0]).all()


def test_win_parts_by_brute_force():
    for W in range(1, 3 * P + 1):
        most = 0
        for lo in range(0, 2 * P + 1):
            touched = (lo + W - 1) // P - lo // P + 1
            most = max(most, touched)
        assert most == WC.win_parts(1 << 20, 16, W), W  # never more than the formula, and attained
    assert WC.win_parts(40, 16, 100) == 2 and WC.win_parts(40, 16, 640) == 3 and WC.win_parts(40, 16, 1) == 1
    assert WC.win_parts(1 << 20, 16, WC.INT32_MAX) == (1 << 24) // P


# ---- quant.DecodeAttention(window=) on CPU tensors: the torch fallback ----

def _run_cpu(case, window):
    from squeezellm_amd.quant import DecodeAttention

    att = DecodeAttention(case.HQ, case.H, case.D, block_size=case.block_size, window=window)
    k, v = AC.cache_view(case, case.k_buf), AC.cache_view(case, case.v_buf)
    y = att(case.q_buf[:, :case.HQ * case.D], k, v, torch.from_numpy(case.table).to(torch.int32), torch.from_numpy(case.lens).to(torch.int32))
    assert att.last_route == "fallback"
    return y


@pytest.mark.parametrize("L,W", WC.PAIRS)
@pytest.mark.parametrize("kind", GEOMS)
def test_the_module_on_cpu_tensors_against_the_oracle(kind, L, W):
    case, want, gate = WC.pair_reference(kind, L, W, 64, 8, 2, "bf16")
    y = _run_cpu(case, W)
    assert y.dtype == case.dtype and _excess(y.double().numpy(), want, gate) <= 1.0


def test_the_module_on_the_long_table_and_its_corner_rows():
    case, want, gate = WC.long_reference("paged", P + 7, 64, 8, 2, "fp16")
    y = _run_cpu(case, P + 7).double().numpy()
    assert _excess(y, want, gate) <= 1.0 and (y[4] == 0).all()
    over = WC.windowed(AC.build("paged", 2, 64, 8, 2, "fp16", 0, (2 * P + 3, WC.SECOND_ROW)), 40)
    over.lens = np.array([2 * P + 3, over.table.shape[1] * 16 + 1])
    assert np.isnan(_run_cpu(over, 40).double().numpy()[1]).all()


def test_window_none_is_todays_module_and_bad_windows_are_value_errors():
    from squeezellm_amd.quant import DecodeAttention

    case, want, gate = AC.reference("paged", 3, 64, 8, 2, "fp16")
    plain = _run_cpu(case, None)
    assert _excess(plain.double().numpy(), want, gate) <= 1.0
    assert torch.equal(_run_cpu(case, 2 * P + 3).view(torch.int16), plain.view(torch.int16))  # every row inside the window
    assert DecodeAttention(8, 2, 64).window is None and DecodeAttention(8, 2, 64, window=4096).window == 4096
    for bad in (0, -1, 1.5, "4096", True, 1 << 31):
        with pytest.raises(ValueError):
            DecodeAttention(8, 2, 64, window=bad)


def test_q_len_on_a_windowed_module_is_the_expansion_under_the_window():
    from squeezellm_amd.quant import DecodeAttention, append_as_decode_rows

    base = AC.build("paged", 2, 64, 8, 2, "fp16", 0, (300, 47))
    att = DecodeAttention(8, 2, 64, block_size=16, window=50)
    k, v = AC.cache_view(base, base.k_buf), AC.cache_view(base, base.v_buf)
    table, lens = torch.from_numpy(base.table).to(torch.int32), torch.tensor([300, 47], dtype=torch.int32)
    q = torch.randn(6, 8 * 64, generator=torch.Generator().manual_seed(5)).to(torch.float16)
    q_lens = torch.tensor([3, 2], dtype=torch.int32)
    y = att(q, k, v, table, lens, q_len=3, q_lens=q_lens)
    t2, l2 = append_as_decode_rows(table, lens, 3, q_lens, 16)
    assert l2.tolist() == [298, 299, 300, 46, 47, 0]
    assert torch.equal(att(q, k, v, t2, l2).view(torch.int16), y.view(torch.int16))
    wide = DecodeAttention(8, 2, 64, block_size=16)(q, k, v, table, lens, q_len=3, q_lens=q_lens)
    assert torch.equal(wide[3:].view(torch.int16), y[3:].view(torch.int16)) and not torch.equal(wide[:3], y[:3])


# ---- the rolling buffer ----

@pytest.mark.parametrize("window,bs", [(40, 16), (64, 16), (7, 5), (1, 4), (5, 1)])
def test_ring_block_table_never_overwrites_an_attended_key(window, bs):
    from squeezellm_amd.quant import ring_block_table

    R = -(-window // bs) + 1
    n = 3 * R * bs
    table = ring_block_table(2, window, bs, n)
    assert table.dtype == torch.int32 and table.shape == (2, -(-n // bs))
    t = table.numpy()
    for b in range(2):
        assert np.array_equal(t[b], b * R + np.arange(t.shape[1]) % R)
    holds = {}  # slot -> the position written there last
    for L in range(1, n + 1):
        p = L - 1
        holds[int(t[1, p // bs]) * bs + p % bs] = p  # the front writes the new key
        for a in range(WC.lo_of(L, window), L):  # every attended key is still where the table says
            assert holds[int(t[1, a // bs]) * bs + a % bs] == a, (L, a)
    assert len(holds) <= R * bs and min(holds) >= R * bs and max(holds) < 2 * R * bs  # row 1's own R blocks
    for bad in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0)):
        with pytest.raises(ValueError):
            ring_block_table(*bad)


def test_fuse_decode_attention_passes_the_window():
    from squeezellm_amd import quant

    front = quant.QuantQKVRopeFused.__new__(quant.QuantQKVRopeFused)
    torch.nn.Module.__init__(front)
    front.__dict__.update(head_dim=64, q=type("M", (), {"outfeatures": 512})(), k=type("M", (), {"outfeatures": 128})())
    holder = torch.nn.Module()
    holder.__dict__["qkv_rope"] = front
    root = torch.nn.Sequential(holder)
    assert quant.fuse_decode_attention(root, window=4096) == 1
    att = holder.__dict__["attend_decode"]
    assert (att.n_heads, att.n_kv_heads, att.head_dim, att.window) == (8, 2, 64, 4096)
    assert quant.fuse_decode_attention(root) == 1 and holder.__dict__["attend_decode"].window is None
