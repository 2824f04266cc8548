"""Tests of the norm fronts on the GPU (sqllm_gated_norm_* / sqllm_qkv_rope_norm_* behind QuantGatedLUTFused.forward and
QuantQKVRopeFused.forward with a norm_weight): RMSNorm as a prologue of the gated and the q/k/v rotary kernels.  Reference,
tolerance and the derivation of P: tests/norm_front_cases.py (its docstring is part of this one), proved without a GPU in
tests/test_norm_front_cpu.py.  Layers, helpers and gates are those of tests/test_gpu_gated.py and tests/test_gpu_qkv_rope.py.

Shapes: the parity shape K = 1024, N = 456 (ragged last column tile); K = 32 (fewer elements than the workgroup has
threads); K = 4128 = 4096 + 32 (more than one round of the sum-of-squares pass, and no whole number of rounds -- as 1024 and
32 are none); the pass's constants are pinned from the source as text.  q/k/v: the grouped-query shape (384, 128, 128, D = 64)
and (456, 456, 132, D = 24) of the existing suite, at K = 1024 (the prologue is one function for both families: its K
classes are walked on the gated entry)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import norm_front_cases as NC
from tests import test_gpu_dequant as DQ
from tests import test_gpu_gated as TG
from tests import test_gpu_linear as TL
from tests import test_gpu_qkv_rope as TQ

gpu_test = pytest.mark.gpu
K, N = TG.K, TG.N
DTYPES = ["float16", "bfloat16"]
OTHER_KS = {32: 132, 4128: 132}  # K -> N (a partial last column tile)
_PAIRS = {}


def test_the_pass_constants_match_the_source_and_the_k_classes_are_inhabited():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "squeezellm_amd", "csrc", "sqllm_norm_front.h")).read()
    assert int(re.search(r"constexpr\s+int\s+kNormVec\s*=\s*(\d+)\s*;", src).group(1)) == NC.NORM_VEC
    assert re.search(r"constexpr\s+int\s+kNormRound\s*=\s*kWaves\s*\*\s*64\s*\*\s*kNormVec\s*;", src)
    kern = open(os.path.join(root, "squeezellm_amd", "csrc", "sqllm_kernels.h")).read()
    assert int(re.search(r"#define\s+SQLLM_WAVES\s+(\d+)", kern).group(1)) == NC.WAVES
    assert NC.NORM_ROUND == NC.WAVES * 64 * NC.NORM_VEC == 4096
    assert "for (int k = kNormVec * tid; k < K; k += kNormRound)" in src
    ks = [K, *OTHER_KS]
    assert any(k < NC.WAVES * 64 for k in ks)                              # fewer elements than threads
    assert any(k % NC.NORM_ROUND and k < NC.NORM_ROUND for k in ks)        # part of one round
    assert any(k > NC.NORM_ROUND and k % NC.NORM_ROUND for k in ks)        # more than one round, the last one partial
    assert any(k // NC.NORM_VEC < NC.WAVES * 64 and (k // NC.NORM_VEC) % 64 for k in ks)  # a wave with idle lanes in the pass


def _pair(device, bits, kind, bias, k=K):
    """(gate, up) as tests/test_gpu_gated.py: pair_layers builds them; the parity shape is that function's own (shared)"""
    from squeezellm_amd import synth

    if k == K:
        return TG.pair_layers(device, bits, kind, bias)
    key = (str(device), bits, kind, bias, k)
    if key not in _PAIRS:
        out = []
        for kd, seed in zip(TG.KINDS[kind], (31 * bits + 7 + k, 31 * bits + 1007 + k)):
            lay = synth.make_layer(k, OTHER_KS[k], bits, sparse_frac=0.0 if kd == "dense" else 0.02, topX=3 if kd == "hybrid" else 0,
                                   heavy_rows=2 if kd != "dense" else 0, bias=bias, device=device, seed=seed)
            npl = TL._npl(lay)
            out.append((lay, npl, DQ.expected(npl)[3], kd))
        _PAIRS[key] = tuple(out)
    return _PAIRS[key]


def _gated_ref(pair, x16, g16, eps, dtype):
    """(fp64 g, fp64 u, tolerance) of a gated norm front"""
    k = x16.shape[-1]
    xn = NC.xn64(NC.widen(x16).reshape(-1, k), NC.widen(g16), eps)
    gs, us = (TL._exact(npl, xn, kd) for _, npl, _, kd in pair)
    Ag, Au = (NC.abs_sum(mag, xn) for _, _, mag, _ in pair)
    for (_, npl, _, _), A in zip(pair, (Ag, Au)):  # every partial sum is in range: no non-finite result is admissible
        assert (A + (0 if npl.get("bias") is None else np.abs(npl["bias"])) < TG.LIMIT).all()
    return gs, us, NC.gated_gate(gs, us, Ag, Au, dtype, NC.P_of(k))


def _inside(y, exact, tol, what="", where=None):
    got = y.float().cpu().numpy().astype(np.float64).reshape(exact.shape)
    sel = np.ones(exact.shape, bool) if where is None else where
    assert np.isfinite(got[sel]).all(), f"{what}: {(~np.isfinite(got[sel])).sum()} non-finite outputs"
    err, t = np.abs(got - exact)[sel], tol[sel]
    print(f"{what}: worst error / tolerance {float((err / t).max()) if err.size else 0.0:.3g}")
    assert (err <= t).all(), f"{what}: {(err > t).sum()} of {err.size} outputs outside the gate; worst {float((err / t).max()):.3g} x"


def _to(gpu, t):
    return t.to(gpu)


# ---- 1. parity ----

def _gated_parity(gpu, bits, kind, rows, bias, dtype, k=K):
    import torch

    pair = _pair(gpu, bits, kind, bias, k)
    mod = TG._module(pair)
    x16, g16 = NC.activations(rows, k, dtype)
    gs, us, tol = _gated_ref(pair, x16, g16, NC.EPS, dtype)
    x, w = _to(gpu, x16), _to(gpu, g16)
    for rep in range(2):  # the second call runs on the workspace the first one left behind
        y = mod(x if rows > 1 else x.reshape(1, 1, k), w, NC.EPS)
        assert y.dtype == getattr(torch, dtype) and y.shape[-1] == pair[0][1]["N"] and mod.last_route == "gated_norm"
        _inside(y, TG._silu(gs) * us, tol, f"w{bits} {kind} K={k} rows={rows} bias={bias} {dtype} call {rep}")
    TG._workspaces_clean(mod)


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("rows", [1, 2, 5, 8, 19])
@pytest.mark.parametrize("kind", ["dense", "spmv", "hybrid"])
@pytest.mark.parametrize("bits", [3, 4])
def test_gated_norm_matches_oracle_and_cleans_up(gpu, bits, kind, rows, bias, dtype):
    _gated_parity(gpu, bits, kind, rows, bias, dtype)


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("kind", ["dense", "hybrid"])
@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("k", sorted(OTHER_KS))
def test_gated_norm_at_the_other_k_classes(gpu, k, bits, kind, rows, dtype):
    _gated_parity(gpu, bits, kind, rows, True, dtype, k)


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
def test_gated_norm_c_abi_with_unfolded_full_rows_and_an_unaligned_vec(gpu, dtype):
    """the descriptor filled in by hand from the layers' raw operands (CSR and top-X rows passed separately: the dense role's
    folded loop and the top-X slab role), a workspace zero-filled once that serves norm and plain launches alternately, and a
    vec that starts 2 bytes past a 16-byte boundary (the pass's narrow loads)"""
    import torch

    from squeezellm_amd import _lib, quant_cuda

    rows = 5
    pair = _pair(gpu, 3, "hybrid", True)
    x16, g16 = NC.activations(rows, K, dtype)
    gs, us, tol = _gated_ref(pair, x16, g16, NC.EPS, dtype)
    buf = torch.zeros(rows * K + 8, dtype=x16.dtype, device=gpu)
    x = buf[1:1 + rows * K].view(rows, K)
    x.copy_(x16)
    assert x.data_ptr() % 16 == 2
    w = _to(gpu, g16)
    g = _lib.SqllmGated()
    for op, (lay, _, _, _) in zip((g.gate, g.up), pair):
        op.bits, op.batch, op.K, op.N = lay["bits"], rows, K, N
        op.vec, op.qweight, op.lookup_table = x.data_ptr(), lay["qweight"].data_ptr(), lay["lookup_table"].data_ptr()
        op.rows, op.cols, op.vals, op.nnz = lay["rows"].data_ptr(), lay["cols"].data_ptr(), lay["vals"].data_ptr(), lay["vals"].numel()
        op.full_rows, op.full_row_indices, op.topX = lay["full_rows"].data_ptr(), lay["full_row_indices"].data_ptr(), lay["full_rows"].shape[1]
    g.bias_gate, g.bias_up = pair[0][0]["bias"].data_ptr(), pair[1][0]["bias"].data_ptr()
    out = torch.empty((rows, N), dtype=x.dtype, device=gpu)
    need = _lib.gated_workspace_bytes(N, rows)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=gpu)
    ws[need:] = 0xA5  # a guard behind the workspace
    g.out, g.workspace, g.act = out.data_ptr(), ws.data_ptr(), _lib.ACT_SILU
    nm = _lib.SqllmRmsNorm(weight=w.data_ptr(), eps=NC.EPS)
    lib, stream = _lib.load(), quant_cuda._raw_stream(x.get_device())
    sfx = "f16" if dtype == "float16" else "bf16"
    plain = None
    for rep in range(2):
        out.zero_()
        assert getattr(lib, "sqllm_gated_norm_" + sfx)(ctypes.byref(g), ctypes.byref(nm), stream) == 0
        torch.cuda.synchronize()
        _inside(out, TG._silu(gs) * us, tol, f"C ABI {dtype} call {rep}")
        assert int(ws[:need].count_nonzero()) == 0 and bool((ws[need:] == 0xA5).all())
        assert getattr(lib, "sqllm_gated_" + sfx)(ctypes.byref(g), stream) == 0  # the parent entry on the same workspace
        torch.cuda.synchronize()
        assert int(ws[:need].count_nonzero()) == 0
        plain = out.clone() if plain is None else plain
        assert torch.equal(out.view(torch.int16), plain.view(torch.int16))


def _qkv_ref(members, x16, g16, eps, pos, cos, sin, D, layout, dtype):
    xn = NC.xn64(NC.widen(x16).reshape(-1, TQ.K), NC.widen(g16), eps)
    P = NC.P_of(TQ.K)
    out = []
    for i, (_, npl, mag, kd) in enumerate(members):
        s, A = TL._exact(npl, xn, kd), NC.abs_sum(mag, xn)
        assert (A + np.abs(npl["bias"]) < TG.LIMIT).all()
        out.append(NC.rotated_gate(s, A, pos, cos, sin, D, layout, dtype, P) if i < 2 else (s, NC.plain_gate(s, A, dtype, P)))
    return out


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 2, 5, 8, 19])
@pytest.mark.parametrize("kind", ["dense", "hybrid"])
@pytest.mark.parametrize("bits", [3, 4])
def test_qkv_rope_norm_matches_oracle_and_cleans_up(gpu, bits, kind, rows, dtype):
    x16, g16 = NC.activations(rows, TQ.K, dtype)
    x, w = _to(gpu, x16), _to(gpu, g16)
    pos = TQ._positions(rows)
    for shape, layout in (("d64", "half"), ("d24", "half"), ("d64", "interleaved")):
        D = TQ.SHAPES[shape][3]
        members = TQ._members(gpu, bits, kind, shape)
        cos, sin = TQ._tables(D)
        ref = _qkv_ref(members, x16, g16, NC.EPS, pos, cos, sin, D, layout, dtype)
        mod = TQ._module(members, D, layout)
        tp, tc, ts = TQ._dev(gpu, pos, cos, sin)
        for rep in range(2):
            outs = mod(x if rows > 1 else x.reshape(1, 1, TQ.K), tp, tc, ts, norm_weight=w, norm_eps=NC.EPS)
            assert mod.last_route == "qkv_rope_norm" and [o.shape[-1] for o in outs] == list(TQ.SHAPES[shape][:3])
            for name, o, (exact, tol) in zip("qkv", outs, ref):
                _inside(o, exact, tol, f"w{bits} {kind} {shape} {layout} rows={rows} {dtype} call {rep} {name}")
        TQ._clean(mod)


# ---- 2. bit-exact identities ----

def _exact_inputs(rows, k, dtype, seed):
    """|x[b, k]| = 2^b with random signs, g[k] in {0.5, 1, 2}, eps = 0: ms = 4^b, r = 2^-b and xn = +-g[k] are exact in every
    summation order and xn is representable in 16 bits (tests/test_norm_front_cpu.py checks the arithmetic)"""
    import torch

    rng = np.random.default_rng(seed)
    x = (2.0 ** np.arange(rows))[:, None] * rng.choice([-1.0, 1.0], (rows, k))
    g = rng.choice([0.5, 1.0, 2.0], k)
    xn = np.sign(x) * g[None, :]
    td = getattr(torch, dtype)
    t = lambda a: torch.from_numpy(a).to(td)  # noqa: E731
    assert all((NC.widen(t(a)) == a).all() for a in (x, g, xn))
    return t(x), t(g), t(xn)


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5, 8])
@pytest.mark.parametrize("bits", [3, 4])
def test_norm_entries_equal_the_parent_entries_fed_xn_bit_for_bit(gpu, bits, rows, dtype):
    import torch

    for k in (K, 4128):
        x16, g16, xn16 = _exact_inputs(rows, k, dtype, 100 * bits + rows + k)
        x, w, xn = _to(gpu, x16), _to(gpu, g16), _to(gpu, xn16)
        mod = TG._module(_pair(gpu, bits, "hybrid", True, k))
        want = mod(xn).clone()
        assert mod.last_route == "gated"
        got = mod(x, w, 0.0)
        assert mod.last_route == "gated_norm" and torch.isfinite(want.float()).all()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), f"gated K={k}: {int((got != want).sum())} outputs differ"
        TG._workspaces_clean(mod)
    x16, g16, xn16 = _exact_inputs(rows, TQ.K, dtype, 7 * bits + rows)
    x, w, xn = _to(gpu, x16), _to(gpu, g16), _to(gpu, xn16)
    pos = TQ._positions(rows)
    for shape in ("d64", "d24"):
        D = TQ.SHAPES[shape][3]
        mod = TQ._module(TQ._members(gpu, bits, "hybrid", shape), D, "half")
        tp, tc, ts = TQ._dev(gpu, pos, *TQ._tables(D))
        want = [o.clone() for o in mod(xn, tp, tc, ts)]
        got = mod(x, tp, tc, ts, norm_weight=w, norm_eps=0.0)
        for name, a, b in zip("qkv", got, want):
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{shape} {name}: {int((a != b).sum())} outputs differ"
        TQ._clean(mod)


# ---- 3. bit reproducibility ----

@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("bits", [3, 4])
def test_five_identical_calls_are_bit_identical(gpu, bits, rows, dtype):
    import torch

    x16, g16 = NC.activations(rows, K, dtype)
    x, w = _to(gpu, x16), _to(gpu, g16)
    mod = TG._module(_pair(gpu, bits, "hybrid", True))
    ys = torch.stack([mod(x, w, NC.EPS).view(torch.int16) for _ in range(5)])
    pos = TQ._positions(rows)
    qmod = TQ._module(TQ._members(gpu, bits, "hybrid", "d24"), 24, "half")
    tp, tc, ts = TQ._dev(gpu, pos, *TQ._tables(24))
    qs = [torch.cat([o.view(torch.int16) for o in qmod(x, tp, tc, ts, norm_weight=w, norm_eps=NC.EPS)], dim=-1) for _ in range(5)]
    torch.cuda.synchronize()
    assert bool((ys == ys[0]).all()) and all(torch.equal(q, qs[0]) for q in qs)


@gpu_test
def test_twenty_calls_of_the_long_row_case_are_identical(gpu):
    """the long-row hybrid case of tests/test_gpu_gated.py ([3-5-float16]: CSR rows of more than 256 non-zeros in both members)"""
    import torch

    x16, g16 = NC.activations(5, K, "float16")
    x, w = _to(gpu, x16), _to(gpu, g16)
    mod = TG._module(_pair(gpu, 3, "hybrid", True))
    ys = torch.stack([mod(x, w, NC.EPS).view(torch.int16) for _ in range(20)])
    torch.cuda.synchronize()
    assert bool((ys == ys[0]).all())


# ---- 4. non-finite values and the range rule ----

@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("poison", ["nan", "+inf", "-inf"])
@pytest.mark.parametrize("bits", [3, 4])
def test_a_non_finite_activation_poisons_its_row_and_no_other(gpu, bits, poison, dtype):
    """NaN in row 1: the row is NaN.  +-inf in row 1: the sum of squares is infinite, r = 0, xn is NaN at that k (inf * 0) and 0
    elsewhere; every output of the row has a dense term at that k, so the row is NaN -- exactly where the formula says.  The
    other rows are inside the gate."""
    import torch

    rows = 5
    pair = _pair(gpu, bits, "hybrid", True)
    x16, g16 = NC.activations(rows, K, dtype)
    clean = torch.ones(rows, dtype=torch.bool)
    clean[1] = False
    gs, us, tol = _gated_ref(pair, torch.where(clean[:, None], x16, torch.ones_like(x16)), g16, NC.EPS, dtype)
    x16 = x16.clone()
    x16[1, K // 2 + 3] = {"nan": float("nan"), "+inf": float("inf"), "-inf": -float("inf")}[poison]
    mod = TG._module(pair)
    sel = np.repeat(clean.numpy()[:, None], N, axis=1)
    for rep in range(2):  # (the flags of the first call must not linger)
        y = mod(_to(gpu, x16), _to(gpu, g16), NC.EPS)
        assert torch.isnan(y[1].float()).all()
        _inside(y, TG._silu(gs) * us, tol, f"{poison} call {rep}", where=sel)
    TG._workspaces_clean(mod)
    # q/k/v: the same row, all three outputs
    pos = TQ._positions(rows)
    qmod = TQ._module(TQ._members(gpu, bits, "hybrid", "d24"), 24, "half")
    tp, tc, ts = TQ._dev(gpu, pos, *TQ._tables(24))
    outs = qmod(_to(gpu, x16), tp, tc, ts, norm_weight=_to(gpu, g16), norm_eps=NC.EPS)
    for o in outs:
        assert torch.isnan(o[1].float()).all() and torch.isfinite(o[[0, 2, 3, 4]].float()).all()
    TQ._clean(qmod)


@gpu_test
@pytest.mark.parametrize("bits", [3, 4])
def test_a_bf16_row_whose_squares_overflow_fp32(gpu, bits):
    """|x| = 2^63 on a whole row: every square is 2^126, finite; their sum passes FLT_MAX in every summation order, so r = 0 and
    xn = 0 (x is finite): the row's sums are the biases -- never a finite wrong number; with one infinite element, NaN."""
    import torch

    rows = 3
    pair = _pair(gpu, bits, "hybrid", True)
    x16, g16 = NC.activations(rows, K, "bfloat16")
    x16 = x16.clone()
    x16[1] = torch.where(torch.arange(K) % 3 == 0, -1.0, 1.0).to(torch.bfloat16) * 2.0 ** 63
    assert torch.isfinite(x16.float() ** 2).all() and float((x16[1].float() ** 2).sum()) == float("inf")
    ref_x = x16.clone()
    ref_x[1] = 0  # what the formula gives: xn[1] = x * g * 0 = 0
    gs, us, tol = _gated_ref(pair, ref_x, g16, NC.EPS, "bfloat16")
    # (row 1 of the reference input: 0 * g / sqrt(0 + eps) = 0 as well)
    mod = TG._module(pair)
    y = mod(_to(gpu, x16), _to(gpu, g16), NC.EPS)
    _inside(y, TG._silu(gs) * us, tol, "overflowing row")
    bias = [npl["bias"].astype(np.float64) for _, npl, _, _ in pair]
    assert np.array_equal(gs[1], bias[0]) and np.array_equal(us[1], bias[1])
    x16[1, 5] = float("inf")
    y = mod(_to(gpu, x16), _to(gpu, g16), NC.EPS)
    assert torch.isnan(y[1].float()).all() and torch.isfinite(y[[0, 2]].float()).all()
    TG._workspaces_clean(mod)


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5])
def test_the_range_rule_sees_the_normalised_sums(gpu, rows, dtype):
    """Weights that are one constant per column (the construction of tests/test_gpu_gated.py's out-of-range case), eps = 0.
    (a) x = 1, g = 2^14: r = 1, xn = 2^14, the gate's sum is 2^24 c -- beyond the range AFTER normalisation: +inf (silu: +inf) or
        -inf (silu: NaN), for both types, never the finite 2^15 a clamp would give.
    (b) x = 2^14, g = 1: r = 2^-14, xn = 1, the sums are 1024 c -- the UN-normalised sums would be 2^24 c, far beyond the range,
        but the normalised ones are not: every column comes out finite and inside the gate.  Scaling the finished sum by r
        instead of the loaded element fails (b): the contributions would have overflowed before the scaling."""
    import torch

    from squeezellm_amd import synth

    n = 64
    lay_g = synth.make_layer(K, n, 4, device=gpu, seed=5)
    lay_u = synth.make_layer(K, n, 4, device=gpu, seed=6)
    consts = np.repeat(np.array([2.0 ** -10, 1.0, -1.0, 1.0 / 16], np.float32), 16)  # 16 columns each
    lay_g["lookup_table"] = torch.from_numpy(np.repeat(consts[:, None], 16, axis=1).copy()).to(gpu)  # every index decodes to it
    lay_u["lookup_table"] = torch.full((n, 16), 2.0 ** -33, device=gpu)
    mod = TG._module(((lay_g, None, None, "dense"), (lay_u, None, None, "dense")))
    td = getattr(torch, dtype)
    one, big = torch.full((rows, K), 1.0, device=gpu, dtype=td), torch.full((rows, K), 2.0 ** 14, device=gpu, dtype=td)
    w_big, w_one = torch.full((K,), 2.0 ** 14, device=gpu, dtype=td), torch.ones(K, device=gpu, dtype=td)
    c = np.tile(consts.astype(np.float64), (rows, 1))
    for rep in range(2):
        # (a)
        y = mod(one, w_big, 0.0).float().cpu().numpy().astype(np.float64)
        g, u = c * K * 2.0 ** 14, np.full((rows, n), 2.0 ** -33 * K * 2.0 ** 14)
        exact = TG._silu(g) * u
        assert exact[0, 16] == 2.0 ** 15 < 65504
        ok = np.abs(y - exact) <= TG._gate(g, u, TG.EPS[dtype])
        assert ok[:, 0:16].all() and np.isposinf(y[:, 16:32]).all() and np.isnan(y[:, 32:48]).all() and (~np.isfinite(y) | ok).all()
        # (b)
        y = mod(big, w_one, 0.0).float().cpu().numpy().astype(np.float64)
        g, u = c * K, np.full((rows, n), 2.0 ** -33 * K)
        assert np.abs(g).max() == 1024 < TG.LIMIT < 2.0 ** 24
        assert np.isfinite(y).all() and (np.abs(y - TG._silu(g) * u) <= TG._gate(g, u, TG.EPS[dtype])).all()  # (xn is exact here: the parent's gate)
    TG._workspaces_clean(mod)


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [3, 8])
@pytest.mark.parametrize("kind", ["dense", "hybrid"])
@pytest.mark.parametrize("bits", [3, 4])
def test_non_finite_activations_where_the_clamped_lanes_run(gpu, bits, kind, rows, dtype):
    """K = 544, N = 132 of tests/nonfinite_cases.py (dead slots at the end of every slice, a partial last column tile, a K of
    which the pass's last wave holds a part), class V: +inf at K - 1 of row 0, -inf at k = 0 of the last row, NaN at K - 32 of a
    middle row.  With the norm in front each of the three rows is NaN throughout (r = 0 or NaN) and every other row is finite and
    inside the gate: what the clamped lanes re-read never reaches a sum."""
    import torch

    from tests import helpers as H
    from tests import nonfinite_cases as NF

    c = NF.linear_case(bits, kind, rows, "V", NF.to_fp16 if dtype == "float16" else NF.to_bf16)
    Kn, Nn = NF.LINEAR_SHAPE
    gate = H.make_case(bits, Kn, Nn, seed=900 + bits)
    bias_g = np.random.default_rng(901 + bits).normal(0, NF.LINEAR_SCALE, Nn).astype(np.float32)
    lay_g = dict(H.to_torch(gate, gpu), bias=torch.from_numpy(bias_g.copy()).to(gpu))
    lay_u = dict(H.to_torch(NF.writable(c["case"]), gpu), bias=torch.from_numpy(c["bias"].copy()).to(gpu))
    npl_g, npl_u = dict(gate, bias=bias_g), dict(c["case"], bias=c["bias"])
    pair = ((lay_g, npl_g, DQ.expected(npl_g)[3], "dense"), (lay_u, npl_u, DQ.expected(npl_u)[3], kind))
    x16 = torch.from_numpy(c["x16"].copy()).to(getattr(torch, dtype)).reshape(rows, Kn)
    bad = ~torch.isfinite(x16.float()).all(dim=1)
    assert int(bad.sum()) == 3 and (rows == 3 or int((~bad).sum()) == rows - 3)
    g16 = NC.activations(rows, Kn, dtype)[1]
    gs, us, tol = _gated_ref(pair, torch.where(bad[:, None], torch.ones_like(x16), x16), g16, NC.EPS, dtype)
    mod = TG._module(pair)
    sel = np.repeat((~bad).numpy()[:, None], Nn, axis=1)
    for rep in range(2):
        y = mod(_to(gpu, x16), _to(gpu, g16), NC.EPS).reshape(rows, Nn)
        assert torch.isnan(y[bad.to(y.device)].float()).all()
        if sel.any():
            _inside(y, TG._silu(gs) * us, tol, f"call {rep}", where=sel)
    TG._workspaces_clean(mod)


# ---- 5. module level ----

@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
def test_module_surface_routes_and_errors(gpu, dtype):
    import torch

    rows = 5
    pair = _pair(gpu, 4, "hybrid", True)
    x16, g16 = NC.activations(rows, K, dtype)
    x, w = _to(gpu, x16), _to(gpu, g16)
    gs, us, tol = _gated_ref(pair, x16, g16, NC.EPS, dtype)
    exact = TG._silu(gs) * us
    mod, parent = TG._module(pair, fused_members=True), TG._module(pair, fused_members=True)
    # norm_weight=None: the parent call, bit for bit, before and after a norm call on the same workspace
    want = parent(x)
    a = mod(x, None)
    assert mod.last_route == "gated" and torch.equal(a.view(torch.int16), want.view(torch.int16))
    mod(x, w, NC.EPS)
    assert mod.last_route == "gated_norm"
    assert torch.equal(mod(x).view(torch.int16), want.view(torch.int16)) and mod.last_route == "gated"
    # the dense route: fp32 from end to end, torch's fp32 GEMM (K additions per sum: the allowance of a sum grows by K 2^-24 A)
    mod.gate.dense_min_rows = 4
    y = mod(x, w, NC.EPS)
    assert mod.last_route == "dense" and y.dtype == x.dtype
    xn = NC.xn64(NC.widen(x16), NC.widen(g16), NC.EPS)
    Ag, Au = (NC.abs_sum(mag, xn) for _, _, mag, _ in pair)
    _inside(y, exact, NC.gated_gate(gs, us, Ag, Au, dtype, NC.P_of(K) + K), "dense route")
    y3 = mod(x[:3].contiguous(), w, NC.EPS)
    assert mod.last_route == "gated_norm"
    _inside(y3, exact[:3], tol[:3], "three rows stay on the kernel")
    mod.gate.dense_min_rows = None
    # the fallback: fp32 activations with an fp32 weight, the operator path's sums (fp32 atomics: the project's slack once more)
    yf = mod(x.float(), w.float(), NC.EPS)
    assert mod.last_route == "fallback" and yf.dtype == torch.float32
    _inside(yf, exact, NC.gated_gate(gs, us, Ag, Au, dtype, NC.P_of(K) + K) + tol, "fallback")
    # errors
    for bad in (w.float(), w[:-1], w.cpu(), w.reshape(1, K)):
        with pytest.raises(ValueError):
            mod(x, bad, NC.EPS)
    with pytest.raises(ValueError):
        mod(x, w, -1.0)
    qmod = TQ._module(TQ._members(gpu, 4, "hybrid", "d64"), 64, "half")
    tp, tc, ts = TQ._dev(gpu, TQ._positions(rows), *TQ._tables(64))
    want = [o.clone() for o in qmod(x, tp, tc, ts)]
    assert qmod.last_route == "qkv_rope"
    qmod(x, tp, tc, ts, norm_weight=w)
    assert qmod.last_route == "qkv_rope_norm"
    again = qmod(x, tp, tc, ts, norm_weight=None)
    assert qmod.last_route == "qkv_rope" and all(torch.equal(p.view(torch.int16), q.view(torch.int16)) for p, q in zip(again, want))
    ref = _qkv_ref(TQ._members(gpu, 4, "hybrid", "d64"), x16, g16, NC.EPS, TQ._positions(rows), *TQ._tables(64), 64, "half", dtype)
    qmod.q.dense_min_rows = 4
    outs = qmod(x, tp, tc, ts, norm_weight=w, norm_eps=NC.EPS)
    assert qmod.last_route == "dense"
    for name, o, (e, t), (_, _, mag, _) in zip("qkv", outs, ref, TQ._members(gpu, 4, "hybrid", "d64")):
        _inside(o, e, t + 2 * K * NC.U * NC.abs_sum(mag, xn).max(), f"dense route {name}")
    qmod.q.dense_min_rows = None
    for bad in (w.float(), w[:-1]):
        with pytest.raises(ValueError):
            qmod(x, tp, tc, ts, norm_weight=bad)


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
def test_captured_norm_forwards_are_one_kernel_node_and_follow_x(gpu, dtype):
    import torch

    hip = ctypes.CDLL("libamdhip64.so")

    def node_types(g):
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

    x16, g16 = NC.activations(1, K, dtype)
    x2_16 = NC.activations(1, K, dtype, seed=9)[0]
    x, w = _to(gpu, x16).reshape(1, 1, K).clone(), _to(gpu, g16)
    gmod = TG._module(_pair(gpu, 4, "hybrid", True), fused_members=True)
    qmod = TQ._module(TQ._members(gpu, 4, "hybrid", "d64"), 64, "half", fused_members=True)
    tp, tc, ts = TQ._dev(gpu, TQ._positions(1), *TQ._tables(64))
    for run in (lambda: [gmod(x, w, NC.EPS)], lambda: list(qmod(x, tp, tc, ts, norm_weight=w, norm_eps=NC.EPS))):
        x.copy_(_to(gpu, x16).reshape(1, 1, K))
        side = torch.cuda.Stream(gpu)
        side.wait_stream(torch.cuda.current_stream(gpu))
        with torch.cuda.stream(side), torch.no_grad():
            want1 = [o.clone() for o in run()]
            x.copy_(_to(gpu, x2_16).reshape(1, 1, K))
            want2 = [o.clone() for o in run()]
            x.copy_(_to(gpu, x16).reshape(1, 1, K))
        torch.cuda.current_stream(gpu).wait_stream(side)
        torch.cuda.synchronize()
        assert not all(torch.equal(a, b) for a, b in zip(want1, want2))
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g), torch.no_grad():
            outs = run()
        assert node_types(g) == [0]  # hipGraphNodeTypeKernel: the norm front's kernel and nothing else
        g.instantiate()
        for src, want in ((x16, want1), (x2_16, want2), (x16, want1)):
            x.copy_(_to(gpu, src).reshape(1, 1, K))  # updated in place: the replay follows it
            g.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(o.view(torch.int16), v.view(torch.int16)) for o, v in zip(outs, want))
    TG._workspaces_clean(gmod)
    TQ._clean(qmod)


@gpu_test
def test_fuse_norm_fronts_on_a_toy_decoder_layer(gpu):
    import torch
    import torch.nn as nn

    from squeezellm_amd import quant, synth

    H_, I_, D = 256, 224, 32
    dtype = "float16"

    class RMSNorm(nn.Module):  # as the checkpoints' modules spell it
        def __init__(self, seed, eps):
            super().__init__()
            gen = torch.Generator().manual_seed(seed)
            self.weight = nn.Parameter((1 + 0.25 * torch.randn(H_, generator=gen)).half().to(gpu), requires_grad=False)
            self.variance_epsilon = eps

        def forward(self, h):
            v = h.float().pow(2).mean(-1, keepdim=True)
            return self.weight * (h.float() * torch.rsqrt(v + self.variance_epsilon)).to(h.dtype)

    def lay(k, n, seed, sparse):
        return synth.make_layer(k, n, 4, sparse_frac=0.02 if sparse else 0.0, topX=3 if sparse else 0, heavy_rows=2 if sparse else 0,
                                bias=True, device=gpu, seed=seed)

    class Attn(nn.Module):
        def __init__(self):
            super().__init__()
            self.lays = [lay(H_, n, 500 + i, i > 0) for i, n in enumerate((256, 64, 64))]
            self.q_proj, self.k_proj, self.v_proj = (quant.QuantLinearLUT.from_operands(l) for l in self.lays)
            self.head_dim = D

    class MLP(nn.Module):
        def __init__(self):
            super().__init__()
            self.lays = [lay(H_, I_, 600 + i, True) for i in range(2)]
            self.gate_proj, self.up_proj = (quant.QuantLinearLUT.from_operands(l) for l in self.lays)
            self.down_proj = quant.QuantLinearLUT.from_operands(synth.make_layer(I_, H_, 4, device=gpu, seed=650))
            self.act_fn = nn.SiLU()

        def forward(self, h):
            return self.down_proj(self.act_fn(self.gate_proj(h)) * self.up_proj(h))

    class Layer(nn.Module):
        def __init__(self):
            super().__init__()
            self.input_layernorm, self.post_attention_layernorm = RMSNorm(1, 1e-5), RMSNorm(2, 1e-6)
            self.self_attn, self.mlp = Attn(), MLP()

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            self.layers = nn.ModuleList([Layer()])
            self.norm = nn.LayerNorm(H_)  # (has a bias: not an RMSNorm, and next to nothing fused)

    toy = Toy()
    quant.fuse_quant_lut(toy)
    assert quant.fuse_norm_fronts(toy) == 0  # nothing fused behind the norms yet
    assert quant.fuse_gated_mlps(toy) == 1 and quant.fuse_qkv_rope(toy) == 1
    keys, n_modules = list(toy.state_dict().keys()), len(list(toy.modules()))
    layer = toy.layers[0]
    rows = 5
    x16 = NC.activations(rows, H_, dtype)[0]
    x = _to(gpu, x16)
    mlp_before = layer.mlp(layer.post_attention_layernorm(x))
    assert quant.fuse_norm_fronts(toy) == 2
    assert list(toy.state_dict().keys()) == keys and len(list(toy.modules())) == n_modules
    assert torch.equal(layer.mlp(layer.post_attention_layernorm(x)), mlp_before)  # every existing forward is what it was
    for child, norm in ((layer.self_attn, layer.input_layernorm), (layer.mlp, layer.post_attention_layernorm)):
        fw, fe = child.__dict__["front_norm"]
        assert fw is norm.weight and fe == norm.variance_epsilon  # by reference
    assert "forward_normed" not in layer.self_attn.__dict__
    # the MLP front against fp64, and forward_normed = the unchanged down projection of exactly that
    wn, en = layer.mlp.front_norm
    pair = tuple((l, TL._npl(l), DQ.expected(TL._npl(l))[3], "hybrid") for l in layer.mlp.lays)
    gs, us, tol = _gated_ref(pair, x16, wn.detach().cpu(), en, dtype)
    front = layer.mlp.gated(x, wn, en)
    assert layer.mlp.gated.last_route == "gated_norm"
    _inside(front, TG._silu(gs) * us, tol, "toy MLP front")
    assert torch.equal(layer.mlp.forward_normed(x), layer.mlp.down_proj(front))
    res = _to(gpu, NC.activations(rows, H_, dtype, seed=3)[0])
    assert torch.equal(layer.mlp.forward_normed_residual(x, res), layer.mlp.down_proj(front, residual=res))
    # the attention front against fp64
    wa, ea = layer.self_attn.front_norm
    pos = TQ._positions(rows)
    cos, sin = TQ._tables(D)
    tp, tc, ts = TQ._dev(gpu, pos, cos, sin)
    outs = layer.self_attn.qkv_rope(x, tp, tc, ts, norm_weight=wa, norm_eps=ea)
    assert layer.self_attn.qkv_rope.last_route == "qkv_rope_norm"
    xn = NC.xn64(NC.widen(x16), NC.widen(wa), ea)
    P = NC.P_of(H_)
    for i, (o, l) in enumerate(zip(outs, layer.self_attn.lays)):
        npl = TL._npl(l)
        mag = DQ.expected(npl)[3]
        s, A = TL._exact(npl, xn, "hybrid" if i else "dense"), NC.abs_sum(mag, xn)
        exact, t = NC.rotated_gate(s, A, pos, cos, sin, D, "half", dtype, P) if i < 2 else (s, NC.plain_gate(s, A, dtype, P))
        _inside(o, exact, t, f"toy attention front {'qkv'[i]}")
    assert quant.fuse_norm_fronts(nn.Linear(4, 4)) == 0
