"""The norm fronts' arithmetic and their tests' tolerance, without a GPU (tests/norm_front_cases.py holds both): a numpy fp32
emulation of the prologue -- the header's formulas with every operation rounded once, the sum of squares in three orders
(sequential, pairwise, and the kernel's own: 512 partial sums, then the tree) -- goes through the fp64 oracle sums and the
gated / linear formulas and must stay inside the gate of tests/test_gpu_norm_front.py; five mutants must fall outside it on
most of the outputs where they differ at all.  The inputs are chosen so that each mutant shows: rows scaled by distinct
factors, one row so small that eps moves its r by tens of percent, biased layers, four channels of one row around 200."""
import numpy as np
import pytest

from tests import norm_front_cases as NC
from tests import test_gpu_gated as TG
from tests import test_gpu_linear as TL

ROWS = 5


def _setup(bits, dtype):
    pair = TG.pair_layers("cpu", bits, "hybrid", True)
    x16, g16 = NC.activations(ROWS, TG.K, dtype)
    return pair, NC.widen(x16), NC.widen(g16)


def _sums(pair, xn):
    return [TL._exact(npl, xn, k) for _, npl, _, k in pair]


def _out(gs, us, dtype):
    g32, u32 = gs.astype(np.float32), us.astype(np.float32)
    with np.errstate(over="ignore"):
        return TG._round_to((g32 / (np.float32(1) + np.exp(-g32))) * u32, dtype)


def test_the_inputs_show_what_they_are_meant_to_show():
    _, x, g = _setup(4, "float16")
    r, r0 = NC.r64(x, NC.EPS)[:, 0], NC.r64(x, 0.0)[:, 0]
    assert len(set(np.round(np.log2(r), 1))) == ROWS                       # distinct factors
    assert 0.5 < r[0] / r0[0] <= 1.0 and abs(r[0] / r0[0] - 1) < 1e-5      # eps is nothing to an ordinary row ...
    assert r[NC.SMALL_ROW] / r0[NC.SMALL_ROW] < 0.9                        # ... and moves the small row's r by more than 10 %
    assert (np.abs(x[NC.MASSIVE_ROW]) > 190).sum() == 4 and np.abs(x).max() < 230
    assert (np.abs(r - 1) > 0.5).sum() >= 3                                # r is far from 1 on most rows
    assert np.abs(g - 1).mean() > 0.1
    assert NC.P_of(1024) == NC.P_of(4096) == 17 and NC.P_of(4128) == 21


def test_the_three_orders_differ_and_the_kernel_order_is_what_the_header_says():
    _, x, _ = _setup(4, "bfloat16")
    x32 = x.astype(np.float32)
    s = {k: f(x32) for k, f in NC.ORDERS.items()}
    exact = (x * x).sum(axis=1)
    depth = {"sequential": x.shape[1], "pairwise": 10, "kernel": 22}  # rounded additions a square passes through at the most
    for k, v in s.items():
        assert v.dtype == np.float32 and (np.abs(v - exact) <= depth[k] * NC.U * exact).all(), k
    assert any((s["kernel"] != s[k]).any() for k in ("sequential", "pairwise"))  # the orders are not the same arithmetic
    # more than one round, and a K that is no whole number of rounds
    xl = np.random.default_rng(5).standard_normal((2, NC.NORM_ROUND + 32)).astype(np.float16).astype(np.float32)
    el = (xl.astype(np.float64) ** 2).sum(axis=1)
    assert (np.abs(NC.sumsq_kernel_order(xl) - el) <= 30 * NC.U * el).all()


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("bits", [3, 4])
def test_gate_admits_the_fp32_prologue_and_rejects_the_mutants(bits, dtype):
    pair, x, g = _setup(bits, dtype)
    P = NC.P_of(TG.K)
    xn = NC.xn64(x, g, NC.EPS)
    assert np.abs(xn[NC.MASSIVE_ROW]).max() > 10  # the massive channels stay massive after the norm (ten times the row's rms)
    gs, us = _sums(pair, xn)
    exact = TG._silu(gs) * us
    Ag, Au = (NC.abs_sum(mag, xn) for _, _, mag, _ in pair)
    tol = NC.gated_gate(gs, us, Ag, Au, dtype, P)
    v_exact, v_tol = us, NC.plain_gate(us, Au, dtype, P)  # the up member alone, as a plain (v-like) output

    for order in NC.ORDERS:
        e32 = NC.xn32(x, g, NC.EPS, order).astype(np.float64)
        g32, u32 = _sums(pair, e32)
        if order != "sequential":  # (P counts the kernel's tree; 1024 additions in a row are another bound, and only the gate is asked of them)
            assert (np.abs(e32 - xn) <= (P - 1) * NC.U * np.abs(xn)).all(), order  # element-wise: the derivation's first-order count
            assert (np.abs(g32 - gs) <= P * NC.U * Ag).all() and (np.abs(u32 - us) <= P * NC.U * Au).all(), order
        assert (np.abs(_out(g32, u32, dtype) - exact) <= tol).all(), order
        assert (np.abs(TG._round_to(u32.astype(np.float32), dtype) - v_exact) <= v_tol).all(), order

    r = NC.r64(x, NC.EPS)
    bias = [npl["bias"].astype(np.float64) for _, npl, _, _ in pair]
    rows_all = np.ones(ROWS, bool)
    small = np.arange(ROWS) == NC.SMALL_ROW

    def after_bias():  # the norm's r applied to the finished sum, after the bias: (bias + W (x g)) r
        gg, uu = _sums(pair, x * g[None, :])
        return gg * r, uu * r

    mutants = {
        "g dropped": (lambda: _sums(pair, x * r), rows_all),
        "eps dropped": (lambda: _sums(pair, NC.xn64(x, g, 0.0)), small),  # (shows on the small row alone, by construction)
        "mean over the round, not over K": (lambda: _sums(pair, x * g[None, :] / np.sqrt((x * x).sum(axis=1, keepdims=True) / NC.NORM_ROUND + NC.EPS)), rows_all),
        "another row's r": (lambda: _sums(pair, x * g[None, :] * np.roll(r, 1, axis=0)), rows_all),
        "norm applied to the finished sum": (after_bias, np.abs(r[:, 0] - 1) > 0.5),
    }
    for name, (make, rows) in mutants.items():
        gm, um = make()
        assert rows.sum() >= 1
        share = (np.abs(_out(gm, um, dtype) - exact) > tol)[rows].mean()
        assert share > 0.5, (name, share)
        share_v = (np.abs(TG._round_to(um.astype(np.float32), dtype) - v_exact) > v_tol)[rows].mean()
        assert share_v > 0.5, (name, "plain", share_v)


def test_the_bit_exact_construction_is_exact_in_every_order():
    """|x[b, k]| = 2^b with random signs, g in {0.5, 1, 2}, eps = 0: ms = 4^b, r = 2^-b, xn = +-g[k] -- exact in fp32 in every
    summation order, and representable in 16 bits (tests/test_gpu_norm_front.py feeds xn to the parent entry)"""
    rng = np.random.default_rng(3)
    for K in (32, 1024, 4128):
        rows = 8
        x = (2.0 ** np.arange(rows))[:, None] * rng.choice([-1.0, 1.0], (rows, K))
        g = rng.choice([0.5, 1.0, 2.0], K)
        want = np.sign(x) * g[None, :]
        for order in NC.ORDERS:
            got = NC.xn32(x, g, 0.0, order)
            assert (got.astype(np.float64) == want).all(), (K, order)
        for t in (np.float16,):
            assert (want.astype(t).astype(np.float64) == want).all() and (x.astype(t).astype(np.float64) == x).all()
