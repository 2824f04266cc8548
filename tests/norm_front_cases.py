"""What the norm fronts' test files share (tests/test_norm_front_cpu.py, tests/test_gpu_norm_front.py).  A plain module: no
test lives here.

Reference.  xn[b, k] = x[b, k] * g[k] / sqrt(mean_k x[b, k]^2 + eps) in fp64 from the 16-bit x and g (eps: the fp32 value the
kernel is given), put through the fp64 oracle sums of tests/test_gpu_linear.py and the gated / rotary formulas of
tests/test_gpu_gated.py / tests/test_gpu_qkv_rope.py.

Tolerance.  Those suites' gates, with the allowance of every SUM (their 1e-6) widened by P * 2^-24 * A[b, n], where
A = sum_k |W terms| |xn| in fp64: what the kernel's fp32 xn may differ from the fp64 xn by, relatively, times the largest
the sum's terms can add up to.  P counts roundings of the kernel's arithmetic (csrc/sqllm_norm_front.h), each of relative
size u = 2^-24 at the most, to first order:

  * the sum of squares.  The squares are exact in fp32 (a 16-bit significand squared has at most 22 bits).  A thread adds
    8 per round into one accumulator (8 R additions, R = ceil(K / 4096) rounds), the butterfly adds 6 levels, the eight wave
    sums 8 more: every square passes through at most d = 8 R + 14 rounded additions of non-negative numbers, so the sum is
    off by at most d u relatively;
  * the division by K and the addition of eps: 2 u;
  * the square root halves what its argument is off by, (d + 2) / 2, and rounds once; the reciprocal rounds once: r is off
    by (d + 2) / 2 + 2 = 4 R + 10;
  * x * g and (x g) * r: 2 more, so xn is off by 4 R + 12;
  * second-order terms (products of these, each below 50 u) are below 1e-5 of that; P = 4 R + 13 covers them.

None of this comes from what the kernel gives: tests/test_norm_front_cpu.py shows that the fp32 formula in three summation
orders stays inside and that five mutants fall outside."""
import math

import numpy as np

NORM_VEC, NORM_ROUND, WAVES = 8, 4096, 8  # csrc/sqllm_norm_front.h: kNormVec, kNormRound (= kWaves * 64 * kNormVec), csrc/sqllm_kernels.h: SQLLM_WAVES
U = 2.0 ** -24
EPS_OUT = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -7}


def P_of(K):
    return 4 * math.ceil(K / NORM_ROUND) + 13


def widen(x16):
    """a 16-bit tensor or array -> fp64 numpy, exactly"""
    if hasattr(x16, "detach"):
        return x16.detach().float().cpu().numpy().astype(np.float64)
    return np.asarray(x16).astype(np.float64)


def r64(x, eps):
    with np.errstate(all="ignore"):
        return 1.0 / np.sqrt((x * x).mean(axis=-1, keepdims=True) + float(np.float32(eps)))


def xn64(x, g, eps):
    """the specification in fp64: x [rows, K] and g [K] already widened"""
    with np.errstate(all="ignore"):
        return x * g[None, :] * r64(x, eps)


def abs_sum(mag, xn):
    """A[b, n] = sum_k |terms of W[n, k]| |xn[b, k]| (mag: tests/test_gpu_dequant.py: expected()[3]); no bias"""
    return np.abs(xn) @ mag.T


# ---- the kernel's arithmetic in numpy fp32 ----

def _f32(a):
    return np.asarray(a, np.float32)


def sumsq_sequential(x32):
    s = np.zeros(x32.shape[0], np.float32)
    for k in range(x32.shape[1]):
        s = s + x32[:, k] * x32[:, k]
    return s


def sumsq_pairwise(x32):
    v = x32 * x32
    n = 1 << (v.shape[1] - 1).bit_length()
    v = np.concatenate([v, np.zeros((v.shape[0], n - v.shape[1]), np.float32)], axis=1)
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    return v[:, 0]


def sumsq_kernel_order(x32):
    """512 partial sums, then the tree: thread t adds the squares of elements [8 t, 8 t + 8) of every round of 4096 in ascending
    k; the 64 lanes of a wave meet in a butterfly (32, 16, 8, 4, 2, 1); the eight wave sums are added in wave order"""
    rows, K = x32.shape
    pad = -K % NORM_ROUND
    v = np.concatenate([x32, np.zeros((rows, pad), np.float32)], axis=1).reshape(rows, -1, WAVES * 64, NORM_VEC)
    acc = np.zeros((rows, WAVES * 64), np.float32)
    for rnd in range(v.shape[1]):
        for j in range(NORM_VEC):
            acc = acc + v[:, rnd, :, j] * v[:, rnd, :, j]
    w = acc.reshape(rows, WAVES, 64)
    for m in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, np.arange(64) ^ m]
    s = np.zeros(rows, np.float32)
    for i in range(WAVES):
        s = s + w[:, i, 0]
    return s


ORDERS = {"sequential": sumsq_sequential, "pairwise": sumsq_pairwise, "kernel": sumsq_kernel_order}


def xn32(x, g, eps, order="kernel"):
    """the header's formulas in fp32, every operation rounded once: -> float32 [rows, K]"""
    x32, g32 = _f32(x), _f32(g)
    with np.errstate(all="ignore"):
        ms = ORDERS[order](x32) / np.float32(x32.shape[1])
        r = np.float32(1.0) / np.sqrt(ms + np.float32(eps))
        out = (x32 * g32[None, :]) * r[:, None]
    assert out.dtype == np.float32 and r.dtype == np.float32
    return out


# ---- the gates ----

def gated_gate(g, u, Ag, Au, dtype, P):
    """tests/test_gpu_gated.py: _gate, the two sums' allowances widened"""
    from tests import test_gpu_gated as TG

    s = np.abs(TG._silu(g))
    return (np.maximum(np.abs(TG._silu(g) * u), 2.0 ** -14) * EPS_OUT[dtype] + 1.1 * np.abs(u) * (1e-6 + P * U * Ag)
            + s * (1e-6 + P * U * Au) + 1e-6)


def plain_gate(s, A, dtype, P):
    """the linear's gate (v of the attention front), the sum's allowance widened"""
    return np.maximum(np.abs(s), 2.0 ** -14) * EPS_OUT[dtype] + 1e-6 + P * U * A


def rotated_gate(s, A, pos, cos, sin, D, layout, dtype, P):
    """tests/test_gpu_qkv_rope.py: _rotated -> (exact, tolerance), the allowance of each of the pair's two sums widened"""
    from tests import test_gpu_qkv_rope as TQ

    lo, hi = TQ._split(s, D, layout)
    a_lo, a_hi = TQ._split(A, D, layout)
    c, sn = TQ._at(cos, pos).astype(np.float64), TQ._at(sin, pos).astype(np.float64)
    e_lo, e_hi = lo * c - hi * sn, hi * c + lo * sn

    def tol(e, a, b, wc, ws):  # wc / ws: the allowance of the sum that meets cos / sin
        return (np.maximum(np.abs(e), 2.0 ** -14) * EPS_OUT[dtype] + np.abs(c) * (1e-6 + P * U * wc) + np.abs(sn) * (1e-6 + P * U * ws)
                + (np.abs(a) + np.abs(b)) * 2.0 ** -22 + 1e-6)

    return TQ._merge(e_lo, e_hi, layout), TQ._merge(tol(e_lo, lo * c, hi * sn, a_lo, a_hi), tol(e_hi, hi * c, lo * sn, a_hi, a_lo), layout)


# ---- operands ----

ROW_SCALES = (1.0, 0.03, 7.0, 2.0 ** -10, 2.5)  # distinct factors; row 3 is small enough for eps to matter
EPS = 1e-6
SMALL_ROW, MASSIVE_ROW = 3, 2


def activations(rows, K, dtype, seed=0, massive=True, scales=ROW_SCALES):
    """x [rows, K] and g [K] as float64 arrays of values that are exact in `dtype`: rows scaled by distinct factors (cycled),
    one of them around 2^-10 (eps = 1e-6 moves its r by tens of percent), four channels of one row around 200 (the
    massive-activation case), g = 1 + N(0, 0.25).  `scales`: the cycle of row factors (tests/test_gpu_csr_span_fronts.py passes
    eight, one per row of the widest batch tile)"""
    import torch

    gen = torch.Generator().manual_seed(1234 + 17 * rows + K + seed)
    x = torch.randn((rows, K), generator=gen, dtype=torch.float64)
    x = x * torch.tensor([scales[b % len(scales)] for b in range(rows)], dtype=torch.float64)[:, None]
    if massive and rows > MASSIVE_ROW:
        for i, k in enumerate((1, K // 3, K // 2 + 5, K - 2)):
            x[MASSIVE_ROW, k] = (200.0 + 7 * i) * (-1) ** i
    g = 1.0 + 0.25 * torch.randn(K, generator=gen, dtype=torch.float64)
    td = getattr(torch, dtype)
    return x.to(td), g.to(td)
