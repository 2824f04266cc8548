"""Models and metrics for the fp32-class accuracy gates (tests/test_precision_cpu.py, tests/test_gpu_precision.py).

The split matrix-core kernels (csrc/sqllm_mfma_split.hip, sqllm_mfma_wide.hip, sqllm_split_common.h) write every fp32 operand as
the exact sum of three bf16 planes, v = hi + mid + lo, and keep six of the nine partial products of w * x.  This file restates
that arithmetic in numpy -- exact planes, the kernel's product order, one fp32 rounding per matrix instruction -- next to the
reference's plain fp32 FMA chain, and the two metrics that can tell them (and their mutants) apart:

  scaled_rms      rms over the outputs of (y - ref) / sqrt(sum of the squared terms): sees what a whole K sum loses;
  worst_over_abs  max over the outputs of |y - ref| / (|mul| + sum of the |terms|): with ONE non-zero term per output it
                  resolves the last mantissa bits of a single product.

Plain numpy, no GPU.  The fp64 reference is built from the unpacked weights (oracle.sqllm_oracle), as tests/helpers.py does.
"""
import numpy as np

from oracle import sqllm_oracle as oracle

U = 2.0 ** -24  # unit round-off of fp32 (half an ulp of 1.0)
SMALL_PRODUCTS = (0, 1, 2)  # model_split's products Am x Bm, Ah x Bl, Al x Bh
LARGE_PRODUCTS = (3, 4, 5)  # Ah x Bm, Am x Bh, Ah x Bh
# (vec plane, weight plane) of the six products in the kernel's order (split_phase / wide_phase: "small partial products first")
PRODUCTS = ((1, 1), (0, 2), (2, 0), (0, 1), (1, 0), (0, 0))
GATE_ONE_HOT_U = 16.0  # worst_over_abs of a split route with one non-zero term per output, in units of U (test_precision_cpu.py derives it)
GATE_DENSE_X_CHAIN = 2.0  # scaled_rms of any route over scaled_rms of the fp32 chain model on the same operands


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def split3(v):
    """The exact three-way bf16 split of split8 / split_entry: mask, subtract, mask, subtract.  Returns (hi, mid, lo) as fp32
    arrays whose low 16 bits are zero.  Every subtraction is exact in fp32 for finite v (the residual of a truncation fits the
    discarded bits), so hi + mid + lo == v, checked here bit for bit in fp64.

    Residuals that would be subnormal: below |v| = 2^-110 the last bits of v lie under bf16's subnormal grid (2^-133), the masks keep
    fewer than 8 significant bits and lo does not fit bf16 any more -- this function refuses such input (the last assertion), as
    the kernels' `>> 16` would lose those bits.  From |v| >= 2^-103 every non-zero plane is a normal bf16 as well (a matrix
    instruction may flush subnormal inputs); the GPU tests draw operands of magnitude 1e-3 .. 1e3, nowhere near."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    assert np.isfinite(v).all(), "the split is exact for finite values only"
    hi = (_bits(v) & np.uint32(0xFFFF0000)).view(np.float32)
    r1 = v - hi
    mid = (_bits(r1) & np.uint32(0xFFFF0000)).view(np.float32)
    lo = r1 - mid
    total = hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64)
    assert np.array_equal(total, v.astype(np.float64)), "hi + mid + lo != v"
    assert np.array_equal(total.astype(np.float32).view(np.uint32) | np.uint32(0x80000000), _bits(v) | np.uint32(0x80000000))
    assert not (_bits(lo) & np.uint32(0xFFFF)).any(), "lo does not fit bf16"
    return hi, mid, lo


def model_split(x, w, drop=None, zero_vec_lo=False):
    """x [B, K] @ w [K, N] as the split kernels compute it: per step of 32 k's six matrix instructions on exact bf16 planes, in the
    order Am Bm, Ah Bl, Al Bh, Ah Bm, Am Bh, Ah Bh (A: vec, B: weights), each adding its 32 exact products to the fp32 accumulator
    with ONE rounding (the 32-term sum itself is taken in fp64: products of two bf16 values have 16 significant bits).
    drop = i leaves product i out; zero_vec_lo zeroes the vec's lo plane (a wrong has_lo decision, a lost plane)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    w = np.ascontiguousarray(w, dtype=np.float32)
    K = x.shape[1]
    assert K % 32 == 0 and w.shape[0] == K
    xp = [p.astype(np.float64) for p in split3(x)]
    wp = [p.astype(np.float64) for p in split3(w)]
    if zero_vec_lo:
        xp[2] = np.zeros_like(xp[2])
    acc = np.zeros((x.shape[0], w.shape[1]), np.float32)
    for k0 in range(0, K, 32):
        for i, (a, b) in enumerate(PRODUCTS):
            if i == drop:
                continue
            acc = (acc.astype(np.float64) + xp[a][:, k0:k0 + 32] @ wp[b][k0:k0 + 32]).astype(np.float32)
    return acc


def model_chain(x, w):
    """x [B, K] @ w [K, N] as ONE fp32 FMA chain in k order per output: the loop of the reference's batched kernels."""
    x = np.ascontiguousarray(x, dtype=np.float32).astype(np.float64)
    w = np.ascontiguousarray(w, dtype=np.float32).astype(np.float64)
    acc = np.zeros((x.shape[0], w.shape[1]), np.float32)
    for k in range(x.shape[1]):  # (a product of two fp32 values is exact in fp64; the sum is then rounded once, to fp32)
        acc = (acc.astype(np.float64) + x[:, k, None] * w[k][None, :]).astype(np.float32)
    return acc


def _csr_chain(x, rows, cols, vals, N):
    """The CSR term as one fp32 FMA chain per (batch row, output) over the row's non-zeros in storage order."""
    x = x.astype(np.float64)
    rows = np.asarray(rows, np.int64)
    counts = np.diff(rows[:N + 1])
    out = np.zeros((x.shape[0], N), np.float32)
    for j in range(int(counts.max()) if counts.size else 0):
        live = np.nonzero(counts > j)[0]
        at = rows[live] + j
        out[:, live] = (out[:, live].astype(np.float64) + x[:, np.asarray(cols)[at]] * np.asarray(vals, np.float64)[at][None, :]).astype(np.float32)
    return out


def model_chain_op(case, x, mul, kind):
    """The whole op the reference's way: every term an fp32 FMA chain from zero, added to mul one after the other in fp32."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    W = oracle.dequantize(case["qweight"], case["lookup_table"], case["bits"], dtype=np.float32)
    out = (np.asarray(mul, np.float64) + model_chain(x, W)).astype(np.float32)
    if kind in ("spmv", "hybrid"):
        out = (out.astype(np.float64) + _csr_chain(x, case["rows"], case["cols"], case["vals"], case["N"])).astype(np.float32)
    if kind == "hybrid":
        t = model_chain(x, case["full_rows"])
        for c, n in enumerate(case["full_row_indices"]):
            out[:, n] = (out[:, n].astype(np.float64) + t[:, c]).astype(np.float32)
    return out


def reference(case, x, mul, kind):
    """fp64 reference of the op and what the metrics scale by, all [B, N]:
    ref    mul + dense (+ CSR) (+ top-X);
    scale  sqrt(sum of the squared terms w x, csr x, full x)  (mul not included);
    A      |mul| + sum of the |terms|;
    T      number of non-zero terms the output receives."""
    x = np.ascontiguousarray(x, dtype=np.float32).astype(np.float64)
    mul = np.asarray(mul, np.float64)
    N = case["N"]
    W = oracle.dequantize(case["qweight"], case["lookup_table"], case["bits"], dtype=np.float64)
    nz = (x != 0).astype(np.float64)
    ref = mul + x @ W
    sq = (x * x) @ (W * W)
    ab = np.abs(x) @ np.abs(W)
    T = nz @ (W != 0).astype(np.float64)
    if kind in ("spmv", "hybrid"):
        r, c, v = case["rows"], case["cols"], np.asarray(case["vals"], np.float64)
        ref = ref + oracle.csr_term(x, r, c, v, N)
        sq += oracle.csr_term(x * x, r, c, v * v, N)
        ab += oracle.csr_term(np.abs(x), r, c, np.abs(v), N)
        T += oracle.csr_term(nz, r, c, (v != 0).astype(np.float64), N)
    if kind == "hybrid":
        f, idx = np.asarray(case["full_rows"], np.float64), case["full_row_indices"]
        ref = ref + oracle.topx_term(x, f, idx, N)
        sq += oracle.topx_term(x * x, f * f, idx, N)
        ab += oracle.topx_term(np.abs(x), np.abs(f), idx, N)
        T += oracle.topx_term(nz, (f != 0).astype(np.float64), idx, N)
    return dict(ref=ref, scale=np.sqrt(sq), A=np.abs(mul) + ab, T=T)


def scaled_rms(y, ref, scale):
    """rms over the outputs of (y - ref) / scale; outputs whose scale is zero must be exact."""
    err = np.asarray(y, np.float64) - ref
    live = scale > 0
    assert not err[~live].any(), "an output without a non-zero term is not exact"
    return float(np.sqrt(np.mean((err[live] / scale[live]) ** 2)))


def over_abs(y, ref, A):
    """|y - ref| / A per output (0 where both vanish, inf where A == 0 and the output is not exact)."""
    err = np.abs(np.asarray(y, np.float64) - ref)
    out = np.zeros_like(err)
    live = A > 0
    out[live] = err[live] / A[live]
    out[~live & (err > 0)] = np.inf
    return out


def worst_over_abs(y, ref, A):
    return float(over_abs(y, ref, A).max())


# ---- operand makers ----


def fp32_born(rng, shape, sigma=1.0):
    """Normal draws kept as fp32: 24 significant bits.  More than 90 % of them have a non-zero lo plane (asserted): the operand
    class the C ABI promises, not "fp32 that was fp16"."""
    n = int(np.prod(shape))
    v = rng.normal(0, sigma, size=max(n, 256)).astype(np.float32)  # (at least 256 draws, so that the fraction below means something)
    assert (split3(v)[2] != 0).mean() > 0.9
    return v[:n].reshape(shape)


def fp16_born(rng, shape, sigma=1.0):
    """Normal draws rounded to fp16 and widened: 11 significant bits, the lo plane always zero (asserted)."""
    v = rng.normal(0, sigma, size=shape).astype(np.float16).astype(np.float32)
    assert not split3(v)[2].any()
    return v


def forced_planes(v):
    """bits | 0x00008080: mid >= 2^-8 and lo >= 2^-16 of the value's leading power of two -- every plane of every value counts."""
    v = (_bits(v) | np.uint32(0x00008080)).view(np.float32)
    hi, mid, lo = split3(v)
    lead = np.exp2(np.floor(np.log2(np.abs(v.astype(np.float64)))))
    assert (np.abs(mid) >= lead * 2.0 ** -8).all() and (np.abs(lo) >= lead * 2.0 ** -16).all()
    return v


def hot_values(rng, n):
    """n forced-plane values of either sign with magnitude in [0.5, ~4): no plane anywhere near the subnormal range"""
    return forced_planes((rng.choice([-1.0, 1.0], size=n) * (0.5 + np.abs(rng.normal(size=n)))).astype(np.float32))


def one_hot_rows(batch, K, hot_k, values):
    """vec [batch, K] whose row b holds exactly one non-zero element, values[b] at k = hot_k[b]."""
    hot_k = np.asarray(hot_k, np.int64)
    assert hot_k.shape == (batch,) and ((0 <= hot_k) & (hot_k < K)).all()
    x = np.zeros((batch, K), np.float32)
    x[np.arange(batch), hot_k] = np.asarray(values, np.float32)
    return x


def planes_hex(v):
    """'value = hi + mid + lo' of one fp32 value, planes as bf16 hex: for failure messages"""
    hi, mid, lo = (int(_bits(p).ravel()[0]) >> 16 for p in split3(np.float32(v).reshape(1)))
    return f"{float(v)!r} [bits {int(_bits(np.float32(v).reshape(1))[0]):08x}: hi {hi:04x} mid {mid:04x} lo {lo:04x}]"
