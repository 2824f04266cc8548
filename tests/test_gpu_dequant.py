"""The dense export on the GPU (sqllm_dequant and the Python surface on top of it) against the numpy oracle.

The expected matrix is built here: oracle.dequantize(...).T in fp32, plus the CSR values and the top-X columns added in
fp32, `.astype(np.float16)` for fp16 output.  Wherever a position receives at most ONE sparse contribution the kernel
must match it bit for bit (the codebook entry, or one fp32 add, rounded once).  A position with several contributions
(the cases build at most 4) is summed in an order the kernel is free to choose: three fp32 roundings of partial sums
that never exceed sum|terms| give |got - exact| <= 3 * 2^-24 * sum|terms| <= 2^-22 * sum|terms|, and fp16 output adds
one rounding of the result, 2^-11 * |exact| (+ 2^-25, half the smallest fp16 subnormal).  Every output buffer is
pre-filled with NaN, so an element the kernel skips fails the comparison."""
import ctypes
import functools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

oracle = H.oracle
NP_DT = {"float16": np.float16, "float32": np.float32}


def contributions(case):
    """(n, k, value) of every sparse contribution of a case, in operand order."""
    K, N = case["K"], case["N"]
    n, k, v = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
    if case.get("rows") is not None and case.get("vals") is not None and len(case["vals"]):
        n.append(np.repeat(np.arange(N), np.diff(case["rows"].astype(np.int64))))
        k.append(case["cols"].astype(np.int64))
        v.append(case["vals"].astype(np.float32))
    if case.get("full_rows") is not None:
        for c, idx in enumerate(case["full_row_indices"]):
            n.append(np.full(K, int(idx), np.int64))
            k.append(np.arange(K))
            v.append(case["full_rows"][:, c].astype(np.float32))
    return np.concatenate(n), np.concatenate(k), np.concatenate(v)


def expected(case):
    """exp32 [N, K] fp32 (sequential fp32 adds), count of sparse contributions, fp64 sum, sum of |terms|."""
    with np.errstate(all="ignore"):
        dense = np.ascontiguousarray(oracle.dequantize(case["qweight"], case["lookup_table"], case["bits"]).T.astype(np.float32))
        n, k, v = contributions(case)
        exp32 = dense.copy()
        np.add.at(exp32, (n, k), v)
        count = np.zeros(dense.shape, np.int64)
        np.add.at(count, (n, k), 1)
        s64 = dense.astype(np.float64)
        np.add.at(s64, (n, k), v.astype(np.float64))
        mag = np.abs(dense.astype(np.float64))
        np.add.at(mag, (n, k), np.abs(v.astype(np.float64)))
    return exp32, count, s64, mag


def check(got, case, dtype, exp=None):
    """Bit-exact where a position has at most one sparse contribution, the derived bound elsewhere."""
    exp32, count, s64, mag = exp if exp is not None else expected(case)
    assert count.max() <= 4
    with np.errstate(all="ignore"):
        want = exp32.astype(NP_DT[dtype])
    assert got.dtype == want.dtype and got.shape == want.shape
    bits_t = np.uint16 if dtype == "float16" else np.uint32
    same = (got.view(bits_t) == want.view(bits_t)) | (np.isnan(got) & np.isnan(want))
    single = count <= 1
    bad = single & ~same
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:4], got[bad][:4], want[bad][:4])
    multi = ~single
    if multi.any():
        bound = 2.0 ** -22 * mag[multi]
        if dtype == "float16":
            bound = bound + 2.0 ** -11 * np.abs(s64[multi]) + 2.0 ** -25
        g64, fin = got[multi].astype(np.float64), np.isfinite(s64[multi])
        assert ((g64 == s64[multi]) | (np.isnan(g64) & np.isnan(s64[multi])))[~fin].all()  # non-finite sums: the same non-finite value
        err = np.abs(g64[fin] - s64[multi][fin])
        assert (err <= bound[fin]).all(), float((err / bound[fin]).max())
    return int(multi.sum())


def run(gpu, case, dtype, pad=0, via="layer"):
    """Decode `case` on the GPU into a NaN-filled [N, K + pad] buffer; returns the whole buffer as numpy."""
    import torch

    from squeezellm_amd import decode

    t = H.to_torch(case, gpu)
    tdt = getattr(torch, dtype)
    buf = torch.full((case["N"], case["K"] + pad), float("nan"), dtype=tdt, device=gpu)
    w = decode.dequantize_layer(t, dtype=tdt, out=buf)
    assert w.shape == (case["N"], case["K"]) and w.data_ptr() == buf.data_ptr()
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@functools.lru_cache(maxsize=None)
def basic_case(bits, K, N):
    case = H.make_case(bits, K, N, sparse=0.05, topX=min(3, N), seed=bits * 1000 + K + N)
    return case, expected(case)


SHAPES = [(32, 4), (96, 68), (160, 132), (4096, 64)]


@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("bits", [3, 4])
def test_bit_exact_against_the_expected_matrix(gpu, bits, K, N, dtype):
    case, exp = basic_case(bits, K, N)
    got = run(gpu, case, dtype)
    check(got, case, dtype, exp)
    # the dense term alone: exactly the codebook entries
    dense = dict(case, rows=None, cols=None, vals=None, full_rows=None, full_row_indices=None)
    check(run(gpu, dense, dtype), dense, dtype)


@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("bits", [3, 4])
def test_leading_dimension_pad_is_not_written(gpu, bits, dtype):
    case, exp = basic_case(bits, 96, 68)
    buf = run(gpu, case, dtype, pad=8)
    assert np.isnan(buf[:, 96:]).all()
    check(np.ascontiguousarray(buf[:, :96]), case, dtype, exp)


def structured_case(bits, K, N, which):
    """The sparse structures of the issue; every position gets at most 4 contributions."""
    rng = np.random.default_rng(bits * 7 + K + len(which))
    case = H.make_case(bits, K, N, seed=K + N + bits)
    entries = []  # (n, k)
    topx = []
    if which == "rows":  # empty rows, the last row and the last column, one row holding 20 % of its columns
        for n in range(0, N, 3):
            if n not in (0, 5, N - 1) and n % 9 != 6:
                entries += [(n, int(k)) for k in rng.choice(K, size=3, replace=False)]
        entries += [(N - 1, K - 1), (N - 1, 0), (0, K - 1)]
        entries += [(5, int(k)) for k in rng.choice(K, size=K // 5, replace=False)]
    elif which == "topx_only":
        topx = [N - 1, 0, 17]
    elif which == "topx_on_csr_row":  # a top-X index equal to a row with CSR entries at the same k: two contributions each
        entries = [(9, k) for k in range(0, K, 5)] + [(N - 1, K - 1)]
        topx = [9, 3, N - 1]
    elif which == "dup_topx":
        topx = [7, 7, N - 2]
        entries = [(N - 3, 1)]
    elif which == "dup_csr":  # duplicate (n, k) entries, twice and three times
        entries = [(4, 2), (4, 2), (4, 3), (N - 1, K - 1), (N - 1, K - 1), (N - 1, K - 1), (20, 0)]
    elif which == "four":  # two duplicate CSR entries under two duplicate top-X indices: 4 contributions
        entries = [(11, 6), (11, 6), (11, K - 1), (12, 0)]
        topx = [11, 11]
    entries.sort(key=lambda e: e[0])  # CSR: rows in order, columns in any
    if entries or which == "rows":
        rows = np.zeros(N + 1, np.int32)
        for n, _ in entries:
            rows[n + 1] += 1
        case.update(rows=np.cumsum(rows).astype(np.int32), cols=np.array([k for _, k in entries], np.int32),
                    vals=rng.normal(0, 0.1, len(entries)).astype(np.float32))
    if topx:
        case.update(full_rows=rng.normal(0, 0.02, (K, len(topx))).astype(np.float32), full_row_indices=np.array(topx, np.int32))
    return case


@pytest.mark.parametrize("which", ["rows", "topx_only", "topx_on_csr_row", "dup_topx", "dup_csr", "four"])
@pytest.mark.parametrize("K,N", [(96, 68), (160, 132)])
@pytest.mark.parametrize("bits", [3, 4])
def test_sparse_structure(gpu, bits, K, N, which):
    case = structured_case(bits, K, N, which)
    exp = expected(case)
    if which == "rows":
        counts = np.diff(case["rows"])
        assert (counts == 0).any() and counts[5] == K // 5 and counts[N - 1] >= 2
    want_multi = {"rows": 0, "topx_only": 0, "topx_on_csr_row": len(range(0, K, 5)) + 1, "dup_topx": K, "dup_csr": 2, "four": K}[which]
    for dtype in ("float16", "float32"):
        assert check(run(gpu, case, dtype), case, dtype, exp) == want_multi
    if which == "four":
        assert exp[1].max() == 4


@pytest.mark.parametrize("with_topx", [False, True])
@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("K,N", [(96, 68), (160, 132)])
@pytest.mark.parametrize("bits", [3, 4])
def test_nnz_zero_with_rows_given(gpu, bits, K, N, dtype, with_topx):
    """nnz == 0 with a non-NULL, all-zero rows (cols / vals NULL or empty), straight through the C ABI -- alone, and beside
    top-X columns: the operands QuantLinearLUT.from_operands builds for a layer whose outliers all moved into full_rows."""
    import torch

    from squeezellm_amd import _lib
    from squeezellm_amd.quant import QuantLinearLUT

    case, _ = basic_case(bits, K, N)
    want = dict(case, rows=None, cols=None, vals=None)
    if not with_topx:
        want.update(full_rows=None, full_row_indices=None)
    exp = expected(want)
    t = H.to_torch(want, gpu)
    rows = torch.zeros(N + 1, dtype=torch.int32, device=gpu)
    empty_i, empty_f = torch.zeros(0, dtype=torch.int32, device=gpu), torch.zeros(0, dtype=torch.float32, device=gpu)
    tdt = getattr(torch, dtype)
    for cols, vals in ((None, None), (empty_i, empty_f)):
        out = torch.full((N, K), float("nan"), dtype=tdt, device=gpu)
        d = _lib.SqllmDequant()
        d.op.bits, d.op.K, d.op.N = bits, K, N
        d.op.qweight, d.op.lookup_table = t["qweight"].data_ptr(), t["lookup_table"].data_ptr()
        d.op.rows, d.op.nnz = rows.data_ptr(), 0
        if cols is not None:
            d.op.cols, d.op.vals = cols.data_ptr() or None, vals.data_ptr() or None
        if with_topx:
            d.op.full_rows, d.op.full_row_indices, d.op.topX = t["full_rows"].data_ptr(), t["full_row_indices"].data_ptr(), t["full_rows"].shape[1]
        d.out, d.ld, d.out_dtype = out.data_ptr(), K, _lib.DTYPE_F16 if dtype == "float16" else _lib.DTYPE_F32
        assert _lib.load().sqllm_dequant(ctypes.byref(d), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        check(out.cpu().numpy(), want, dtype, exp)
    if with_topx:  # the same state as a module: empty CSR buffers next to the top-X columns
        m = QuantLinearLUT.from_operands(dict(t, rows=rows, cols=empty_i, vals=empty_f))
        assert m.numvals == 0 and m.topX > 0 and m.rows.numel() == N + 1
        check(m.dequantize(tdt).cpu().numpy(), want, dtype, exp)


@pytest.mark.parametrize("bits", [3, 4])
def test_non_finite_values_propagate(gpu, bits):
    K, N = 96, 68
    case = H.make_case(bits, K, N, sparse=0.05, topX=2, seed=5)
    lut = case["lookup_table"].copy()
    lut[3, 1], lut[10, 0], lut[11, 2], lut[20, 5] = np.nan, np.inf, -np.inf, 70000.0  # (70000: finite in fp32, beyond fp16)
    case["lookup_table"] = lut
    vals = case["vals"].copy()
    vals[7] = np.inf
    case["vals"] = vals
    idx = oracle.unpack_indices(case["qweight"], bits)  # [K, N]: the poisoned entries are in use
    assert (idx[:, 3] == 1).any() and (idx[:, 10] == 0).any() and (idx[:, 11] == 2).any() and (idx[:, 20] == 5).any()
    exp = expected(case)
    for dtype in ("float16", "float32"):
        got = run(gpu, case, dtype)
        check(got, case, dtype, exp)
        single = exp[1] <= 1
        assert np.isnan(got[3][single[3]]).any() and np.isposinf(got[10][single[10]]).any() and np.isneginf(got[11][single[11]]).any()
        big = (idx[:, 20] == 5) & (exp[1][20] == 0)
        assert big.any()
        if dtype == "float16":
            assert np.isposinf(got[20][big]).all()  # a finite sum above 65504
        else:
            assert (got[20][big] == np.float32(70000.0)).all()


@pytest.mark.parametrize("dtype", ["float16", "float32"])
def test_repeatable_and_capturable(gpu, dtype):
    import torch

    from squeezellm_amd.quant import QuantLinearLUT

    case, exp = basic_case(3, 160, 132)
    m = QuantLinearLUT.from_operands(H.to_torch(case, gpu))
    tdt = getattr(torch, dtype)
    a = torch.full((132, 160), float("nan"), dtype=tdt, device=gpu)
    b = torch.full_like(a, float("nan"))
    m.dequantize(tdt, out=a)
    m.dequantize(tdt, out=b)
    torch.cuda.synchronize()
    first = a.cpu().numpy()
    assert first.tobytes() == b.cpu().numpy().tobytes()
    check(first, case, dtype, exp)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m.dequantize(tdt, out=b)
    b.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert b.cpu().numpy().tobytes() == first.tobytes()


def test_module_dequantize_honours_include_sparse(gpu):
    import torch

    from squeezellm_amd.quant import QuantLinearLUT

    case, exp = basic_case(4, 96, 68)
    m = QuantLinearLUT.from_operands(H.to_torch(case, gpu))
    assert m.include_sparse and m.numvals > 0 and m.topX > 0
    check(m.dequantize(torch.float32).cpu().numpy(), case, "float32", exp)
    m.include_sparse = False  # the buffers stay; the forward (op_kind) and the export drop the sparse terms
    assert m.op_kind(True) == "dense"
    dense = dict(case, rows=None, cols=None, vals=None, full_rows=None, full_row_indices=None)
    for dtype in ("float16", "float32"):
        check(m.dequantize(getattr(torch, dtype)).cpu().numpy(), dense, dtype)


@pytest.mark.parametrize("bits", [3, 4])
def test_to_linear_agrees_with_the_oracle_forward(gpu, bits):
    import torch

    case = H.make_case(bits, 160, 132, sparse=0.05, topX=3, seed=11)
    case["bias"] = np.random.default_rng(3).normal(0, 0.1, 132).astype(np.float32)
    from squeezellm_amd.quant import QuantLinearLUT

    m = QuantLinearLUT.from_operands(H.to_torch(case, gpu))
    lin = m.to_linear(torch.float32)
    assert isinstance(lin, torch.nn.Linear) and lin.weight.shape == (132, 160) and lin.weight.dtype == torch.float32
    assert lin.bias is not None and lin.bias.data_ptr() != m.bias.data_ptr() and torch.equal(lin.bias.data, m.bias)
    x = np.random.default_rng(4).standard_normal((3, 160)).astype(np.float32)
    y = lin(torch.from_numpy(x).to(gpu))
    ref = oracle.quantlinear_forward(x, case)  # fp64 accumulation
    assert H.rel_err(y.detach().cpu().numpy(), ref.astype(np.float32)) <= 2e-5  # tests/test_gpu_module.py: the operator path in fp32
    half = m.to_linear()
    assert half.weight.dtype == torch.float16 and half.bias.dtype == torch.float16
    nobias = QuantLinearLUT.from_operands(H.to_torch(dict(case, bias=None), gpu)).to_linear(torch.float32)
    assert nobias.bias is None


def test_to_dense_state_dict(gpu):
    import torch

    from squeezellm_amd import checkpoint, decode

    names = ["model.layers.0.self_attn.q_proj", "model.layers.0.mlp.down_proj"]
    c0 = H.make_case(4, 96, 68, sparse=0.05, seed=21)
    c0["bias"] = np.arange(68, dtype=np.float32)
    c1 = H.make_case(3, 160, 132, seed=22)
    layers = {n: H.to_torch(c, "cpu") for n, c in zip(names, (c0, c1))}
    extra = {"model.embed_tokens.weight": torch.randn(10, 96), "model.norm.weight": torch.ones(96), "lm_head.weight": torch.randn(10, 96).half()}
    sd = checkpoint.to_state_dict(layers, dict(extra))
    dense = checkpoint.to_dense_state_dict(sd, topX=2, dtype=torch.float16, device=gpu)
    assert set(dense) == set(extra) | {f"{n}.weight" for n in names} | {f"{names[0]}.bias"}
    for k, v in extra.items():
        assert dense[k] is v
    b = dense[f"{names[0]}.bias"]  # beside its weight: same device, same dtype, rounded once from the checkpoint's value
    assert b.dtype == torch.float16 and b.device == dense[f"{names[0]}.weight"].device
    assert torch.equal(b.cpu(), torch.from_numpy(c0["bias"]).to(torch.float16))
    for n, c in zip(names, (c0, c1)):
        lay = checkpoint.layer_operands(sd, n, topX=2, device=gpu)
        w = dense[f"{n}.weight"]
        assert w.dtype == torch.float16 and w.shape == (c["N"], c["K"]) and w.is_cuda
        assert torch.equal(w, decode.dequantize_layer(lay, torch.float16))
        check(w.cpu().numpy(), c, "float16")  # (moving outliers into top-X columns leaves every sum a single add)
    w32 = checkpoint.to_dense_state_dict(sd, dtype=torch.float32, device=gpu)[f"{names[1]}.weight"]
    check(w32.cpu().numpy(), c1, "float32")


@pytest.mark.parametrize("bits", [3, 4])
def test_reconstruction_error(gpu, bits):
    import torch

    from squeezellm_amd import nuq

    rng = np.random.default_rng(bits)
    N, K = 64, 128
    w = rng.normal(0, 0.02, (N, K)).astype(np.float32)
    g = (rng.random((N, K)).astype(np.float32) + 0.1) ** 2
    wt, gt = torch.from_numpy(w).to(gpu), torch.from_numpy(g).to(gpu)
    lay = nuq.quantize_linear(wt, gt, bits, sensitivity=2.0, topX=2)
    case = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in lay.items()}
    assert case["vals"] is not None and len(case["vals"]) > 0
    exp32, count, _, _ = expected(case)
    assert count.max() <= 1
    d = w.astype(np.float64) - exp32.astype(np.float64)
    for grad, weights in ((gt, g.astype(np.float64)), (None, np.ones_like(d))):
        got = nuq.reconstruction_error(wt, grad, lay)
        assert set(got) == {"sse", "weighted_sse", "max_abs"}
        for key, want in (("sse", (d * d).sum()), ("weighted_sse", (weights * d * d).sum()), ("max_abs", np.abs(d).max())):
            assert want > 0 and abs(got[key] - want) <= 1e-12 * want, (key, got[key], want)
    # at most 2^bits distinct values per row (dyadic, so that every mean of equal values is exact): fit and pack are lossless
    levels = rng.choice(np.arange(-512, 512), size=(N, 1 << bits)) / np.float32(1024)
    w0 = np.take_along_axis(levels, rng.integers(0, 1 << bits, (N, K)), axis=1).astype(np.float32)
    w0t = torch.from_numpy(w0).to(gpu)
    lay0 = nuq.quantize_linear(w0t, None, bits)
    assert nuq.reconstruction_error(w0t, None, lay0) == {"sse": 0.0, "weighted_sse": 0.0, "max_abs": 0.0}


@functools.lru_cache(maxsize=None)
def prefill_case(bits):
    case = H.make_case(bits, 128, 68, sparse=0.05, topX=3, seed=31 + bits)
    rng = np.random.default_rng(bits)
    bias = rng.normal(0, 0.1, 68).astype(np.float32)
    x = rng.standard_normal((40, 128)).astype(np.float16)
    _, _, w64, _ = expected(case)
    return case, bias, x, w64


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("bits", [3, 4])
def test_prefill_route(gpu, bits, with_bias):
    import torch

    from squeezellm_amd.quant import QuantLinearLUTFused

    case, bias, x, w64 = prefill_case(bits)
    case = dict(case, bias=bias if with_bias else None)
    assert QuantLinearLUTFused.dense_min_rows is None
    m = QuantLinearLUTFused.from_operands(H.to_torch(case, gpu))
    base = QuantLinearLUTFused.from_operands(H.to_torch(case, gpu))  # dense_min_rows = None: the fused kernel at every row count
    assert m.last_route is None
    m.dense_min_rows = 16
    xt = torch.from_numpy(x).to(gpu)
    y = m(xt)
    assert m.last_route == "dense" and y.dtype == torch.float16 and y.shape == (40, 68)
    x64 = x.astype(np.float64)
    b64 = bias.astype(np.float64) if with_bias else np.zeros(68)
    y64 = x64 @ w64.T + b64
    sparse = dict(rows=case["rows"], cols=case["cols"], vals=case["vals"], full_rows=case["full_rows"], full_row_indices=case["full_row_indices"])
    fwd = oracle.matvec(x.astype(np.float32), case["qweight"], np.zeros((40, 68), np.float32), case["lookup_table"], bits, **sparse) + b64
    assert np.abs(fwd - y64).max() <= 1e-12 * np.abs(y64).max()  # the fp64 oracle forward IS x @ W^T + bias of the expected matrix
    bound = 2.0 ** -10 * (np.abs(x64) @ np.abs(w64).T + np.abs(b64)) + 2.0 ** -10 * np.abs(fwd) + 2.0 ** -24
    err = np.abs(y.cpu().numpy().astype(np.float64) - fwd)
    assert (err <= bound).all(), float((err / bound).max())
    # below the threshold, and at any row count without one: the fused kernel, byte for byte
    y8, b8 = m(xt[:8]), base(xt[:8])
    assert m.last_route == "fused" and base.last_route == "fused"
    assert y8.cpu().numpy().tobytes() == b8.cpu().numpy().tobytes()
    b40 = base(xt)
    assert base.last_route == "fused" and base.dense_min_rows is None
    m.dense_min_rows = None
    y40 = m(xt)
    assert m.last_route == "fused" and y40.cpu().numpy().tobytes() == b40.cpu().numpy().tobytes()
    assert (np.abs(b40.cpu().numpy().astype(np.float64) - fwd) <= bound).all()
