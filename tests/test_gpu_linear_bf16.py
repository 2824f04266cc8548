"""GPU tests of bf16 at the two ends of the fused linear (sqllm_linear_bf16), of the bf16 dense export (sqllm_dequant with
SQLLM_DTYPE_BF16) and of the Python surface on top of both.

numpy has no bf16: activations are widened with `tensor.float()` (exact) and the oracle is the fp64 matvec of
tests/helpers.py on those widened activations, plus the bias -- the scheme of tests/test_gpu_linear.py.  Tolerance of the
fused route: max(|exact|, 2^-14) * 2^-7 + 1e-6, i.e. one bf16 ulp at the element's magnitude (8 significant bits where
fp16 has 11) plus that file's absolute slack."""
import ctypes

import numpy as np
import pytest

from tests import helpers as H
from tests import test_gpu_dequant as DQ
from tests import test_gpu_linear as TL

pytestmark = pytest.mark.gpu

oracle = H.oracle
LIMIT = 131072.0  # what one contribution to the fixed-point word may carry


def _tol(exact, eps):
    return np.maximum(np.abs(exact), 2.0 ** -14) * eps + 1e-6


def _check_bf16(got, exact):
    """`got`: a bf16 (or fp16) tensor; every element finite and within one bf16 ulp of `exact`."""
    g = got.float().cpu().numpy().astype(np.float64).reshape(exact.shape)
    assert np.isfinite(g).all(), f"{(~np.isfinite(g)).sum()} non-finite outputs"
    bad = np.abs(g - exact) > _tol(exact, 2.0 ** -7)
    assert not bad.any(), f"{bad.sum()} of {bad.size} outputs off by more than 1 bf16 ulp; worst {np.abs(g - exact).max()}"


def _exact(npl, x, kind):
    """fp64 result for the 16-bit activations `x` (a tensor), widened exactly"""
    return TL._exact(npl, x.float().cpu().numpy(), kind)


def _abs_sum(npl, mag, x):
    """sum_k |terms of W[n, k]| |x[b, k]| + |bias[n]| in fp64 (mag = sum of |terms| per weight, tests/test_gpu_dequant.py:
    expected): an upper bound of every partial sum of every output"""
    s = np.abs(x.float().cpu().numpy().astype(np.float64)).reshape(-1, npl["K"]) @ mag.T
    if npl.get("bias") is not None:
        s = s + np.abs(npl["bias"].astype(np.float64))
    return s


def _fused(lay):
    from squeezellm_amd import quant

    mod = quant.QuantLinearLUT.from_operands(lay)
    assert quant.fuse_quant_lut(mod) == 1 and type(mod) is quant.QuantLinearLUTFused
    return mod


def _workspaces_clean(mod):
    import torch

    bufs = [v for v in mod._ws.values() if isinstance(v, torch.Tensor)]
    assert bufs
    for ws in bufs:
        assert int(ws.count_nonzero()) == 0, "workspace must be left zero-filled"


_LAYERS = {}


def parity_layer(gpu, bits, kind, bias):
    """one layer per (bits, kind, bias), shared by the row counts: torch operands, numpy operands, sum of |terms| per weight"""
    from squeezellm_amd import synth

    key = (str(gpu), bits, kind, bias)
    if key not in _LAYERS:
        K, N = 1024, 456  # ragged last column tile (456 = 7 * 64 + 8)
        lay = synth.make_layer(K, N, bits, sparse_frac=0.0 if kind == "dense" else 0.01, topX=3 if kind == "hybrid" else 0,
                               heavy_rows=2 if kind != "dense" else 0, bias=bias, device=gpu, seed=31 * bits + 7)
        npl = TL._npl(lay)
        _LAYERS[key] = (lay, npl, DQ.expected(npl)[3])
    return _LAYERS[key]


# ---- 1. parity ----

@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("kind", ["dense", "spmv", "hybrid"])
@pytest.mark.parametrize("rows", [1, 2, 5, 8, 19])
@pytest.mark.parametrize("bias", [False, True])
def test_bf16_forward_matches_oracle_and_cleans_up(gpu, bits, kind, rows, bias):
    import torch

    lay, npl, mag = parity_layer(gpu, bits, kind, bias)
    K, N = lay["K"], lay["N"]
    mod = _fused(lay)
    g = torch.Generator(device=gpu).manual_seed(rows)
    x = torch.randn((rows, K), device=gpu, generator=g).to(torch.bfloat16)
    assert (_abs_sum(npl, mag, x) < LIMIT).all()  # every contribution is in range: no non-finite result is admissible
    exact = _exact(npl, x, kind)
    for rep in range(3):  # the second and third call run on the workspace the previous one left behind
        y = mod(x if rows > 1 else x.reshape(1, 1, K))
        assert y.dtype == torch.bfloat16 and y.shape[-1] == N and mod.last_route == "fused"
        _check_bf16(y.reshape(rows, N), exact)
    _workspaces_clean(mod)


# ---- 2. one module, both types ----

@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("rows", [1, 5])
def test_fp16_and_bf16_calls_alternate_on_one_module(gpu, bits, rows):
    import torch

    lay, npl, mag = parity_layer(gpu, bits, "hybrid", True)
    K, N = lay["K"], lay["N"]
    mod = _fused(lay)
    g = torch.Generator(device=gpu).manual_seed(11 + rows)
    x32 = torch.randint(-64, 65, (rows, K), device=gpu, generator=g).float() / 16  # exact in fp16 and in bf16
    xs = {torch.float16: x32.half(), torch.bfloat16: x32.to(torch.bfloat16)}
    assert all(torch.equal(v.float(), x32) for v in xs.values())
    assert (_abs_sum(npl, mag, x32) < LIMIT).all()
    exact = _exact(npl, x32, "hybrid")
    got = {torch.float16: [], torch.bfloat16: []}
    for dt in (torch.float16, torch.bfloat16, torch.float16, torch.bfloat16):
        y = mod(xs[dt] if rows > 1 else xs[dt].reshape(1, 1, K)).reshape(rows, N)
        assert y.dtype == dt and mod.last_route == "fused"
        got[dt].append(y.clone())
    torch.cuda.synchronize()
    assert len(mod._desc) == 1  # one descriptor and one workspace serve both types
    for y in got[torch.float16]:
        TL._check_fp16(y.cpu().numpy(), exact)
    for y in got[torch.bfloat16]:
        _check_bf16(y, exact)
    for dt in got:
        assert got[dt][0].view(torch.int16).cpu().numpy().tobytes() == got[dt][1].view(torch.int16).cpu().numpy().tobytes()
    _workspaces_clean(mod)


# ---- 3. determinism ----

@pytest.mark.parametrize("bits", [3, 4])
def test_bf16_forward_is_deterministic(gpu, bits):
    import torch

    lay, npl, mag = parity_layer(gpu, bits, "hybrid", True)
    K, N = lay["K"], lay["N"]
    g = torch.Generator(device=gpu).manual_seed(3)
    x = torch.randn((19, K), device=gpu, generator=g).to(torch.bfloat16)
    exact = _exact(npl, x, "hybrid")
    a, b = _fused(lay)(x), _fused(lay)(x)  # fresh modules, the same operands
    torch.cuda.synchronize()
    assert a.view(torch.int16).cpu().numpy().tobytes() == b.view(torch.int16).cpu().numpy().tobytes()
    _check_bf16(a, exact)
    for rows in (1, 2, 5, 8):
        y = _fused(lay)(x[:rows].contiguous()).reshape(rows, N)
        _check_bf16(y, exact[:rows])
        d = np.abs(y.float().cpu().numpy().astype(np.float64) - a[:rows].float().cpu().numpy().astype(np.float64))
        assert (d <= _tol(exact[:rows], 2.0 ** -7)).all()


# ---- 4. the range rule ----

@pytest.mark.parametrize("rows", [1, 5])
def test_bf16_out_of_range_contributions_are_infinite_never_wrong(gpu, rows):
    """K = 1024 weights that are one constant per column, x = 2^14 everywhere: the exact result is 2^24 c.  At most 63
    contributions exist per column and each carries at most 131072, so a column whose sum is 2^24 has a contribution
    beyond the range and must come out infinite; a column inside the range must come out exact."""
    import torch

    from squeezellm_amd import synth

    K, N = 1024, 64
    lay = synth.make_layer(K, N, 4, device=gpu, seed=5)
    consts = np.repeat(np.array([2.0 ** -10, 1.0, -1.0, 1.0 / 16], np.float32), 16)  # 16 columns each
    lay["lookup_table"] = torch.from_numpy(np.repeat(consts[:, None], 16, axis=1).copy()).to(gpu)  # every index decodes to it
    mod = _fused(lay)
    x = torch.full((rows, K), 2.0 ** 14, device=gpu, dtype=torch.bfloat16)
    assert float(x.float().min()) == 2.0 ** 14
    exact = np.tile(consts.astype(np.float64) * K * 2.0 ** 14, (rows, 1))
    abs_sum = np.abs(exact)  # (one sign per column: sum |terms| = |sum|)
    assert exact[0, 0] == 16384 and exact[0, 16] == 2.0 ** 24 > 63 * LIMIT and exact[0, 48] == 2.0 ** 20
    for rep in range(2):  # (the flags of the first call must not linger)
        y = mod(x if rows > 1 else x.reshape(1, 1, K)).reshape(rows, N).float().cpu().numpy().astype(np.float64)
        assert (y[:, 0:16] == 16384.0).all()
        assert np.isposinf(y[:, 16:32]).all() and np.isneginf(y[:, 32:48]).all()
        mid = y[:, 48:64]  # 2^20: finite and right, or +inf -- which one depends on how K is sliced
        assert (np.isposinf(mid) | (np.abs(mid - 2.0 ** 20) <= _tol(exact[:, 48:64], 2.0 ** -7))).all()
        fin = np.isfinite(y)
        assert (np.abs(y[fin] - exact[fin]) <= _tol(exact[fin], 2.0 ** -7)).all()  # never a finite wrong value
        assert (abs_sum[~fin] >= LIMIT).all() and not np.isnan(y).any()
    _workspaces_clean(mod)


# ---- 5. non-finite operands ----

@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("poison", ["nan", "+inf", "-inf", "+inf,-inf"])
def test_bf16_linear_propagates_nan_and_inf_like_the_operator_path(gpu, bits, rows, poison):
    import torch

    from squeezellm_amd import quant

    lay, npl, mag = parity_layer(gpu, bits, "hybrid", True)
    K, N = lay["K"], lay["N"]
    plain = quant.QuantLinearLUT.from_operands(lay)
    fused = _fused(lay)
    g = torch.Generator(device=gpu).manual_seed(5)
    x = torch.randn((rows, K), device=gpu, generator=g).to(torch.bfloat16)
    exact = _exact(npl, x, "hybrid")  # (before the poison: the rows that stay clean are compared with it)
    vals = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
    for j, name in enumerate(poison.split(",")):
        x[rows - 1, 37 + 500 * j] = vals[name]  # (two poisons land in different K slices of the tile; dense weights are never zero)
    xin = x if rows > 1 else x.reshape(1, 1, K)
    want = plain(xin.float()).reshape(rows, N).float().cpu()  # the fp32 operator path on the widened activations
    for rep in range(2):  # second call: the flags of the first must not linger in the workspace
        y = fused(xin)
        assert y.dtype == torch.bfloat16
        got = y.reshape(rows, N).float().cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(torch.isposinf(got), torch.isposinf(want)) and torch.equal(torch.isneginf(got), torch.isneginf(want))
        fin = torch.isfinite(want).numpy()
        assert fin[: rows - 1].all() and not fin[rows - 1].any()  # the poisoned row is non-finite in every column
        g64 = got.numpy().astype(np.float64)
        assert (np.abs(g64[fin] - exact[fin]) <= _tol(exact[fin], 2.0 ** -7)).all()
    _workspaces_clean(fused)


# ---- 6. C ABI, groups, graphs ----

@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("batched", [False, True])
def test_bf16_linear_sequence_groups_and_graph(gpu, bits, batched):
    import torch

    from squeezellm_amd import decode, synth

    shapes = [(256, 256)] * 3 + [(256, 704)] * 2  # q / k / v-like and gate / up-like groups
    lays = [synth.make_layer(K, N, bits, sparse_frac=0.005, topX=2, heavy_rows=1, bias=(i % 2 == 0), device=gpu, seed=60 + i)
            for i, (K, N) in enumerate(shapes)]
    rows = 4 if batched else 1
    xa = torch.randn((rows, 256), device=gpu).to(torch.bfloat16)
    xb = torch.randn((rows, 256), device=gpu).to(torch.bfloat16)
    xs = [xa, xa, xa, xb, xb]
    ys = [torch.full((rows, N), 7.0, device=gpu, dtype=torch.bfloat16) for _, N in shapes]  # must be overwritten
    seq = decode.OpSequence(lays, xs, ys, batched=batched, fuse_shared_input=True, linear=True)
    assert [len(g) for g in seq.groups] == [3, 2] and seq.io_dtype is torch.bfloat16
    exact = [_exact(TL._npl(l), x, "hybrid") for l, x in zip(lays, xs)]
    seq.launch()
    torch.cuda.synchronize()
    for y, e in zip(ys, exact):
        _check_bf16(y, e)
    g = seq.graph()
    for y in ys:
        y.fill_(-3.0)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    for y, e in zip(ys, exact):
        _check_bf16(y, e)


def test_linear_sequence_takes_one_dtype(gpu):
    import torch

    from squeezellm_amd import decode, synth

    lays = [synth.make_layer(256, 256, 4, device=gpu, seed=s) for s in range(2)]
    mk = lambda dt: torch.zeros(256, device=gpu, dtype=dt)  # noqa: E731
    h, b = torch.float16, torch.bfloat16
    for xd, yd in (((h, b), (h, b)), ((b, b), (b, h)), ((b, b), (h, h)), ((h, b), (h, h))):
        with pytest.raises(ValueError):
            decode.OpSequence(lays, [mk(d) for d in xd], [mk(d) for d in yd], linear=True)
    with pytest.raises(ValueError):
        decode.OpSequence(lays, [mk(torch.float32)] * 2, [mk(torch.float32)] * 2, linear=True)
    assert decode.OpSequence(lays, [mk(h)] * 2, [mk(h), mk(h)], linear=True).io_dtype is h
    assert decode.OpSequence(lays, [mk(b)] * 2, [mk(b), mk(b)], linear=True).io_dtype is b


def test_captured_bf16_module_forward_holds_its_kernel_only(gpu):
    """as tests/test_gpu_linear.py: test_captured_module_forwards_hold_their_kernels_only -- after an eager call, a captured
    bf16 forward of the fused class is ONE kernel node (no zero fill, no cast, no memory node)."""
    import torch

    from squeezellm_amd import synth

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

    K, N = 512, 328
    mods = [_fused(synth.make_layer(K, N, 4 if i % 2 else 3, sparse_frac=0.01, topX=3, heavy_rows=1, bias=bool(i % 2), device=gpu, seed=50 + i))
            for i in range(2)]
    x = torch.randn((1, 1, K), device=gpu).to(torch.bfloat16)
    outs = []

    def run():
        outs.clear()
        with torch.no_grad():
            for m in mods:
                outs.append(m(x))

    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    want = [o.clone() for o in outs]
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        run()
    assert node_types(g) == [0] * len(mods)  # hipGraphNodeTypeKernel: nothing but the linears
    g.instantiate()
    for _ in range(2):
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for o, w in zip(outs, want):
            assert o.dtype == torch.bfloat16 and torch.equal(o, w)


# ---- 7. dense export ----

def _export_cases(bits, K):
    N = 68
    yield "dense", H.make_case(bits, K, N, seed=K + bits)
    yield "csr+topx", H.make_case(bits, K, N, sparse=0.05, topX=3, seed=K + bits + 1)
    for which in ("rows", "topx_only", "topx_on_csr_row", "dup_csr"):
        yield which, DQ.structured_case(bits, K, N, which)


@pytest.mark.parametrize("K", [512, 544])  # one whole chunk of 512 k's; a second, short one
@pytest.mark.parametrize("bits", [3, 4])
def test_bf16_export_rounds_the_fp32_sum_once(gpu, bits, K):
    import torch

    from squeezellm_amd import decode

    for tag, case in _export_cases(bits, K):
        t = H.to_torch(case, gpu)
        N = case["N"]
        w32 = decode.dequantize_layer(t, dtype=torch.float32)
        want = w32.to(torch.bfloat16)
        got = decode.dequantize_layer(t, dtype=torch.bfloat16)
        assert got.dtype == torch.bfloat16 and got.shape == (N, K) and got.is_contiguous()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), tag
        # into a view with row stride K + 8: the columns beyond K are left alone
        buf = torch.full((N, K + 8), float("nan"), dtype=torch.bfloat16, device=gpu)
        w = decode.dequantize_layer(t, dtype=torch.bfloat16, out=buf)
        assert w.shape == (N, K) and w.data_ptr() == buf.data_ptr()
        assert torch.isnan(buf[:, K:]).all() and torch.equal(buf[:, :K].contiguous().view(torch.int16), want.view(torch.int16)), tag
    with pytest.raises(TypeError, match="bfloat16"):
        decode.dequantize_layer(t, dtype=torch.float64)


@pytest.mark.parametrize("bits", [3, 4])
def test_bf16_export_through_the_module_and_the_checkpoint(gpu, bits):
    import torch

    from squeezellm_amd import checkpoint, decode
    from squeezellm_amd.quant import QuantLinearLUT

    case = H.make_case(bits, 160, 68, sparse=0.05, topX=3, seed=21 + bits)
    case["bias"] = np.arange(68, dtype=np.float32) / 7
    t = H.to_torch(case, gpu)
    want = decode.dequantize_layer(t, dtype=torch.float32).to(torch.bfloat16)
    m = QuantLinearLUT.from_operands(t)
    assert torch.equal(m.dequantize(dtype=torch.bfloat16).view(torch.int16), want.view(torch.int16))
    lin = m.to_linear(torch.bfloat16)
    assert lin.weight.dtype == torch.bfloat16 and lin.bias.dtype == torch.bfloat16
    assert torch.equal(lin.weight.data.view(torch.int16), want.view(torch.int16))
    assert torch.equal(lin.bias.data, m.bias.to(torch.bfloat16))
    name = "model.layers.0.self_attn.q_proj"
    sd = checkpoint.to_state_dict({name: H.to_torch(case, "cpu")}, {})
    dense = checkpoint.to_dense_state_dict(sd, topX=3, dtype=torch.bfloat16, device=gpu)
    w = dense[f"{name}.weight"]
    lay = checkpoint.layer_operands(sd, name, topX=3, device=gpu)
    assert w.dtype == torch.bfloat16 and dense[f"{name}.bias"].dtype == torch.bfloat16
    assert torch.equal(w.view(torch.int16), decode.dequantize_layer(lay, torch.float32).to(torch.bfloat16).view(torch.int16))


# ---- 8. the prefill route ----

@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("bits", [3, 4])
def test_bf16_prefill_route(gpu, bits, with_bias):
    import torch

    from squeezellm_amd.quant import QuantLinearLUTFused

    case, bias, x16, w64 = DQ.prefill_case(bits)  # 40 rows, K = 128, N = 68
    case = dict(case, bias=bias if with_bias else None)
    m = QuantLinearLUTFused.from_operands(H.to_torch(case, gpu))
    base = QuantLinearLUTFused.from_operands(H.to_torch(case, gpu))  # no threshold: the fused kernel at every row count
    m.dense_min_rows = 16
    xt = torch.from_numpy(x16).to(gpu).to(torch.bfloat16)
    y = m(xt)
    assert m.last_route == "dense" and y.dtype == torch.bfloat16 and y.shape == (40, 68)
    xw = xt.float().cpu().numpy()  # the widened activations
    x64 = xw.astype(np.float64)
    b64 = bias.astype(np.float64) if with_bias else np.zeros(68)
    sparse = dict(rows=case["rows"], cols=case["cols"], vals=case["vals"], full_rows=case["full_rows"], full_row_indices=case["full_row_indices"])
    fwd = oracle.matvec(xw, case["qweight"], np.zeros((40, 68), np.float32), case["lookup_table"], bits, **sparse) + b64
    assert np.abs(fwd - (x64 @ w64.T + b64)).max() <= 1e-12 * np.abs(fwd).max()
    bound = 2.0 ** -7 * (np.abs(x64) @ np.abs(w64).T + np.abs(b64)) + 2.0 ** -7 * np.abs(fwd) + 2.0 ** -24
    err = np.abs(y.float().cpu().numpy().astype(np.float64) - fwd)
    assert (err <= bound).all(), float((err / bound).max())
    # below the threshold: the fused kernel, byte for byte what a module without a threshold gives
    y8, b8 = m(xt[:8]), base(xt[:8])
    assert m.last_route == "fused" and base.last_route == "fused" and y8.dtype == torch.bfloat16
    assert torch.equal(y8.view(torch.int16), b8.view(torch.int16))
    _check_bf16(y8, fwd[:8])


# ---- 9. one full-size case ----

def test_bf16_linear_full_size_hybrid_w4(gpu):
    """LLaMA-7B gate_proj shape (K = 4096, N = 11008), w4 s45 + top-X, one row, through the C ABI directly: K slices and
    several CSR chunks per row."""
    import torch

    from squeezellm_amd import _lib, synth

    K, N = 4096, 11008
    lay = synth.make_layer(K, N, 4, sparse_frac=0.0045, topX=10, heavy_rows=10, bias=True, device=gpu, seed=9)
    x = torch.randn(K, device=gpu).to(torch.bfloat16)
    out = torch.empty(N, device=gpu, dtype=torch.bfloat16)
    ws = torch.zeros(_lib.linear_workspace_bytes(N, 0), dtype=torch.uint8, device=gpu)
    lin = _lib.SqllmLinear()
    o = lin.op
    o.bits, o.batch, o.K, o.N = 4, 0, K, N
    o.vec, o.qweight, o.mul, o.lookup_table = x.data_ptr(), lay["qweight"].data_ptr(), out.data_ptr(), lay["lookup_table"].data_ptr()
    o.rows, o.cols, o.vals, o.nnz = lay["rows"].data_ptr(), lay["cols"].data_ptr(), lay["vals"].data_ptr(), lay["vals"].numel()
    o.full_rows, o.full_row_indices, o.topX = lay["full_rows"].data_ptr(), lay["full_row_indices"].data_ptr(), 10
    lin.bias, lin.workspace = lay["bias"].data_ptr(), ws.data_ptr()
    lib = _lib.load()
    exact = _exact(TL._npl(lay), x.reshape(1, K), "hybrid")
    for _ in range(2):
        assert lib.sqllm_linear_bf16(ctypes.byref(lin), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        _check_bf16(out.reshape(1, N), exact)
    assert int(ws.count_nonzero()) == 0


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("kind", ["dense", "hybrid"])
@pytest.mark.parametrize("rows", [1, 3, 8])
@pytest.mark.parametrize("cls", ["V", "C"])
def test_bf16_linear_nonfinite_operands_where_the_masked_lanes_run(gpu, bits, kind, rows, cls):
    """tests/test_gpu_linear.py's test of the same name in bfloat16: K = 544, N = 132, activations (V) or codebook entries (C) poisoned, the
    pattern from the term-wise model of tests/nonfinite_cases.py on the bf16-born activations plus bias -- not from the operator path --,
    finite outputs within one bf16 ulp, workspaces left zero."""
    from tests import nonfinite_cases as NC

    mod = NC.run_linear(gpu, _fused, bits, kind, rows, cls, "bfloat16")
    _workspaces_clean(mod)
