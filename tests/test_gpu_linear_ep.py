"""Tests of the fused linear with an epilogue (sqllm_linear_ep_f16 / sqllm_linear_ep_bf16 behind QuantLinearLUTFused.forward's
`act`, `residual` and `out`): out = OT(act(bias + sum) + residual) as one kernel.  Modelled on tests/test_gpu_gated.py; layers and
helpers are those of tests/test_gpu_linear_bf16.py (the parity shape K = 1024, N = 456) and tests/test_gpu_csr_span.py (ladder "a").

Reference: the fp64 oracle sum of tests/helpers.py on the exactly widened activations, plus the bias (g), then the activation's
formula in fp64 (include/sqllm_hip.h: the table), plus the widened residual (r).  Tolerance, derived and not measured:

    max(|exact|, 2^-14) * eps + L * 1e-6 + (|act(g)| + |r|) * 2^-22 + 1e-6,      eps = 2^-11 (fp16) or 2^-7 (bf16)

one rounding to the output type at the result's magnitude; the project's absolute slack of 1e-6 on the sum (tests/test_gpu_linear.py)
carried through the activation, whose slope is at most L (1 for identity and relu, max |silu'| = 1.0998 -> 1.1, max |gelu'| = 1.1290
-> 1.13 for both GELU forms); a few fp32 roundings of the activation's value and of the sum with the residual; 1e-6 of slack.

The first test below needs no GPU: it shows that the formulas evaluated in fp32 stay inside this gate -- without a residual, with a
random one and with one that cancels the result, r ~ -act(g) -- and that the likely mistakes fall outside it."""
import ctypes
import math

import numpy as np
import pytest

from tests import test_gpu_csr_span as CS
from tests import test_gpu_gated as GT
from tests import test_gpu_linear as TL
from tests import test_gpu_linear_bf16 as BF

gpu_test = pytest.mark.gpu
EPS = GT.EPS
LIMIT = BF.LIMIT
K, N = 1024, 456
ACTS = ("relu", "silu", "gelu", "gelu_tanh")
LIP = {None: 1.0, "relu": 1.0, "silu": 1.1, "gelu": 1.13, "gelu_tanh": 1.13}
DTYPES = ["float16", "bfloat16"]
_erf = np.vectorize(math.erf, otypes=[np.float64])


def _act64(act, g):
    """the table's formula in fp64 (non-finite values included: what IEEE arithmetic gives)"""
    with np.errstate(all="ignore"):
        if act is None:
            return g.copy()
        if act == "relu":
            return np.where(g > 0, g, np.where(g != g, g, 0.0))
        if act == "silu":
            return g / (1.0 + np.exp(-g))
        if act == "gelu":
            return 0.5 * g * (1.0 + _erf(g * 0.70710678))
        assert act == "gelu_tanh"
        return 0.5 * g * (1.0 + np.tanh(0.79788456 * (g + 0.044715 * g * g * g)))


def _act32(act, v):
    """the same formulas with every operation in fp32 (v: float32 array)"""
    import torch

    assert v.dtype == np.float32
    f = np.float32
    with np.errstate(all="ignore"):
        if act is None:
            out = v.copy()
        elif act == "relu":
            out = np.where(v > 0, v, np.where(v != v, v, f(0)))
        elif act == "silu":
            out = v / (f(1) + np.exp(-v))
        elif act == "gelu":
            out = f(0.5) * v * (f(1) + torch.erf(torch.from_numpy(v * f(0.70710678))).numpy())
        else:
            out = f(0.5) * v * (f(1) + np.tanh(f(0.79788456) * (v + f(0.044715) * v * v * v)))
    assert out.dtype == np.float32
    return out


def _gate(exact, a, r, eps, L):
    """the tolerance of the module docstring: exact = a + r, a = act(g) in fp64, r the widened residual (zeros without one)"""
    return np.maximum(np.abs(exact), 2.0 ** -14) * eps + L * 1e-6 + (np.abs(a) + np.abs(r)) * 2.0 ** -22 + 1e-6


def _res(device, rows, n, dtype, seed=0):
    import torch

    g = torch.Generator(device=device).manual_seed(1000 + rows + seed)
    return torch.randn((rows, n), device=device, generator=g).to(getattr(torch, dtype))


def _w(t):
    """a 16-bit tensor widened exactly to fp64 numpy"""
    return t.float().cpu().numpy().astype(np.float64)


_G = {}


def _sum(device, bits, kind, bias, rows, dtype, npl, x):
    """fp64 oracle sums + bias for the 16-bit activations GT._x(device, rows, dtype), computed once per key"""
    key = (str(device), bits, kind, bias, rows, dtype)
    if key not in _G:
        _G[key] = BF._exact(npl, x, kind)
    return _G[key]


def _check(y, g, act, r, dtype, where=None, note=""):
    """y against act(g) + r in the gate, printing the worst ratio first"""
    import torch

    assert y.dtype == getattr(torch, dtype)
    got = _w(y).reshape(g.shape)
    r64 = np.zeros_like(g) if r is None else _w(r).reshape(g.shape)
    a = _act64(act, g)
    sel = np.ones(g.shape, bool) if where is None else where
    assert np.isfinite(got[sel]).all(), f"{(~np.isfinite(got[sel])).sum()} non-finite outputs {note}"
    with np.errstate(invalid="ignore"):  # (outside `where` the operands may be non-finite)
        exact = a + r64
        err, tol = np.abs(got - exact)[sel], _gate(exact, a, r64, EPS[dtype], LIP[act])[sel]
    print(f"{note} act={act} residual={r is not None} {dtype}: worst error / gate = {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), f"{(err > tol).sum()} of {err.size} outputs outside the gate; worst {float((err / tol).max()):.3g} x {note}"


def _call(mod, x, act=None, residual=None, out=None):
    mod.act = act
    try:
        return mod(x, residual=residual, out=out)
    finally:
        mod.act = None


def _bits16(t):
    import torch

    return t.view(torch.int16).cpu().numpy().tobytes()


# ---- 0. the tolerance itself (no GPU) ----

@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gate_admits_the_fp32_formulas_and_rejects_the_mutants(bits, dtype):
    import torch

    from squeezellm_amd import quant

    lay, npl, _ = BF.parity_layer("cpu", bits, "hybrid", True)
    x = GT._x("cpu", 5, dtype)
    g = BF._exact(npl, x, "hybrid")
    g32 = g.astype(np.float32)
    bias = npl["bias"].astype(np.float64)
    eps = EPS[dtype]
    rnd = _w(_res("cpu", 5, N, dtype))
    for act in (None,) + ACTS:
        a, a32 = _act64(act, g), _act32(act, g32)
        draws = {"none": np.zeros_like(g), "random": rnd, "cancelling": GT._round_to(-a32, dtype)}
        for name, r in draws.items():
            exact = a + r
            tol = _gate(exact, a, r, eps, LIP[act])
            f32 = a32 + r.astype(np.float32)  # (a 16-bit value: exact in fp32)
            assert f32.dtype == np.float32
            ratio = np.abs(GT._round_to(f32, dtype) - exact) / tol
            print(f"w{bits} {dtype} act={act} residual={name}: fp32 evaluation / gate = {float(ratio.max()):.3f}")
            assert (ratio <= 1.0).all(), (act, name, float(ratio.max()))
        # the torch form of the formulas (quant._torch_epilogue: the dense route and the other dtypes) is the same fp32 evaluation
        t32 = quant._torch_epilogue(torch.from_numpy(g32), act, torch.from_numpy(rnd.astype(np.float32)), torch.float32).numpy()
        assert t32.dtype == np.float32 and (np.abs(t32 - (a32 + rnd.astype(np.float32))) <= (np.abs(a32) + np.abs(rnd)) * 2.0 ** -22 + 1e-7).all()
        # the mistakes, on the random residual: share of the outputs they put outside the gate
        exact = a + rnd
        tol = _gate(exact, a, rnd, eps, LIP[act])
        r32 = rnd.astype(np.float32)

        def outside(f32, among=None):
            bad = np.abs(GT._round_to(f32.astype(np.float32), dtype) - exact) > tol
            return float(bad.mean() if among is None else bad[among].mean())

        g0 = (g - bias).astype(np.float32)
        # (relu cannot show a dropped bias where the argument is negative with and without it: those outputs are the residual
        # either way -- the share is taken among the others.  The residual added first shows everywhere but where g and g + r
        # are both positive: that share is taken among all outputs)
        before = g32 + r32
        vis_before = None
        vis_bias = None if act != "relu" else (g32 > 0) | (g0 > 0)
        shares = {"dropped residual": outside(a32)}
        # (the dropped bias is shown without a residual: a residual of magnitude 1 raises the result's bf16 rounding step above
        # most of the biases, which are a few hundredths)
        exact, tol = a, _gate(a, a, np.zeros_like(a), eps, LIP[act])
        shares["dropped bias"] = outside(_act32(act, g0), vis_bias)
        exact, tol = a + rnd, _gate(a + rnd, a, rnd, eps, LIP[act])
        if act is not None:  # (identity: the same sum either way)
            shares["residual before the activation"] = outside(_act32(act, before), vis_before)
        print(f"w{bits} {dtype} act={act}: outside the gate {shares}")
        assert all(s > 0.5 for s in shares.values()), (act, shares)
    # an fmaxf-style relu loses a NaN; the table's formula keeps it
    v = np.array([np.nan, -1.0, 2.0, -np.inf, np.inf], np.float32)
    assert not np.isnan(np.fmax(v, np.float32(0))).any()
    for got in (_act32("relu", v), _act64("relu", v.astype(np.float64))):
        assert np.isnan(got[0]) and got[1] == 0 and got[2] == 2 and got[3] == 0 and np.isposinf(got[4])


def test_table_of_non_finite_values_is_what_the_formulas_give():
    """include/sqllm_hip.h: the +inf / -inf / NaN columns of the table, from the fp32 formulas"""
    v = np.array([np.inf, -np.inf, np.nan], np.float32)
    want = {None: ("+inf", "-inf", "nan"), "relu": ("+inf", "0", "nan"), "silu": ("+inf", "nan", "nan"), "gelu": ("+inf", "nan", "nan"),
            "gelu_tanh": ("+inf", "nan", "nan")}
    name = lambda f: "nan" if np.isnan(f) else "+inf" if np.isposinf(f) else "-inf" if np.isneginf(f) else "0" if f == 0 else "finite"  # noqa: E731
    import torch

    from squeezellm_amd import _lib, quant

    assert quant._EP_ACT == {None: _lib.ACT_IDENTITY, "relu": _lib.ACT_RELU, "silu": _lib.ACT_SILU, "gelu": _lib.ACT_GELU, "gelu_tanh": _lib.ACT_GELU_TANH}
    for act, row in want.items():
        assert tuple(name(f) for f in _act32(act, v)) == row == tuple(name(f) for f in _act64(act, v.astype(np.float64))), act
        assert tuple(name(f) for f in quant._torch_epilogue(torch.from_numpy(v), act, None, torch.float32).numpy()) == row, act
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.float32(np.inf) + np.float32(-np.inf))


# ---- 1. parity ----

def _parity(gpu, bits, kind, rows, bias, dtype, act, with_residual):
    lay, npl, mag = BF.parity_layer(gpu, bits, kind, bias)
    mod = BF._fused(lay)
    x = GT._x(gpu, rows, dtype)
    assert (BF._abs_sum(npl, mag, x) < LIMIT).all()  # every partial sum is in range: no non-finite result is admissible
    g = _sum(gpu, bits, kind, bias, rows, dtype, npl, x)
    r = _res(gpu, rows, N, dtype) if with_residual else None
    xin, rin = (x, r) if rows > 1 else (x.reshape(1, 1, K), None if r is None else r.reshape(1, 1, N))
    for rep in range(3):  # the second and third call run on the workspace the previous one left behind
        y = _call(mod, xin, act, rin)
        assert y.shape == (*xin.shape[:-1], N) and mod.last_route == "fused_ep"
        _check(y.reshape(rows, N), g, act, r, dtype, note=f"w{bits} {kind} rows={rows} bias={bias}")
    BF._workspaces_clean(mod)


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("bits", [3, 4])
def test_every_activation_with_and_without_residual(gpu, bits, act, with_residual, rows, dtype):
    _parity(gpu, bits, "hybrid", rows, True, dtype, act, with_residual)


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("kind", ["dense", "spmv", "hybrid"])
@pytest.mark.parametrize("bits", [3, 4])
def test_batch_tiles_and_grid_rows(gpu, bits, kind, bias, dtype):
    """rows 1, 2, 3, 5, 8: the batch tiles 1, 2, 4 (three rows of it), 8 (five rows of it), 8; 9: a second grid row of one batch row"""
    for rows in (1, 2, 3, 5, 8, 9):
        _parity(gpu, bits, kind, rows, bias, dtype, "relu", True)


# ---- 2. in place, identity ----

@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5, 9])
@pytest.mark.parametrize("bits", [3, 4])
def test_in_place_equals_out_of_place(gpu, bits, rows, dtype):
    """out is residual: h += act(linear(x)).  The dense layer: its sum is a sum of fixed-point words, the same in every run"""
    lay, npl, mag = BF.parity_layer(gpu, bits, "dense", True)
    mod = BF._fused(lay)
    x = GT._x(gpu, rows, dtype)
    r = _res(gpu, rows, N, dtype)
    for act in (None, "gelu"):
        want = _call(mod, x, act, r)
        assert want.data_ptr() != r.data_ptr()
        h = r.clone()
        y = _call(mod, x, act, h, out=h)
        assert y is h and mod.last_route == "fused_ep"
        assert _bits16(h) == _bits16(want)
        _check(h, _sum(gpu, bits, "dense", True, rows, dtype, npl, x), act, r, dtype)
    BF._workspaces_clean(mod)


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("bits", [3, 4])
def test_identity_without_residual_is_the_plain_linear(gpu, bits, rows, dtype):
    """bf16: the same range rule, bit for bit.  fp16: the plain linear clamps where this one flags, so bit for bit wherever every
    contribution is in range -- asserted of these operands"""
    import torch

    lay, npl, mag = BF.parity_layer(gpu, bits, "dense", True)
    mod = BF._fused(lay)
    x = GT._x(gpu, rows, dtype)
    assert (BF._abs_sum(npl, mag, x) < LIMIT).all()
    plain = mod(x)
    assert mod.last_route == "fused"
    out = torch.full((rows, N), 7.0, device=gpu, dtype=x.dtype)
    y = _call(mod, x, None, None, out=out)
    assert y is out and mod.last_route == "fused_ep"
    assert _bits16(out) == _bits16(plain)
    BF._workspaces_clean(mod)


# ---- 3. non-finite operands ----

@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", [None] + list(ACTS))
@pytest.mark.parametrize("bits", [3, 4])
def test_non_finite_operands_follow_the_table(gpu, bits, act, dtype):
    """4 rows of positive activations: row 0 has a +inf, row 1 a -inf, row 2 a NaN in x (dense weights are never zero: every sum of
    those rows is non-finite, +inf or -inf by the sign of the weight -- NaN where terms of both signs meet), row 3 is clean.  The
    residual has -inf, +inf and NaN planted on column ranges of every row.  Expected: the table's formula in fp32 on the fp32 operator
    path's sums, plus the residual -- pattern of NaN / +inf / -inf equal, finite outputs inside the gate."""
    import torch

    from squeezellm_amd import quant

    lay, npl, mag = BF.parity_layer(gpu, bits, "hybrid", True)
    rows = 4
    x = GT._x(gpu, rows, dtype, positive=True)
    exact_clean = BF._exact(npl, x, "hybrid")  # (before the poison: row 3 is compared with it)
    x[0, 37], x[1, 37], x[2, 37] = float("inf"), float("-inf"), float("nan")
    r = _res(gpu, rows, N, dtype)
    r[:, 0:48], r[:, 48:96], r[:, 96:120] = float("-inf"), float("inf"), float("nan")
    lin32 = quant.QuantLinearLUT.from_operands(lay)(x.float()).float().cpu().numpy()  # the fp32 operator path on the widened activations
    assert not np.isfinite(lin32[:3]).any() and np.isfinite(lin32[3]).all()
    assert np.isposinf(lin32[0]).any() and np.isneginf(lin32[0]).any() and np.isnan(lin32[2]).all()
    r32 = r.float().cpu().numpy()
    with np.errstate(all="ignore"):
        a32 = _act32(act, lin32)
        want = a32 + r32
    # the rows of the table are all present
    neg, pos = np.isneginf(lin32), np.isposinf(lin32)
    if act == "relu":
        assert (a32[neg] == 0).all() and neg[:, 120:].any()  # relu(-inf) = 0: the output is the residual itself
    elif act is not None:
        assert np.isnan(a32[neg]).all()
    else:
        assert np.isneginf(a32[neg]).all()
    assert np.isposinf(a32[pos]).all() and np.isnan(a32[np.isnan(lin32)]).all()
    assert np.isnan(want[:, 0:48][pos[:, 0:48]]).all() and pos[:, 0:48].any()  # +inf + (-inf) = NaN
    assert np.isnan(want[:, 96:120]).all()  # a NaN residual
    assert np.isposinf(want[3, 48:96]).all() and np.isneginf(want[3, 0:48]).all()  # finite + an infinite residual
    mod = BF._fused(lay)
    fin = np.isfinite(want)
    assert fin[3, 120:].all()
    clean = np.zeros((rows, N), bool)
    clean[3, 120:] = True
    for rep in range(2):  # second call: the flags of the first must not linger
        y = _call(mod, x, act, r)
        got = y.float().cpu().numpy()
        assert (np.isnan(got) == np.isnan(want)).all(), (int(np.isnan(got).sum()), int(np.isnan(want).sum()))
        assert (np.isposinf(got) == np.isposinf(want)).all() and (np.isneginf(got) == np.isneginf(want)).all()
        if act == "relu":  # 0 + r, r a value of the output type: exactly r
            sel = neg & fin
            assert sel.any() and (got[sel] == r32[sel]).all()
        _check(y, np.where(clean, exact_clean, 0.0), act, r, dtype, where=clean)
    BF._workspaces_clean(mod)


# ---- 4. the range rule ----

@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5])
def test_out_of_range_contribution_with_a_negative_residual_is_infinite(gpu, rows, dtype):
    """The construction of test_gpu_linear_bf16's out-of-range case: weights that are one constant per column, x = 2^14 everywhere,
    so the sum is 2^24 c; the residual is -49152 everywhere.  Columns of sum 2^24: at most 63 contributions, so every one of them
    is beyond 131072 -- the result is +inf (fp16 too: no clamp), never a finite number; of sum -2^24: -inf.  Columns in range come
    out right (16384 - 49152 = -32768)."""
    import torch

    from squeezellm_amd import synth

    n = 64
    lay = synth.make_layer(K, n, 4, device=gpu, seed=5)
    consts = np.repeat(np.array([2.0 ** -10, 1.0, -1.0, 1.0 / 16], np.float32), 16)  # 16 columns each
    lay["lookup_table"] = torch.from_numpy(np.repeat(consts[:, None], 16, axis=1).copy()).to(gpu)  # every index decodes to it
    mod = BF._fused(lay)
    dt = getattr(torch, dtype)
    x = torch.full((rows, K), 2.0 ** 14, device=gpu, dtype=dt)
    r = torch.full((rows, n), -49152.0, device=gpu, dtype=dt)
    assert float(x.float().min()) == 2.0 ** 14 and float(r.float().max()) == -49152.0
    g = np.tile(consts.astype(np.float64) * K * 2.0 ** 14, (rows, 1))
    assert g[0, 0] == 16384 and g[0, 16] == 2.0 ** 24 > 63 * LIMIT and g[0, 48] == 2.0 ** 20
    exact = g - 49152.0
    tol = _gate(exact, g, np.full_like(g, 49152.0), EPS[dtype], 1.0)
    for rep in range(2):  # (the flags of the first call must not linger)
        y = _w(_call(mod, x, None, r)).reshape(rows, n)
        assert (y[:, 0:16] == -32768.0).all(), y[0, 0:16]
        assert np.isposinf(y[:, 16:32]).all(), y[0, 16:32]  # never finite
        assert np.isneginf(y[:, 32:48]).all(), y[0, 32:48]
        mid = y[:, 48:64]  # 2^20: finite and right (bf16) or +inf -- how K is sliced decides; in fp16 +inf either way
        assert (np.isposinf(mid) | (np.abs(mid - exact[:, 48:64]) <= tol[:, 48:64])).all()
        assert dtype == "bfloat16" or np.isposinf(mid).all()
    BF._workspaces_clean(mod)


# ---- 5. workspace, capture ----

@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("bits", [3, 4])
def test_plain_and_epilogue_launches_alternate_on_one_workspace(gpu, bits, rows, dtype):
    import torch

    lay, npl, mag = BF.parity_layer(gpu, bits, "hybrid", True)
    mod = BF._fused(lay)
    x = GT._x(gpu, rows, dtype)
    g = _sum(gpu, bits, "hybrid", True, rows, dtype, npl, x)
    r = _res(gpu, rows, N, dtype)
    for i, act in enumerate((None, "silu", None, "gelu_tanh", "relu", None)):
        if i % 2 == 0:
            y = mod(x)
            assert mod.last_route == "fused"
            _check(y, g, None, None, dtype)
        else:
            y = _call(mod, x, act, r)
            assert mod.last_route == "fused_ep"
            _check(y, g, act, r, dtype)
        torch.cuda.synchronize()
        assert len([k for k in mod._ws if k != "retired" and k[1] != "graph"]) == 1  # one workspace for both entry points
        BF._workspaces_clean(mod)
    assert len(mod._desc) == 1 and len(mod._ep_desc) == 1


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 5])
def test_captured_epilogue_forward_holds_its_kernel_only(gpu, rows, dtype):
    """as tests/test_gpu_gated.py: after one eager call of that size, a captured forward with activation and residual is ONE kernel
    node (no zero fill, no memory node); replays equal the eager result bit for bit."""
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

    lay, npl, mag = BF.parity_layer(gpu, 4, "dense", True)  # (dense: the same bits in every run)
    mod = BF._fused(lay)
    mod.act = "gelu"
    x = GT._x(gpu, rows, dtype)
    r = _res(gpu, rows, N, dtype)
    out = torch.zeros((rows, N), device=gpu, dtype=x.dtype)

    def run():
        with torch.no_grad():
            mod(x, residual=r, out=out)

    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    want = out.clone()
    _check(want, _sum(gpu, 4, "dense", True, rows, dtype, npl, x), "gelu", r, dtype)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        run()
    assert node_types(g) == [0]  # hipGraphNodeTypeKernel: the epilogue kernel and nothing else
    g.instantiate()
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert _bits16(out) == _bits16(want)
    BF._workspaces_clean(mod)


# ---- 6. the CSR span classes ----

@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 3, 8])
@pytest.mark.parametrize("bits", [3, 4])
def test_span_ladder_with_gelu_and_residual(gpu, bits, rows, dtype):
    """ladder "a" of tests/test_gpu_csr_span.py (K = 512, N = 8192: chunks in one group, in row groups and in the fallback at the
    linears' span limit of 2048 rows) under the epilogue policy; a failure names the span classes of the failing columns"""
    import torch

    lay, npl, mag = CS.ladder_layer(gpu, bits, "a")
    x = CS._x(gpu, rows, dtype)
    assert (BF._abs_sum(npl, mag, x) < LIMIT).all()
    g = CS._sum(gpu, bits, "a", 0, x, (rows, dtype, False))
    r = _res(gpu, rows, CS.N, dtype)
    mod = CS._linear_module(lay)
    labels2 = CS._tile_labels("linear", rows, "a")
    assert any(CS.CLASSES[2] in s for s in labels2.ravel()) and (rows == 1 or any(CS.CLASSES[1] in s for s in labels2.ravel()))
    for rep in range(3):
        y = _call(mod, x if rows > 1 else x.reshape(1, 1, CS.K), "gelu", r if rows > 1 else r.reshape(1, 1, CS.N))
        assert mod.last_route == "fused_ep"
        try:
            _check(y.reshape(rows, CS.N), g, "gelu", r, dtype)
        except AssertionError as e:
            a = _act64("gelu", g)
            bad = ~(np.abs(_w(y).reshape(g.shape) - (a + _w(r))) <= _gate(a + _w(r), a, _w(r), EPS[dtype], LIP["gelu"]))
            raise AssertionError(f"{e} -- by span class: {CS._by_class2(bad, labels2)}") from None
    CS._descriptor_csr(next(iter(mod._ep_desc.values()))[1][0].lin.op, lay, 0)
    BF._workspaces_clean(mod)


# ---- 7. the module ----

@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
def test_module_surface(gpu, dtype):
    import torch

    from squeezellm_amd import quant

    assert quant.QuantLinearLUTFused.act is None
    lay, npl, mag = BF.parity_layer(gpu, 4, "hybrid", True)
    mod = BF._fused(lay)
    rows = 5
    x = GT._x(gpu, rows, dtype)
    g = _sum(gpu, 4, "hybrid", True, rows, dtype, npl, x)
    r = _res(gpu, rows, N, dtype)
    # no epilogue: today's path
    y = mod(x)
    assert mod.last_route == "fused" and "_ep_desc" not in mod.__dict__
    _check(y, g, None, None, dtype)
    # residual alone; a 3-D input; act as an instance attribute
    y = mod(x, residual=r)
    assert mod.last_route == "fused_ep" and y.shape == (rows, N) and y.data_ptr() != r.data_ptr()
    _check(y, g, None, r, dtype)
    y3 = mod(x.reshape(1, rows, K), residual=r.reshape(1, rows, N))
    assert y3.shape == (1, rows, N)
    _check(y3.reshape(rows, N), g, None, r, dtype)
    mod.act = "relu"
    y = mod(x)
    assert mod.last_route == "fused_ep"
    _check(y, g, "relu", None, dtype)
    out = torch.empty((rows, N), device=gpu, dtype=x.dtype)
    assert mod(x, residual=r, out=out) is out
    _check(out, g, "relu", r, dtype)
    # bad arguments
    other = torch.float16 if dtype == "bfloat16" else torch.bfloat16
    bad = [dict(residual=r.to(other)), dict(residual=r[:, :-4]), dict(residual=r[:4]), dict(residual=r.t().contiguous().t()), dict(residual=r.cpu()),
           dict(out=out.to(other)), dict(out=out[:, :-4]), dict(out=out.cpu()), dict(residual=r.reshape(1, rows, N)), dict(residual=1.0)]
    both = torch.empty((rows + 1, N), device=gpu, dtype=x.dtype)
    bad.append(dict(residual=both[:rows], out=both[1:]))  # a partial overlap
    for kw in bad:
        with pytest.raises(ValueError):
            mod(x, **kw)
    with pytest.raises(ValueError):
        mod(x[:, :-32].contiguous(), residual=r)
    mod.act = "tanh"
    with pytest.raises(ValueError):
        mod(x)
    mod.act = None
    _check(mod(x), g, None, None, dtype)
    assert mod.last_route == "fused"
    BF._workspaces_clean(mod)


@gpu_test
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", [None] + list(ACTS))
def test_dense_route_applies_the_epilogue_within_the_gate(gpu, act, dtype):
    """dense_min_rows = 4, 5 rows: the layer's matrix in fp32, torch's fp32 GEMM, then bias, activation and residual in fp32 with
    one rounding -- against the reference and the gate of the kernel, with and without a residual and into `out`.  3 rows stay
    on the kernel.  (With the 16-bit matrix and GEMM of the route without an epilogue the gate cannot hold: weights and sum are
    rounded before the epilogue sees them.  Measured so on an MI355X: 5 - 23 % of the outputs outside it, by up to 209 x.)"""
    lay, npl, mag = BF.parity_layer(gpu, 4, "hybrid", True)
    mod = BF._fused(lay)
    mod.dense_min_rows = 4
    x = GT._x(gpu, 5, dtype)
    g = _sum(gpu, 4, "hybrid", True, 5, dtype, npl, x)
    r = _res(gpu, 5, N, dtype)
    y3 = _call(mod, x[:3].contiguous(), act, r[:3].contiguous())
    assert mod.last_route == "fused_ep"
    _check(y3, g[:3], act, r[:3], dtype, note="kernel")
    for res in (r, None):  # (without a residual into `out`: with act None, no residual and no out the call has no epilogue)
        y = _call(mod, x, act, res, out=None if res is not None else x.new_empty((5, N)))
        assert mod.last_route == "dense" and y.dtype == x.dtype and y.shape == (5, N)
        _check(y, g, act, res, dtype, note="dense route")
    plain = mod(x)  # no epilogue: the 16-bit dense route, as before
    assert mod.last_route == "dense" and plain.dtype == x.dtype


@gpu_test
@pytest.mark.parametrize("act", [None, "silu", "gelu_tanh"])
def test_fp32_input_takes_the_parents_path_and_torch(gpu, act):
    """fp32 activations: QuantLinearLUT.forward, then activation and residual in torch -- against the reference of the kernel on
    the same (bf16-representable) operands, inside the kernel's gate for bf16 outputs, and so within twice that gate of the kernel"""
    import torch

    lay, npl, mag = BF.parity_layer(gpu, 4, "hybrid", True)
    mod = BF._fused(lay)
    x16 = GT._x(gpu, 5, "bfloat16")
    r16 = _res(gpu, 5, N, "bfloat16")
    g = _sum(gpu, 4, "hybrid", True, 5, "bfloat16", npl, x16)
    y32 = _call(mod, x16.float(), act, r16.float())
    assert y32.dtype == torch.float32 and y32.shape == (5, N) and "_ws" not in mod.__dict__
    a = _act64(act, g)
    exact, r64 = a + _w(r16), _w(r16)
    tol = _gate(exact, a, r64, EPS["bfloat16"], LIP[act])
    err = np.abs(y32.cpu().numpy().astype(np.float64) - exact)
    print(f"fp32 path act={act}: worst error / gate = {float((err / tol).max()):.3f}")
    assert (err <= tol).all()
    yk = _call(mod, x16, act, r16)
    assert mod.last_route == "fused_ep"
    _check(yk, g, act, r16, "bfloat16")
    assert (np.abs(_w(yk) - y32.cpu().numpy().astype(np.float64)) <= 2 * tol).all()
    out = torch.empty_like(y32)
    assert _call(mod, x16.float(), act, r16.float(), out=out) is out
    assert (np.abs(out.cpu().numpy().astype(np.float64) - exact) <= tol).all()


@gpu_test
def test_fuse_gated_mlps_installs_forward_residual(gpu):
    import torch
    import torch.nn as nn

    from squeezellm_amd import quant, synth

    class MLP(nn.Module):
        def __init__(self, fused_down):
            super().__init__()
            lays = [synth.make_layer(256, 224, 4, sparse_frac=0.02, topX=3, heavy_rows=2, bias=True, device=gpu, seed=710 + j) for j in range(2)]
            self.gate_proj, self.up_proj = (quant.QuantLinearLUT.from_operands(lay) for lay in lays)
            self.down_lay = synth.make_layer(224, 64, 4, sparse_frac=0.02, heavy_rows=1, bias=True, device=gpu, seed=930)
            self.down_proj = quant.QuantLinearLUT.from_operands(self.down_lay)
            if fused_down:
                quant.fuse_quant_lut(self.down_proj)
            self.act_fn = nn.SiLU()

        def forward(self, x):
            return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))

    toy = nn.ModuleList([MLP(True), MLP(False)])
    keys = list(toy.state_dict().keys())
    assert quant.fuse_gated_mlps(toy) == 2
    assert list(toy.state_dict().keys()) == keys
    assert "forward_residual" in toy[0].__dict__ and "forward_residual" not in toy[1].__dict__  # (a plain down projection: left alone)
    m = toy[0]
    x = GT._x(gpu, 5, "float16")[:, :256].contiguous()
    r = _res(gpu, 5, 64, "float16")
    h = m.__dict__["gated"](x)
    y = m.forward_residual(x, r)
    assert m.down_proj.last_route == "fused_ep" and y.shape == (5, 64) and y.dtype == torch.float16
    g = BF._exact(TL._npl(m.down_lay), h, "spmv")  # the down projection's fp64 sum on the front the kernel was given
    _check(y, g, None, r, "float16")
    assert torch.equal(m(x), m.down_proj(h))  # the plain forward is what it was
    BF._workspaces_clean(m.down_proj)
