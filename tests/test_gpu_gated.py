"""Tests of the gated fused linear (sqllm_gated_f16 / sqllm_gated_bf16 behind quant.QuantGatedLUTFused): silu(gate(x)) * up(x)
as one kernel.  Modelled on tests/test_gpu_linear_bf16.py, whose layer construction and helpers it reuses.

Gate and up are two different synth.make_layer layers (different seeds, different biases: a swap of the roles fails) of the
project's parity shape, K = 1024, N = 456 (ragged last column tile); with sparse_frac = 0.01 plus two heavy rows the CSR
exceeds one 1024-non-zero chunk, so rows spread over two chunks occur.

Reference: silu(g) * u in fp64, g and u the fp64 oracle sums of tests/helpers.py on the exactly widened activations plus
the biases.  Tolerance: one rounding to the output type at the result's magnitude plus the project's absolute slack of 1e-6
per sum (tests/test_gpu_linear.py), propagated through the product with |silu'| <= 1.1:

    max(|exact|, 2^-14) * eps + (1.1 |u| + |silu(g)|) * 1e-6 + 1e-6,      eps = 2^-11 (fp16) or 2^-7 (bf16)

The first test below needs no GPU: it shows in numpy that the formula evaluated in fp32 on fp32-rounded g, u stays inside
this gate for the operands drawn here, and that swapped roles and a dropped bias fall outside it on most elements."""
import ctypes

import numpy as np
import pytest

from tests import test_gpu_dequant as DQ
from tests import test_gpu_linear as TL
from tests import test_gpu_linear_bf16 as BF

gpu_test = pytest.mark.gpu
EPS = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -7}
LIMIT = BF.LIMIT
K, N = 1024, 456
KINDS = {"dense": ("dense", "dense"), "spmv": ("spmv", "spmv"), "hybrid": ("hybrid", "hybrid"), "mixed": ("dense", "hybrid")}


def _silu(g):
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g))


def _gate(g, u, eps):
    """the tolerance of the module docstring for fp64 sums g, u"""
    return np.maximum(np.abs(_silu(g) * u), 2.0 ** -14) * eps + (1.1 * np.abs(u) + np.abs(_silu(g))) * 1e-6 + 1e-6


def _chain_bound(g, u, Eg, Eu, e):
    """|out - silu(g) u| for a front computed step by step in a 16-bit type of ulp e: sums known to Eg, Eu, then silu and the
    product rounded one by one (|silu'| <= 1.1; the term in 2 e: those two roundings)"""
    s = np.abs(_silu(g))
    return 1.1 * Eg * (np.abs(u) + Eu) + s * Eu + 2 * e * (s + 1.1 * Eg) * (np.abs(u) + Eu) + 2.0 ** -24


def _round_to(v32, dtype):
    """fp32 -> the output type (round to nearest even) -> fp64"""
    if dtype == "float16":
        return v32.astype(np.float16).astype(np.float64)
    b = v32.astype(np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).astype(np.float64)


_PAIRS = {}


def pair_layers(device, bits, kind, bias):
    """(gate, up), each (torch operands, numpy operands, sum of |terms| per weight, oracle kind): one pair per (bits, kind, bias),
    shared by the row counts and the output types; the construction of test_gpu_linear_bf16.parity_layer with two seeds"""
    from squeezellm_amd import synth

    key = (str(device), bits, kind, bias)
    if key not in _PAIRS:
        out = []
        for k, seed in zip(KINDS[kind], (31 * bits + 7, 31 * bits + 1007)):
            lay = synth.make_layer(K, N, bits, sparse_frac=0.0 if k == "dense" else 0.01, topX=3 if k == "hybrid" else 0,
                                   heavy_rows=2 if k != "dense" else 0, bias=bias, device=device, seed=seed)
            npl = TL._npl(lay)
            out.append((lay, npl, DQ.expected(npl)[3], k))
        _PAIRS[key] = tuple(out)
    return _PAIRS[key]


def _x(device, rows, dtype, positive=False):
    import torch

    g = torch.Generator(device=device).manual_seed(rows)
    x = torch.randn((rows, K), device=device, generator=g)
    return (x.abs() + 0.25 if positive else x).to(getattr(torch, dtype))


_SUMS = {}


def _sums(pair, x, key=None):
    """fp64 (g, u) for the 16-bit activations x, computed once per key"""
    if key is None or key not in _SUMS:
        val = tuple(BF._exact(npl, x, k) for _, npl, _, k in pair)
        if key is None:
            return val
        _SUMS[key] = val
    return _SUMS[key]


def _module(pair, fused_members=False):
    from squeezellm_amd import quant

    mods = [quant.QuantLinearLUT.from_operands(lay) for lay, _, _, _ in pair]
    if fused_members:
        for m in mods:
            quant.fuse_quant_lut(m)
    return quant.QuantGatedLUTFused(*mods)


def _check(y, g, u, dtype, where=None):
    import torch

    assert y.dtype == getattr(torch, dtype)
    got = y.float().cpu().numpy().astype(np.float64).reshape(g.shape)
    sel = np.ones(g.shape, bool) if where is None else where
    assert np.isfinite(got[sel]).all(), f"{(~np.isfinite(got[sel])).sum()} non-finite outputs"
    err, tol = np.abs(got - _silu(g) * u)[sel], _gate(g, u, EPS[dtype])[sel]
    assert (err <= tol).all(), f"{(err > tol).sum()} of {err.size} outputs outside the gate; worst {float((err / tol).max()):.3g} x"


def _workspaces_clean(mod):
    import torch

    bufs = [v for v in mod._ws.values() if isinstance(v, torch.Tensor)] + list(mod._ws.get("retired", []))
    assert bufs
    for ws in bufs:
        assert int(ws.count_nonzero()) == 0, "workspace must be left zero-filled"


# ---- 0. the tolerance itself (no GPU) ----

@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_gate_admits_the_fp32_formula_and_rejects_the_mutants(bits, dtype):
    pair = pair_layers("cpu", bits, "hybrid", True)
    x = _x("cpu", 5, dtype)
    g, u = _sums(pair, x)
    tol = _gate(g, u, EPS[dtype])
    exact = _silu(g) * u
    g32, u32 = g.astype(np.float32), u.astype(np.float32)
    with np.errstate(over="ignore"):
        f32 = (g32 / (np.float32(1) + np.exp(-g32))) * u32
    assert f32.dtype == np.float32
    assert (np.abs(_round_to(f32, dtype) - exact) <= tol).all()
    # swapped roles: silu(u) * g
    assert (np.abs(_round_to((_silu(u) * g).astype(np.float32), dtype) - exact) > tol).mean() > 0.5
    # dropped bias (the gate's): g without bias_gate
    g0 = g - pair[0][1]["bias"].astype(np.float64)
    assert (np.abs(_round_to((_silu(g0) * u).astype(np.float32), dtype) - exact) > tol).mean() > 0.5


# ---- 1. parity ----

@gpu_test
def test_parity_cases_include_several_k_slices(gpu):
    """sqllm_plan_query plans ONE op on the operator route; the gated launch is a two-op group of the fused linear, whose
    planner shares the workgroup target between the members.  So this shows that the shape slices K for a single op (w4: four
    slices), not what the pair's plan is.  What the counted completion needs is checked where it is certain: the w4 pair is
    run once more with option target_wgs raised so far that every tile is cut into the smallest slices the planner makes."""
    from squeezellm_amd import _lib

    slices = []
    for bits in (3, 4):
        for kind in ("dense", "spmv", "hybrid"):
            lay = pair_layers(gpu, bits, kind, False)[0][0]
            nnz = 0 if lay["vals"] is None else lay["vals"].numel()
            assert kind == "dense" or nnz > 1024  # more than one CSR chunk
            for rows in (1, 2, 5, 8, 19):
                slices.append(_lib.plan_query(bits, K, N, 0 if rows == 1 else rows, nnz, 3 if kind == "hybrid" else 0)["k_slices"])
    assert max(slices) >= 2, slices


def _parity(gpu, bits, kind, rows, bias, dtype):
    pair = pair_layers(gpu, bits, kind, bias)
    mod = _module(pair)
    x = _x(gpu, rows, dtype)
    for _, npl, mag, _ in pair:
        assert (BF._abs_sum(npl, mag, x) < LIMIT).all()  # every partial sum is in range: no non-finite result is admissible
    g, u = _sums(pair, x, (bits, kind, rows, bias, dtype))
    for rep in range(3):  # the second and third call run on the workspace the previous one left behind
        y = mod(x if rows > 1 else x.reshape(1, 1, K))
        assert y.shape[-1] == N and mod.last_route == "gated"
        _check(y.reshape(rows, N), g, u, dtype)
    _workspaces_clean(mod)


@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("rows", [1, 2, 5, 8, 19])
@pytest.mark.parametrize("kind", ["dense", "spmv", "hybrid"])
@pytest.mark.parametrize("bits", [3, 4])
def test_gated_forward_matches_oracle_and_cleans_up(gpu, bits, kind, rows, bias, dtype):
    _parity(gpu, bits, kind, rows, bias, dtype)


@gpu_test
@pytest.mark.parametrize("rows", [1, 5])
def test_gated_forward_with_many_k_slices(gpu, rows):
    """target_wgs = 4096: more workgroups asked for than the shape has 32-unit slices (8 column tiles x 4), so each member's
    tiles are cut into the four slices a w4 op of K = 1024 can have -- a column completes after four dense contributions
    and its CSR chunks, whoever comes last"""
    from squeezellm_amd import _lib

    old = _lib.get_option("target_wgs")
    _lib.set_option("target_wgs", 4096)
    try:
        _parity(gpu, 4, "hybrid", rows, True, "float16")
    finally:
        _lib.set_option("target_wgs", old)


@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_gated_forward_with_mixed_members(gpu, dtype):
    """gate dense-only, up with CSR and top-X rows"""
    _parity(gpu, 4, "mixed", 5, True, dtype)


# ---- 2. bit-reproducible ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("bits", [3, 4])
def test_gated_forward_is_bit_reproducible(gpu, bits, rows, dtype):
    """Five calls, bit for bit.  (A CSR row of more than 256 non-zeros -- a heavy row, a top-X row folded into the CSR -- is held
    by three and more waves of a chunk; their fp32 sums meet in wave order in the gated kernels, csr_role with kOrderedCsr.  Added
    in arrival order, as the linears add them, one output of 2280 differed by one fp16 ulp within 20 calls of [3-5-float16].)"""
    import torch

    pair = pair_layers(gpu, bits, "hybrid", True)
    mod = _module(pair)
    x = _x(gpu, rows, dtype)
    ys = [mod(x).clone() for _ in range(5)]
    torch.cuda.synchronize()
    for y in ys[1:]:
        assert torch.equal(y.view(torch.int16), ys[0].view(torch.int16))
    _check(ys[0], *_sums(pair, x, (bits, "hybrid", rows, True, dtype)), dtype)


@gpu_test
def test_twenty_calls_of_the_long_row_case_are_identical(gpu):
    """[3-5-float16] of the test above, the case with an output on a rounding boundary, four times as often; the pair has CSR rows
    of more than 256 non-zeros in both members"""
    import torch

    from squeezellm_amd import quant

    pair = pair_layers(gpu, 3, "hybrid", True)
    mod = _module(pair)
    for m in (mod.gate, mod.up):
        rows = quant.QuantLinearLUTFused._csr_with_topx(m)[0].long()
        assert int(((rows[1:] - rows[:-1]) > 256).sum()) >= 3
    x = _x(gpu, 5, "float16")
    ys = torch.stack([mod(x).view(torch.int16) for _ in range(20)])
    torch.cuda.synchronize()
    assert bool((ys == ys[0]).all())


# ---- 3. non-finite operands ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("poison", ["nan_x", "+inf_gate", "-inf_gate", "+inf_up_zero_gate"])
@pytest.mark.parametrize("bits", [3, 4])
def test_gated_nonfinite_operands_follow_the_fp32_formula(gpu, bits, poison, rows, dtype):
    """Activations are positive here, so that an infinite codebook entry gives an infinite sum of ONE sign (with mixed
    signs every such column is NaN whatever the rule).  The NaN / +inf / -inf pattern is that of torch's silu(g32) * u32."""
    import torch

    from squeezellm_amd import synth

    # fresh layers (they are edited): a dense-only gate, an up with CSR and top-X rows
    lay_g = synth.make_layer(K, N, bits, bias=True, device=gpu, seed=400 + bits)
    lay_u = synth.make_layer(K, N, bits, sparse_frac=0.01, topX=3, heavy_rows=2, bias=True, device=gpu, seed=500 + bits)
    x = _x(gpu, rows, dtype, positive=True)
    cols = [5, 64, 200, 455]
    if poison == "nan_x":
        x[rows - 1, 37] = float("nan")
    elif poison == "+inf_gate":
        lay_g["lookup_table"][cols, 2] = float("inf")
    elif poison == "-inf_gate":
        lay_g["lookup_table"][cols, 2] = float("-inf")
    else:  # g == 0 exactly on these columns (zero codebook, zero bias, no sparse terms in the gate), u = +inf there
        lay_g["lookup_table"][cols, :] = 0.0
        lay_g["bias"][cols] = 0.0
        lay_u["lookup_table"][cols, 1] = float("inf")
    pair = ((lay_g, TL._npl(lay_g), None, "dense"), (lay_u, TL._npl(lay_u), None, "hybrid"))
    with np.errstate(all="ignore"):
        g, u = _sums(pair, x)
    want = torch.nn.functional.silu(torch.from_numpy(g.astype(np.float32))) * torch.from_numpy(u.astype(np.float32))
    hit = ~torch.isfinite(want)
    if poison == "nan_x":
        assert hit[rows - 1].all() and not hit[: rows - 1].any() and torch.isnan(want[rows - 1]).all()
    else:
        assert hit[:, cols].all() and int(hit.sum()) == rows * len(cols)
        if poison == "+inf_gate":
            assert torch.isinf(want[:, cols]).all()  # silu(+inf) = +inf, times u: the infinity of u's sign
        else:
            assert torch.isnan(want[:, cols]).all()  # silu(-inf) = NaN; 0 * inf = NaN
    mod = _module(pair)
    fin = torch.isfinite(want).numpy()
    with np.errstate(all="ignore"):
        gf, uf = np.where(fin, g, 0.0), np.where(fin, u, 0.0)
    for rep in range(2):  # second call: the flags and pair words of the first must not linger
        y = mod(x if rows > 1 else x.reshape(1, 1, K)).reshape(rows, N)
        got = y.float().cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(torch.isposinf(got), torch.isposinf(want)) and torch.equal(torch.isneginf(got), torch.isneginf(want))
        _check(y, gf, uf, dtype, where=fin)
    _workspaces_clean(mod)


@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 3, 8])
@pytest.mark.parametrize("cls", ["V", "C"])
@pytest.mark.parametrize("kind", ["dense", "hybrid"])
@pytest.mark.parametrize("bits", [3, 4])
def test_gated_nonfinite_operands_where_the_masked_lanes_run(gpu, bits, kind, cls, rows, dtype):
    """K = 544, N = 132 (dead slots at the end of every slice, a partial last column tile).  The up member carries the poison class of
    tests/nonfinite_cases.py -- V: +inf at K - 1, -inf at k = 0 and NaN at K - 32 of the shared activations, in different rows; C: +inf,
    -inf and NaN codebook entries in three columns under strictly positive activations --, the gate is a finite dense layer.  Expected
    pattern: the term-wise model of that module for g and for u (order-independent, proved against the fp64 oracle on the CPU), put
    through silu(g) * u: NaN where g is NaN or -inf or u is NaN; otherwise infinite where g is +inf or u is infinite, with the sign of
    g (of +inf) times the sign of u -- signs of finite sums from the fp64 oracle.  Not compared against another path of the library."""
    import torch

    from tests import helpers as H
    from tests import nonfinite_cases as NC

    c = NC.linear_case(bits, kind, rows, cls, NC.to_fp16 if dtype == "float16" else NC.to_bf16)
    Kn, Nn = NC.LINEAR_SHAPE
    gate = H.make_case(bits, Kn, Nn, seed=900 + bits)
    bias_g = np.random.default_rng(901 + bits).normal(0, NC.LINEAR_SCALE, Nn).astype(np.float32)
    lay_g = dict(H.to_torch(gate, gpu), bias=torch.from_numpy(bias_g.copy()).to(gpu))
    lay_u = dict(H.to_torch(NC.writable(c["case"]), gpu), bias=torch.from_numpy(c["bias"].copy()).to(gpu))
    pair = ((lay_g, dict(gate, bias=bias_g), None, "dense"), (lay_u, dict(c["case"], bias=c["bias"]), None, kind))
    x = torch.from_numpy(c["x16"].copy()).to(gpu).to(getattr(torch, dtype))
    with np.errstate(all="ignore"):
        g, u = _sums(pair, x)
    gn, gp, gm = NC.pattern_model(gate, c["x16"], np.broadcast_to(bias_g, (rows, Nn)), "dense")
    un, up, um = c["nan"], c["pos"], c["neg"]
    for model, exact in (((gn, gp, gm), g), ((un, up, um), u)):  # (the oracle's sums agree with the model's pattern: shown on the CPU as well)
        assert all(np.array_equal(m, e) for m, e in zip(model, NC.pattern_of(exact)))
    nan = gn | gm | un
    infinite = (gp | up | um) & ~nan
    with np.errstate(all="ignore"):
        sign = np.where(gp, 1.0, np.sign(g)) * np.where(up, 1.0, np.where(um, -1.0, np.sign(u)))
    assert (sign[infinite] != 0).all() and (cls != "C" or (infinite.sum() == 2 * rows and nan.sum() == rows))
    want = (nan, infinite & (sign > 0), infinite & (sign < 0))
    fin = ~(nan | infinite)
    with np.errstate(all="ignore"):
        gf, uf = np.where(fin, g, 0.0), np.where(fin, u, 0.0)
    mod = _module(pair)
    for rep in range(2):  # second call: the flags and pair words of the first must not linger
        y = mod(x if rows > 1 else x.reshape(1, 1, Kn)).reshape(rows, Nn)
        got_np = y.float().cpu().numpy()
        if cls == "C":  # the dense role's narrower contract (include/sqllm_hip.h): the column of a +-inf codebook entry is NaN or that infinity
            admit = np.isnan(got_np) & (up | um) & infinite
            got_np = np.where(admit, np.where(sign > 0, np.inf, -np.inf), got_np)
        got = NC.pattern_of(got_np)
        for name, a, b in zip(("NaN", "+inf", "-inf"), got, want):
            assert np.array_equal(a, b), (f"w{bits} {kind} class {cls} rows={rows} {dtype} call {rep}: {name} pattern differs in {int((a != b).sum())} outputs, "
                                          f"first at (row, col) {tuple(np.argwhere(a != b)[0])}")
        _check(y, gf, uf, dtype, where=fin)
    _workspaces_clean(mod)


# ---- 4. the range rule ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 5])
def test_gated_out_of_range_gate_is_never_finite_and_wrong(gpu, rows, dtype):
    """The construction of test_gpu_linear_bf16's out-of-range case: weights that are one constant per column, x = 2^14
    everywhere, so g = 2^24 c.  u = 2^-9 on every column: the exact product of a gate of 2^24 is 2^15, FINITE in fp16 and
    in bf16 -- a clamped gate (the fp16 linear's rule) would return a finite wrong number there.  Such a column has a
    contribution beyond 131072 (at most 63 of them), so it must come out infinite or NaN; a gate of -2^24 is -inf, whose
    silu is NaN; columns in range must come out right."""
    import torch

    from squeezellm_amd import synth

    n = 64
    lay_g = synth.make_layer(K, n, 4, device=gpu, seed=5)
    lay_u = synth.make_layer(K, n, 4, device=gpu, seed=6)
    consts = np.repeat(np.array([2.0 ** -10, 1.0, -1.0, 1.0 / 16], np.float32), 16)  # 16 columns each
    lay_g["lookup_table"] = torch.from_numpy(np.repeat(consts[:, None], 16, axis=1).copy()).to(gpu)  # every index decodes to it
    lay_u["lookup_table"] = torch.full((n, 16), 2.0 ** -33, device=gpu)
    pair = ((lay_g, None, None, "dense"), (lay_u, None, None, "dense"))
    mod = _module(pair)
    x = torch.full((rows, K), 2.0 ** 14, device=gpu, dtype=getattr(torch, dtype))
    assert float(x.float().min()) == 2.0 ** 14
    g = np.tile(consts.astype(np.float64) * K * 2.0 ** 14, (rows, 1))
    u = np.full((rows, n), 2.0 ** -33 * K * 2.0 ** 14)
    exact = _silu(g) * u
    assert g[0, 0] == 16384 and g[0, 16] == 2.0 ** 24 > 63 * LIMIT and g[0, 48] == 2.0 ** 20 and u[0, 0] == 2.0 ** -9
    assert exact[0, 0] == 32 and exact[0, 16] == 2.0 ** 15 < 65504 and exact[0, 32] == 0 and exact[0, 48] == 2.0 ** 11
    tol = _gate(g, u, EPS[dtype])
    for rep in range(2):  # (the flags of the first call must not linger)
        y = mod(x if rows > 1 else x.reshape(1, 1, K)).reshape(rows, n).float().cpu().numpy().astype(np.float64)
        ok = np.abs(y - exact) <= tol
        assert ok[:, 0:16].all(), y[0, 0:16]  # in range: right
        assert (~np.isfinite(y[:, 16:48])).all(), y[0, 16:48]  # a contribution beyond the range: never a finite number
        assert np.isposinf(y[:, 16:32]).all() and np.isnan(y[:, 32:48]).all()  # g = +inf: +inf * u; g = -inf: NaN
        assert (~np.isfinite(y) | ok).all()  # (columns 48..63, g = 2^20: finite and right, or +inf -- how K is sliced decides)
    _workspaces_clean(mod)


# ---- 5. capture ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_captured_gated_forward_holds_its_kernel_only(gpu, dtype):
    """as tests/test_gpu_linear.py: test_captured_module_forwards_hold_their_kernels_only -- after one eager call, a captured
    forward is ONE kernel node (no zero fill, no cast, no memory node); replays equal the eager result bit for bit."""
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

    mod = _module(pair_layers(gpu, 4, "hybrid", True), fused_members=True)
    x = _x(gpu, 1, dtype).reshape(1, 1, K)
    outs = []

    def run():
        outs.clear()
        with torch.no_grad():
            outs.append(mod(x))

    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    want = outs[0].clone()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        run()
    assert node_types(g) == [0]  # hipGraphNodeTypeKernel: the gated kernel and nothing else
    g.instantiate()
    for _ in range(2):
        outs[0].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert outs[0].dtype == want.dtype and torch.equal(outs[0].view(torch.int16), want.view(torch.int16))
    _workspaces_clean(mod)


# ---- 6. surface ----

@gpu_test
def test_fp32_input_takes_the_fallback(gpu):
    import torch

    pair = pair_layers(gpu, 4, "hybrid", True)
    mod = _module(pair)
    x = torch.randn((3, K), device=gpu)
    y = mod(x)
    assert mod.last_route == "fallback" and y.dtype == torch.float32
    g, u = mod.gate(x), mod.up(x)
    ref = torch.nn.functional.silu(g) * u
    # (the operator path adds with fp32 atomics, in no fixed order: two runs agree to the project's slack of 1e-6 per sum)
    assert ((y - ref).abs() <= 2 * ((1.1 * u.abs() + torch.nn.functional.silu(g).abs()) * 1e-6 + 1e-6)).all()
    assert "_ws" not in mod.__dict__


@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_dense_route_from_dense_min_rows(gpu, dtype):
    """dense_min_rows = 4 on the gate, 5 rows: both members go down their dense route (the layer's matrix in the
    activations' type, torch's GEMM, the bias added in fp32, each sum rounded to 16 bits), silu and the product are evaluated
    in fp32 on those two and rounded once.  The sums themselves are rounded to 16 bits here, which the gated kernel's are
    not, so the one-rounding gate cannot hold for this route by construction; the bound is derived from its steps instead.
    With e = one ulp of the type (2^-10 / 2^-7, as tests/test_gpu_linear_bf16.py: test_bf16_prefill_route takes it):
        Eg = e * (sum_k |W[n,k]| |x[b,k]| + |bias|) + e |g| + 2^-24      (rounded weights, fp32 accumulation, rounded sum), Eu alike
        |out - silu(g) u| <= 1.1 Eg (|u| + Eu) + |silu(g)| Eu + eps (|silu(g)| + 1.1 Eg) (|u| + Eu) + 2^-24
    (|silu'| <= 1.1; eps = e / 2: the one rounding of the product).  3 rows stay on the gated kernel."""
    import torch

    pair = pair_layers(gpu, 4, "hybrid", True)
    mod = _module(pair, fused_members=True)
    mod.gate.dense_min_rows = 4
    x = _x(gpu, 5, dtype)
    g, u = _sums(pair, x, (4, "hybrid", 5, True, dtype))
    y = mod(x)
    assert mod.last_route == "dense" and y.dtype == x.dtype and y.shape == (5, N)
    e = 2 * EPS[dtype]
    Eg, Eu = (e * BF._abs_sum(npl, mag, x) + e * np.abs(s) + 2.0 ** -24 for (_, npl, mag, _), s in zip(pair, (g, u)))
    s = np.abs(_silu(g))
    bound = 1.1 * Eg * (np.abs(u) + Eu) + s * Eu + EPS[dtype] * (s + 1.1 * Eg) * (np.abs(u) + Eu) + 2.0 ** -24
    err = np.abs(y.float().cpu().numpy().astype(np.float64) - _silu(g) * u)
    assert (err <= bound).all(), float((err / bound).max())
    y3 = mod(x[:3].contiguous())
    assert mod.last_route == "gated"
    _check(y3, g[:3], u[:3], dtype)


@gpu_test
def test_fuse_gated_mlps_on_a_toy_model(gpu):
    import torch
    import torch.nn as nn

    from squeezellm_amd import quant, synth

    class MLP(nn.Module):
        def __init__(self, seed, act, fused):
            super().__init__()
            # 256 -> 224 (a ragged last column tile, and a K the down projection can take) -> 64; MLP 1: a dense-only gate
            bits, kinds = (4, ("hybrid", "hybrid")) if seed == 0 else (3, ("dense", "hybrid"))
            lays = [synth.make_layer(256, 224, bits, sparse_frac=0.0 if k == "dense" else 0.02, topX=3 if k == "hybrid" else 0,
                                     heavy_rows=2 if k != "dense" else 0, bias=True, device=gpu, seed=700 + 10 * seed + j)
                    for j, k in enumerate(kinds)]
            pair = tuple((lay, TL._npl(lay), None, k) for lay, k in zip(lays, kinds))
            self.gate_proj, self.up_proj = (quant.QuantLinearLUT.from_operands(lay) for lay in lays)
            self.down_proj = quant.QuantLinearLUT.from_operands(synth.make_layer(224, 64, bits, device=gpu, seed=900 + seed))
            self.act_fn = act
            self.pair = pair
            if fused:
                quant.fuse_quant_lut(self)

        def forward(self, x):
            return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            self.layers = nn.ModuleList([MLP(0, nn.SiLU(), True), MLP(1, nn.SiLU(), False), MLP(0, nn.GELU(), True)])
            self.norm = nn.LayerNorm(8)

    toy = Toy()
    keys = list(toy.state_dict().keys())
    n_modules = len(list(toy.modules()))
    x = _x(gpu, 5, "float16")[:, :256].contiguous()
    before = [m(x) for m in toy.layers]
    assert quant.fuse_gated_mlps(toy) == 2
    assert list(toy.state_dict().keys()) == keys and len(list(toy.modules())) == n_modules
    assert "gated" not in toy.layers[2].__dict__ and "forward" not in toy.layers[2].__dict__  # another activation: left alone
    assert torch.equal(toy.layers[2](x), before[2])
    for i in (0, 1):
        m = toy.layers[i]
        gated = m.__dict__["gated"]
        assert type(gated) is quant.QuantGatedLUTFused and gated.gate is m.gate_proj and gated.up is m.up_proj
        front = gated(x)
        assert gated.last_route == "gated"
        # the MLP front against the oracle; the converted forward is the unchanged down projection of exactly that
        g, u = _sums(m.pair, x)
        _check(front, g, u, "float16")
        y = m(x)
        assert torch.equal(y, m.down_proj(front)) and y.shape == before[i].shape
        # ... and the unconverted front rounds each sum to fp16 (the plain class before it adds the bias), then silu and the
        # product: both fronts lie around the same exact value, one inside the gate, the other inside the chain's bound
        e = 2.0 ** -10
        Eg, Eu = ((np.maximum(np.abs(s), 2.0 ** -14) + np.abs(npl["bias"])) * e + 1e-6 for (_, npl, _, _), s in zip(m.pair, (g, u)))
        old = (nn.functional.silu(m.gate_proj(x)) * m.up_proj(x)).float().cpu().numpy().astype(np.float64)
        d = np.abs(front.float().cpu().numpy().astype(np.float64) - old)
        assert (d <= _chain_bound(g, u, Eg, Eu, e) + _gate(g, u, EPS["float16"])).all()
        _workspaces_clean(gated)
    assert quant.fuse_gated_mlps(nn.Linear(4, 4)) == 0


@gpu_test
def test_constructor_rejects_mismatched_members(gpu):
    import torch.nn as nn

    from squeezellm_amd import quant, synth

    mk = lambda n, bits: quant.QuantLinearLUT.from_operands(synth.make_layer(256, n, bits, device=gpu, seed=n + bits))  # noqa: E731
    with pytest.raises(ValueError, match="shape"):
        quant.QuantGatedLUTFused(mk(128, 4), mk(192, 4))
    with pytest.raises(ValueError, match="bit width"):
        quant.QuantGatedLUTFused(mk(128, 4), mk(128, 3))
    with pytest.raises(TypeError):
        quant.QuantGatedLUTFused(mk(128, 4), nn.Linear(256, 128))
    mod = quant.QuantGatedLUTFused(mk(128, 4), mk(128, 4))
    assert list(mod.state_dict().keys()) == [] and list(mod.children()) == [] and mod.last_route is None
