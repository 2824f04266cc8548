"""Tests of the attention front (sqllm_qkv_rope_f16 / sqllm_qkv_rope_bf16 behind quant.QuantQKVRopeFused): q_proj, k_proj, v_proj
and the rotary position embedding of q and k as one kernel.  Modelled on tests/test_gpu_gated.py, whose helpers it reuses.

q, k and v are three different synth.make_layer layers (three seeds, three biases) over K = 1024.  Reference: the fp64 oracle
sums of tests/helpers.py on the exactly widened activations plus the biases, rotated in fp64 by the fp32 table entries the
kernel is given.  Tolerance of a rotated element, from the formats and the project's slack (none of it from the kernel):

    max(|exact|, 2^-14) * eps + (|cos| + |sin|) * 1e-6 + (|lo cos| + |hi sin|) * 2^-22 + 1e-6,   eps = 2^-11 (fp16) or 2^-7 (bf16)

(for the pair's upper column |hi cos| + |lo sin|): one rounding to the output type; 1e-6 per sum (tests/test_gpu_linear.py),
carried through the rotation by |cos| and |sin|; the two fp32 products and the add, with or without contraction; the absolute
slack.  v is not rotated: its tolerance is the linear's, max(|exact|, 2^-14) * eps + 1e-6.

The first test needs no GPU: it shows in numpy that the fp32 formula passes in its contracted and uncontracted forms, and that
five mutants fall outside on most elements.  Tables of the parity tests hold angles drawn uniformly in [0, 2 pi) per (p, j), so
that every mutant is visible at every element."""
import ctypes

import numpy as np
import pytest

from tests import test_gpu_gated as TG
from tests import test_gpu_linear as TL
from tests import test_gpu_linear_bf16 as BF

gpu_test = pytest.mark.gpu
EPS = {"float16": 2.0 ** -11, "bfloat16": 2.0 ** -7, "float32": 2.0 ** -24}
K = 1024
N_POS = 37
# (N_q, N_k, N_v, D): ragged last tile, partners in one lane group | D no power of two, pairs straddling tile boundaries, a
# narrower v | partner exactly one tile away, grouped-query | partner half a wave away
SHAPES = {"d8": (456, 456, 456, 8), "d24": (456, 456, 132, 24), "d128": (384, 128, 128, 128), "d64": (384, 128, 128, 64)}
CONFIGS = [("d8", "half"), ("d8", "interleaved"), ("d24", "half"), ("d128", "half"), ("d128", "interleaved"), ("d64", "half")]
KINDS = {"dense": (False, False, False), "hybrid": (True, True, True), "mixed": (False, True, True)}  # sparse terms of q, k, v
# non-monotonic, the last and the first table row in front: every row count sees position n_pos - 1, two rows and more see 0
POSITIONS = [N_POS - 1, 0, 17, 5, 30, 11, 23, 2, 29, 8, 35, 14, 1, 20, 33, 6, 26, 12, 19]


# ---- operands, shared ----

_LAYERS, _SUMS, _TABLES = {}, {}, {}


def _layer(device, bits, N, sparse, member):
    """(torch operands, numpy operands, sum of |terms| per weight, oracle kind): one per (bits, width, sparse terms, member)"""
    from squeezellm_amd import synth
    from tests import test_gpu_dequant as DQ

    key = (str(device), bits, N, sparse, member)
    if key not in _LAYERS:
        lay = synth.make_layer(K, N, bits, sparse_frac=0.01 if sparse else 0.0, topX=3 if sparse else 0, heavy_rows=2 if sparse else 0,
                               bias=True, device=device, seed=31 * bits + 7 + 1000 * member)
        npl = TL._npl(lay)
        _LAYERS[key] = (lay, npl, DQ.expected(npl)[3], "hybrid" if sparse else "dense")
    return _LAYERS[key]


def _members(device, bits, kind, shape):
    return tuple(_layer(device, bits, n, sp, m) for m, (n, sp) in enumerate(zip(SHAPES[shape][:3], KINDS[kind])))


def _x(device, rows, dtype):
    return TG._x(device, rows, dtype)  # seeded by the row count


def _sums(members, x, rows, dtype):
    """fp64 (s_q, s_k, s_v) for the activations x, each computed once per layer, row count and type"""
    out = []
    for lay, npl, _, k in members:
        key = (id(npl), rows, dtype)
        if key not in _SUMS:
            _SUMS[key] = BF._exact(npl, x, k)
        out.append(_SUMS[key])
    return out


def _tables(D):
    """fp32 (cos, sin) [N_POS, D / 2] of angles uniform in [0, 2 pi), from a seeded generator"""
    if D not in _TABLES:
        ang = np.random.default_rng(1000 + D).uniform(0.0, 2 * np.pi, (N_POS, D // 2))
        _TABLES[D] = (np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32))
    return _TABLES[D]


def _identity_tables(D):
    return np.ones((N_POS, D // 2), np.float32), np.zeros((N_POS, D // 2), np.float32)


# ---- the rotation in numpy ----

def _split(v, D, layout):
    """[rows, N] -> (lo, hi), each [rows, heads, D / 2]"""
    h = v.reshape(v.shape[0], -1, D)
    return (h[..., : D // 2], h[..., D // 2:]) if layout == "half" else (h[..., 0::2], h[..., 1::2])


def _merge(lo, hi, layout):
    out = np.concatenate((lo, hi), axis=-1) if layout == "half" else np.stack((lo, hi), axis=-1)
    return out.reshape(lo.shape[0], -1)


def _at(table, pos):
    """table rows of the positions, [rows, 1, D / 2], in the table's type"""
    return table[np.asarray(pos)][:, None, :]


def _rotated(s, pos, cos, sin, D, layout, dtype):
    """(exact, tolerance) of a rotated member, both [rows, N] fp64, for fp64 sums s and the fp32 tables"""
    lo, hi = _split(s, D, layout)
    c, sn = _at(cos, pos).astype(np.float64), _at(sin, pos).astype(np.float64)
    e_lo, e_hi = lo * c - hi * sn, hi * c + lo * sn
    table = (np.abs(c) + np.abs(sn)) * 1e-6

    def tol(e, a, b):
        return np.maximum(np.abs(e), 2.0 ** -14) * EPS[dtype] + table + (np.abs(a) + np.abs(b)) * 2.0 ** -22 + 1e-6

    return _merge(e_lo, e_hi, layout), _merge(tol(e_lo, lo * c, hi * sn), tol(e_hi, hi * c, lo * sn), layout)


def _plain(s, dtype):
    return s, np.maximum(np.abs(s), 2.0 ** -14) * EPS[dtype] + 1e-6


def _f32_formula(s, pos, cos, sin, D, layout, contracted=0, sign=1.0):
    """the header's formula on fp32-rounded sums in fp32: as written (two products, one add, each rounded), or with one product
    fused into the add (1: the first one, 2: the second one -- evaluated in fp64, where an fp32 product is exact, and rounded once)"""
    lo, hi = _split(s.astype(np.float32), D, layout)
    c, sn = _at(cos, pos), _at(sin, pos) * np.float32(sign)
    assert lo.dtype == c.dtype == sn.dtype == np.float32
    with np.errstate(all="ignore"):
        if not contracted:
            o_lo, o_hi = lo * c - hi * sn, hi * c + lo * sn
            assert o_lo.dtype == np.float32
        else:
            w = lambda a: a.astype(np.float64)  # noqa: E731
            if contracted == 1:
                o_lo, o_hi = w(lo) * w(c) - w(hi * sn), w(hi) * w(c) + w(lo * sn)
            else:
                o_lo, o_hi = w(lo * c) - w(hi) * w(sn), w(hi * c) + w(lo) * w(sn)
            o_lo, o_hi = o_lo.astype(np.float32), o_hi.astype(np.float32)
    return _merge(o_lo, o_hi, layout)


def _positions(rows):
    return POSITIONS[:rows]


# ---- 0. the tolerance itself (no GPU) ----

@pytest.mark.parametrize("shape,layout", [("d8", "half"), ("d8", "interleaved"), ("d24", "half")])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("bits", [3, 4])
def test_tolerance_admits_the_fp32_formula_and_rejects_the_mutants(bits, dtype, shape, layout):
    D = SHAPES[shape][3]
    members = _members("cpu", bits, "hybrid", shape)
    rows = 5
    x = _x("cpu", rows, dtype)
    sq, sk, sv = _sums(members, x, rows, dtype)
    pos = _positions(rows)
    assert pos[0] == N_POS - 1 and pos[1] == 0 and sorted(pos) != pos
    cos, sin = _tables(D)
    other = "interleaved" if layout == "half" else "half"
    for s in (sq, sk):
        exact, tol = _rotated(s, pos, cos, sin, D, layout, dtype)
        for contracted in (0, 1, 2):
            got = TG._round_to(_f32_formula(s, pos, cos, sin, D, layout, contracted), dtype)
            assert (np.abs(got - exact) <= tol).all(), contracted
        mutants = {
            "sine term's sign flipped": _f32_formula(s, pos, cos, sin, D, layout, sign=-1.0),
            "the other layout's partner": _f32_formula(s, pos, cos, sin, D, other),
            "position off by one": _f32_formula(s, [(p + 1) % N_POS for p in pos], cos, sin, D, layout),
            "no rotation": s.astype(np.float32),
        }
        for name, m in mutants.items():
            assert (np.abs(TG._round_to(m, dtype) - exact) > tol).mean() > 0.5, name
    # v treated as a third rotated member (D divides 456; for the narrower v of d24, 132 = 5.5 heads, the first 120 columns)
    nv = sv.shape[1] // D * D
    exact, tol = _plain(sv[:, :nv], dtype)
    assert (np.abs(TG._round_to(sv[:, :nv].astype(np.float32), dtype) - exact) <= tol).all()
    m = _f32_formula(sv[:, :nv], pos, cos, sin, D, layout)
    assert (np.abs(TG._round_to(m, dtype) - exact) > tol).mean() > 0.5


# ---- helpers of the GPU tests ----

def _module(members, D, layout, fused_members=False):
    from squeezellm_amd import quant

    mods = [quant.QuantLinearLUT.from_operands(lay) for lay, _, _, _ in members]
    if fused_members:
        for m in mods:
            quant.fuse_quant_lut(m)
    return quant.QuantQKVRopeFused(*mods, head_dim=D, layout=layout)


def _dev(gpu, pos, cos, sin):
    import torch

    return (torch.tensor(list(pos), dtype=torch.int32, device=gpu), torch.from_numpy(cos.copy()).to(gpu), torch.from_numpy(sin.copy()).to(gpu))


def _np64(y, rows):
    return y.float().cpu().numpy().astype(np.float64).reshape(rows, -1)


def _inside(y, exact, tol, what, where=None):
    got = _np64(y, exact.shape[0])
    sel = np.ones(exact.shape, bool) if where is None else where
    assert np.isfinite(got[sel]).all(), f"{what}: {(~np.isfinite(got[sel])).sum()} non-finite outputs"
    err, t = np.abs(got - exact)[sel], tol[sel]
    assert (err <= t).all(), f"{what}: {(err > t).sum()} of {err.size} outputs outside the tolerance; worst {float((err / t).max()):.3g} x"


def _check(outs, sums, pos, cos, sin, D, layout, dtype, what=""):
    import torch

    for y in outs:
        assert y.dtype == getattr(torch, dtype)
    _inside(outs[0], *_rotated(sums[0], pos, cos, sin, D, layout, dtype), f"{what} q")
    _inside(outs[1], *_rotated(sums[1], pos, cos, sin, D, layout, dtype), f"{what} k")
    _inside(outs[2], *_plain(sums[2], dtype), f"{what} v")


def _clean(mod):
    TG._workspaces_clean(mod)


def _in_range(members, x):
    for _, npl, mag, _ in members:
        assert (BF._abs_sum(npl, mag, x) < BF.LIMIT).all()  # every partial sum is in range: no non-finite result is admissible


# ---- 1. parity ----

def _parity(gpu, bits, kind, rows, dtype, configs=CONFIGS):
    x = _x(gpu, rows, dtype)
    pos = _positions(rows)
    for shape, layout in configs:
        D = SHAPES[shape][3]
        members = _members(gpu, bits, kind, shape)
        _in_range(members, x)
        sums = _sums(members, x, rows, dtype)
        cos, sin = _tables(D)
        mod = _module(members, D, layout)
        tp, tc, ts = _dev(gpu, pos, cos, sin)
        for rep in range(2):  # the second call runs on the workspace the first one left behind
            outs = mod(x if rows > 1 else x.reshape(1, 1, K), tp, tc, ts)
            assert mod.last_route == "qkv_rope" and [o.shape[-1] for o in outs] == list(SHAPES[shape][:3])
            _check(outs, sums, pos, cos, sin, D, layout, dtype, f"{shape} {layout} call {rep}")
        _clean(mod)


@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 2, 5, 8, 19])
@pytest.mark.parametrize("kind", ["dense", "hybrid", "mixed"])
@pytest.mark.parametrize("bits", [3, 4])
def test_qkv_rope_matches_oracle_and_cleans_up(gpu, bits, kind, rows, dtype):
    """every shape class and both layouts (CONFIGS) per case: the oracle sums are shared, a launch costs microseconds"""
    _parity(gpu, bits, kind, rows, dtype)


@gpu_test
def test_the_sparse_members_spread_rows_over_two_csr_chunks(gpu):
    for n in (456, 132, 128, 384):
        lay = _layer(gpu, 4, n, True, 1)[0]
        assert lay["vals"].numel() > 1024


@gpu_test
@pytest.mark.parametrize("rows", [1, 5])
def test_qkv_rope_with_many_k_slices(gpu, rows):
    """target_wgs = 4096: more workgroups asked for than the shapes have 32-unit slices, so every member's tiles are cut into
    the four slices a w4 op of K = 1024 can have -- a column completes after four dense contributions and its CSR chunks,
    whoever comes last, and only then meets its partner"""
    from squeezellm_amd import _lib

    old = _lib.get_option("target_wgs")
    _lib.set_option("target_wgs", 4096)
    try:
        _parity(gpu, 4, "hybrid", rows, "float16", [("d8", "half"), ("d128", "interleaved")])
    finally:
        _lib.set_option("target_wgs", old)


# ---- 2. bit-exact equalities, run twice ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 5, 19])
@pytest.mark.parametrize("bits", [3, 4])
def test_v_and_identity_rotation_equal_the_linear_bit_for_bit(gpu, bits, rows, dtype):
    """out_v, and out_q / out_k under cos = 1, sin = 0, against sqllm_linear_bf16 (bf16) or sqllm_linear_ep_f16 with the identity
    and no residual (fp16: the fused module's forward with `out` given) on the same operands"""
    import torch

    from squeezellm_amd import quant

    x = _x(gpu, rows, dtype)
    for shape, layout in (("d8", "interleaved"), ("d24", "half"), ("d128", "half")):
        D = SHAPES[shape][3]
        members = _members(gpu, bits, "mixed", shape)
        _in_range(members, x)
        mod = _module(members, D, layout, fused_members=True)
        tp, tc, ts = _dev(gpu, _positions(rows), *_identity_tables(D))
        outs = mod(x, tp, tc, ts)
        for y, m in zip(outs, (mod.q, mod.k, mod.v)):
            if dtype == "bfloat16":
                want = m(x)
                assert m.last_route == "fused"
            else:
                want = m(x, out=torch.empty((rows, m.outfeatures), dtype=x.dtype, device=gpu))
                assert m.last_route == "fused_ep"
            assert type(m) is quant.QuantLinearLUTFused and torch.equal(y.view(torch.int16), want.view(torch.int16))
        # ... and v is the same under the random tables
        outs2 = mod(x, tp, *_dev(gpu, [], *_tables(D))[1:])
        assert torch.equal(outs2[2].view(torch.int16), outs[2].view(torch.int16))
        _clean(mod)


@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("bits", [3, 4])
def test_two_runs_are_bit_identical(gpu, bits, rows, dtype):
    """hybrid members: CSR rows of more than 256 non-zeros are held by several waves of a chunk (kOrderedCsr), and which column
    of a pair finishes first differs from run to run"""
    import torch

    x = _x(gpu, rows, dtype)
    pos = _positions(rows)
    for shape, layout in (("d8", "half"), ("d128", "interleaved")):
        D = SHAPES[shape][3]
        members = _members(gpu, bits, "hybrid", shape)
        cos, sin = _tables(D)
        tp, tc, ts = _dev(gpu, pos, cos, sin)
        mod = _module(members, D, layout)
        runs = [[o.clone() for o in mod(x, tp, tc, ts)] for _ in range(4)]
        torch.cuda.synchronize()
        for r in runs[1:]:
            for a, b in zip(r, runs[0]):
                assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        _check(runs[0], _sums(members, x, rows, dtype), pos, cos, sin, D, layout, dtype)
        _clean(mod)


# ---- 3. positions outside the tables, non-finite input ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("layout", ["half", "interleaved"])
def test_out_of_range_positions_give_nan_rows_and_read_nothing(gpu, layout, dtype):
    """positions -1 and n_pos in two rows of five: every q and k output of those rows is NaN (the kernel reads no table entry for
    them), v and the other rows stay inside the tolerance"""
    rows, shape = 5, "d8"
    D = SHAPES[shape][3]
    members = _members(gpu, 4, "mixed", shape)
    x = _x(gpu, rows, dtype)
    sums = _sums(members, x, rows, dtype)
    cos, sin = _tables(D)
    pos = [3, -1, 0, N_POS, N_POS - 1]
    bad = np.array([False, True, False, True, False])
    safe = [p if 0 <= p < N_POS else 0 for p in pos]
    mod = _module(members, D, layout)
    tp, tc, ts = _dev(gpu, pos, cos, sin)
    for rep in range(2):  # (the pair words of the first call must not linger)
        outs = mod(x, tp, tc, ts)
        for y, s in zip(outs[:2], sums[:2]):
            got = _np64(y, rows)
            assert np.isnan(got[bad]).all() and np.isfinite(got[~bad]).all()
            exact, tol = _rotated(s, safe, cos, sin, D, layout, dtype)
            _inside(y, exact, tol, "rows in range", where=np.broadcast_to(~bad[:, None], exact.shape))
        _inside(outs[2], *_plain(sums[2], dtype), "v")
    _clean(mod)


@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("layout", ["half", "interleaved"])
@pytest.mark.parametrize("bits", [3, 4])
def test_an_infinite_activation_follows_the_fp32_formula(gpu, bits, layout, dtype):
    """+inf at one k of one row of three: every sum of that row is +-inf by the sign of its weight there (NaN where the dense and
    the sparse term disagree), and a rotated output is inf * cos - inf * sin in IEEE fp32: an infinity or NaN by the signs.  The
    expected NaN / +inf / -inf pattern is the fp32 formula's on the oracle's sums."""
    import torch

    rows, shape, row = 3, "d8", 1
    D = SHAPES[shape][3]
    members = _members(gpu, bits, "mixed", shape)
    x = _x(gpu, rows, dtype).clone()
    x[row, 37] = float("inf")
    with np.errstate(all="ignore"):
        sums = [BF._exact(npl, x, k) for _, npl, _, k in members]
    for s in sums:
        assert (~np.isfinite(s[row])).all() and np.isfinite(np.delete(s, row, axis=0)).all()
    cos, sin = _tables(D)
    pos = _positions(rows)
    want = [_f32_formula(s, pos, cos, sin, D, layout) for s in sums[:2]] + [sums[2].astype(np.float32)]
    assert all(np.isinf(w[row]).any() and np.isnan(w[row]).any() for w in want[:2])  # both outcomes occur
    finite = np.ones((rows, 1), bool)
    finite[row] = False
    mod = _module(members, D, layout)
    tp, tc, ts = _dev(gpu, pos, cos, sin)
    for rep in range(2):  # (the flags and pair words of the first call must not linger)
        outs = mod(x, tp, tc, ts)
        for i, (y, w, s) in enumerate(zip(outs, want, sums)):
            got, w = y.float().cpu(), torch.from_numpy(w)
            assert torch.equal(torch.isnan(got), torch.isnan(w)), i
            assert torch.equal(torch.isposinf(got), torch.isposinf(w)) and torch.equal(torch.isneginf(got), torch.isneginf(w)), i
            with np.errstate(all="ignore"):
                sf = np.where(finite, s, 0.0)
                exact, tol = _rotated(sf, pos, cos, sin, D, layout, dtype) if i < 2 else _plain(sf, dtype)
            _inside(y, exact, tol, "finite rows", where=np.broadcast_to(finite, exact.shape))
    _clean(mod)


# ---- 4. capture ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_captured_call_is_one_kernel_node_and_follows_the_positions(gpu, dtype):
    """after one eager call, a captured forward is ONE kernel node (no zero fill, no cast, no memory node); a replay after the
    positions tensor was updated in place rotates by the new positions"""
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

    rows, shape, layout = 2, "d128", "half"
    D = SHAPES[shape][3]
    members = _members(gpu, 4, "hybrid", shape)
    mod = _module(members, D, layout, fused_members=True)
    x = _x(gpu, rows, dtype)
    sums = _sums(members, x, rows, dtype)
    cos, sin = _tables(D)
    pos = [4, 9]
    tp, tc, ts = _dev(gpu, pos, cos, sin)
    outs = []

    def run():
        outs.clear()
        with torch.no_grad():
            outs.extend(mod(x, tp, tc, ts))

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
    assert node_types(g) == [0]  # hipGraphNodeTypeKernel: the q/k/v kernel and nothing else
    g.instantiate()
    for o in outs:
        o.zero_()
    g.replay()
    torch.cuda.synchronize()
    for o, w in zip(outs, want):
        assert torch.equal(o.view(torch.int16), w.view(torch.int16))
    for pos in ([10, 0], [N_POS - 1, 21]):
        tp.copy_(torch.tensor(pos, dtype=torch.int32, device=gpu))  # in place: the graph holds the tensor's address
        g.replay()
        torch.cuda.synchronize()
        _check(outs, sums, pos, cos, sin, D, layout, dtype, f"replay at {pos}")
    assert not torch.equal(outs[0].view(torch.int16), want[0].view(torch.int16)) and torch.equal(outs[2].view(torch.int16), want[2].view(torch.int16))
    _clean(mod)


# ---- 5. the three entries ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("layout", ["half", "interleaved"])
def test_c_abi_directly(gpu, layout, dtype):
    """the descriptor filled in by hand from the layers' raw operands (CSR and top-X rows passed separately, not folded), a
    workspace of sqllm_qkv_rope_workspace_bytes zero-filled once, two launches on it"""
    import torch

    from squeezellm_amd import _lib, quant_cuda

    rows, shape = 5, "d24"
    Nq, Nk, Nv, D = SHAPES[shape]
    members = _members(gpu, 3, "mixed", shape)
    x = _x(gpu, rows, dtype)
    sums = _sums(members, x, rows, dtype)
    cos, sin = _tables(D)
    pos = _positions(rows)
    tp, tc, ts = _dev(gpu, pos, cos, sin)
    r = _lib.SqllmQkvRope()
    outs = []
    for op, name, (lay, _, _, _) in zip((r.q, r.k, r.v), "qkv", members):
        op.bits, op.batch, op.K, op.N = lay["bits"], rows, K, lay["N"]
        op.vec, op.qweight, op.lookup_table = x.data_ptr(), lay["qweight"].data_ptr(), lay["lookup_table"].data_ptr()
        if lay["vals"] is not None:
            op.rows, op.cols, op.vals, op.nnz = lay["rows"].data_ptr(), lay["cols"].data_ptr(), lay["vals"].data_ptr(), lay["vals"].numel()
            op.full_rows, op.full_row_indices, op.topX = lay["full_rows"].data_ptr(), lay["full_row_indices"].data_ptr(), lay["full_rows"].shape[1]
        setattr(r, "bias_" + name, lay["bias"].data_ptr())
        outs.append(torch.empty((rows, lay["N"]), dtype=x.dtype, device=gpu))
        setattr(r, "out_" + name, outs[-1].data_ptr())
    r.cos, r.sin, r.positions = tc.data_ptr(), ts.data_ptr(), tp.data_ptr()
    r.n_pos, r.head_dim, r.layout = N_POS, D, _lib.ROPE_INTERLEAVED if layout == "interleaved" else _lib.ROPE_HALF
    need = _lib.qkv_rope_workspace_bytes(Nq, Nk, Nv, rows)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=gpu)
    ws[need:] = 0xA5  # a guard behind the workspace
    r.workspace = ws.data_ptr()
    dev = x.get_device()
    fn = getattr(_lib.load(), "sqllm_qkv_rope_f16" if dtype == "float16" else "sqllm_qkv_rope_bf16")
    for rep in range(2):
        for o in outs:
            o.zero_()
        assert fn(ctypes.byref(r), quant_cuda._raw_stream(dev)) == 0
        torch.cuda.synchronize()
        _check(outs, sums, pos, cos, sin, D, layout, dtype, f"call {rep}")
        assert int(ws[:need].count_nonzero()) == 0 and bool((ws[need:] == 0xA5).all())


@gpu_test
def test_module_surface(gpu):
    """leading dimensions, int64 positions, the constructor's checks, nothing owned"""
    import torch
    import torch.nn as nn

    from squeezellm_amd import quant

    shape, layout, dtype, rows = "d128", "half", "float16", 8
    D = SHAPES[shape][3]
    members = _members(gpu, 4, "dense", shape)
    mod = _module(members, D, layout)
    assert list(mod.state_dict().keys()) == [] and list(mod.children()) == [] and list(mod.buffers()) == [] and mod.last_route is None
    x = _x(gpu, rows, dtype)
    sums = _sums(members, x, rows, dtype)
    cos, sin = _tables(D)
    pos = _positions(rows)
    tp, tc, ts = _dev(gpu, pos, cos, sin)
    outs = mod(x.reshape(2, 4, K), tp.reshape(2, 4).long(), tc, ts)
    assert [tuple(o.shape) for o in outs] == [(2, 4, n) for n in SHAPES[shape][:3]] and mod.last_route == "qkv_rope"
    _check(outs, sums, pos, cos, sin, D, layout, dtype)
    _clean(mod)
    q, k, v = mod.q, mod.k, mod.v
    with pytest.raises(ValueError, match="head_dim"):
        quant.QuantQKVRopeFused(q, k, v, head_dim=96)
    with pytest.raises(ValueError, match="head_dim"):
        quant.QuantQKVRopeFused(q, k, v, head_dim=3)
    with pytest.raises(ValueError, match="layout"):
        quant.QuantQKVRopeFused(q, k, v, head_dim=D, layout="neox")
    with pytest.raises(TypeError):
        quant.QuantQKVRopeFused(q, nn.Linear(K, 128), v, head_dim=D)
    with pytest.raises(ValueError, match="bit width"):
        quant.QuantQKVRopeFused(q, quant.QuantLinearLUT.from_operands(_layer(gpu, 3, 128, False, 1)[0]), v, head_dim=D)
    with pytest.raises(ValueError, match="positions"):
        mod(x, tp[:3], tc, ts)
    with pytest.raises(ValueError, match="cos"):
        mod(x, tp, tc[:, :5], ts)


@gpu_test
@pytest.mark.parametrize("layout", ["half", "interleaved"])
def test_fp32_input_takes_the_fallback(gpu, layout):
    """fp32 activations: the operator path and the rotation in torch, in fp32 -- inside the tolerance with eps = 2^-24"""
    import torch

    shape, rows = "d24", 5
    D = SHAPES[shape][3]
    members = _members(gpu, 4, "mixed", shape)
    mod = _module(members, D, layout)
    x = _x(gpu, rows, "float16").float()
    sums = [BF._exact(npl, x, k) for _, npl, _, k in members]
    cos, sin = _tables(D)
    pos = _positions(rows)
    outs = mod(x, *_dev(gpu, pos, cos, sin))
    assert mod.last_route == "fallback" and "_ws" not in mod.__dict__
    _check(outs, sums, pos, cos, sin, D, layout, "float32")
    # ... and a position outside the tables is a NaN row there as well
    tp, tc, ts = _dev(gpu, [0, N_POS, 1, 2, -1], cos, sin)
    oq, ok, ov = mod(x, tp, tc, ts)
    assert torch.isnan(oq[[1, 4]]).all() and torch.isfinite(oq[[0, 2, 3]]).all() and torch.isnan(ok[[1, 4]]).all() and torch.isfinite(ov).all()


@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_dense_route_from_dense_min_rows(gpu, dtype):
    """dense_min_rows = 4 on q, 5 rows: the members' fp32 dense matrices and torch's fp32 GEMM, rotated in fp32 and rounded once --
    the same formulas, so the same tolerance plus the fp32 GEMM's own rounding of the sums (K products of an fp32 dot:
    K * 2^-24 * sum_k |W x|, carried through the rotation like the per-sum slack).  Three rows stay on the kernel."""
    from squeezellm_amd import quant

    shape, layout, rows = "d24", "half", 5
    D = SHAPES[shape][3]
    members = _members(gpu, 4, "mixed", shape)
    mod = _module(members, D, layout, fused_members=True)
    mod.q.dense_min_rows = 4
    x = _x(gpu, rows, dtype)
    sums = _sums(members, x, rows, dtype)
    cos, sin = _tables(D)
    pos = _positions(rows)
    tp, tc, ts = _dev(gpu, pos, cos, sin)
    outs = mod(x, tp, tc, ts)
    assert mod.last_route == "dense" and type(mod.q) is quant.QuantLinearLUTFused
    for i, (y, s, (_, npl, mag, _)) in enumerate(zip(outs, sums, members)):
        gemm = K * 2.0 ** -24 * BF._abs_sum(npl, mag, x)  # per sum
        if i < 2:
            exact, tol = _rotated(s, pos, cos, sin, D, layout, dtype)
            lo, hi = _split(gemm, D, layout)
            c, sn = np.abs(_at(cos, pos)).astype(np.float64), np.abs(_at(sin, pos)).astype(np.float64)
            tol = tol + _merge(lo * c + hi * sn, hi * c + lo * sn, layout)
        else:
            exact, tol = _plain(s, dtype)
            tol = tol + gemm
        _inside(y, exact, tol, "qkv"[i])
    outs3 = mod(x[:3].contiguous(), tp[:3].contiguous(), tc, ts)
    assert mod.last_route == "qkv_rope"
    _check(outs3, [s[:3] for s in sums], pos[:3], cos, sin, D, layout, dtype)
    _clean(mod)


# ---- 6. the other API ----

def test_rope_tables_against_a_direct_fp64_computation():
    import torch

    from squeezellm_amd import quant

    for D, n_pos, theta in ((128, 300, 10000.0), (64, 50, 500000.0), (8, 7, 10000.0), (24, 11, 100.0)):
        cos, sin = quant.rope_tables(D, n_pos, theta)
        assert cos.dtype == sin.dtype == torch.float32 and tuple(cos.shape) == tuple(sin.shape) == (n_pos, D // 2)
        ang = np.arange(n_pos, dtype=np.float64)[:, None] * theta ** (-2.0 * np.arange(D // 2, dtype=np.float64) / D)[None, :]
        # rounded once from fp64: equal to the direct computation's rounding, or its neighbour where the two libraries' last fp64
        # bit straddles an fp32 rounding boundary (an fp32 ulp below 1 is at most 2^-24)
        assert np.abs(cos.numpy().astype(np.float64) - np.cos(ang)).max() <= 2.0 ** -24
        assert np.abs(sin.numpy().astype(np.float64) - np.sin(ang)).max() <= 2.0 ** -24
        assert (cos.numpy() == np.cos(ang).astype(np.float32)).mean() > 0.99 and (sin.numpy() == np.sin(ang).astype(np.float32)).mean() > 0.99
        assert float(cos[0].min()) == 1.0 and float(sin[0].abs().max()) == 0.0
    with pytest.raises(ValueError):
        quant.rope_tables(7, 4)
    with pytest.raises(ValueError):
        quant.rope_tables(8, 0)


@gpu_test
def test_fuse_qkv_rope_on_a_toy_model(gpu):
    import torch
    import torch.nn as nn

    from squeezellm_amd import quant

    shape = "d128"
    Nq, Nk, Nv, D = SHAPES[shape]

    class Attn(nn.Module):
        def __init__(self, bits, head_dim, names=("q_proj", "k_proj", "v_proj")):
            super().__init__()
            self.members = _members(gpu, bits, "mixed", shape)
            for name, (lay, _, _, _) in zip(names, self.members):
                setattr(self, name, quant.QuantLinearLUT.from_operands(lay))
            self.o_proj = nn.Linear(Nq, 16)
            if head_dim is not None:
                self.head_dim = head_dim

        def forward(self, x):
            return self.o_proj(self.q_proj(x).float())

    class Toy(nn.Module):
        def __init__(self):
            super().__init__()
            # 0, 1: convertible; 2: no head_dim; 3: a head_dim that does not divide k's width; 4: other names
            self.layers = nn.ModuleList([Attn(4, D), Attn(3, D), Attn(4, None), Attn(4, 256), Attn(4, D, ("wq", "wk", "wv"))])
            self.norm = nn.LayerNorm(8)

    toy = Toy().to(gpu)
    keys = list(toy.state_dict().keys())
    n_modules = len(list(toy.modules()))
    forwards = [m.forward.__func__ for m in toy.layers]
    assert quant.fuse_qkv_rope(toy) == 2
    assert list(toy.state_dict().keys()) == keys and len(list(toy.modules())) == n_modules
    assert all("forward" not in m.__dict__ and m.forward.__func__ is f for m, f in zip(toy.layers, forwards))
    for i in (2, 3, 4):
        assert "qkv_rope" not in toy.layers[i].__dict__
    x = _x(gpu, 5, "float16")
    pos = _positions(5)
    cos, sin = _tables(D)
    for i in (0, 1):
        m = toy.layers[i]
        f = m.qkv_rope
        assert type(f) is quant.QuantQKVRopeFused and f.q is m.q_proj and f.k is m.k_proj and f.v is m.v_proj
        assert (f.head_dim, f.layout) == (D, "half")
        outs = f(x, *_dev(gpu, pos, cos, sin))
        assert f.last_route == "qkv_rope"
        _check(outs, _sums(m.members, x, 5, "float16"), pos, cos, sin, D, "half", "float16")
        _clean(f)
    assert quant.fuse_qkv_rope(toy, q="wq", k="wk", v="wv", head_dim=64) == 1 and toy.layers[4].qkv_rope.head_dim == 64
    assert quant.fuse_qkv_rope(nn.Linear(4, 4)) == 0
