"""The sparse role of the fused linears (csr_role, squeezellm_amd/csrc/sqllm_roles.h) across its three SPAN CLASSES.  A chunk of
1024 consecutive non-zeros needs n row pointers; with nb = the rows of the batch tile and CAP = kCsrSpanMax = 2048 (fp16 and bf16
linear) or kCsrSpanMax - kCsrEdge = 1792 (the gated kernels, whose last 256 accumulator floats hold the wave-ordered edge slots):

    one group    n * nb <= CAP        all batch rows accumulate in LDS in one zero / accumulate / flush round
    row groups   n <= CAP < n * nb    the batch goes through g = CAP / n rows at a time (sums re-zeroed, x re-gathered)
    fallback     n > CAP              searches in global memory, one uncounted fixed-point add per non-zero, a counting pass

The suites of tests/test_gpu_linear_bf16.py and tests/test_gpu_gated.py (K = 1024, N = 456: every chunk spans about 90 rows) only
ever run the first, and so do those of tests/test_gpu_qkv_rope.py and tests/test_gpu_norm_front.py (N <= 456).  Here the layers
are "span ladders": synth.make_layer's dense operands and bias at K = 512, N = 8192 with a CSR built from a per-row count vector
(ladder_counts) whose 11 chunks span 16 ... 2211 rows.  This file runs the fp16 / bf16 linears and the gated pair on them;
tests/test_gpu_linear_ep.py runs the epilogue linear on ladder "a"; tests/test_gpu_csr_span_fronts.py runs the attention front and
both norm fronts (qkv_rope, gated_norm, qkv_rope_norm: CAP = 1792 like the gated pair) with this file's ladders, class model and
helpers, which it imports.

Two ladders, "a" and "b", differ in the seed and in four of the six heavy rows, so their chunk boundaries differ; they are the gate
and the up of the gated pair, and the fp16 / bf16 linears run on BOTH of them.  The class conditions of section 1 below are
assertions over the chunks an entry runs -- the 22 chunks of the two ladders.  (Ladder "a" alone has ONE chunk beyond 2048 rows and
ONE chunk in the gated kernels' row-group band at two rows; "at least two" needs the second ladder.  Two of the conditions cannot
hold for any CSR and are asserted as such: at nb = 1 the row-group class is empty, n <= CAP < n; at nb = 2 a row-group chunk has
g = 1.)

Reference and gates are the existing suites', unchanged: the fp64 oracle sums of tests/helpers.py on the exactly widened
activations plus the bias; one fp16 / bf16 ulp at the element's magnitude + 1e-6 (tests/test_gpu_linear.py, test_gpu_linear_bf16.py)
and test_gpu_gated._gate for the pair.  They hold for the fallback class by derivation, not by measurement: there every
non-zero's product is rounded to the 2^-28 fixed point on its own instead of once per row and chunk; a ladder row has at most 460
non-zeros and at most 8 dense K slices, so the fixed-point error of a sum stays below 468 * 2^-29 = 8.7e-7, inside the 1e-6 slack.

A failing parity assertion names the span class(es) of the chunks that hold the failing columns' rows."""
import os
import re

import numpy as np
import pytest

from tests import test_gpu_dequant as DQ
from tests import test_gpu_gated as GT
from tests import test_gpu_linear as TL
from tests import test_gpu_linear_bf16 as BF

gpu_test = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = BF.LIMIT
K, N = 512, 8192
T = 512  # threads of a chunk's workgroup: one sampled probe of `rows` each
CHUNK, SPAN_MAX, EDGE = 1024, 2048, 256  # SQLLM_CSR_CHUNK, kCsrSpanMax, kCsrEdge (pinned to the source below)
CAPS = {"linear": SPAN_MAX, "gated": SPAN_MAX - EDGE}
ENTRIES = {"f16": ("linear", "float16"), "bf16": ("linear", "bfloat16"), "gated_f16": ("gated", "float16"), "gated_bf16": ("gated", "bfloat16")}
TILE_ROWS = (1, 2, 3, 8)  # nb of the batch tiles 1, 2, 4 (three rows of it) and 8; 19 rows are 8 + 8 + 3
HEAVY_NNZ = 460
HEAVY = {"a": (300, 1500, 3000, 5500, 7500, 8191), "b": (200, 1300, 3000, 5400, 7600, 8191)}
EPS_LIN = {"float16": 2.0 ** -10, "bfloat16": 2.0 ** -7}  # the linears' gates take one ulp, the pair's half of one (GT.EPS)
CLASSES = ("one group", "row groups", "fallback")


# ---- the ladder ----

def ladder_counts(heavy):
    """non-zeros per row: 4 on rows 0..1023, 1 on 1024..2047, 1024 spread evenly over 2048..3947, 1 on every third row of
    3948..7019, 2 on every fifth of 7020..8190, and six heavy rows of 460 (several waves of a chunk each; some straddle a chunk boundary)"""
    c = np.zeros(N, np.int64)
    c[:1024] = 4
    c[1024:2048] = 1
    r = np.arange(1900)
    c[2048:3948] = (r + 1) * 1024 // 1900 - r * 1024 // 1900
    c[3948:7020:3] = 1
    c[7020:8191:5] = 2
    c[list(heavy)] = HEAVY_NNZ
    return c


def ladder_rows(which):
    rows = np.zeros(N + 1, np.int64)
    rows[1:] = np.cumsum(ladder_counts(HEAVY[which]))
    return rows


_LADDERS = {}


def ladder_layer(device, bits, which, topX=0):
    """(torch operands, numpy operands, sum of |terms| per weight) of a ladder: make_layer's dense operands (+ top-X rows) and bias,
    then rows / cols / vals replaced -- columns sorted and distinct per row, values randn * 0.1.  One per key, never edited."""
    import torch

    from squeezellm_amd import synth

    key = (str(device), bits, which, topX)
    if key not in _LADDERS:
        seed = 900 + 31 * bits + (1000 if which == "b" else 0)
        lay = synth.make_layer(K, N, bits, topX=topX, bias=True, device=device, seed=seed)
        rng = np.random.default_rng(seed)
        cnt = ladder_counts(HEAVY[which])
        cols = np.concatenate([np.sort(rng.choice(K, int(c), replace=False)) for c in cnt if c]).astype(np.int32)
        vals = (rng.standard_normal(cols.size) * 0.1).astype(np.float32)
        rows = ladder_rows(which).astype(np.int32)
        assert int(rows[-1]) == cols.size == vals.size
        lay.update(rows=torch.from_numpy(rows).to(device), cols=torch.from_numpy(cols).to(device), vals=torch.from_numpy(vals).to(device))
        if topX:  # (section 3) a repeated index, and the last column
            fi = lay["full_row_indices"].clone()
            fi[1] = fi[0]
            fi[topX - 1] = N - 1
            lay["full_row_indices"] = fi
        npl = TL._npl(lay)
        _LADDERS[key] = (lay, npl, DQ.expected(npl)[3])
    return _LADDERS[key]


def _kind(lay):
    return "hybrid" if lay["full_rows"] is not None else "spmv"


def _x(device, rows, dtype, positive=False):
    import torch

    g = torch.Generator(device=device).manual_seed(rows)
    x = torch.randn((rows, K), device=device, generator=g)
    return (x.abs() + 0.25 if positive else x).to(getattr(torch, dtype))


_SUMS = {}


def _sum(device, bits, which, topX, x, key):
    """fp64 oracle sums (+ bias) of a ladder for the 16-bit activations x, computed once per key"""
    key = (str(device), bits, which, topX) + key
    if key not in _SUMS:
        lay, npl, _ = ladder_layer(device, bits, which, topX)
        _SUMS[key] = BF._exact(npl, x, _kind(lay))
    return _SUMS[key]


# ---- the class model: n per chunk exactly as csr_role derives it ----

def span_model(rows, n_out=N):
    """[(e0, e1, c_lo, c_hi, n)] per chunk of CHUNK non-zeros.  csr_role: thread t probes rows[min(t * S, N)] with the sample
    stride S = (N + T) / T; cnt_lo / cnt_hi count the samples (t * S <= N) at or below the chunk's first / last non-zero;
    c_lo = (cnt_lo - 1) * S, c_hi = cnt_hi * S clipped to N; n = c_hi - c_lo + 1 row pointers are staged."""
    rows = np.asarray(rows, np.int64)
    nnz = int(rows[n_out])
    S = (n_out + T) // T
    si = np.arange(T) * S
    probe, ok = rows[np.minimum(si, n_out)], si <= n_out
    out = []
    for ch in range((nnz + CHUNK - 1) // CHUNK):
        e0, e1 = ch * CHUNK, min(ch * CHUNK + CHUNK, nnz)
        cnt_lo, cnt_hi = int((ok & (probe <= e0)).sum()), int((ok & (probe <= e1 - 1)).sum())
        c_lo, c_hi = max(cnt_lo - 1, 0) * S, min(cnt_hi * S, n_out)
        out.append((e0, e1, c_lo, c_hi, c_hi - c_lo + 1))
    return out


def chunk_class(n, nb, cap):
    return CLASSES[0] if n * nb <= cap else CLASSES[1] if n <= cap else CLASSES[2]


def group_rows(n, nb, cap):
    """g of csr_role: batch rows per zero / accumulate / flush round of a chunk that accumulates in LDS"""
    return max(1, min(cap // n, nb))


def chunks_of_rows(rows):
    """(non-zeros, first chunk, last chunk) per CSR row; csr_chunks_of_row = last - first + 1 where the row is not empty"""
    rows = np.asarray(rows, np.int64)
    return np.diff(rows), rows[:-1] // CHUNK, (rows[1:] - 1) // CHUNK


def column_classes(rows, nb, cap):
    """per output column (= CSR row): the class(es) of the chunk(s) that hold its non-zeros, as a string ("-": an empty row)"""
    cls = np.array([CLASSES.index(chunk_class(s[4], nb, cap)) for s in span_model(rows)])
    cnt, first, last = chunks_of_rows(rows)
    mask = np.where(cnt > 0, (1 << cls[np.minimum(first, len(cls) - 1)]) | (1 << cls[np.minimum(last, len(cls) - 1)]), 0)
    names = np.array(["-"] + [" + ".join(c for i, c in enumerate(CLASSES) if m >> i & 1) for m in range(1, 8)])
    return names[mask]


def _labels(kind, nb):
    """span class per output column for an entry kind at a tile of nb rows: of ladder a, of ladder b, of the pair"""
    a, b = (column_classes(ladder_rows(w), nb, CAPS[kind]) for w in "ab")
    return {"a": a, "b": b, "pair": np.char.add(np.char.add("gate ", a), np.char.add(" / up ", b))}


def _tile_rows(rows):
    """nb of the batch tiles a call of `rows` rows runs (sqllm_kernels.h: batch_tile)"""
    bt = 1 if rows <= 1 else 2 if rows == 2 else 4 if rows <= 4 else 8
    return sorted({min(bt, rows - b0) for b0 in range(0, rows, bt)})


def _tile_labels(kind, rows, which):
    """per (batch row, column): the class at the row's own tile -- [rows, N] of strings"""
    bt = 1 if rows <= 1 else 2 if rows == 2 else 4 if rows <= 4 else 8
    per_nb = {nb: _labels(kind, nb)[which] for nb in _tile_rows(rows)}
    return np.stack([per_nb[min(bt, rows - b // bt * bt)] for b in range(rows)])


def _by_class2(bad, labels2):
    names = sorted(set(labels2.ravel().tolist()))
    return "; ".join(f"[{n}] {int((bad & (labels2 == n)).sum())} of {int((labels2 == n).sum())}" for n in names)


# ---- 1. the model and the conditions it enforces (no GPU) ----

def test_model_constants_match_the_source():
    src = open(os.path.join(ROOT, "squeezellm_amd", "csrc", "sqllm_kernels.h")).read()
    assert int(re.search(r"#define\s+SQLLM_CSR_CHUNK\s+(\d+)", src).group(1)) == CHUNK
    assert re.search(r"constexpr\s+int\s+kCsrChunk\s*=\s*SQLLM_CSR_CHUNK\s*;", src)
    assert int(re.search(r"constexpr\s+int\s+kCsrSpanMax\s*=\s*(\d+)\s*;", src).group(1)) == SPAN_MAX
    assert int(re.search(r"constexpr\s+int\s+kCsrEdge\s*=\s*(\d+)\s*;", src).group(1)) == EDGE
    assert int(re.search(r"#define\s+SQLLM_WAVES\s+(\d+)", src).group(1)) * 64 == T
    roles = open(os.path.join(ROOT, "squeezellm_amd", "csrc", "sqllm_roles.h")).read()
    assert "constexpr int CAP = kCsrSpanMax - (ORD ? kCsrEdge : 0);" in roles and "const int S = (N + T) / T;" in roles


def test_ladder_a_spans_are_the_documented_ones():
    rows = ladder_rows("a")
    assert int(rows[-1]) == 10391
    assert [s[4] for s in span_model(rows)] == [273, 154, 273, 273, 613, 766, 1055, 2211, 2024, 696, 16]
    # the staged pointers bracket the chunk: rows[c_lo] <= e0, and rows[c_hi] > e1 - 1 or c_hi is the end
    for which in "ab":
        rows = ladder_rows(which)
        for e0, e1, c_lo, c_hi, n in span_model(rows):
            assert rows[c_lo] <= e0 and (rows[c_hi] > e1 - 1 or c_hi == N) and n >= 2


@pytest.mark.parametrize("nb", TILE_ROWS)
@pytest.mark.parametrize("kind", ["linear", "gated"])
def test_ladders_inhabit_every_class(kind, nb):
    """Conditions on the CSR the kernels receive (no top-X rows here, or unfolded ones: the ladder's own rows), over the chunks of
    both ladders, per entry kind and tile."""
    cap = CAPS[kind]
    chunks = []  # (ladder, chunk, n, class, holds a row of more than 256 non-zeros, holds a row spread over two chunks, empty rows at its start)
    for which in "ab":
        rows = ladder_rows(which)
        cnt, first, last = chunks_of_rows(rows)
        for ch, (e0, e1, c_lo, c_hi, n) in enumerate(span_model(rows)):
            held = (cnt > 0) & (first <= ch) & (last >= ch)
            owner = int(np.searchsorted(rows, e0, side="right")) - 1  # the row of the chunk's first non-zero
            lead = 0  # empty rows right below it, inside the staged span: their pointers equal the owner's
            while owner - lead - 1 >= c_lo and cnt[owner - lead - 1] == 0:
                lead += 1
            chunks.append((which, ch, n, chunk_class(n, nb, cap), bool((cnt[held] > 256).any()), bool((last[held] > first[held]).any()), lead))
    for c in chunks:
        print(f"{kind} CAP {cap} nb {nb}: ladder {c[0]} chunk {c[1]:2d} n {c[2]:4d} g {group_rows(c[2], nb, cap) if c[2] <= cap else '-'} {c[3]}"
              f"{' heavy' if c[4] else ''}{' straddle' if c[5] else ''}{f' {c[6]} empty rows first' if c[6] else ''}")
    for name in CLASSES:
        mine = [c for c in chunks if c[3] == name]
        if name == "row groups" and nb == 1:
            assert not mine  # n <= CAP < n * 1: empty for every CSR
            continue
        assert len(mine) >= 2, (name, len(mine))
        assert any(c[4] for c in mine), f"{name}: no row of more than 256 non-zeros"
        assert any(c[5] for c in mine), f"{name}: no row with csr_chunks_of_row >= 2"
    assert any(1792 < c[2] <= 2048 for c in chunks)  # in LDS for the linears, the fallback of the gated kernels
    gs = [group_rows(c[2], nb, cap) for c in chunks if c[3] == "row groups"]
    if nb > 2:
        assert any(2 <= g < nb for g in gs), gs  # groups of more than one row
    else:
        assert all(g == 1 for g in gs)  # (nb = 2: a row-group chunk has CAP / n = 1)
    assert any(c[6] > 0 for c in chunks)  # a run of empty rows at a chunk's start
    # the two members' chunk boundaries differ
    assert [s[4] for s in span_model(ladder_rows("a"))] != [s[4] for s in span_model(ladder_rows("b"))]


# ---- 2. parity ----

def _descriptor_csr(lin_op, lay, topX):
    """the kernel got the ladder's own CSR: nothing folded in, the top-X rows (if any) beside it"""
    assert lin_op.nnz == lay["vals"].numel() and lin_op.rows == lay["rows"].data_ptr() and lin_op.topX == topX


def _check_linear(y, exact, dtype, labels2):
    try:
        if dtype == "float16":
            TL._check_fp16(y.cpu().numpy().reshape(exact.shape), exact)
        else:
            BF._check_bf16(y, exact)
    except AssertionError as e:
        got = y.float().cpu().numpy().astype(np.float64).reshape(exact.shape)
        bad = ~(np.abs(got - exact) <= BF._tol(exact, EPS_LIN[dtype]))
        raise AssertionError(f"{e} -- by span class: {_by_class2(bad, labels2)}") from None


def _check_pair(y, g, u, dtype, labels2):
    try:
        GT._check(y, g, u, dtype)
    except AssertionError as e:
        got = y.float().cpu().numpy().astype(np.float64).reshape(g.shape)
        bad = ~(np.abs(got - GT._silu(g) * u) <= GT._gate(g, u, GT.EPS[dtype]))
        raise AssertionError(f"{e} -- by span class: {_by_class2(bad, labels2)}") from None


def _linear_module(lay, fold=True):
    mod = BF._fused(lay)
    if not fold:
        mod.fold_topx = False
    return mod


def _pair_module(lays, fold=True):
    from squeezellm_amd import quant

    mods = [quant.QuantLinearLUT.from_operands(lay) for lay in lays]
    if not fold:
        for m in mods:
            m.fold_topx = False
    return quant.QuantGatedLUTFused(*mods)


def _parity(gpu, bits, rows, entry, topX=0):
    import torch

    kind, dtype = ENTRIES[entry]
    x = _x(gpu, rows, dtype)
    xin = x if rows > 1 else x.reshape(1, 1, K)
    ladders = {w: ladder_layer(gpu, bits, w, topX) for w in "ab"}
    for lay, npl, mag in ladders.values():
        assert (BF._abs_sum(npl, mag, x) < LIMIT).all()  # every partial sum is in range: no non-finite result is admissible
    sums = {w: _sum(gpu, bits, w, topX, x, (rows, dtype, False)) for w in "ab"}
    if kind == "linear":
        for w in "ab":  # both ladders: the class conditions count the chunks of the two
            lay = ladders[w][0]
            mod = _linear_module(lay, fold=not topX)
            labels2 = _tile_labels(kind, rows, w)
            for rep in range(3):  # the second and third call run on the workspace the previous one left behind
                y = mod(xin)
                assert y.dtype == getattr(torch, dtype) and y.shape[-1] == N and mod.last_route == "fused"
                _check_linear(y.reshape(rows, N), sums[w], dtype, labels2)
            _descriptor_csr(next(iter(mod._desc.values()))[1][0].op, lay, topX)
            BF._workspaces_clean(mod)
    else:
        mod = _pair_module([ladders[w][0] for w in "ab"], fold=not topX)
        labels2 = _tile_labels(kind, rows, "pair")
        for rep in range(3):
            y = mod(xin)
            assert y.shape[-1] == N and mod.last_route == "gated"
            _check_pair(y.reshape(rows, N), sums["a"], sums["b"], dtype, labels2)
        desc = next(iter(mod._desc.values()))[2][0]
        _descriptor_csr(desc.gate, ladders["a"][0], topX)
        _descriptor_csr(desc.up, ladders["b"][0], topX)
        GT._workspaces_clean(mod)


@gpu_test
@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("rows", [1, 2, 3, 8, 19])
@pytest.mark.parametrize("bits", [3, 4])
def test_span_ladder_matches_oracle_and_cleans_up(gpu, bits, rows, entry):
    """The gates are the existing suites', unchanged (module docstring: they hold for the fallback by derivation)."""
    _parity(gpu, bits, rows, entry)


@gpu_test
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_span_ladder_with_many_k_slices(gpu, entry):
    """target_wgs = 4096 (tests/test_gpu_gated.py: test_gated_forward_with_many_k_slices): every tile is cut into the smallest K
    slices the planner makes, so a column completes after several dense contributions plus its chunks -- two on the heavy rows
    that straddle a chunk boundary -- whoever comes last"""
    from squeezellm_amd import _lib

    old = _lib.get_option("target_wgs")
    _lib.set_option("target_wgs", 4096)
    try:
        _parity(gpu, 4, 3, entry)
    finally:
        _lib.set_option("target_wgs", old)


# ---- 3. top-X rows passed unfolded ----

@gpu_test
@pytest.mark.parametrize("entry", ["bf16", "gated_f16", "gated_bf16"])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("bits", [3, 4])
def test_span_ladder_with_unfolded_topx_rows(gpu, bits, rows, entry):
    """fold_topx = False on the members and 70 top-X rows with a repeated index and the last column: the dense role gets more than
    64 top-X columns (tests/test_gpu_linear.py checks that for fp16 only) while the CSR classes stay as built; _parity reads
    topX == 70 and the ladder's own CSR back from the descriptor."""
    _parity(gpu, bits, rows, entry, topX=70)


# ---- 4. flags and the range rule through the CSR, on later row groups ----

def _poison_targets(which, cap, nb=8):
    """CSR entries to poison, in rows whose chunks accumulate in LDS: {name: (row, index into vals)} -- a light row (at most 4
    non-zeros) in the one-group chunk and in the row-group chunk of the largest n (g = 1: every batch row its own group), one in a
    row-group chunk of 2 <= g < nb, and the last non-zero of the first chunk's part of a heavy row that straddles two chunks."""
    rows = ladder_rows(which)
    spans = span_model(rows)
    cls = [chunk_class(s[4], nb, cap) for s in spans]
    cnt, first, last = chunks_of_rows(rows)

    def light_in(ch):
        return int(np.flatnonzero((cnt >= 1) & (cnt <= 4) & (first == ch) & (last == ch))[0])

    def largest(pred):
        return max((i for i in range(len(spans)) if pred(i)), key=lambda i: spans[i][4])

    out = {}
    for name, ch in (("one group", largest(lambda i: cls[i] == CLASSES[0] and ((cnt <= 4) & (cnt >= 1) & (first == i) & (last == i)).any())),
                     ("row groups", largest(lambda i: cls[i] == CLASSES[1])),
                     ("row groups g>=2", largest(lambda i: cls[i] == CLASSES[1] and group_rows(spans[i][4], nb, cap) >= 2))):
        r = light_in(ch)
        out[name] = (r, int(rows[r]))
    strad = [r for r in np.flatnonzero((cnt > 256) & (last > first)) if CLASSES[2] not in (cls[first[r]], cls[last[r]])]
    strad.sort(key=lambda r: CLASSES[1] not in (cls[first[r]], cls[last[r]]))  # one with a row-group chunk first
    r = int(strad[0])
    out["heavy straddling"] = (r, spans[first[r]][1] - 1)
    assert rows[r] <= out["heavy straddling"][1] < rows[r + 1]
    return out


def _poisoned(gpu, bits, which, value, cap):
    """a copy of ladder `which` with `value` at the targets' entries: (torch operands, numpy operands, targets)"""
    lay, npl, _ = ladder_layer(gpu, bits, which)
    tg = _poison_targets(which, cap)
    lay, npl = dict(lay), dict(npl)
    lay["vals"], npl["vals"] = lay["vals"].clone(), npl["vals"].copy()
    for r, e in tg.values():
        lay["vals"][e] = value
        npl["vals"][e] = value
    return lay, npl, tg


def _tol_scaled(exact, eps, rho):
    """the linears' gate (BF._tol) with its absolute slack of 1e-6 times rho; rho = 1: BF._tol itself"""
    return np.maximum(np.abs(exact), 2.0 ** -14) * eps + 1e-6 * rho


def _gate_scaled(g, u, eps, rho_g, rho_u):
    """the pair's gate (GT._gate) with the slack of 1e-6 PER SUM times that sum's rho; rho = 1: GT._gate itself"""
    return np.maximum(np.abs(GT._silu(g) * u), 2.0 ** -14) * eps + (1.1 * np.abs(u) * rho_g + np.abs(GT._silu(g)) * rho_u) * 1e-6 + 1e-6


@gpu_test
@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("poison", ["+inf", "-inf", "nan", "range"])
@pytest.mark.parametrize("bits", [3, 4])
def test_flags_and_range_rule_through_the_csr(gpu, bits, poison, entry):
    """8 rows, positive activations (an infinite value gives an infinite sum of ONE sign).  "+inf" / "-inf" / "nan": a CSR value is
    that; the NaN / +inf / -inf pattern of all 8 batch rows is the fp32 formula's -- torch on the fp32 sums, silu(g32) * u32 for the
    pair (both members are poisoned there, at their own targets).  "range": the value is 2^10 and the activations of its column are
    2^8, one product of 2^18 > 131072: the bf16 linear and both gated types must return a non-finite value, the fp16 linear inf; for
    the pair the gate is poisoned and u is made small on those columns, so that the exact product is finite in the output type and a
    clamped gate would be a finite wrong number.  All other outputs -- every fallback-class column among them -- are finite and
    inside the gate; the second call shows no lingering flag; the workspace is left clean.
    The gates are the suites', with one derived change in the "range" variant.  Their absolute slack of 1e-6 per sum stands for the
    fp32 rounding inside the contributions, which is proportional to the magnitude of the partial sums, sum_k |W x| + |bias| (about
    9 on these operands).  Activations of 2^8 on up to four columns raise that magnitude of EVERY output (dense weights of 0.02 on
    those columns: + 5 each), and an output that cancels to 2e-4 then misses 1e-6 by fp32 rounding alone (seen: 3.1e-6 on one
    output of 65536).  The slack of a sum is therefore multiplied by rho = its magnitude with the 2^8 columns over its magnitude
    with the activations as drawn -- computed from the operands, per output, never from a result; rho = 1 in the other variants,
    where the formulas are the suites' own (asserted below).
    Only rows whose chunks accumulate in LDS are poisoned (_poison_targets): in the fallback class a flag can be lost, which
    include/sqllm_hip.h documents (sqllm_linear_bf16, sqllm_gated)."""
    import torch

    kind, dtype = ENTRIES[entry]
    cap, rows = CAPS[kind], 8
    value = {"+inf": float("inf"), "-inf": float("-inf"), "nan": float("nan"), "range": 2.0 ** 10}[poison]
    x = _x(gpu, rows, dtype, positive=True)
    x0 = x.clone()  # as drawn: before the "range" variant raises columns to 2^8
    members = "a" if kind == "linear" else ("a" if poison == "range" else "ab")
    lays, npls, hit_cols = {}, {}, set()
    for w in "ab" if kind == "gated" else "a":
        if w in members:
            lays[w], npls[w], tg = _poisoned(gpu, bits, w, value, cap)
            assert len({r for r, _ in tg.values()}) == 4
            for name, (r, e) in tg.items():
                assert column_classes(ladder_rows(w), rows, cap)[r].find(CLASSES[2]) < 0, name  # in LDS
                hit_cols.add(r)
                if poison == "range":
                    x[:, int(npls[w]["cols"][e])] = 2.0 ** 8
        else:
            lay, npl, _ = ladder_layer(gpu, bits, w)
            lays[w], npls[w] = dict(lay), dict(npl)
    if poison == "range" and kind == "gated":  # u small on the poisoned gate columns: a constant codebook, and the row's CSR values scaled down
        cols = sorted(hit_cols)
        rb = ladder_rows("b")
        lays["b"]["lookup_table"], lays["b"]["vals"] = lays["b"]["lookup_table"].clone(), lays["b"]["vals"].clone()
        lays["b"]["lookup_table"][cols, :] = 2.0 ** -16
        for c in cols:
            lays["b"]["vals"][int(rb[c]):int(rb[c + 1])] *= 2.0 ** -10
        npls["b"] = TL._npl(lays["b"])
    hit_cols = sorted(hit_cols)
    # how far the 2^8 activations raise sum_k |W x| + |bias| of each clean output (1 in the other variants; the poisoned and the
    # edited columns are not clean outputs, so the ladders' own magnitudes serve)
    rho = {w: BF._abs_sum(*ladder_layer(gpu, bits, w)[1:], x) / BF._abs_sum(*ladder_layer(gpu, bits, w)[1:], x0) for w in lays}
    assert all((r >= 1).all() for r in rho.values()) and (poison == "range" or all((r == 1).all() for r in rho.values()))
    with np.errstate(all="ignore"):
        sums = {w: BF._exact(npls[w], x, "spmv") for w in lays}
        g32 = torch.from_numpy(sums["a"].astype(np.float32))
        if kind == "linear":
            want32, exact = g32, sums["a"]
            tol = _tol_scaled(exact, EPS_LIN[dtype], rho["a"])
        else:
            u32 = torch.from_numpy(sums["b"].astype(np.float32))
            want32, exact = torch.nn.functional.silu(g32) * u32, GT._silu(sums["a"]) * sums["b"]
            tol = _gate_scaled(sums["a"], sums["b"], GT.EPS[dtype], rho["a"], rho["b"])
            if poison != "range":
                fin = np.isfinite(exact)
                assert (tol[fin] == GT._gate(sums["a"], sums["b"], GT.EPS[dtype])[fin]).all()
    hit = np.zeros((rows, N), bool)
    hit[:, hit_cols] = True
    if poison == "range":
        top = 65504.0 if dtype == "float16" else 3.38e38
        assert (sums["a"][hit] > LIMIT).all() and np.isfinite(exact).all()
        assert kind == "linear" or (np.abs(exact[hit]) < top).all()  # finite in the output type: a clamp would go unnoticed as inf
    else:
        assert (~np.isfinite(want32.numpy()) == hit).all()
        if poison == "nan":
            assert torch.isnan(want32[:, hit_cols]).all()
        elif kind == "linear":
            assert (want32[:, hit_cols] == value).all()
        # (the pair: silu(+inf) u is the infinity of u's sign, silu(-inf) is NaN, silu(g) * inf the infinity of silu(g)'s sign)
    mod = _linear_module(lays["a"]) if kind == "linear" else _pair_module([lays["a"], lays["b"]])
    labels2 = _tile_labels(kind, rows, "a" if kind == "linear" else "pair")
    for rep in range(2):  # second call: the flags of the first must not linger
        y = mod(x)
        assert y.dtype == getattr(torch, dtype)
        got = y.float().cpu()
        if poison == "range":
            where = got[:, hit_cols]
            if entry == "f16":
                assert torch.isposinf(where).all(), where
            else:
                assert (~torch.isfinite(where)).all(), f"{int(torch.isfinite(where).sum())} finite values where a product is out of range: {where}"
        else:
            assert torch.equal(torch.isnan(got), torch.isnan(want32)), (int(torch.isnan(got).sum()), int(torch.isnan(want32).sum()))
            assert torch.equal(torch.isposinf(got), torch.isposinf(want32)) and torch.equal(torch.isneginf(got), torch.isneginf(want32))
        g64 = got.numpy().astype(np.float64)
        assert np.isfinite(g64[~hit]).all(), _by_class2(~np.isfinite(g64) & ~hit, labels2)
        bad = ~hit & ~(np.abs(g64 - np.where(hit, 0.0, exact)) <= np.where(hit, 0.0, tol))
        worst = [(int(b), int(n), float(g64[b, n]), float(exact[b, n]), float(tol[b, n])) for b, n in np.argwhere(bad)[:4]]
        assert not bad.any(), f"{int(bad.sum())} clean outputs outside the gate -- by span class: {_by_class2(bad, labels2)}; (row, column, got, exact, gate): {worst}"
    (BF if kind == "linear" else GT)._workspaces_clean(mod)


# ---- 5. run-to-run identity of the gated kernel ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("rows", [3, 8])
@pytest.mark.parametrize("bits", [3, 4])
def test_gated_span_ladder_is_bit_reproducible(gpu, bits, rows, dtype):
    """Five calls, bit for bit, over all columns.  In the row-group chunks the edge table (the wave-ordered slots of the rows that
    waves share) is re-zeroed per group of batch rows; in the fallback the adds are integer and a lane's sums come out of a fixed
    DPP order, so identity is expected there as well -- the two are asserted separately, so that a difference names where it is.
    (The fp16 / bf16 linears add shared rows in arrival order by design: nothing is asserted about them.)"""
    import torch

    mod = _pair_module([ladder_layer(gpu, bits, w)[0] for w in "ab"])
    x = _x(gpu, rows, dtype)
    ys = torch.stack([mod(x).view(torch.int16) for _ in range(5)])
    torch.cuda.synchronize()
    diff = (ys != ys[0]).any(dim=0).cpu().numpy()
    labels2 = _tile_labels("gated", rows, "pair")
    fb = np.char.find(labels2, CLASSES[2]) >= 0
    assert not (diff & ~fb).any(), f"outputs of chunks that accumulate in LDS differ between runs: {_by_class2(diff & ~fb, labels2)}"
    assert not (diff & fb).any(), f"outputs of fallback-class columns differ between runs: {_by_class2(diff & fb, labels2)}"
    _check_pair(mod(x), _sum(gpu, bits, "a", 0, x, (rows, dtype, False)), _sum(gpu, bits, "b", 0, x, (rows, dtype, False)), dtype, labels2)


# ---- 6. the gates reject the role's likely defects (no GPU) ----

def _chunk_share(npl, x64, ch):
    """[rows, N] fp64: what chunk `ch` contributes to every output"""
    rows = npl["rows"].astype(np.int64)
    e0, e1 = ch * CHUNK, min(ch * CHUNK + CHUNK, int(rows[-1]))
    rid = np.repeat(np.arange(N), np.diff(rows))[e0:e1]
    prod = x64[:, npl["cols"][e0:e1]] * npl["vals"][e0:e1].astype(np.float64)
    return np.stack([np.bincount(rid, weights=p, minlength=N) for p in prod])


def _wave_share(npl, x64, ch, wave, r):
    """[rows] fp64: the part of row r's sum that wave `wave` of chunk `ch` holds (64 lanes x 2 consecutive non-zeros)"""
    rows = npl["rows"].astype(np.int64)
    lo, hi = max(int(rows[r]), ch * CHUNK + 128 * wave), min(int(rows[r + 1]), ch * CHUNK + 128 * wave + 128)
    return x64[:, npl["cols"][lo:hi]] @ npl["vals"][lo:hi].astype(np.float64)


@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("bits", [3, 4])
def test_gates_admit_the_fp32_formula_and_reject_the_role_defects(bits, entry):
    """In numpy, on the gate ladder at 8 rows: the fp32 formula on the true sums stays inside the entry's gate everywhere, and each
    defect below, applied to the true sums and then put through the same formula, leaves more than half of the outputs it touches
    outside it.  (The pair's up sums are the true ones throughout: the defect sits in the gate member.)"""
    kind, dtype = ENTRIES[entry]
    cap, nb = CAPS[kind], 8
    lay, npl, _ = ladder_layer("cpu", bits, "a")
    x = _x("cpu", nb, dtype)
    x64 = x.float().numpy().astype(np.float64)
    s = _sum("cpu", bits, "a", 0, x, (nb, dtype, False))
    u = _sum("cpu", bits, "b", 0, x, (nb, dtype, False)) if kind == "gated" else None
    rows = ladder_rows("a")
    spans = span_model(rows)
    cls = [chunk_class(sp[4], nb, cap) for sp in spans]
    cnt, first, last = chunks_of_rows(rows)

    def out_of_gate(sums):
        s32 = sums.astype(np.float32)
        if kind == "linear":
            return np.abs(GT._round_to(s32, dtype) - s) > BF._tol(s, EPS_LIN[dtype])
        u32 = u.astype(np.float32)
        with np.errstate(over="ignore"):
            f32 = (s32 / (np.float32(1) + np.exp(-s32))) * u32
        assert f32.dtype == np.float32
        return np.abs(GT._round_to(f32, dtype) - GT._silu(s) * u) > GT._gate(s, u, GT.EPS[dtype])

    assert not out_of_gate(s).any()
    # (1) the batch rows of the second row group receive the first group's sparse sums
    for ch in [i for i, c in enumerate(cls) if c == CLASSES[1]]:
        g = group_rows(spans[ch][4], nb, cap)
        second = np.arange(g, min(2 * g, nb))
        share = _chunk_share(npl, x64, ch)
        held = np.flatnonzero((cnt > 0) & (first <= ch) & (last >= ch))
        d = s.copy()
        d[second] += share[second - g] - share[second]
        assert out_of_gate(d)[np.ix_(second, held)].mean() > 0.5, ("second row group", ch)
    # (2) an edge-slot sum is added to the neighbouring batch row: the part of a heavy row in the first wave that holds it
    in_lds_heavy = [(int(r), int(ch)) for r in np.flatnonzero(cnt > 256) for ch in range(first[r], last[r] + 1) if cls[ch] != CLASSES[2]]
    assert len(in_lds_heavy) >= 4
    d = s.copy()
    for r, ch in in_lds_heavy:
        wave = (max(int(rows[r]), ch * CHUNK) - ch * CHUNK) // 128
        q = _wave_share(npl, x64, ch, wave, r)
        d[:, r] += np.roll(q, 1) - q
    assert out_of_gate(d)[:, sorted({r for r, _ in in_lds_heavy})].mean() > 0.5
    # (3) one chunk's share of a straddling heavy row is dropped
    strad = np.flatnonzero((cnt > 256) & (last > first))
    assert len(strad) >= 3
    d = s.copy()
    for r in strad:
        d[:, r] -= _chunk_share(npl, x64, int(last[r]))[:, r]
    assert out_of_gate(d)[:, strad].mean() > 0.5
    # (4) the fallback's sums land one row off (c_lo + r + 1)
    for ch in [i for i, c in enumerate(cls) if c == CLASSES[2]]:
        share = _chunk_share(npl, x64, ch)
        assert (share[:, N - 1] == 0).all()
        d = s - share + np.roll(share, 1, axis=1)
        touched = np.flatnonzero((share != 0).any(axis=0) | (np.roll(share, 1, axis=1) != 0).any(axis=0))
        assert out_of_gate(d)[:, touched].mean() > 0.5, ("fallback one row off", ch)
