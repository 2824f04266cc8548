"""The sparse role (csr_role, squeezellm_amd/csrc/sqllm_roles.h) across its three SPAN CLASSES under the two newest finishing and vec
policies: RopeFinish (the attention front, sqllm_rope_finish.h) and RmsVec (the norm fronts, sqllm_norm_front.h).  The suites of
tests/test_gpu_qkv_rope.py and tests/test_gpu_norm_front.py run at N <= 456, where every chunk of 1024 non-zeros spans about 90 rows:
the first class only.  Here the six entries -- qkv_rope, gated_norm and qkv_rope_norm, each in fp16 and bf16 -- run on the span
ladders of tests/test_gpu_csr_span.py (K = 512, N = 8192; that file's docstring describes the classes, the ladders and the class
model, all reused from it as CS).  All six have kOrderedCsr = true: CAP = 1792, pinned to the source below.

Members.  gated_norm: gate = ladder "a", up = ladder "b" (CS._pair_module).  q/k/v: q = "a", k = "b", v = "a" -- v is not rotated,
so a q / v mix-up shows.  Rotary configs: head dimension 128 in the half layout (the partner is one 64-column tile away) and 64
interleaved (the partner is next door).  Tables TQ._tables (uniform angles), positions TQ._positions.

What only these shapes reach:
  * RmsVec in a LATER row group: every re-gather is scaled by r of batch row bs + bb, a v_readlane by a run-time index; the other
    suites stay in one group, bs == 0.  The fallback class walks the batch one row per round through the same line.  The norm
    activations are NC.activations with EIGHT row factors (NORM_SCALES), one per row of the widest batch tile: with the five of
    the other suites, rows 0 and 5 of a tile share a factor, and a kernel that took row 0's r for row 5 -- every later group of a
    g = 1 chunk -- would differ by 2 % there.  Section 1 asserts a factor of more than 2 between r of any later-group row b and r
    of rows b - g and b mod g.
  * RopeFinish::done() called by the fallback's counting pass, and pairs whose two columns finish in chunks of different classes
    (section 1 counts them: both in the fallback; one in the fallback and one empty, finished by a dense workgroup; ...).
  * the wave-ordered edge slots re-zeroed per row group, under the run-to-run identity both fronts promise.

References and gates are the existing suites', unchanged: TQ._rotated / TQ._plain on BF._exact sums for the plain rotary entries;
NC.gated_gate / NC.rotated_gate / NC.plain_gate on TL._exact(npl, NC.xn64(...)) with P = NC.P_of(512) for the norm entries.  They
hold for the fallback class by the derivation of tests/test_gpu_csr_span.py: there every non-zero's product is rounded to the 2^-28
fixed point on its own; a ladder row has at most 460 non-zeros and at most 8 dense K slices, so a sum is off by at most
468 * 2^-29 = 8.7e-7, inside the 1e-6 per sum that the rotation carries through |cos| and |sin| (and the pair through 1.1 |u| and
|silu(g)|).  No gate is widened from what a kernel returns.

Every parity assertion prints the worst error / tolerance per span class and names the span classes of failing outputs; for a
rotated output the class is that of its own column AND of its partner's ("a / partner b")."""
import os
import re

import numpy as np
import pytest

from tests import norm_front_cases as NC
from tests import test_gpu_csr_span as CS
from tests import test_gpu_gated as GT
from tests import test_gpu_linear as TL
from tests import test_gpu_linear_bf16 as BF
from tests import test_gpu_norm_front as NF
from tests import test_gpu_qkv_rope as TQ

gpu_test = pytest.mark.gpu
K, N = CS.K, CS.N
CAP = CS.CAPS["gated"]  # 1792: every entry here
LIMIT = CS.LIMIT
# entry -> (family, type, norm prologue)
ENTRIES = {"qkv_rope_f16": ("rope", "float16", False), "qkv_rope_bf16": ("rope", "bfloat16", False),
           "gated_norm_f16": ("gated", "float16", True), "gated_norm_bf16": ("gated", "bfloat16", True),
           "qkv_rope_norm_f16": ("rope", "float16", True), "qkv_rope_norm_bf16": ("rope", "bfloat16", True)}
ROUTES = {("rope", False): "qkv_rope", ("gated", True): "gated_norm", ("rope", True): "qkv_rope_norm"}
MEMBERS = {"rope": "aba", "gated": "ab"}  # the ladders of q, k, v | gate, up
ROPE_CONFIGS = [(128, "half"), (64, "interleaved")]
# the row factors of the norm activations: NC.ROW_SCALES (the small row, the massive row 2) and three more, so that the eight rows
# of a batch tile have r more than a factor of 2 apart, pair by pair (asserted in section 1)
NORM_SCALES = NC.ROW_SCALES + (0.2, 60.0, 0.006)
P = NC.P_of(K)


# ---- operands and references, one per key ----

def _partner(D, layout):
    """the column each column of a rotated member is paired with"""
    c = np.arange(N)
    if layout == "interleaved":
        return c ^ 1
    r = c % D
    return c - r + (r + D // 2) % D


def _configs(family):
    return ROPE_CONFIGS if family == "rope" else [(None, None)]


_ACTS, _NSUMS = {}, {}


def _norm_acts(rows, dtype):
    """(x16, g16) of the norm entries, CPU tensors"""
    if (rows, dtype) not in _ACTS:
        _ACTS[(rows, dtype)] = NC.activations(rows, K, dtype, scales=NORM_SCALES)
    return _ACTS[(rows, dtype)]


def _norm_sum(device, bits, which, topX, rows, dtype):
    """(fp64 sums + bias, A) of a ladder on the fp64 normalised activations; every partial sum in range"""
    key = (str(device), bits, which, topX, rows, dtype)
    if key not in _NSUMS:
        lay, npl, mag = CS.ladder_layer(device, bits, which, topX)
        x16, g16 = _norm_acts(rows, dtype)
        xn = NC.xn64(NC.widen(x16), NC.widen(g16), NC.EPS)
        s, A = TL._exact(npl, xn, CS._kind(lay)), NC.abs_sum(mag, xn)
        assert (A + np.abs(npl["bias"]) < LIMIT).all()  # no non-finite result is admissible
        _NSUMS[key] = (s, A)
    return _NSUMS[key]


def _plain_sum(device, bits, which, topX, x, rows, dtype, positive=False):
    lay, npl, mag = CS.ladder_layer(device, bits, which, topX)
    assert (BF._abs_sum(npl, mag, x) < LIMIT).all()  # every partial sum is in range: no non-finite result is admissible
    return CS._sum(device, bits, which, topX, x, (rows, dtype, positive))


def _inputs(device, rows, entry):
    """(x on the device, norm weight on the device or None, eps)"""
    family, dtype, norm = ENTRIES[entry]
    if norm:
        x16, g16 = _norm_acts(rows, dtype)
        return x16.to(device), g16.to(device), NC.EPS
    return CS._x(device, rows, dtype), None, None


def _member_refs(device, bits, rows, entry, topX, x):
    """{ladder: (sums, A or None)}"""
    family, dtype, norm = ENTRIES[entry]
    if norm:
        return {w: _norm_sum(device, bits, w, topX, rows, dtype) for w in "ab"}
    return {w: (_plain_sum(device, bits, w, topX, x, rows, dtype), None) for w in "ab"}


def _expected(entry, refs, pos, D, layout):
    """[(exact, tolerance)] per output of the entry: the existing suites' references and gates"""
    family, dtype, norm = ENTRIES[entry]
    (sa, Aa), (sb, Ab) = refs["a"], refs["b"]
    if family == "gated":
        return [(GT._silu(sa) * sb, NC.gated_gate(sa, sb, Aa, Ab, dtype, P))]
    cos, sin = TQ._tables(D)
    if norm:
        return [NC.rotated_gate(sa, Aa, pos, cos, sin, D, layout, dtype, P), NC.rotated_gate(sb, Ab, pos, cos, sin, D, layout, dtype, P),
                (sa, NC.plain_gate(sa, Aa, dtype, P))]
    return [TQ._rotated(sa, pos, cos, sin, D, layout, dtype), TQ._rotated(sb, pos, cos, sin, D, layout, dtype), TQ._plain(sa, dtype)]


_LABELS = {}


def _labels(entry, rows, D, layout):
    """per output of the entry: (span class per (batch row, column) as [rows, N] strings -- a rotated output: "own / partner
    <its>" --, the classes that string names as a bit mask per (batch row, column)); the class is that of the row's own batch
    tile, as CS._tile_labels has it"""
    family = ENTRIES[entry][0]
    key = (family, rows, D, layout)
    if key not in _LABELS:
        per_nb = {}
        for nb in CS._tile_rows(rows):
            lab = CS._labels("gated", nb)
            if family == "gated":
                cols = [lab["pair"]]
            else:
                p = _partner(D, layout)
                cols = [np.char.add(np.char.add(lab[w], " / partner "), lab[w][p]) for w in "ab"] + [lab["a"]]
            per_nb[nb] = [(c, np.array([sum(1 << i for i, name in enumerate(CS.CLASSES) if name in s) for s in c.tolist()])) for c in cols]
        bt = 1 if rows <= 1 else 2 if rows == 2 else 4 if rows <= 4 else 8  # (CS._tile_labels)
        nbs = [min(bt, rows - b // bt * bt) for b in range(rows)]
        _LABELS[key] = [(np.stack([per_nb[nb][i][0] for nb in nbs]), np.stack([per_nb[nb][i][1] for nb in nbs])) for i in range(len(per_nb[nbs[0]]))]
        if family == "gated":
            assert np.array_equal(_LABELS[key][0][0], CS._tile_labels("gated", rows, "pair"))
    return _LABELS[key]


def _mask_name(m):
    return " + ".join(c for i, c in enumerate(CS.CLASSES) if m >> i & 1) or "-"


def _fallback(lab):
    return (lab[1] & 4) != 0


def _inside(y, exact, tol, what, lab, where=None):
    """every selected output finite and inside the gate; prints the worst error / tolerance per span class (of the column and, for a
    rotated output, its partner); a failure names the classes of the failing outputs"""
    labels2, masks = lab
    got = y.float().cpu().numpy().astype(np.float64).reshape(exact.shape)
    sel = np.ones(exact.shape, bool) if where is None else where
    nf = sel & ~np.isfinite(got)
    assert not nf.any(), f"{what}: {int(nf.sum())} non-finite outputs -- by span class: {CS._by_class2(nf, labels2)}"
    with np.errstate(all="ignore"):
        ratio = np.where(sel, np.abs(got - exact) / tol, 0.0)
    print(f"{what}: worst error / tolerance by span class: " + "; ".join(f"[{_mask_name(m)}] {float(ratio[masks == m].max()):.3g}" for m in np.unique(masks)))
    bad = sel & ~(np.abs(got - exact) <= tol)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(sel.sum())} outputs outside the gate; worst {float(ratio.max()):.3g} x -- by span class: {CS._by_class2(bad, labels2)}"


def _module(entry, lays, D, layout, fold=True):
    """lays: {ladder: torch operands}"""
    family = ENTRIES[entry][0]
    if family == "gated":
        return CS._pair_module([lays[w] for w in MEMBERS[family]], fold=fold)
    mod = TQ._module([(lays[w], None, None, None) for w in MEMBERS[family]], D, layout)
    if not fold:
        for m in (mod.q, mod.k, mod.v):
            m.fold_topx = False
    return mod


def _call(mod, entry, x, w, eps, rope):
    """-> the entry's outputs as [rows, N] tensors; the route is the entry's own"""
    import torch

    family, dtype, norm = ENTRIES[entry]
    rows = x.shape[0]
    xin = x if rows > 1 else x.reshape(1, 1, K)
    if family == "gated":
        outs = [mod(xin, w, eps)]
    elif norm:
        outs = list(mod(xin, *rope, norm_weight=w, norm_eps=eps))
    else:
        outs = list(mod(xin, *rope))
    assert mod.last_route == ROUTES[(family, norm)]
    for o in outs:
        assert o.dtype == getattr(torch, dtype) and o.shape[-1] == N
    return [o.reshape(rows, N) for o in outs]


def _descriptors(mod, entry, lays, topX):
    """each descriptor holds the ladder's own CSR: nothing folded in, the top-X rows (if any) beside it"""
    family = ENTRIES[entry][0]
    if family == "gated":
        d = next(iter(mod._desc.values()))[2][0]
        ops = (d.gate, d.up)
    else:
        d = next(iter(mod._desc.values()))[1][0]
        ops = (d.q, d.k, d.v)
    for op, w in zip(ops, MEMBERS[family]):
        CS._descriptor_csr(op, lays[w], topX)


def _clean(mod, entry):
    (GT._workspaces_clean if ENTRIES[entry][0] == "gated" else TQ._clean)(mod)


NAMES = {"rope": "qkv", "gated": ("pair",)}


# ---- 1. the conditions (no GPU) ----

def test_every_front_policy_orders_its_csr_adds():
    """CAP = kCsrSpanMax - kCsrEdge = 1792 for all six entries: both finishing policies say kOrderedCsr = true, and the three kernel
    files of the entries instantiate the role with them (the norm ones with RmsVec as well)"""
    csrc = os.path.join(CS.ROOT, "squeezellm_amd", "csrc")
    src = lambda name: open(os.path.join(csrc, name)).read()  # noqa: E731
    assert re.search(r"struct\s+RopeFinish\s*\{[^}]*?static\s+constexpr\s+bool\s+kOrderedCsr\s*=\s*true\s*;", src("sqllm_rope_finish.h"))
    assert re.search(r"struct\s+PairFinish\s*\{[^}]*?static\s+constexpr\s+bool\s+kOrderedCsr\s*=\s*true\s*;", src("sqllm_pair_finish.h"))
    for name, fin in (("sqllm_linear_qkv.hip", "RopeFinish"), ("sqllm_linear_qkv_norm.hip", "RopeFinish"), ("sqllm_linear_gated_norm.hip", "PairFinish")):
        text = src(name)
        assert f"using FIN = {fin}<OT>;" in text and re.search(r"csr_role<T, BT, XT, AT, false, false, NoGate, kCsrChunk, FIN[,>]", text), name
    for name in ("sqllm_linear_qkv_norm.hip", "sqllm_linear_gated_norm.hip"):
        assert "using VP = RmsVec<XT, BT>;" in src(name)
    assert "constexpr int CAP = kCsrSpanMax - (ORD ? kCsrEdge : 0);" in src("sqllm_roles.h") and CAP == CS.SPAN_MAX - CS.EDGE == 1792


@pytest.mark.parametrize("nb", CS.TILE_ROWS)
def test_ladders_inhabit_every_class_and_every_kind_of_pair(nb):
    """The class conditions of tests/test_gpu_csr_span.py at CAP 1792 (that file's own test, called: it prints the table), and per
    rotary config and rotated member the pairs by the classes of their two columns.  "Different classes" counts an empty CSR row
    -- finished by a dense workgroup -- as a class of its own, as the pairs this file is about do; the pairs with one column in LDS
    and one in the fallback are counted on their own and required where the ladders have them (head dimension 128: the partner
    is 64 columns away; next-door partners of different classes need two adjacent non-empty rows across a chunk boundary)."""
    CS.test_ladders_inhabit_every_class("gated", nb)
    for D, layout in ROPE_CONFIGS:
        p = _partner(D, layout)
        assert (p[p] == np.arange(N)).all() and (p != np.arange(N)).all()
        lo = np.flatnonzero(np.arange(N) < p)
        assert lo.size == N // 2 and (p[lo] - lo == (1 if layout == "interleaved" else D // 2)).all()
        total = np.zeros(4, np.int64)
        for member, w in (("q", "a"), ("k", "b")):
            lab = CS.column_classes(CS.ladder_rows(w), nb, CAP)
            a, b = lab[lo], lab[p[lo]]
            fa, fb = np.char.find(a, CS.CLASSES[2]) >= 0, np.char.find(b, CS.CLASSES[2]) >= 0
            counts = np.array([(a != b).sum(), (fa & fb).sum(), (((a == "-") & fb) | ((b == "-") & fa)).sum(),
                               ((a != "-") & (b != "-") & (fa != fb)).sum()])
            print(f"D {D} {layout} nb {nb} {member} (ladder {w}): pairs of different classes {counts[0]}, both in the fallback {counts[1]}, "
                  f"one empty and one in the fallback {counts[2]}, one in LDS and one in the fallback {counts[3]}")
            assert counts[0] > 1500 and counts[1] >= 26 and counts[2] >= 1, (member, counts)
            total += counts
        if layout == "half":
            assert total[3] >= 1, "no pair with one column accumulated in LDS and one in the fallback"


@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_later_row_groups_have_an_r_of_their_own(dtype):
    """For every chunk that is not in the one-group class and every batch row b of a later group, r of row b is more than a factor
    of 2 from r of row b - g (the previous group's row), of row b mod g (bb instead of bs + bb) and of row 0, within the row's own
    batch tile.  (Fallback chunks: g = 1.)  The exact inputs of section 6 have r = 2^-b: distinct by construction."""
    seen = set()
    for rows in (2, 3, 8, 19):
        x16, g16 = _norm_acts(rows, dtype)
        r = NC.r64(NC.widen(x16), NC.EPS)[:, 0]
        assert np.isfinite(r).all() and (r > 0).all()
        bt = 2 if rows == 2 else 4 if rows <= 4 else 8
        for b0 in range(0, rows, bt):
            nb = min(bt, rows - b0)
            assert nb in CS._tile_rows(rows)
            for w in "ab":
                for e0, e1, c_lo, c_hi, n in CS.span_model(CS.ladder_rows(w)):
                    if CS.chunk_class(n, nb, CAP) == CS.CLASSES[0]:
                        continue
                    g = CS.group_rows(n, nb, CAP) if n <= CAP else 1
                    seen.add(g)
                    for bb in range(g, nb):
                        for other in (bb - g, bb % g, 0):
                            f = r[b0 + bb] / r[b0 + other]
                            assert max(f, 1 / f) > 2, (rows, b0, bb, other, g, f)
    assert {1, 2} <= seen and max(seen) > 2, seen  # single rows, pairs, and groups of more than two


# ---- 2. parity ----

def _parity(gpu, bits, rows, entry, topX=0, calls=3):
    family, dtype, norm = ENTRIES[entry]
    x, w, eps = _inputs(gpu, rows, entry)
    lays = {lw: CS.ladder_layer(gpu, bits, lw, topX)[0] for lw in "ab"}
    refs = _member_refs(gpu, bits, rows, entry, topX, x)
    pos = TQ._positions(rows)
    for D, layout in _configs(family):
        mod = _module(entry, lays, D, layout, fold=not topX)
        rope = TQ._dev(gpu, pos, *TQ._tables(D)) if family == "rope" else None
        want = _expected(entry, refs, pos, D, layout)
        labels = _labels(entry, rows, D, layout)
        for rep in range(calls):  # the later calls run on the workspace and the pair words the earlier ones left
            outs = _call(mod, entry, x, w, eps, rope)
            for name, o, (exact, tol), lab in zip(NAMES[family], outs, want, labels):
                _inside(o, exact, tol, f"{entry} w{bits} rows={rows} topX={topX} D={D} {layout} call {rep} {name}", lab)
        _descriptors(mod, entry, lays, topX)
        _clean(mod, entry)


@gpu_test
@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("rows", [1, 2, 3, 8, 19])
@pytest.mark.parametrize("bits", [3, 4])
def test_front_span_ladder_matches_oracle_and_cleans_up(gpu, bits, rows, entry):
    """The gates are the existing suites', unchanged (module docstring: they hold for the fallback by derivation)."""
    _parity(gpu, bits, rows, entry)


# ---- 3. many K slices ----

@gpu_test
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_front_span_ladder_with_many_k_slices(gpu, entry):
    """target_wgs = 4096 (tests/test_gpu_csr_span.py: test_span_ladder_with_many_k_slices): a column completes after several dense
    contributions plus its chunks, whoever comes last -- and only then meets its partner"""
    from squeezellm_amd import _lib

    old = _lib.get_option("target_wgs")
    _lib.set_option("target_wgs", 4096)
    try:
        _parity(gpu, 4, 3, entry)
    finally:
        _lib.set_option("target_wgs", old)


# ---- 4. top-X rows passed unfolded ----

@gpu_test
@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("bits", [3, 4])
def test_front_span_ladder_with_unfolded_topx_rows(gpu, bits, rows, entry):
    """fold_topx = False on the members and 70 top-X rows with a repeated index and the last column: for the norm entries topx_role
    runs with RmsVec beside wide-span chunks, and the CSR classes stay as built; _descriptors reads topX == 70 and the ladder's own
    CSR back from every member's descriptor."""
    _parity(gpu, bits, rows, entry, topX=70)


# ---- 5. run-to-run identity ----

@gpu_test
@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("rows", [3, 8])
@pytest.mark.parametrize("bits", [3, 4])
def test_front_span_ladder_is_bit_reproducible(gpu, bits, rows, entry):
    """Five calls, bit for bit, over all columns of all outputs.  In the row-group chunks the edge table is re-zeroed per group of
    batch rows; in the fallback the adds are integer and a lane's sums come out of a fixed DPP order.  The two are asserted
    separately, so that a difference names where it is (a rotated output counts as fallback when its column or its partner's is)."""
    import torch

    family, dtype, norm = ENTRIES[entry]
    x, w, eps = _inputs(gpu, rows, entry)
    lays = {lw: CS.ladder_layer(gpu, bits, lw)[0] for lw in "ab"}
    pos = TQ._positions(rows)
    for D, layout in _configs(family):
        mod = _module(entry, lays, D, layout)
        rope = TQ._dev(gpu, pos, *TQ._tables(D)) if family == "rope" else None
        runs = [[o.view(torch.int16).clone() for o in _call(mod, entry, x, w, eps, rope)] for _ in range(5)]
        torch.cuda.synchronize()
        labels = _labels(entry, rows, D, layout)
        for i, (name, lab) in enumerate(zip(NAMES[family], labels)):
            diff = torch.stack([r[i] != runs[0][i] for r in runs[1:]]).any(dim=0).cpu().numpy()
            fb = _fallback(lab)
            assert not (diff & ~fb).any(), f"{entry} D={D} {layout} {name}: outputs of chunks that accumulate in LDS differ between runs: {CS._by_class2(diff & ~fb, lab[0])}"
            assert not (diff & fb).any(), f"{entry} D={D} {layout} {name}: outputs of fallback-class columns differ between runs: {CS._by_class2(diff & fb, lab[0])}"
        _clean(mod, entry)
    _parity(gpu, bits, rows, entry, calls=1)


# ---- 6. the norm entries equal their parents fed xn, bit for bit ----

@gpu_test
@pytest.mark.parametrize("entry", [e for e in ENTRIES if ENTRIES[e][2]])
@pytest.mark.parametrize("rows", [3, 8])
@pytest.mark.parametrize("bits", [3, 4])
def test_norm_entries_equal_their_parents_fed_xn_on_the_ladder(gpu, bits, rows, entry):
    """The exact inputs of tests/test_gpu_norm_front.py (|x[b, k]| = 2^b, g in {0.5, 1, 2}, eps = 0: r = 2^-b, and xn = +-g is exact
    in 16 bits and in every summation order): gated_norm(x, g) == gated(xn) and qkv_rope_norm(x, g) == qkv_rope(xn) as int16 over
    all columns.  Both sides add the same fp32 values in the same fixed order, so one wrong r in a later row group or in a
    fallback round -- a factor of 2 at least -- changes bits."""
    import torch

    family, dtype, norm = ENTRIES[entry]
    x16, g16, xn16 = NF._exact_inputs(rows, K, dtype, 100 * bits + rows)
    x, w, xn = x16.to(gpu), g16.to(gpu), xn16.to(gpu)
    parent = {e: v for e, v in ENTRIES.items() if v == (family, dtype, False)}
    lays = {lw: CS.ladder_layer(gpu, bits, lw)[0] for lw in "ab"}
    pos = TQ._positions(rows)
    for D, layout in _configs(family):
        mod = _module(entry, lays, D, layout)
        rope = TQ._dev(gpu, pos, *TQ._tables(D)) if family == "rope" else None
        if family == "gated":
            want = [mod(xn).reshape(rows, N).clone()]
            assert mod.last_route == "gated"
        else:
            want = [o.clone() for o in _call(mod, next(iter(parent)), xn, None, None, rope)]
        got = _call(mod, entry, x, w, 0.0, rope)
        for name, a, b, lab in zip(NAMES[family], got, want, _labels(entry, rows, D, layout)):
            assert torch.isfinite(b.float()).all()
            diff = (a.view(torch.int16) != b.view(torch.int16)).cpu().numpy()
            assert not diff.any(), f"{entry} D={D} {layout} {name}: {int(diff.sum())} outputs differ from the parent's -- by span class: {CS._by_class2(diff, lab[0])}"
        _clean(mod, entry)


# ---- 7. flags (and, for the plain rotary entries, the range rule) through the CSR on later row groups ----

def _rotated_scaled(s, rho, pos, cos, sin, D, layout, dtype):
    """TQ._rotated with the slack of 1e-6 PER SUM times that sum's rho (tests/test_gpu_csr_span.py: _tol_scaled derives rho from
    the operands); rho = 1: TQ._rotated itself (asserted where it is used)"""
    lo, hi = TQ._split(s, D, layout)
    r_lo, r_hi = TQ._split(rho, D, layout)
    c, sn = TQ._at(cos, pos).astype(np.float64), TQ._at(sin, pos).astype(np.float64)
    e_lo, e_hi = lo * c - hi * sn, hi * c + lo * sn

    def tol(e, a, b, wc, ws):  # wc / ws: rho of the sum that meets cos / sin
        return np.maximum(np.abs(e), 2.0 ** -14) * TQ.EPS[dtype] + (np.abs(c) * wc + np.abs(sn) * ws) * 1e-6 + (np.abs(a) + np.abs(b)) * 2.0 ** -22 + 1e-6

    return TQ._merge(e_lo, e_hi, layout), TQ._merge(tol(e_lo, lo * c, hi * sn, r_lo, r_hi), tol(e_hi, hi * c, lo * sn, r_hi, r_lo), layout)


def _variants():
    return [(e, p) for e in ENTRIES for p in ("+inf", "-inf", "nan") + (("range",) if not ENTRIES[e][2] else ())]


@gpu_test
@pytest.mark.parametrize("entry,poison", _variants())
@pytest.mark.parametrize("bits", [3, 4])
def test_front_flags_and_range_rule_through_the_csr(gpu, bits, poison, entry):
    """8 rows.  "+inf" / "-inf" / "nan": a CSR value is that, at the entries CS._poison_targets(ladder, 1792) picks -- one per row,
    in rows whose chunks accumulate in LDS only (in the fallback class a flag can be lost: include/sqllm_hip.h) -- in EVERY member,
    at its own ladder's targets.  The expected NaN / +inf / -inf pattern is the fp32 formula's: TQ._f32_formula on the fp32-rounded
    oracle sums (both columns of a hit pair are non-finite, with the signs the table entries give), silu(g32) * u32 for the pair.
    All other outputs -- every fallback-class column among them -- are finite and inside the gate; a second call shows no lingering
    flag; workspaces and pair planes are left clean.
    "range" (the two plain rotary entries; tests/test_gpu_norm_front.py has the rule for normalised sums, whose input cannot be set
    to 2^8 by column): the value is 2^10 and the activations of its column are 2^8 -- one product beyond 131072: the hit column and
    its partner are non-finite in both output types.  The clean outputs are held to the gate with the slack of each sum scaled by
    rho, its magnitude with the 2^8 columns over its magnitude as drawn (CS.test_flags_and_range_rule_through_the_csr derives it)."""
    import torch

    family, dtype, norm = ENTRIES[entry]
    rows = 8
    value = {"+inf": float("inf"), "-inf": float("-inf"), "nan": float("nan"), "range": 2.0 ** 10}[poison]
    if norm:
        x16, g16 = _norm_acts(rows, dtype)
        x, w, eps = x16.to(gpu), g16.to(gpu), NC.EPS
        xin = NC.xn64(NC.widen(x16), NC.widen(g16), NC.EPS)
    else:
        x, w, eps = CS._x(gpu, rows, dtype, positive=True).clone(), None, None
    x0 = x.clone()
    lays, npls, hits = {}, {}, {}
    for lw in "ab":
        lays[lw], npls[lw], tg = CS._poisoned(gpu, bits, lw, value, CAP)
        assert len({r for r, _ in tg.values()}) == 4
        for name, (r, e) in tg.items():
            assert CS.column_classes(CS.ladder_rows(lw), rows, CAP)[r].find(CS.CLASSES[2]) < 0, name  # in LDS
            if poison == "range":
                x[:, int(npls[lw]["cols"][e])] = 2.0 ** 8
        hits[lw] = sorted({r for r, _ in tg.values()})
    if not norm:
        xin = x.float().cpu().numpy().astype(np.float64)
    # how far the 2^8 activations raise sum_k |W x| + |bias| of each clean output (1 in the other variants; the poisoned columns
    # are not clean outputs, so the ladders' own magnitudes serve) -- from the operands, per output, never from a result
    mags = {lw: BF._abs_sum(*CS.ladder_layer(gpu, bits, lw)[1:], x) for lw in "ab"}
    rho = {lw: mags[lw] / BF._abs_sum(*CS.ladder_layer(gpu, bits, lw)[1:], x0) for lw in "ab"}
    assert all((r >= 1).all() for r in rho.values()) and (poison == "range" or all((r == 1).all() for r in rho.values()))
    assert norm or all((np.delete(mags[lw], hits[lw], axis=1) < LIMIT).all() for lw in "ab")  # the clean sums stay in range
    with np.errstate(all="ignore"):
        sums = {lw: TL._exact(npls[lw], xin, "spmv") for lw in "ab"}  # of the poisoned layers
    # the clean outputs' reference: the ladders' own sums (they differ from the poisoned layers' in the hit columns only)
    if poison == "range":
        refs = {lw: (sums[lw], None) for lw in "ab"}
        for lw in "ab":
            assert np.isfinite(sums[lw]).all() and (sums[lw][:, hits[lw]] > LIMIT).all()
    elif norm:
        refs = {lw: _norm_sum(gpu, bits, lw, 0, rows, dtype) for lw in "ab"}
    else:
        refs = {lw: (_plain_sum(gpu, bits, lw, 0, x, rows, dtype, positive=True), None) for lw in "ab"}
    for lw in "ab":
        clean = np.ones(N, bool)
        clean[hits[lw]] = False
        assert np.array_equal(refs[lw][0][:, clean], sums[lw][:, clean]) and np.isfinite(refs[lw][0][:, clean]).all()
    pos = TQ._positions(rows)
    hit_mask = {lw: np.isin(np.arange(N), hits[lw]) for lw in "ab"}
    for D, layout in _configs(family):
        # which outputs a poisoned entry reaches, and the fp32 formula's pattern there
        if family == "gated":
            reach = [np.broadcast_to(hit_mask["a"] | hit_mask["b"], (rows, N))]
            with np.errstate(all="ignore"):
                want32 = [torch.nn.functional.silu(torch.from_numpy(sums["a"].astype(np.float32))) * torch.from_numpy(sums["b"].astype(np.float32))]
            want = _expected(entry, refs, pos, D, layout)
        else:
            p = _partner(D, layout)
            cos, sin = TQ._tables(D)
            reach = [np.broadcast_to(hit_mask[lw] | hit_mask[lw][p], (rows, N)) for lw in "ab"] + [np.broadcast_to(hit_mask["a"], (rows, N))]
            with np.errstate(all="ignore"):
                want32 = [torch.from_numpy(TQ._f32_formula(sums[lw], pos, cos, sin, D, layout)) for lw in "ab"] + [torch.from_numpy(sums["a"].astype(np.float32))]
            if poison == "range":
                want = [_rotated_scaled(sums[lw], rho[lw], pos, cos, sin, D, layout, dtype) for lw in "ab"]
                want.append((sums["a"], CS._tol_scaled(sums["a"], TQ.EPS[dtype], rho["a"])))
            else:
                want = _expected(entry, refs, pos, D, layout)
                if not norm:  # rho = 1: the scaled gates are the suite's own
                    for lw, (exact, tol) in zip("ab", want):
                        assert np.array_equal(_rotated_scaled(refs[lw][0], rho[lw], pos, cos, sin, D, layout, dtype)[1], tol)
                    assert np.array_equal(CS._tol_scaled(refs["a"][0], TQ.EPS[dtype], rho["a"]), want[2][1])
        if poison != "range":
            for w32, rc in zip(want32, reach):
                assert np.array_equal(~np.isfinite(w32.numpy()), rc)  # every output a poisoned sum reaches, and no other
                if poison == "nan":
                    assert torch.isnan(w32[torch.from_numpy(rc.copy())]).all()
        mod = _module(entry, lays, D, layout)
        rope = TQ._dev(gpu, pos, *TQ._tables(D)) if family == "rope" else None
        labels = _labels(entry, rows, D, layout)
        for rep in range(2):  # second call: the flags and pair words of the first must not linger
            outs = _call(mod, entry, x, w, eps, rope)
            for name, o, w32, rc, (exact, tol), lab in zip(NAMES[family], outs, want32, reach, want, labels):
                got = o.float().cpu()
                what = f"{entry} w{bits} {poison} D={D} {layout} call {rep} {name}"
                if poison == "range":
                    there = got[torch.from_numpy(rc.copy())]
                    assert (~torch.isfinite(there)).all(), f"{what}: {int(torch.isfinite(there).sum())} finite values where a product is out of range"
                else:
                    assert torch.equal(torch.isnan(got), torch.isnan(w32)), (what, int(torch.isnan(got).sum()), int(torch.isnan(w32).sum()))
                    assert torch.equal(torch.isposinf(got), torch.isposinf(w32)) and torch.equal(torch.isneginf(got), torch.isneginf(w32)), what
                with np.errstate(all="ignore"):
                    _inside(o, np.where(rc, 0.0, exact), np.where(rc, 1.0, tol), what, lab, where=~rc)
        _clean(mod, entry)


# ---- 8. the gates reject the likely defects (no GPU) ----

@pytest.mark.parametrize("entry", list(ENTRIES))
@pytest.mark.parametrize("bits", [3, 4])
def test_front_gates_admit_the_fp32_formula_and_reject_the_defects(bits, entry):
    """In numpy, on the ladders at 8 rows, per rotary config: the entry's fp32 formula on the true sums (norm entries: the sums of
    NC.xn32 in kernel order) stays inside its gate everywhere, and each defect below, applied to the true sums of ONE member (q, or
    the gate) and put through the same formula, leaves more than half of the outputs it touches -- for a rotated member the
    partners' outputs included -- outside it.  (1) - (4) are those of tests/test_gpu_csr_span.py; (5), (6): the norm entries' r of
    another row in the later row groups and the fallback rounds; (7): the rotary finisher of a fallback chunk's column pairing it
    with the slot of its neighbour -- modelled as the column's finished sum arriving as column c + 1's."""
    family, dtype, norm = ENTRIES[entry]
    nb = 8
    lay, npl, _ = CS.ladder_layer("cpu", bits, "a")
    npl_b = CS.ladder_layer("cpu", bits, "b")[1]
    if norm:
        x16, g16 = _norm_acts(nb, dtype)
        xw, gw = NC.widen(x16), NC.widen(g16)
        x64, r = NC.xn64(xw, gw, NC.EPS), NC.r64(xw, NC.EPS)[:, 0]
        refs = {w: _norm_sum("cpu", bits, w, 0, nb, dtype) for w in "ab"}
        xk = NC.xn32(xw, gw, NC.EPS, "kernel").astype(np.float64)
        formula_sums = {"a": TL._exact(npl, xk, "spmv"), "b": TL._exact(npl_b, xk, "spmv")}
    else:
        x = CS._x("cpu", nb, dtype)
        x64 = x.float().numpy().astype(np.float64)
        refs = {w: (_plain_sum("cpu", bits, w, 0, x, nb, dtype), None) for w in "ab"}
        formula_sums = {w: refs[w][0] for w in "ab"}
    s = refs["a"][0]
    rows = CS.ladder_rows("a")
    spans = CS.span_model(rows)
    cls = [CS.chunk_class(sp[4], nb, CAP) for sp in spans]
    cnt, first, last = CS.chunks_of_rows(rows)
    pos = TQ._positions(nb)
    for D, layout in _configs(family):
        exact, tol = _expected(entry, refs, pos, D, layout)[0]
        partner = _partner(D, layout) if family == "rope" else np.arange(N)

        def out_of_gate(sums, other=refs["b"][0]):
            s32 = sums.astype(np.float32)
            if family == "rope":
                f32 = TQ._f32_formula(s32, pos, *TQ._tables(D), D, layout)
            else:
                with np.errstate(over="ignore"):
                    f32 = (s32 / (np.float32(1) + np.exp(-s32))) * other.astype(np.float32)
            assert f32.dtype == np.float32
            return np.abs(GT._round_to(f32, dtype) - exact) > tol

        def touch(cols):
            cols = np.asarray(cols, np.int64)
            return np.unique(np.concatenate([cols, partner[cols]]))

        assert not out_of_gate(formula_sums["a"], formula_sums["b"]).any()
        # (1) the batch rows of the second row group receive the first group's sparse sums
        for ch in [i for i, c in enumerate(cls) if c == CS.CLASSES[1]]:
            g = CS.group_rows(spans[ch][4], nb, CAP)
            second = np.arange(g, min(2 * g, nb))
            share = CS._chunk_share(npl, x64, ch)
            held = np.flatnonzero((cnt > 0) & (first <= ch) & (last >= ch))
            d = s.copy()
            d[second] += share[second - g] - share[second]
            assert out_of_gate(d)[np.ix_(second, touch(held))].mean() > 0.5, ("second row group", ch)
        # (2) an edge-slot sum is added to the neighbouring batch row: the part of a heavy row in the first wave that holds it
        in_lds_heavy = [(int(rr), int(ch)) for rr in np.flatnonzero(cnt > 256) for ch in range(first[rr], last[rr] + 1) if cls[ch] != CS.CLASSES[2]]
        assert len(in_lds_heavy) >= 4
        d = s.copy()
        for rr, ch in in_lds_heavy:
            wave = (max(int(rows[rr]), ch * CS.CHUNK) - ch * CS.CHUNK) // 128
            q = CS._wave_share(npl, x64, ch, wave, rr)
            d[:, rr] += np.roll(q, 1) - q
        assert out_of_gate(d)[:, touch(sorted({rr for rr, _ in in_lds_heavy}))].mean() > 0.5
        # (3) one chunk's share of a straddling heavy row is dropped
        strad = np.flatnonzero((cnt > 256) & (last > first))
        assert len(strad) >= 3
        d = s.copy()
        for rr in strad:
            d[:, rr] -= CS._chunk_share(npl, x64, int(last[rr]))[:, rr]
        assert out_of_gate(d)[:, touch(strad)].mean() > 0.5
        # (4) the fallback's sums land one row off (c_lo + r + 1)
        fallback_chunks = [i for i, c in enumerate(cls) if c == CS.CLASSES[2]]
        assert fallback_chunks
        for ch in fallback_chunks:
            share = CS._chunk_share(npl, x64, ch)
            assert (share[:, N - 1] == 0).all()
            d = s - share + np.roll(share, 1, axis=1)
            touched = np.flatnonzero((share != 0).any(axis=0) | (np.roll(share, 1, axis=1) != 0).any(axis=0))
            assert out_of_gate(d)[:, touch(touched)].mean() > 0.5, ("fallback one row off", ch)
        # (5), (6) the chunk's share of a later group's batch row b is computed with r of row b - g | of row 0
        if norm:
            for ch in [i for i, c in enumerate(cls) if c != CS.CLASSES[0]]:
                g = CS.group_rows(spans[ch][4], nb, CAP) if cls[ch] == CS.CLASSES[1] else 1
                later = np.arange(g, nb)
                share = CS._chunk_share(npl, x64, ch)
                held = np.flatnonzero((share != 0).any(axis=0))
                for name, src in (("r of row b - g", later - g), ("r of row 0", np.zeros_like(later))):
                    d = s.copy()
                    d[later] += share[later] * (r[src] / r[later] - 1.0)[:, None]
                    assert out_of_gate(d)[np.ix_(later, touch(held))].mean() > 0.5, (name, ch, cls[ch])
        # (7) a fallback chunk's column is paired through the slot of c + 1
        if family == "rope":
            for ch in fallback_chunks:
                held = np.flatnonzero((cnt > 0) & (first <= ch) & (last >= ch))
                held = held[held < N - 1]
                d = s.copy()
                d[:, held + 1] = s[:, held]
                assert out_of_gate(d)[:, touch(held + 1)].mean() > 0.5, ("pair slot of c + 1", ch)
