"""Non-finite operand cases shared by tests/test_nonfinite_cases_cpu.py (which proves them) and the GPU files that run them
(tests/test_gpu_nonfinite_routes.py, the fused linears' files).  A plain module: no test lives here.

Shapes: the smallest at which every clamp of the kernels exists -- K = 544 is 68 units of 8 k's (4-bit) / 17 units of 32 (3-bit), two
top-X slabs of 256 k's plus 32 k's; N = 132 ends in a partial column tile; K = 1056 gives a ragged chunk share per wave with waves that
hold no unit (RAGGED in tests/test_gpu_cols_batch1.py).

One launch carries one POISON CLASS (V vec, C codebook, S CSR values, F full rows, M mul).  The expected NaN / +inf / -inf pattern is a
TERM-WISE model (pattern_model) that does not depend on the order of summation: every term of an output -- its `mul` element, every
dense product lut[c][idx] * x[k], every CSR product, every top-X product -- is classified on its two factors alone, and the output is
  NaN      if any term is NaN (a NaN factor, or 0 x inf), or if +inf and -inf terms are both present,
  +-inf    otherwise, if a term of that sign is infinite,
  finite   otherwise.
The generator never makes a 0 x inf term from live data (asserted in make: no operand element that meets a term is zero)."""
import functools

import numpy as np

from tests import helpers as H

SHAPES = {4: [(544, 132), (1056, 200)], 3: [(544, 132), (1056, 260)]}
GROUP_K, GROUP_WIDTHS = 544, (132, 260, 64, 200)
LINEAR_SHAPE, LINEAR_ROWS = (544, 132), (1, 3, 8)
CLASSES = ("V", "C", "S", "F", "M")
KINDS = ("dense", "spmv", "hybrid")
ONE_ROW_VARIANTS = 4  # class V at one row: one poison per launch, over the four positions of v_positions in turn


def applies(cls, kind):
    return {"V": True, "C": True, "S": kind in ("spmv", "hybrid"), "F": kind == "hybrid", "M": True}[cls]


def variants(cls, batch):
    return range(ONE_ROW_VARIANTS) if cls == "V" and batch <= 1 else range(1)


def v_positions(K):
    """(k, value) of class V's poisons: row 0, the last row, a middle row; at one row the three in turn and a +inf in mid-K"""
    return [(K - 1, np.inf), (0, -np.inf), (K - 32, np.nan), (K // 2 + 3, np.inf)]


@functools.lru_cache(maxsize=None)
def _base(bits, K, N, kind):
    """Finite operands of one op, with three columns that are in neither the CSR nor the top-X set (class C's), apart from the heavy
    column.  The seed is searched, deterministically, until the sets are disjoint."""
    free = (1, N // 2 + 1, N - 2)  # first tile, a middle one, the (partial) last tile
    if kind == "dense":
        return H.make_case(bits, K, N, seed=4000 * bits + K + N), free, None
    for seed in range(4000 * bits + K + N, 4000 * bits + K + N + 64):
        case = H.make_case(bits, K, N, sparse=0.03, topX=3, heavy_rows=1, empty_rows=free, seed=seed)
        counts = np.diff(case["rows"])
        heavy = int(np.argmax(counts))
        nonempty = np.nonzero(counts)[0]
        taken = set(case["full_row_indices"].tolist()) | {heavy}
        # class S poisons the first and the last non-zero of the matrix and the last one of the heavy column: three different columns,
        # none of them a top-X column (whose terms would be of mixed sign there)
        if taken.isdisjoint(free) and len(taken) == 4 and counts[heavy] > K // 8 and len({int(nonempty[0]), int(nonempty[-1])} | taken) == 6:
            if kind == "spmv":
                case["full_rows"] = case["full_row_indices"] = None
            return case, free, heavy
    raise AssertionError("no seed gives disjoint poison columns")


def _pattern_terms(X, W, present=None):
    """per (row, column): is there a NaN / +inf / -inf term among X[r, k] * W[k, c], k over the PRESENT entries of W"""
    P = np.ones(W.shape, bool) if present is None else present
    f = lambda m: m.astype(np.float64)  # noqa: E731  (counts of at most K: exact)
    xnan, xinf, x0, xpos, xneg = np.isnan(X), np.isinf(X), X == 0, X > 0, X < 0
    wnan, winf, w0, wpos, wneg = P & np.isnan(W), P & np.isinf(W), P & (W == 0), P & (W > 0), P & (W < 0)
    nan = f(xnan) @ f(P) + f(~xnan) @ f(wnan) + f(xinf) @ f(w0) + f(x0) @ f(winf)
    pos = f(xpos & xinf) @ f(wpos) + f(xpos) @ f(wpos & winf) + f(xneg & xinf) @ f(wneg) + f(xneg) @ f(wneg & winf)
    neg = f(xpos & xinf) @ f(wneg) + f(xpos) @ f(wneg & winf) + f(xneg & xinf) @ f(wpos) + f(xneg) @ f(wpos & winf)
    return nan > 0, pos > 0, neg > 0


def pattern_model(case, x, mul, kind):
    """(is NaN, is +inf, is -inf), each [rows, N], of mul + op(x) by the term-wise model of the module docstring"""
    X = np.asarray(x, np.float64).reshape(-1, case["K"])
    M = np.asarray(mul, np.float64).reshape(X.shape[0], case["N"])
    K, N = case["K"], case["N"]
    nan, pos, neg = np.isnan(M), np.isposinf(M), np.isneginf(M)
    W = H.oracle.dequantize(case["qweight"], case["lookup_table"], case["bits"]).astype(np.float64)
    terms = [_pattern_terms(X, W)]
    if kind in ("spmv", "hybrid"):
        S, P = np.zeros((K, N)), np.zeros((K, N), bool)
        col = np.repeat(np.arange(N), np.diff(case["rows"]))
        assert not P[case["cols"], col].any()
        S[case["cols"], col], P[case["cols"], col] = case["vals"], True
        assert P.sum() == case["vals"].size  # (no duplicate position: one term each)
        terms.append(_pattern_terms(X, S, P))
    if kind == "hybrid":
        t = _pattern_terms(X, case["full_rows"].astype(np.float64))
        scat = np.zeros((case["full_rows"].shape[1], N))
        scat[np.arange(scat.shape[0]), case["full_row_indices"]] = 1
        terms.append(tuple((m.astype(np.float64) @ scat) > 0 for m in t))
    for tn, tp, tm in terms:
        nan, pos, neg = nan | tn, pos | tp, neg | tm
    nan = nan | (pos & neg)
    return nan, pos & ~nan, neg & ~nan


def pattern_of(y):
    y = np.asarray(y).reshape(-1, np.asarray(y).shape[-1])
    return np.isnan(y), np.isposinf(y), np.isneginf(y)


def vec(bits, K, batch, cls, variant=0, scale=1.0):
    """vec of a launch, [rows, K] fp32: a function of (bits, K, batch, class, variant) alone, so the ops of a group share it.  Class V
    and M: Gaussian; the classes that poison a weight operand: strictly positive, so that an infinite weight gives ONE infinity."""
    rows = max(batch, 1)
    rng = np.random.default_rng([bits, K, rows, CLASSES.index(cls), variant])
    x = rng.normal(size=(rows, K)).astype(np.float32)
    if cls in ("C", "S", "F"):
        x = np.abs(x) + np.float32(0.01)
    x *= np.float32(scale)
    poisoned = np.zeros(rows, bool)
    if cls == "V":
        pos = v_positions(K)
        if rows == 1:
            x[0, pos[variant][0]] = pos[variant][1]
            poisoned[0] = True
        else:
            x[0, pos[0][0]], x[rows - 1, pos[1][0]] = pos[0][1], pos[1][1]
            poisoned[[0, rows - 1]] = True
            if rows >= 3:
                x[rows // 2, pos[2][0]] = pos[2][1]
                poisoned[rows // 2] = True
    return x, poisoned


@functools.lru_cache(maxsize=None)
def make(bits, K, N, kind, batch, cls, variant=0, scale=1.0):
    """One case: dict(case, x [rows, K], mul [rows, N], kind, named, clean) -- arrays read-only, shared between tests.
      named: list of (what, rows, cols, sign, mode): in the reference the outputs rows x cols are infinite and not NaN -- of that sign
             (sign 0: either) -- every one of them (mode "all") or at least one (mode "any"): the outputs that DISCRIMINATE, i.e. where a
             kernel that forms 0 x inf, or inf - inf of its own making, shows NaN instead;
      clean: bool [rows, N], outputs that no poison reaches: finite.
    batch 0 is the one-row op with a 1-D vec (callers pass x[0], mul[0]).  scale: of vec's finite elements (the fused linears keep sums small)."""
    assert applies(cls, kind) and variant in variants(cls, batch)
    base, free, heavy = _base(bits, K, N, kind)
    case = dict(base)
    rows = max(batch, 1)
    x, row_poisoned = vec(bits, K, batch, cls, variant, scale)
    mul = np.random.default_rng([bits, K, N, rows, 7]).normal(0, 0.5 * scale, (rows, N)).astype(np.float32)
    clean = np.ones((rows, N), bool)
    named = []
    every = np.arange(rows)
    sparse_cols = np.nonzero(np.diff(case["rows"]))[0] if kind != "dense" else None
    if cls == "V":
        clean[row_poisoned] = False
        if rows > 1 or variant == 0:  # the row with +inf at K - 1
            named.append(("any column", [0], np.arange(N), 0, "any"))
            if kind == "hybrid":
                named.append(("top-X columns", [0], case["full_row_indices"], 0, "any"))
            if kind != "dense":
                named.append(("columns with CSR non-zeros", [0], sparse_cols, 0, "any"))
        elif np.isinf(v_positions(K)[variant][1]):
            named.append(("any column", [0], np.arange(N), 0, "any"))
        if rows > 1:
            named.append(("any column of the -inf row", [rows - 1], np.arange(N), 0, "any"))
    elif cls == "C":
        idx = H.oracle.unpack_indices(case["qweight"], bits)
        lut = case["lookup_table"].copy()
        lut[free[0], idx[K - 1, free[0]]] = np.inf
        lut[free[1], idx[K - 1, free[1]]] = -np.inf
        lut[free[2], idx[0, free[2]]] = np.nan
        case["lookup_table"] = lut
        clean[:, list(free)] = False
        named += [("codebook +inf column", every, [free[0]], +1, "all"), ("codebook -inf column", every, [free[1]], -1, "all")]
    elif cls == "S":
        vals = case["vals"].copy()
        r = case["rows"]
        first, last = int(sparse_cols[0]), int(sparse_cols[-1])
        vals[0], vals[-1], vals[r[heavy + 1] - 1] = np.inf, -np.inf, np.nan
        case["vals"] = vals
        clean[:, [first, last, heavy]] = False
        named += [("column of the first non-zero", every, [first], +1, "all"), ("column of the last non-zero", every, [last], -1, "all")]
    elif cls == "F":
        fr = case["full_rows"].copy()
        fr[K - 1, 0], fr[0, 1], fr[K - 32, 2] = np.inf, -np.inf, np.nan
        case["full_rows"] = fr
        fi = case["full_row_indices"]
        clean[:, fi] = False
        named += [("top-X column 0", every, [fi[0]], +1, "all"), ("top-X column 1", every, [fi[1]], -1, "all")]
    else:  # M: three elements of the incoming mul, in different rows where there are as many
        spots = [(0, N - 1, np.inf), ((rows - 1) // 2 if rows < 3 else rows // 2, 0, -np.inf), (rows - 1, N // 2, np.nan)]
        for r_, c_, v_ in spots:
            mul[r_, c_] = v_
            clean[r_, c_] = False
        named += [("mul +inf", [spots[0][0]], [spots[0][1]], +1, "all"), ("mul -inf", [spots[1][0]], [spots[1][1]], -1, "all")]
    # no 0 x inf from live data: no element that meets a term is zero
    live = [x, H.oracle.dequantize(case["qweight"], case["lookup_table"], bits)]
    live += [case["vals"]] if kind != "dense" else []
    live += [case["full_rows"]] if kind == "hybrid" else []
    assert all((a != 0).all() for a in live)
    for a in [x, mul] + [v for v in case.values() if isinstance(v, np.ndarray)]:
        a.setflags(write=False)
    return dict(case=case, x=x, mul=mul, kind=kind, named=named, clean=clean)


@functools.lru_cache(maxsize=None)
def reference(bits, K, N, kind, batch, cls, variant=0):
    """helpers.oracle_ref of make(...)'s operands, [rows, N] fp64: computed once, shared, read-only"""
    c = make(bits, K, N, kind, batch, cls, variant)
    with np.errstate(all="ignore"):
        ref = np.asarray(H.oracle_ref(c["case"], c["x"], c["mul"], kind), np.float64)
    ref.setflags(write=False)
    return ref


def operator_cases():
    """every (bits, K, N, kind, batch, class, variant) that the route file can ask for: what the CPU test proves.  Batches: the union
    of the routes' thinned batches; the grouped routes' rows (1, 4, 8, 13) at K = 544 over the group widths."""
    out = []
    for bits in (3, 4):
        for kind in KINDS:
            for cls in CLASSES:
                if not applies(cls, kind):
                    continue
                shapes = [(K, N, b) for K, N in SHAPES[bits] for b in (0, 1, 2, 3, 6, 7, 9, 13, 16, 17, 65, 130)]
                shapes += [(GROUP_K, N, b) for N in GROUP_WIDTHS for b in (1, 4, 8, 13)]
                for K, N, b in dict.fromkeys(shapes):
                    out += [(bits, K, N, kind, b, cls, v) for v in variants(cls, b)]
    return out


# ---- the fused linears (16-bit activations, bias): classes V and C ----

LINEAR_SCALE = 0.25  # of vec and bias: |sum| stays below ~10, far inside the fp16 range


def linear_case(bits, kind, rows, cls, to16):
    """A fused linear's case: make(...) at LINEAR_SHAPE with vec scaled down and rounded to the 16-bit type by `to16` (float32 ->
    float32 holding 16-bit-born values; non-finite elements pass through), bias in place of mul.  Returns dict(case, x16 [rows, K], bias
    [N], nan / pos / neg: the model's pattern of bias + op(x16), named, clean).  Class V at one row: variant 0 (+inf at K - 1)."""
    K, N = LINEAR_SHAPE
    c = make(bits, K, N, kind, rows, cls, 0, LINEAR_SCALE)
    x16 = to16(c["x"])
    assert (x16[np.isfinite(x16)] != 0).all() and np.array_equal(np.isfinite(x16), np.isfinite(c["x"]))
    bias = (np.random.default_rng([bits, N, 11]).normal(0, LINEAR_SCALE, N)).astype(np.float32)
    nan, pos, neg = pattern_model(c["case"], x16, np.broadcast_to(bias, (rows, N)), kind)
    return dict(case=c["case"], x16=x16, bias=bias, nan=nan, pos=pos, neg=neg, named=c["named"], clean=c["clean"], kind=kind)


def writable(case):
    """a copy of a case's arrays (the shared ones are read-only; torch.from_numpy wants writable memory)"""
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}


def to_fp16(a):
    return a.astype(np.float16).astype(np.float32)


def to_bf16(a):
    """fp32 -> bf16 (round to nearest even; NaN and the infinities pass through) -> fp32"""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return np.where(np.isnan(a), np.float32(np.nan), b.astype(np.uint32).view(np.float32))


LINEAR_EPS = {"float16": 2.0 ** -10, "bfloat16": 2.0 ** -7}  # one ulp of the output type (tests/test_gpu_linear.py, test_gpu_linear_bf16.py)


def admit_nan_for_codebook_infinity(got, named):
    """The NARROWER class-C contract of the fp32 chain kernels' dense role and of the fp32 matrix-instruction kernel (include/sqllm_hip.h,
    "Non-finite operands"; DESIGN.md, "Clamp sites"): a +-inf codebook entry makes its column non-finite in every row -- NaN or that
    infinity -- and nothing else is touched.  Returns a copy of `got` [rows, N] in which a NaN in the outputs that class C names
    (the +inf and the -inf column, every row) is replaced by the infinity named: the caller's exact comparison then asserts exactly
    that contract -- those outputs NaN or that infinity, every other output as in the reference."""
    got = np.array(got, copy=True).reshape(-1, np.asarray(got).shape[-1])
    for _, rows, cols, sign, mode in named:
        assert sign != 0 and mode == "all"
        sub = got[np.ix_(np.asarray(rows), np.asarray(cols))]
        sub[np.isnan(sub)] = sign * np.inf
        got[np.ix_(np.asarray(rows), np.asarray(cols))] = sub
    return got


def compare_linear(got, c, exact, eps, what):
    """`got` [rows, N] fp64 of a fused linear against the case's model pattern; its finite outputs within one ulp of the output type of
    `exact` (+ the files' absolute slack of 1e-6)"""
    for name, g, m in zip(("NaN", "+inf", "-inf"), pattern_of(got), (c["nan"], c["pos"], c["neg"])):
        if not np.array_equal(g, m):
            row, col = np.argwhere(g != m)[0]
            raise AssertionError(f"{what}: {name} pattern differs in {int((g != m).sum())} outputs ({int(g.sum())} got, {int(m.sum())} in the model); "
                                 f"first at row {row} col {col}: got {got[row, col]!r}, exact {exact[row, col]!r}")
    fin = ~(c["nan"] | c["pos"] | c["neg"])
    tol = np.maximum(np.abs(exact[fin]), 2.0 ** -14) * eps + 1e-6
    bad = np.abs(got[fin] - exact[fin]) > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} finite outputs off by more than one ulp of the output type"


def run_linear(gpu, fuse, bits, kind, rows, cls, dtype):
    """One fused-linear case on the GPU: module from `fuse(layer)`, two calls (the flags of the first must not linger), pattern and
    finite outputs checked; returns the module, whose workspace the caller asserts zero."""
    import torch

    c = linear_case(bits, kind, rows, cls, to_fp16 if dtype == "float16" else to_bf16)
    K, N = LINEAR_SHAPE
    lay = dict(H.to_torch(writable(c["case"]), gpu), bias=torch.from_numpy(c["bias"].copy()).to(gpu))
    mod = fuse(lay)
    x = torch.from_numpy(c["x16"].copy()).to(gpu).to(getattr(torch, dtype))
    assert torch.equal(x.float().cpu(), torch.from_numpy(c["x16"].copy())) or cls == "V"  # (16-bit-born: the cast is exact; NaN != NaN)
    with np.errstate(all="ignore"):
        exact = np.asarray(H.oracle_ref(c["case"], c["x16"], np.broadcast_to(c["bias"], (rows, N)).copy(), kind), np.float64)
    what = f"w{bits} {kind} class {cls} rows={rows} {dtype} K={K} N={N}"
    for rep in range(2):
        y = mod(x if rows > 1 else x.reshape(1, 1, K))
        assert y.dtype == getattr(torch, dtype)
        got = y.reshape(rows, N).float().cpu().numpy().astype(np.float64)
        if cls == "C":  # (the dense role of the fused linears is the chain kernels': the narrower contract)
            got = admit_nan_for_codebook_infinity(got, c["named"])
        compare_linear(got, c, exact, LINEAR_EPS[dtype], f"{what} call {rep}")
    return mod
