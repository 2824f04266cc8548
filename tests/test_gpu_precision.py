"""fp32-class accuracy of every dense route, on the operand class the C ABI promises: a vec with 24 significant bits.

The neighbouring files feed fp16-born vec (lo plane zero, three bits of mid) and gate max|y - ref| / max|ref| at 2e-5; a split kernel
that lost one small partial product, read a wrong lo plane or took the five-product path for a vec with lo bits sits at ~1e-5 and
passes them (tests/test_precision_cpu.py proves both statements on the CPU).  Here every route of ROUTES / GROUP_ROUTES is driven
with operands whose every plane counts, against a numpy fp64 reference (tests/precision.py), under two gates that come from the
arithmetic, not from what the kernels give:

  (a) ONE non-zero vec element per batch row, mul = 0, forced-plane operands.  Chain routes: every output equals fl32(w * x) bit
      for bit (one product; every other k adds zero).  Split routes: |y - w x| <= 16 u |w x| (P.GATE_ONE_HOT_U; u = 2^-24).
  (b) the same with the CSR and top-X terms present: |y - ref| <= (T + c) u A, T = non-zero terms of the output, A = the sum of
      their magnitudes.  The T terms are T products (each rounded once, together <= u A) combined by T - 1 additions of non-zero
      operands (each <= u A; adding zero is exact): chain routes (T - 1 + 1) u A, stated with c = 1 for the second-order terms;
      split routes pay (a)'s 16 u |w x| <= 16 u A for the dense product instead of one rounding: c = 16.
  (c) dense fp32-born vec, small fp32-born mul: scaled_rms(route) <= 2 x scaled_rms(fp32 chain model on the same operands).
  (d) the has_lo decision of the wide form and the plane writers (sqllm_split_vec, sqllm_prepare_small): ONE forced-plane
      element in an otherwise fp16-born vec, and the converse.

Which kernel a label reaches is not taken on trust: tests/test_precision_cpu.py::test_route_manifest plans every row of the
tables below through the host layer linked against recording launchers and checks launcher and instantiation.
"""
import contextlib
import functools
import os

import numpy as np
import pytest

from tests import helpers as H
from tests import precision as P

pytestmark = pytest.mark.gpu

HUGE = 1 << 30
U = P.U
SHAPES = {4: [(256, 192), (1024, 132), (32, 8)], 3: [(192, 260), (1024, 776), (32, 8)]}  # ragged tiles in K and N, a single unit
C_SPLIT, C_CHAIN = 16, 1  # (b): the c of (T + c) u A


def _route(label, arith, batches, options, expect, entry="module", plannable=True, sparse_for_planes=False):
    return dict(label=label, arith=arith, batches=tuple(batches), options=options, expect=expect, entry=entry, plannable=plannable,
                sparse_for_planes=sparse_for_planes)


def _both(**kw):
    return dict(dense=kw, hybrid=kw)


# What each case is MEANT to reach.  expect[kind]: the dense launcher and the LaunchArgs fields that define the label (checked by
# the route manifest); "row_blocks": by batch.  A fused small launch takes scratch only for an op with sparse terms, so its
# planes / transposed vec exist for the hybrid kind alone -- sparse_for_planes: gate (a) then runs on hybrid operands whose CSR
# values and full rows are zero (the same plan, one non-zero term).
_SMALL = (7, 9, 13, 16)
_TILE_BLOCKS = {16: 1, 17: 2, 33: 4, 64: 4, 65: 4}
ROUTES = [
    _route("fused batch-1", "chain", (0, 1), dict(cols_min_batch=HUGE), _both(launcher="launch_fused")),
    _route("batch-1 column-lane", "chain", (0, 1), dict(cols_min_batch=1, cols_max_batch=1), _both(launcher="launch_batched_cols")),
    _route("batch tiles of exactly 2..8 rows", "chain", range(2, 9), dict(cols_min_batch=HUGE, mfma_min_batch=HUGE), _both(launcher="launch_fused")),
    _route("column-lane passes of 2..8 rows", "chain", range(2, 9), dict(cols_min_batch=2, cols_max_batch=8, mfma_min_batch=HUGE),
           _both(launcher="launch_batched_cols")),
    _route("fused small launch, planes + transposed vec", "split", _SMALL, dict(mfma_min_batch=7),
           dict(dense=dict(launcher="launch_small_split", planes=False, xT=False), hybrid=dict(launcher="launch_small_split", planes=True, xT=True)),
           sparse_for_planes=True),
    _route("fused small launch, in-register split (small_planes = 0)", "split", _SMALL, dict(mfma_min_batch=7, small_planes=0),
           dict(dense=dict(launcher="launch_small_split", planes=False, xT=False), hybrid=dict(launcher="launch_small_split", planes=False, xT=True))),
    _route("fused small launch, in-register split (no workspace)", "split", _SMALL, dict(mfma_min_batch=7),
           _both(launcher="launch_small_split", planes=False, xT=False), entry="ws-null"),
    _route("fused small launch, stream-ordered scratch", "split", _SMALL, dict(mfma_min_batch=7), _both(launcher="launch_small_split"),
           entry="named", plannable=False, sparse_for_planes=True),  # (its scratch is allocated on the stream: not plannable without a device)
    _route("tile form, 1 / 2 / 4 row blocks, sparse workgroups in the grid", "split", (16, 17, 33, 64, 65), dict(mfma_fuse_small=0),
           dict(dense=dict(launcher="launch_batched_mfma_split", wide=0, row_blocks=_TILE_BLOCKS),
                hybrid=dict(launcher="launch_batched_mfma_split_all", wide=0, row_blocks=_TILE_BLOCKS))),
    _route("tile form, 1 / 2 / 4 row blocks, sparse launch of its own", "split", (16, 17, 33, 64, 65), dict(mfma_fuse_small=0, mfma_fuse_sparse=0),
           _both(launcher="launch_batched_mfma_split", wide=0, row_blocks=_TILE_BLOCKS)),
    _route("wide form, planes", "split", (17, 130), dict(mfma_wide_min_batch=17, split_planes_min_batch=1),
           _both(launcher="launch_batched_mfma_split", wide=1, planes=True, flags=True)),
    _route("wide form, in-register split", "split", (17, 130), dict(mfma_wide_min_batch=17, split_planes_min_batch=HUGE),
           _both(launcher="launch_batched_mfma_split", wide=1, planes=False, flags=False)),
    _route("fp32 matrix instruction (control)", "chain", (9, 16, 17, 33, 65), dict(mfma_split=0), _both(launcher="launch_batched_mfma")),
]
# decode.OpSequence(fuse_shared_input=True): (rows, ops in the group) per case; widths of the group's ops, ragged
GROUP_WIDTHS = (132, 260, 64, 200)
GROUP_ROUTES = [
    dict(_route("grouped batch tiles", "chain", (), dict(cols_min_batch=HUGE, mfma_min_batch=HUGE), _both(launcher="launch_fused")),
         cases=((1, 2), (4, 3), (8, 4)), workspace=True),
    dict(_route("grouped column-lane passes", "chain", (), dict(cols_min_batch=1, cols_max_batch=8, mfma_min_batch=HUGE), _both(launcher="launch_batched_cols")),
         cases=((1, 3), (4, 4), (8, 2)), workspace=True),
    dict(_route("grouped fused small launch, workspace", "split", (), dict(mfma_min_batch=8),
                dict(dense=dict(launcher="launch_small_split", planes=False, xT=False), hybrid=dict(launcher="launch_small_split", planes=True, xT=True)),
                sparse_for_planes=True), cases=((8, 2), (13, 3), (13, 4)), workspace=True),
    dict(_route("grouped fused small launch, no workspace", "split", (), dict(mfma_min_batch=8), _both(launcher="launch_small_split"),
                entry="named", plannable=False, sparse_for_planes=True), cases=((8, 3), (13, 2)), workspace=False),
]
ALL_ROUTES = ROUTES + GROUP_ROUTES
assert len({r["label"] for r in ALL_ROUTES}) == len(ALL_ROUTES)


def make_operands(bits, K, N, kind, forced=False):
    """Seeded operands of one op; kind "hybrid0": the hybrid op's operands with every CSR value and full-row entry zero."""
    sparse = kind != "dense"
    case = H.make_case(bits, K, N, sparse=0.03 if sparse else 0, topX=3 if sparse else 0, heavy_rows=1 if sparse and N >= 8 else 0,
                       seed=bits * 1000 + K + N)
    if forced:
        case["lookup_table"] = P.forced_planes(case["lookup_table"])
    if kind == "hybrid0":
        case["vals"] = np.zeros_like(case["vals"])
        case["full_rows"] = np.zeros_like(case["full_rows"])
    return case


def route_cases(route, bits):
    """(shape list, batch, widths of the ops) of a route: what the GPU tests run and the manifest plans"""
    if "cases" in route:
        return [(1024, batch, GROUP_WIDTHS[:n]) for batch, n in route["cases"]] + [(192 if bits == 3 else 256, route["cases"][0][0], GROUP_WIDTHS[:2])]
    return [(K, batch, (N,)) for K, N in SHAPES[bits] for batch in route["batches"]]


@pytest.fixture(scope="module")
def qc():
    from squeezellm_amd import quant_cuda

    return quant_cuda


@contextlib.contextmanager
def options(opts):
    from squeezellm_amd import _lib

    old = {k: _lib.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            _lib.set_option(k, v)


def launch(qc, gpu, route, cases, kind, x, muls):
    """ys[i] = muls[i] + op_i(x) on the route: a single op through its entry, a group through decode.OpSequence"""
    import torch

    from squeezellm_amd import decode

    op_kind = "hybrid" if kind == "hybrid0" else kind
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(gpu)
    ys = [torch.from_numpy(np.ascontiguousarray(m)).to(gpu) for m in muls]
    with options(route["options"]):
        if "cases" in route:
            lays = [dict(H.to_torch(c, gpu), bits=c["bits"], K=c["K"], N=c["N"]) for c in cases]
            seq = decode.OpSequence(lays, [xt] * len(cases), ys, batched=True, fuse_shared_input=True, workspace=route["workspace"])
            assert [len(g) for g in seq.groups] == [len(cases)] and (route["workspace"] or seq._ws is None)
            seq.launch()
        else:
            H.call_op(qc, H.to_torch(cases[0], gpu), xt, ys[0], op_kind, x.ndim == 2, entry=route["entry"])
        torch.cuda.synchronize()
    return [y.cpu().numpy() for y in ys]


def hot_sets(batch, K, rng):
    """Hot positions per batch row, several sets: k = 0, K - 1, a k of the last unit, the middle, around a 32-k step; the first row at
    k = 0 and the last at K - 1 in one set, the other way round in the next."""
    pool = [0, K - 1, K - 5, K // 2 + 3, 31 % K, 32 % K, K - 32, 7]
    rows = max(batch, 1)
    sets = []
    for s in range(2 if rows >= 4 else 4):
        hk = np.array([pool[(b + 3 * s) % len(pool)] for b in range(rows)])
        hk[0], hk[-1] = (0, K - 1) if s % 2 == 0 else (K - 1, 0)
        if rows == 1:
            hk[0] = pool[s]
        if s >= 1 and rows > 2:
            hk[1:-1] = rng.integers(0, K, rows - 2)
        sets.append(hk)
    return sets


MEASURED = {}  # (label, bits) -> {figure: worst seen}


def _note(route, bits, name, value):
    m = MEASURED.setdefault((route["label"], bits), {})
    m[name] = max(m.get(name, 0.0), float(value))


def _describe(route, case, x, y, ref, bad):
    """the worst element of a failing case: route label, element, its k and the planes of the operands involved"""
    b, n = np.unravel_index(int(np.argmax(bad)), bad.shape)
    ks = np.nonzero(x[b])[0]
    W = H.oracle.dequantize(case["qweight"], case["lookup_table"], case["bits"])
    k = int(ks[0]) if ks.size else -1
    ops = f"x = {P.planes_hex(x[b, k])}, w = {P.planes_hex(W[k, n])}" if ks.size == 1 else f"{ks.size} non-zero vec elements in the row"
    return (f"route '{route['label']}' w{case['bits']} K={case['K']} N={case['N']} batch={x.shape[0]}: worst at row {b} col {n} (k = {k}): "
            f"got {float(y[b, n])!r} want {float(ref[b, n])!r}, |err| = {abs(float(y[b, n]) - float(ref[b, n])) / U:.3g} u; {ops}")


def _as2d(a):
    return a.reshape(1, -1) if a.ndim == 1 else a


def run_one_hot(qc, gpu, route, bits, kind):
    """gates (a) (kind dense / hybrid0) and (b) (kind hybrid) over the route's shapes, batches and hot sets"""
    rng = np.random.default_rng(17 + bits)
    c = C_SPLIT if route["arith"] == "split" else C_CHAIN
    for K, batch, widths in route_cases(route, bits):
        cases = [make_operands(bits, K, N, kind, forced=True) for N in widths]
        rows = max(batch, 1)
        for hot_k in hot_sets(batch, K, rng):
            x = P.one_hot_rows(rows, K, hot_k, P.hot_values(rng, rows))
            xin = x[0] if batch == 0 else x
            ys = launch(qc, gpu, route, cases, kind, xin, [np.zeros((rows, N) if batch else N, np.float32) for N in widths])
            for case, y in zip(cases, ys):
                y = _as2d(y)
                r = P.reference(case, x, np.zeros_like(y), "hybrid" if kind != "dense" else "dense")
                rel = P.over_abs(y, r["ref"], r["A"])
                assert (r["T"] >= 1).all()
                if kind == "hybrid":
                    bound = (r["T"] + c) * U
                    _note(route, bits, "hybrid_over_bound", (rel / bound).max())
                    assert (rel <= bound).all(), _describe(route, case, x, y, r["ref"], rel / bound)
                    continue
                assert (r["T"] == 1).all()
                _note(route, bits, "one_hot_u", rel.max() / U)
                if route["arith"] == "chain":
                    W = H.oracle.dequantize(case["qweight"], case["lookup_table"], bits)
                    want = W[hot_k, :] * x[np.arange(rows), hot_k][:, None]  # fl32(w * x)
                    assert np.array_equal(y.view(np.uint32), want.view(np.uint32)), _describe(route, case, x, y, want, y != want)
                else:
                    assert rel.max() <= P.GATE_ONE_HOT_U * U, _describe(route, case, x, y, r["ref"], rel)


@functools.lru_cache(maxsize=None)
def dense_operands(bits, K, N, batch, kind, born="fp32", rep=0):
    """operands of gate (c) and the scaled error the fp32 chain model makes on them (cached: routes share batches and shapes).  vec depends
    on (bits, K, batch, rep) alone: the ops of a group share it."""
    case = make_operands(bits, K, N, kind)
    rows = max(batch, 1)
    x = (P.fp32_born if born == "fp32" else P.fp16_born)(np.random.default_rng(bits * 7 + K + 31 * batch + 7919 * rep), (rows, K))
    mul = P.fp32_born(np.random.default_rng(bits * 7 + K + N + 31 * batch + 7919 * rep + 1), (rows, N), 0.05)
    r = P.reference(case, x, mul, kind)
    chain_err = (P.model_chain_op(case, x, mul, kind).astype(np.float64) - r["ref"]) / r["scale"]
    return case, x, mul, r, chain_err


MIN_OUTPUTS = 256  # gate (c) compares two rms figures: a case with fewer outputs is repeated with fresh vec / mul until it has as many


def run_dense(qc, gpu, route, bits, kind):
    """gate (c)"""
    for K, batch, widths in route_cases(route, bits):
        rows = max(batch, 1)
        reps = -(-MIN_OUTPUTS // (rows * min(widths)))
        errs = [[] for _ in widths]
        for rep in range(reps):
            ops = [dense_operands(bits, K, N, batch, kind, "fp32", rep) for N in widths]
            x = ops[0][1]
            ys = launch(qc, gpu, route, [o[0] for o in ops], kind, x[0] if batch == 0 else x, [o[2][0] if batch == 0 else o[2] for o in ops])
            for i, ((case, _, mul, r, chain_err), y) in enumerate(zip(ops, ys)):
                errs[i].append(((_as2d(y).astype(np.float64) - r["ref"]) / r["scale"], chain_err, case, x, _as2d(y), r))
        for per_op in errs:
            got = float(np.sqrt(np.mean(np.concatenate([e[0].ravel() for e in per_op]) ** 2)))
            chain = float(np.sqrt(np.mean(np.concatenate([e[1].ravel() for e in per_op]) ** 2)))
            _note(route, bits, "dense_x_chain", got / chain)
            e = max(per_op, key=lambda e: np.abs(e[0]).max())
            assert got <= P.GATE_DENSE_X_CHAIN * chain, (f"scaled rms {got:.3g} against {chain:.3g} of the fp32 chain model ({got / chain:.2f} x); "
                                                         + _describe(route, e[2], e[3], e[4], e[5]["ref"], np.abs(e[0])))


_IDS = [r["label"] for r in ALL_ROUTES]


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("route", ALL_ROUTES, ids=_IDS)
def test_one_hot_dense(qc, gpu, route, bits):
    """(a): one product per output.  Chain routes bit for bit fl32(w * x); split routes within 16 u."""
    run_one_hot(qc, gpu, route, bits, "hybrid0" if route["sparse_for_planes"] else "dense")


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("route", ALL_ROUTES, ids=_IDS)
def test_one_hot_hybrid(qc, gpu, route, bits):
    """(b): the hot element's CSR hits and top-X entries arrive too: (T + c) u A per output."""
    run_one_hot(qc, gpu, route, bits, "hybrid")


@pytest.mark.parametrize("kind", ["dense", "hybrid"])
@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("route", ALL_ROUTES, ids=_IDS)
def test_dense_vec_against_the_chain_model(qc, gpu, route, bits, kind):
    """(c): fp32-born vec and weights over all of K: no worse than twice the reference's own fp32 chain, by the CPU model of it."""
    run_dense(qc, gpu, route, bits, kind)


# ---- (d) the has_lo decision and the plane writers ----


def flag_workgroup(row, k, K):
    """workgroup of sqllm_split_vec (256 of them, 256 threads each, grid-stride) that handles vec[row][k]: fragment f = (row block of 16,
    k block of 32, lane = 16 * ((k / 8) % 4) + row % 16), k blocks per row block K / 32 + 1"""
    f = ((row // 16) * (K // 32 + 1) + k // 32) * 64 + 16 * ((k // 8) % 4) + row % 16
    return (f >> 8) & 255


def lo_positions(batch, K):
    """(row, k) of the one element with lo bits: first row / first k, last row / last k, an element of the last flag workgroup that has
    work, and a row of the last, partly filled row block next to its padding"""
    last_wg = max(flag_workgroup(r, k, K) for r in range(batch) for k in range(0, K, 8))
    in_last = next((r, k + 3) for r in range(batch - 1, -1, -1) for k in range(K - 8, -1, -8) if flag_workgroup(r, k, K) == last_wg)
    return [(0, 0), (batch - 1, K - 1), in_last, (batch - 2, K // 2 + 1)], last_wg


D_ROUTES = [r for r in ROUTES if r["label"] in ("wide form, planes", "fused small launch, planes + transposed vec")]
# wide form: 500 rows x K = 1024 make 32 x 33 x 64 = 67584 fragments, more than the 65536 threads of sqllm_split_vec's grid: all
# 256 flag words carry work and the last row block of 64 holds 52 rows.  Fused small launch: 13 of 16 rows.
D_BATCH = {"wide form, planes": 500, "fused small launch, planes + transposed vec": 13}


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("route", D_ROUTES, ids=[r["label"] for r in D_ROUTES])
def test_one_element_with_lo_bits(qc, gpu, route, bits):
    """(d): vec is fp16-born everywhere -- the row of the hot element: zero, which is an fp16 value too, so that the one-hot bound (b)
    applies to that element's outputs -- except ONE forced-plane element.  The wide form must take all six products on the strength of
    that one flag (its row misses the bound by >= 2^-16 |w x| = 256 u otherwise), the fused small launch must find the element's lo plane
    where sqllm_prepare_small wrote it; every other row stays within gate (c).  Then the converse: the element fp16-born as well (the
    wide form's five-product path), same bounds."""
    K, N, kind = 1024, 132, "hybrid"
    batch = D_BATCH[route["label"]]
    case, x0, mul, _, chain_err = dense_operands(bits, K, N, batch, kind, born="fp16")
    positions, last_wg = lo_positions(batch, K)
    if batch == 500:
        assert last_wg == 255
    rng = np.random.default_rng(5 + bits)
    for (row, k), hot in [(p, h) for p in positions for h in ("forced", "fp16-born")]:
        x = x0.copy()
        x[row] = 0
        x[row, k] = P.hot_values(rng, 1)[0] if hot == "forced" else np.float32(np.float16(0.5 + abs(rng.normal())))
        assert bool(P.split3(x)[2].any()) == (hot == "forced")
        m = mul.copy()
        m[row] = 0
        y = launch(qc, gpu, route, [case], kind, x, [m])[0]
        r = P.reference(case, x, m, kind)
        rel = P.over_abs(y, r["ref"], r["A"])
        bound = (r["T"][row] + C_SPLIT) * U
        _note(route, bits, "lo_element_over_bound", (rel[row] / bound).max())
        assert (rel[row] <= bound).all(), f"{hot} element at ({row}, {k}): " + _describe(route, case, x[row:row + 1], y[row:row + 1], r["ref"][row:row + 1], rel[row:row + 1] / bound)
        others = np.arange(batch) != row
        got = P.scaled_rms(y[others], r["ref"][others], r["scale"][others])
        chain = float(np.sqrt(np.mean(chain_err[others] ** 2)))
        _note(route, bits, "lo_rows_x_chain", got / chain)
        assert got <= P.GATE_DENSE_X_CHAIN * chain, f"{hot} element at ({row}, {k}): the other rows' scaled rms is {got / chain:.2f} x the chain model's"


REPORT = os.path.join(H.ROOT, "profiles", "precision_routes.txt")


def test_zz_write_measured_figures():
    """Writes what the cases above observed, per route and bit width, to profiles/precision_routes.txt (or $SQLLM_PRECISION_REPORT)
    -- only after a run of the whole file: a selection of cases leaves the committed figures alone.  These are measurements; no gate
    above comes from them."""
    want = {(r["label"], b) for r in ALL_ROUTES for b in (3, 4)}
    full = want <= set(MEASURED) and all({"one_hot_u", "hybrid_over_bound", "dense_x_chain"} <= set(MEASURED[k]) for k in want)
    if not full:
        return
    lines = ["# tests/test_gpu_precision.py on an MI355X: worst figure per route and bit width over its shapes, batches and hot sets.",
             "# one_hot_u: worst |y - w x| / |w x| in units of u = 2^-24, gate (a): chain routes bit for bit (one rounding: <= 1), split routes <= 16",
             "# hybrid_over_bound: worst |y - ref| / ((T + c) u A), gate (b): <= 1",
             "# dense_x_chain: scaled rms over the CPU fp32 chain model's on the same operands, gate (c): <= 2",
             "# lo_element_over_bound / lo_rows_x_chain: gate (d), same bounds",
             f"{'route':66s} bits  one_hot_u  hybrid_over_bound  dense_x_chain  lo_element_over_bound  lo_rows_x_chain"]
    for r in ALL_ROUTES:
        for b in (3, 4):
            m = MEASURED[(r["label"], b)]
            f = lambda n: f"{m[n]:.3f}" if n in m else "-"  # noqa: E731
            lines.append(f"{r['label']:66s} w{b}    {f('one_hot_u'):>9s}  {f('hybrid_over_bound'):>17s}  {f('dense_x_chain'):>13s}  {f('lo_element_over_bound'):>21s}  {f('lo_rows_x_chain'):>15s}")
            assert m["one_hot_u"] <= (P.GATE_ONE_HOT_U if r["arith"] == "split" else 1.0) and m["hybrid_over_bound"] <= 1 and m["dense_x_chain"] <= P.GATE_DENSE_X_CHAIN
    path = os.environ.get("SQLLM_PRECISION_REPORT", REPORT)
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
