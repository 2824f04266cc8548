"""The head of the column-lane kernel's one-row pieces (csrc/sqllm_kernels.hip: dense_role_cols, BT == 1): vec's first group of 32 k's is
requested with the piece's first loads, above the table build, from the piece's own u0 / u1 -- against the fp64 C oracle at the project's
2e-5, on the smallest shapes at which that request can go wrong.  A 4-bit unit is 8 k's, a chunk 4 units per wave; a 3-bit unit 32 k's, a
chunk 2; wave w of a piece takes units u0 + w, u0 + w + 8, ...:
  empty   4-bit K = 32 (4 units), 3-bit K = 96 (3 units), N = 64: waves without any unit (n_w == 0) -- the request must stay in bounds
          and read the line of zeros;
  dead    4-bit K = 64 (8 units): every wave's share is one unit, the first chunk's other three are dead;
  ragged  4-bit K = 320 (40 units: five per wave, not a whole chunk pair), N = 72 (a partial last tile);
  cross   4-bit K = 512 (64 units per tile), N = 192 (three tiles).  On three workgroups (target_wgs = 3) the planner gives every workgroup one
          whole tile -- as many workgroups as tiles is read tile by tile (sqllm_ranges.h: units_stride_of), so no plan of three workgroups has
          a range across tiles at this shape; it runs as such.  The ranges that CROSS a tile boundary come from target_wgs = 2, 4 and 5 (96,
          48 and 40 units per workgroup): two pieces, and the second piece's request must use its own u0 (0) where the first piece's is
          32 / 48 / 40 / 56.  The first test of the file pins those plans.
One row, forced onto the column-lane route (cols_min_batch = cols_max_batch = 1) and by the default routing, through the three entries of
tests/helpers.py:call_op; dense-only and with a CSR term (the sparse roles share the grid); singly and as a group of two ops over one vec.
Non-finite operands (tests/nonfinite_cases.py: pattern_model, pattern_of): +inf, -inf and NaN in the last live unit of a ragged share --
the dead units behind it must read zeros, so every output keeps the sign the term-wise model gives it and none turns NaN."""
import functools

import numpy as np
import pytest

from tests import helpers as H
from tests import nonfinite_cases as NF

pytestmark = pytest.mark.gpu

TOL_FP64 = 2e-5
FORCE = {"cols_min_batch": 1, "cols_max_batch": 1}
# name -> (bits, K, N, [cut options])
CASES = {
    "empty-w4": (4, 32, 64, [{}]),
    "empty-w3": (3, 96, 64, [{}]),
    "dead-w4": (4, 64, 64, [{}]),
    "ragged-w4": (4, 320, 72, [{}]),
    "cross-w4": (4, 512, 192, [{"target_wgs": 3}, {"target_wgs": 2}, {"target_wgs": 4}, {"target_wgs": 5}]),
}
GROUP_N2 = 136  # the second op of a group: three tiles, the last one partial


def _set(opts):
    from squeezellm_amd import _lib

    for k, v in opts.items():
        _lib.set_option(k, v)


def _clear(opts):
    from squeezellm_amd import _lib

    for k in opts:
        _lib.set_option(k, 0)


@functools.lru_cache(maxsize=None)
def _op(bits, K, N, sparse, j=0):
    """(case, x, y0, fp64 reference) of an op: computed once, shared, never written (the ops of a group share x)"""
    case = H.make_case(bits, K, N, sparse=0.03 if sparse else 0.0, seed=13 * bits + K + 5 * N + j + (1000 if sparse else 0))
    x = np.random.default_rng(K + bits).standard_normal(K).astype(np.float32)
    y0 = (np.random.default_rng(N + j).standard_normal(N) * 0.01).astype(np.float32)
    ref = H.c_matvec(H.c_oracle(), case, x, y0, batched=False)
    for a in (x, y0, ref):
        a.setflags(write=False)
    return case, x, y0, ref


def _pieces(p, U):
    """(workgroup, tile, u0, u1) of every piece, as dense_role_cols walks its range (tests/test_cols_batch1_cut_cpu.py: _walk)"""
    tiles, upw, ks, blocks = p["col_tiles"], p["groups_per_wave"], p["k_slices"], p["dense_blocks"]
    stride = ks * upw if blocks == tiles * ks else U
    total, out = tiles * stride, []
    for bid in range(blocks):
        gpos, gend = bid * upw, min(bid * upw + upw, total)
        while gpos < gend:
            ct = gpos // stride
            u0 = gpos - ct * stride
            if u0 >= U:
                gpos = (ct + 1) * stride
                continue
            u1 = min(U, u0 + gend - gpos)
            gpos += u1 - u0
            if u1 == U:
                gpos = (ct + 1) * stride
            out.append((bid, ct, u0, u1))
    return out


def _single(gpu, bits, K, N, opts, sparse, entries):
    import torch

    from squeezellm_amd import quant_cuda as qc

    case, x, y0, ref = _op(bits, K, N, sparse)
    t = H.to_torch(case, gpu)
    xt = torch.from_numpy(x.copy()).to(gpu)
    _set(opts)
    try:
        for entry in entries:
            y = torch.from_numpy(y0.copy()).to(gpu)
            H.call_op(qc, t, xt, y, "spmv" if sparse else "dense", False, entry=entry)
            torch.cuda.synchronize()
            err = H.rel_err(y.cpu().numpy(), ref)
            print(f"w{bits} {K}x{N} {opts} sparse={sparse} entry={entry}: rel err {err:.3e}")
            assert err <= TOL_FP64, f"w{bits} {K}x{N} {opts} sparse={sparse} {entry}: rel err {err:.2e}"
    finally:
        _clear(opts)


def _group(gpu, bits, K, widths, opts, sparse):
    import torch

    from squeezellm_amd import decode

    ops = [_op(bits, K, N, sparse, j) for j, N in enumerate(widths)]
    layers = [H.to_torch(c, gpu) for c, _, _, _ in ops]
    x = torch.from_numpy(ops[0][1].copy()).to(gpu)
    ys = [torch.from_numpy(o[2].copy()).to(gpu) for o in ops]
    _set(opts)
    try:
        seq = decode.OpSequence(layers, [x] * len(ops), ys, batched=False, fuse_shared_input=True)
        assert seq.groups == [list(range(len(ops)))]
        seq.launch()
        torch.cuda.synchronize()
        for N, y, o in zip(widths, ys, ops):
            err = H.rel_err(y.cpu().numpy(), o[3])
            print(f"w{bits} K={K} N={N} of {widths} {opts} sparse={sparse}: rel err {err:.3e}")
            assert err <= TOL_FP64, f"w{bits} K={K} N={N} of {widths} {opts} sparse={sparse}: rel err {err:.2e}"
    finally:
        _clear(opts)


def test_the_cross_case_has_ranges_across_tile_boundaries():
    """what "cross-w4" relies on (the plan itself needs no GPU work): on 2, 4 and 5 workgroups there are workgroups of two pieces whose second piece
    starts at its tile's unit 0 while the first one starts elsewhere; on three workgroups every workgroup has one whole tile"""
    from squeezellm_amd import _lib

    bits, K, N, cuts = CASES["cross-w4"]
    for cut in cuts:
        opts = dict(FORCE, **cut)
        _set(opts)
        try:
            p = _lib.plan_query(bits, K, N)
        finally:
            _clear(opts)
        pieces = _pieces(p, K // 8)
        seen = np.zeros((p["col_tiles"], K // 8), np.int32)
        for _, ct, u0, u1 in pieces:
            seen[ct, u0:u1] += 1
        assert (seen == 1).all(), (cut, pieces)
        assert p["dense_blocks"] == cut["target_wgs"], (cut, p)
        second = [(b, ct, u0, u1) for i, (b, ct, u0, u1) in enumerate(pieces) if i and pieces[i - 1][0] == b]
        if cut["target_wgs"] == 3:
            assert not second and [pc[1:] for pc in pieces] == [(0, 0, 64), (1, 0, 64), (2, 0, 64)], pieces
            continue
        assert second and all(u0 == 0 for _, _, u0, _ in second), (cut, pieces)
        assert any(pieces[i - 1][2] != 0 for i, pc in enumerate(pieces) if i and pieces[i - 1][0] == pc[0]), (cut, pieces)  # a first piece with u0 != 0


@pytest.mark.parametrize("route", ["cols", "default"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_single_ops_three_entries(gpu, name, route):
    bits, K, N, cuts = CASES[name]
    for cut in cuts:
        opts = dict(FORCE, **cut) if route == "cols" else dict(cut)
        _single(gpu, bits, K, N, opts, sparse=False, entries=H.ENTRIES)
        _single(gpu, bits, K, N, opts, sparse=True, entries=("named",))  # (once with a CSR term: the sparse roles share the grid)


@pytest.mark.parametrize("route", ["cols", "default"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_groups_of_two_ops_over_one_vec(gpu, name, route):
    bits, K, N, cuts = CASES[name]
    for cut in cuts:
        if "target_wgs" in cut:  # (the launch's: its ops share it)
            cut = {"target_wgs": 2 * cut["target_wgs"]}
        opts = dict(FORCE, **cut) if route == "cols" else dict(cut)
        _group(gpu, bits, K, (N, GROUP_N2), opts, sparse=False)
    _group(gpu, bits, K, (N, GROUP_N2), dict(FORCE, **cuts[0]) if route == "cols" else dict(cuts[0]), sparse=True)


# ---- non-finite vec in the last live unit of a ragged share ----
# (bits, K, N): 4-bit 40 units, five per wave: the second chunk of every wave is one live unit and three dead ones; 4-bit 8 units: one live
# unit and three dead ones in the FIRST chunk (the hoisted request's own); 3-bit 3 units: waves 0-2 one live + one dead, waves 3-7 empty
NONFINITE = [(4, 320, 72), (4, 64, 64), (3, 96, 64)]


def _last_live_positions(bits, K):
    """(k, value): +inf in the last k of the last unit (the last wave that has one), -inf in the first k of wave 0's last unit, NaN in between"""
    ku = 8 if bits == 4 else 32
    U = K // ku
    last_of_wave0 = (U - 1) // 8 * 8  # wave 0's units are 0, 8, 16, ...
    mid = (last_of_wave0 + U - 1) // 2
    return [(K - 1, np.inf), (last_of_wave0 * ku, -np.inf), (mid * ku + ku // 2, np.nan)]


@pytest.mark.parametrize("route", ["cols", "default"])
@pytest.mark.parametrize("bits,K,N", NONFINITE)
def test_nonfinite_vec_in_the_last_live_unit(gpu, bits, K, N, route):
    import torch

    from squeezellm_amd import quant_cuda as qc

    case, x0, y0, _ = _op(bits, K, N, False)
    assert (H.oracle.dequantize(case["qweight"], case["lookup_table"], bits) != 0).all()  # (no 0 x inf from live data)
    t = H.to_torch(case, gpu)
    opts = FORCE if route == "cols" else {}
    _set(opts)
    try:
        for k, v in _last_live_positions(bits, K):
            x = x0.copy()
            assert (x != 0).all()
            x[k] = v
            with np.errstate(all="ignore"):
                ref = np.asarray(H.oracle_ref(case, x, y0.copy(), "dense"), np.float64)
            model = NF.pattern_model(case, x, y0, "dense")
            for m, r in zip(model, NF.pattern_of(ref)):
                assert np.array_equal(m[0], r[0])  # (the oracle agrees with the term-wise model)
            for entry in H.ENTRIES:
                y = torch.from_numpy(y0.copy()).to(gpu)
                H.call_op(qc, t, torch.from_numpy(x).to(gpu), y, "dense", False, entry=entry)
                torch.cuda.synchronize()
                got = y.cpu().numpy()
                for what, g, m in zip(("NaN", "+inf", "-inf"), NF.pattern_of(got), model):
                    assert np.array_equal(g[0], m[0]), (f"w{bits} {K}x{N} {route} {entry} x[{k}]={v}: {what} pattern differs in "
                                                        f"{int((g[0] != m[0]).sum())} outputs ({int(g[0].sum())} got, {int(m[0].sum())} in the model)")
                fin = np.isfinite(ref)
                if fin.any():
                    assert H.rel_err(got[fin], ref[fin]) <= TOL_FP64
    finally:
        _clear(opts)
