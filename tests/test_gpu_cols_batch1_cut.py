"""The column-lane kernel at one row under the cuts of cut_ranges_one_row (csrc/sqllm_capi.hip) against the fp64 C oracle, on the smallest
shapes where such a cut can go wrong.  The route is forced with cols_min_batch = cols_max_batch = 1.  K (units of 8 k's at 4 bits, 32 at
3 bits; the kernel's quantum is 64 / 32 units per workgroup):
  4-bit 512   64 units: one quantum per tile            3-bit 1024   32 units: one quantum
  4-bit 1280  160 units: ragged last range, guarded pair 3-bit 2560   80 units = 2.5 quanta
  4-bit 2816  352 units = 5.5 quanta
N = 64 (one tile) and 136 (partial last tile); a two-op group of N = (136, 72) and a three-op group of N = 64 each.  Cuts: the default on the
real CU count; the default on a pretended part of 3 CUs -- there the plan of cut_ranges for the (136, 72) group crosses tile boundaries and the
one-row cut replaces it (tests/test_cols_batch1_cut_cpu.py::test_small_group_on_three_cus_is_recut pins that it does; the single ops and the
one-tile group keep the plan of cut_ranges there) --; the cut by slots alone (cols_slot_cut = 1), which re-cuts every launch here; and target_wgs
values that ask cut_ranges for one, two and three ranges per tile of the first op.
Eager, and once per K as a captured graph replayed twice.  Tolerance: the project's 2e-5 (fp32 accumulation vs the fp64 oracle, max-norm relative)."""
import functools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

TOL_FP64 = 2e-5
KS = [(4, 512), (4, 1280), (4, 2816), (3, 1024), (3, 2560)]
LAUNCHES = [(64,), (136,), (136, 72), (64, 64, 64)]
FORCE = {"cols_min_batch": 1, "cols_max_batch": 1}


def _cuts(widths):
    tiles = -(-widths[0] // 64)
    cuts = {"default": {}, "default-3cus": {"cu_count": 3}, "slots": {"cols_slot_cut": 1}}
    for p in (1, 2, 3):  # (target_wgs is the launch's: its ops share it)
        cuts[f"p{p}"] = {"target_wgs": tiles * p * len(widths)}
    return cuts


@functools.lru_cache(maxsize=None)
def _op(bits, K, N, j):
    """(case, x, y0, fp64 reference) of op j of a launch: computed once, shared, never written"""
    case = H.make_case(bits, K, N, seed=11 * bits + K + 3 * N + j)
    rng = np.random.default_rng(K + bits)  # (the ops of a launch share x)
    x = rng.standard_normal(K).astype(np.float32)
    y0 = (np.random.default_rng(N + j).standard_normal(N) * 0.01).astype(np.float32)
    ref = H.c_matvec(H.c_oracle(), case, x, y0, batched=False)
    for a in (x, y0, ref):
        a.setflags(write=False)
    return case, x, y0, ref


def _run(gpu, bits, K, widths, opts, graph):
    import torch

    from squeezellm_amd import _lib, decode

    ops = [_op(bits, K, N, j) for j, N in enumerate(widths)]
    layers = [H.to_torch(c, gpu) for c, _, _, _ in ops]
    x = torch.from_numpy(ops[0][1].copy()).to(gpu)
    y0s = [torch.from_numpy(o[2].copy()).to(gpu) for o in ops]
    ys = [y.clone() for y in y0s]
    opts = dict(FORCE, **opts)
    for k, v in opts.items():
        _lib.set_option(k, v)
    try:
        seq = decode.OpSequence(layers, [x] * len(ops), ys, batched=False, fuse_shared_input=True)
        assert seq.groups == [list(range(len(ops)))]
        rounds = 1
        if graph:
            g, rounds = seq.graph(warmup=0), 2
        for r in range(rounds):
            for y, y0 in zip(ys, y0s):
                y.copy_(y0)
            g.replay() if graph else seq.launch()
            torch.cuda.synchronize()
            for N, y, o in zip(widths, ys, ops):
                err = H.rel_err(y.cpu().numpy(), o[3])
                print(f"w{bits} K={K} N={N} of {widths} {opts} graph={graph} round {r}: rel err {err:.3e}")
                assert err <= TOL_FP64, f"w{bits} K={K} N={N} of {widths} {opts}: rel err {err:.2e}"
    finally:
        for k in opts:
            _lib.set_option(k, 0)


@pytest.mark.parametrize("widths", LAUNCHES, ids=lambda w: "x".join(map(str, w)))
@pytest.mark.parametrize("bits,K", KS)
def test_every_cut_eager(gpu, bits, K, widths):
    from squeezellm_amd import _lib

    for name, opts in _cuts(widths).items():
        if len(widths) == 1 and name in ("p1", "p2", "p3"):  # the cut asked for is the cut planned
            for k, v in dict(FORCE, **opts).items():
                _lib.set_option(k, v)
            try:
                p = _lib.plan_query(bits, K, widths[0])
            finally:
                for k in dict(FORCE, **opts):
                    _lib.set_option(k, 0)
            U = K // (8 if bits == 4 else 32)
            assert p["dense_blocks"] == p["col_tiles"] * p["k_slices"] and p["k_slices"] == -(-U // p["groups_per_wave"]), (name, p)
            want = -(-(-(-U // int(name[1]))) // 8) * 8  # ceil(U / p) in whole waves
            assert p["groups_per_wave"] == want, (name, p)
        _run(gpu, bits, K, widths, opts, graph=False)


@pytest.mark.parametrize("bits,K", KS)
def test_captured_graph_replayed_twice(gpu, bits, K):
    _run(gpu, bits, K, (136, 72), {"cols_slot_cut": 1}, graph=True)
    _run(gpu, bits, K, (136, 72), {"cu_count": 3}, graph=True)
    _run(gpu, bits, K, (64, 64, 64), {"cols_slot_cut": 1}, graph=True)
