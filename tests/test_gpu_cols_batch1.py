"""The column-lane kernel's one-row decode (csrc/sqllm_kernels.hip: dense_role_cols, BT == 1: vec by groups of 32 k's, counted LDS
waits, unguarded chunk pairs + a guarded tail) against the fp64 C oracle: the 7B and 13B linears at 3 and 4 bits, as single ops
through the three entries of tests/helpers.py:call_op and as the q/k/v and gate/up groups of a decoder layer, with the route forced
onto the column-lane kernel (cols_min_batch = cols_max_batch = 1) and by the default routing; K ranges that leave a wave a ragged
share of units (K not a multiple of the chunk) and N not a multiple of the 64-column tile included.
Tolerance: the project's 2e-5 (fp32 accumulation vs the fp64 oracle, max-norm relative)."""
import functools

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

TOL_FP64 = 2e-5

SHAPES = {  # name -> (K, N)
    "7b-attn": (4096, 4096), "7b-gateup": (4096, 11008), "7b-down": (11008, 4096),
    "13b-attn": (5120, 5120), "13b-gateup": (5120, 13824), "13b-down": (13824, 5120),
}
# K: 33 / 65 / 130 / 344 units of 32 k's -- at 4 bits a chunk is 4 units of 8 k's per wave (256 k's per workgroup step), at 3 bits 2 units of 32
# (512): none of these is a whole number of chunks per wave, and 1056 leaves some waves without any unit; N: partial last column tile
RAGGED = [(1056, 1000), (2080, 4100), (4160, 4164), (11008, 200), (4128, 11012)]
ROUTES = {"cols": {"cols_min_batch": 1, "cols_max_batch": 1}, "default": {}}


@functools.lru_cache(maxsize=4)
def _case(bits, K, N):
    return H.make_case(bits, K, N, seed=7 * bits + K % 1000 + N % 1000)


def _with_route(route, fn):
    from squeezellm_amd import _lib

    opts = ROUTES[route]
    for k, v in opts.items():
        _lib.set_option(k, v)
    try:
        return fn()
    finally:
        for k in opts:
            _lib.set_option(k, 0)


def _check_single(gpu, bits, K, N, route, entries, batched):
    import torch

    from squeezellm_amd import quant_cuda as qc

    case = _case(bits, K, N)
    rng = np.random.default_rng(K + N + bits)
    x = rng.standard_normal((1, K) if batched else K).astype(np.float32)
    y0 = (rng.standard_normal((1, N) if batched else N) * 0.01).astype(np.float32)
    ref = H.c_matvec(H.c_oracle(), case, x, y0, batched=batched)
    t = H.to_torch(case, gpu)
    xt = torch.from_numpy(x).to(gpu)

    def run():
        for entry in entries:
            y = torch.from_numpy(y0.copy()).to(gpu)
            H.call_op(qc, t, xt, y, "dense", batched, entry=entry)
            torch.cuda.synchronize()
            err = H.rel_err(y.cpu().numpy(), ref)
            print(f"w{bits} {K}x{N} route={route} entry={entry} batched={batched}: rel err {err:.3e}")
            assert err <= TOL_FP64, f"w{bits} {K}x{N} {route} {entry}: rel err {err:.2e}"

    _with_route(route, run)


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("bits", [4, 3])
def test_single_ops_three_entries(gpu, bits, shape, route):
    K, N = SHAPES[shape]
    _check_single(gpu, bits, K, N, route, H.ENTRIES, batched=False)
    _check_single(gpu, bits, K, N, route, ("named",), batched=True)  # (a *_batched call with one row takes the same routes)


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("KN", RAGGED, ids=lambda kn: f"{kn[0]}x{kn[1]}")
@pytest.mark.parametrize("bits", [4, 3])
def test_ragged_ranges_and_partial_tiles(gpu, bits, KN, route):
    _check_single(gpu, bits, KN[0], KN[1], route, H.ENTRIES, batched=False)


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("model", ["llama-7b", "llama-13b"])
@pytest.mark.parametrize("bits", [4, 3])
def test_decoder_layer_groups(gpu, bits, model, route):
    """q/k/v as ONE launch of three ops and gate/up as ONE launch of two (decode.OpSequence, fuse_shared_input), dense-only: the launches
    the default routing gives the column-lane kernel at one row -- every op against the C oracle, launched directly and as a graph replay."""
    import torch

    from squeezellm_amd import decode, synth

    spec = synth.MODEL_SHAPES[model]["linears"]
    layers = [dict(synth.make_layer(K, N, bits, sparse_frac=0.0, topX=0, device=gpu, seed=50 * bits + j), name=name)
              for j, (name, K, N) in enumerate(spec)]
    g = torch.Generator(device=gpu)
    g.manual_seed(4321)
    shared = {"k_proj": "q_proj", "v_proj": "q_proj", "up_proj": "gate_proj"}
    xs, last = [], {}
    for l in layers:
        src = shared.get(l["name"])
        xs.append(last[src] if src in last else torch.randn((l["K"],), device=gpu, generator=g))
        last[l["name"]] = xs[-1]
    ys0 = [torch.randn((l["N"],), device=gpu, generator=g) * 0.01 for l in layers]
    lib = H.c_oracle()
    refs = [H.c_matvec(lib, {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in l.items()}, x.cpu().numpy(),
                       y0.cpu().numpy(), batched=False) for l, x, y0 in zip(layers, xs, ys0)]

    def run():
        for graph in (False, True):
            ys = [y.clone() for y in ys0]
            seq = decode.OpSequence(layers, xs, ys, batched=False, fuse_shared_input=True)
            assert seq.groups == [[0, 1, 2], [3], [4, 5], [6]]
            if graph:
                gr = seq.graph(warmup=0)
                for y, y0 in zip(ys, ys0):
                    y.copy_(y0)
                gr.replay()
            else:
                seq.launch()
            torch.cuda.synchronize()
            for l, y, ref in zip(layers, ys, refs):
                err = H.rel_err(y.cpu().numpy(), ref)
                print(f"{model} w{bits} {l['name']} route={route} graph={graph}: rel err {err:.3e}")
                assert err <= TOL_FP64, f"{model} w{bits} {l['name']} {route}: rel err {err:.2e}"

    _with_route(route, run)
