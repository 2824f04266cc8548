"""How long does making a checkpoint take?  Wall time of squeezellm_amd.nuq.fit_lut (sort, the exact weighted k-means
kernel, index assignment) over the seven linears of one LLaMA-7B decoder layer -- 42,496 output channels -- at 3 and 4
bits, on synthetic fp16 weights (Student t) and log-normal Fisher weights.  Prints one line per linear and one JSON
line: rows/s per bit width and the whole-model projection (x 32 layers).

The reference's route (quantization/nuq.py: one sklearn KMeans per row on the CPU) measures ~8 ms per row at 4 bits
and ~24 ms per row at 3 bits single-threaded at K = 4096, 3 to 9 CPU-hours for the ~1.36 M rows of LLaMA-7B.

    python tools/nuq_bench.py [--bits 3 4] [--layers 32] [--reps 1]

--encode times the step AFTER the fit instead: weight + codebooks (+ a 0.45 % outlier mask) -> packed operands, the torch
route (nuq.assign_indices + pack.pack_layer, what quantize_linear chained before) against pack.encode_layer (the
sqllm_encode kernels) in the same process, alternating, on the seven 7B linears and the 13B gate/up shape: median wall
time over --reps runs after a warm-up (a device synchronise on both sides of every timed region) and
torch.cuda.max_memory_allocated above what was allocated before the call, after a reset.

    python tools/nuq_bench.py --encode [--bits 3 4] [--reps 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from squeezellm_amd import nuq, pack  # noqa: E402

HIDDEN, INTER = 4096, 11008
LINEARS = [("q_proj", HIDDEN, HIDDEN), ("k_proj", HIDDEN, HIDDEN), ("v_proj", HIDDEN, HIDDEN), ("o_proj", HIDDEN, HIDDEN),
           ("gate_proj", INTER, HIDDEN), ("up_proj", INTER, HIDDEN), ("down_proj", HIDDEN, INTER)]  # (name, N, K)


def synthetic(N, K, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    # Student t with 3 degrees of freedom: normal / sqrt(chi2_3 / 3)
    z = torch.randn(N, K, device="cuda", generator=gen)
    chi = (torch.randn(3, N, K, device="cuda", generator=gen) ** 2).sum(0) / 3
    w = (0.02 * z / chi.sqrt()).half()
    g = torch.exp(-12.0 + 2.0 * torch.randn(N, K, device="cuda", generator=gen))
    return w, g


ENCODE_SHAPES = LINEARS + [("13b_gate_up", 13824, 5120)]


def _timed(fn, reps):
    """(median seconds, peak bytes above the starting allocation) of fn(), after one warm-up call."""
    fn()
    times, peak = [], 0
    for _ in range(reps):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
        del out
    return statistics.median(times), peak


def encode_leg(bits_list, reps):
    """One line per (shape, bits, mask): both routes' median time and peak memory; one JSON line at the end."""
    results = []
    for i, (name, N, K) in enumerate(ENCODE_SHAPES):
        w, g = synthetic(N, K, 100 + i)
        del g
        gen = torch.Generator(device="cuda").manual_seed(200 + i)
        mask = torch.rand(N, K, device="cuda", generator=gen) < 0.0045
        for b in bits_list:
            # codebooks: per-row quantiles of the weights (the leg times what follows the fit, whatever the fit gave)
            q = (torch.arange(1 << b, device="cuda", dtype=torch.float32) + 0.5) / (1 << b)
            lut = torch.quantile(w[:, :: max(1, K // 1024)].float(), q, dim=1).t().contiguous()
            for m in (None, mask):
                def torch_route():
                    w32 = w.to(torch.float32)
                    if m is None:
                        return pack.pack_layer(nuq.assign_indices(w32, lut), lut, b)
                    return pack.pack_layer(nuq.assign_indices(w32 * ~m, lut), lut, b, w32 * m)

                def kernel_route():
                    return pack.encode_layer(w, lut, b, m)

                a, k = torch_route(), kernel_route()
                for key in ("qweight", "rows", "cols", "vals"):  # the same operands, or the timing means nothing
                    assert (a[key] is None and k[key] is None) or torch.equal(a[key], k[key]), (name, b, key)
                del a, k
                tt, tp = _timed(torch_route, reps)
                kt, kp = _timed(kernel_route, reps)
                r = dict(shape=name, N=N, K=K, bits=b, mask=m is not None, torch_ms=round(tt * 1e3, 3), torch_peak_mb=round(tp / 2**20, 1),
                         encode_ms=round(kt * 1e3, 3), encode_peak_mb=round(kp / 2**20, 1))
                results.append(r)
                print(f"w{b} {name:11s} N={N:5d} K={K:5d} mask={int(r['mask'])}: torch {r['torch_ms']:9.2f} ms {r['torch_peak_mb']:8.1f} MB | "
                      f"encode_layer {r['encode_ms']:8.3f} ms {r['encode_peak_mb']:7.1f} MB | x{tt / kt:6.1f} time, x{tp / max(kp, 1):5.1f} memory", flush=True)
        del w, mask
        torch.cuda.empty_cache()
    print(json.dumps({"encode": results}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encode", action="store_true", help="time the step after the fit: torch packer against pack.encode_layer")
    ap.add_argument("--bits", type=int, nargs="+", default=[3, 4])
    ap.add_argument("--layers", type=int, default=32, help="decoder layers of the model the projection is for")
    ap.add_argument("--reps", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nuq_bench needs a GPU"
    if a.encode:
        return encode_leg(a.bits, max(a.reps, 3))
    mats = {name: synthetic(N, K, i) for i, (name, N, K) in enumerate(LINEARS)}
    rows = sum(N for _, N, _ in LINEARS)
    w0, g0 = synthetic(64, 512, 99)
    for b in a.bits:  # warm-up: library load, kernels, allocator
        nuq.fit_lut(w0, g0, b)
    torch.cuda.synchronize()
    result = {"layer_rows": rows, "layers": a.layers}
    for b in a.bits:
        total = 0.0
        for name, N, K in LINEARS:
            w, g = mats[name]
            best = float("inf")
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                lut, idx, cost = nuq.fit_lut(w, g, b)
                torch.cuda.synchronize()
                best = min(best, time.perf_counter() - t0)
            assert bool(torch.isfinite(lut).all()) and bool(torch.isfinite(cost).all())
            total += best
            print(f"w{b} {name:9s} N={N:5d} K={K:5d}: {best * 1e3:9.1f} ms  {N / best:9.0f} rows/s", flush=True)
        result[f"w{b}_layer_s"] = round(total, 4)
        result[f"w{b}_rows_per_s"] = round(rows / total, 1)
        result[f"w{b}_model_projected_s"] = round(total * a.layers, 2)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
