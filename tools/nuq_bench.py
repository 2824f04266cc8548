"""How long does making a checkpoint take?  Wall time of squeezellm_amd.nuq.fit_lut (sort, the exact weighted k-means
kernel, index assignment) over the seven linears of one LLaMA-7B decoder layer -- 42,496 output channels -- at 3 and 4
bits, on synthetic fp16 weights (Student t) and log-normal Fisher weights.  Prints one line per linear and one JSON
line: rows/s per bit width and the whole-model projection (x 32 layers).

The reference's route (quantization/nuq.py: one sklearn KMeans per row on the CPU) measures ~8 ms per row at 4 bits
and ~24 ms per row at 3 bits single-threaded at K = 4096, 3 to 9 CPU-hours for the ~1.36 M rows of LLaMA-7B.

    python tools/nuq_bench.py [--bits 3 4] [--layers 32] [--reps 1]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from squeezellm_amd import nuq  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, nargs="+", default=[3, 4])
    ap.add_argument("--layers", type=int, default=32, help="decoder layers of the model the projection is for")
    ap.add_argument("--reps", type=int, default=1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nuq_bench needs a GPU"
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
