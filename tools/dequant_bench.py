#!/usr/bin/env python
"""Measure the dense export (sqllm_dequant) and the prefill route built on it.

  1. kernel: every distinct linear shape of LLaMA 7B / 13B (synth.MODEL_SHAPES), w3 / w4, s0 / s45 with top-10, fp16 / fp32
     output -- bytes moved (packed words + codebooks + sparse operands + output), HIP-event time per call, TB/s and the
     fraction of the 8 TB/s HBM peak.  Each repeat times one replay of a captured graph of back-to-back calls (kernel nodes
     only: no host work between them) over as many DIFFERENT output buffers as fit 1 GiB (2 to 8), so the stores go to
     HBM and not to a cache that still holds the previous call's lines.
  2. prefill: QuantLinearLUTFused.forward at 128 / 512 / 2048 rows on 13B gate/up and o_proj, the fused kernel
     (dense_min_rows = None) against the dense route (dense_min_rows = 1), alternating in one process.

Median and min..max over the repeats are reported; the first `--warmup` repeats are dropped.

    python tools/dequant_bench.py [--repeats 7] [--warmup 2] [--only kernel|prefill] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from squeezellm_amd import decode, synth  # noqa: E402
from squeezellm_amd.quant import QuantLinearLUTFused  # noqa: E402

HBM_PEAK = 8.0e12


def timed(fn, repeats, warmup):
    """ms per call of fn(): median, min, max over `repeats` event-timed runs after `warmup` untimed ones."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def dequant_bytes(lay, itemsize):
    K, N, bits = lay["K"], lay["N"], lay["bits"]
    b = K * N * bits // 8 + N * (1 << bits) * 4 + N * K * itemsize
    if lay["vals"] is not None:
        b += 8 * lay["vals"].numel() + 4 * (N + 1)
    if lay["full_rows"] is not None:
        b += 4 * K * lay["full_rows"].shape[1] + 4 * lay["full_rows"].shape[1]
    return b


def bench_kernel(args, emit):
    shapes = []
    for model in ("llama-7b", "llama-13b"):
        for _, K, N in synth.MODEL_SHAPES[model]["linears"]:
            if (model, K, N) not in shapes:
                shapes.append((model, K, N))
    emit("kernel: model K N bits sparse dtype | MB moved | us median (min..max) | TB/s | of 8 TB/s")
    for model, K, N in shapes:
        for bits in (3, 4):
            for sparse in (0.0, 0.0045):
                lay = synth.make_layer(K, N, bits, sparse_frac=sparse, topX=10 if sparse else 0, heavy_rows=10 if sparse else 0)
                for dtype in (torch.float16, torch.float32):
                    item = 2 if dtype is torch.float16 else 4
                    n_out = max(2, min(8, (1 << 30) // (N * K * item)))
                    outs = [torch.empty((N, K), dtype=dtype, device="cuda") for _ in range(n_out)]

                    # the calls are captured once and the GRAPH is timed: issued from Python, every call costs tens of us of
                    # host work (descriptor filling, ctypes) and the events would measure the issue rate, not the kernel
                    for o in outs:
                        decode.dequantize_layer(lay, dtype, out=o)
                    torch.cuda.synchronize()
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        for o in outs:
                            decode.dequantize_layer(lay, dtype, out=o)
                    fn = g.replay

                    med, lo, hi = (t / n_out for t in timed(fn, args.repeats, args.warmup))
                    moved = dequant_bytes(lay, item)
                    tbs = moved / (med * 1e-3) / 1e12
                    rec = dict(kind="kernel", model=model, K=K, N=N, bits=bits, sparse=sparse, dtype=str(dtype).split(".")[-1],
                               bytes=moved, us=med * 1e3, us_min=lo * 1e3, us_max=hi * 1e3, tb_s=tbs, frac_peak=tbs * 1e12 / HBM_PEAK)
                    emit(f"kernel: {model} {K} {N} w{bits} s{int(sparse * 10000)} {rec['dtype']} | {moved / 1e6:.1f} | "
                         f"{rec['us']:.1f} ({rec['us_min']:.1f}..{rec['us_max']:.1f}) | {tbs:.2f} | {rec['frac_peak']:.2f}", rec)
                    del outs


def bench_prefill(args, emit):
    emit("prefill: shape bits sparse rows | fused ms median (min..max) | dense ms median (min..max) | fused / dense")
    for name, K, N in (("13b gate/up", 5120, 13824), ("13b o_proj", 5120, 5120)):
        for bits in (3, 4):
            for sparse in (0.0, 0.0045):
                lay = synth.make_layer(K, N, bits, sparse_frac=sparse, topX=10 if sparse else 0, heavy_rows=10 if sparse else 0)
                m = QuantLinearLUTFused.from_operands(lay)
                for rows in (128, 512, 2048):
                    x = torch.randn((rows, K), device="cuda", dtype=torch.float16)
                    res = {"fused": [], "dense": []}
                    for rep in range(args.warmup + args.repeats):  # alternating: both routes see the same clocks
                        for route, thr in (("fused", None), ("dense", 1)):
                            m.dense_min_rows = thr
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            m(x)
                            e1.record()
                            e1.synchronize()
                            assert m.last_route == route
                            if rep >= args.warmup:
                                res[route].append(e0.elapsed_time(e1))
                    f, d = res["fused"], res["dense"]
                    rec = dict(kind="prefill", shape=name, K=K, N=N, bits=bits, sparse=sparse, rows=rows,
                               fused_ms=statistics.median(f), fused_min=min(f), fused_max=max(f),
                               dense_ms=statistics.median(d), dense_min=min(d), dense_max=max(d))
                    emit(f"prefill: {name} w{bits} s{int(sparse * 10000)} {rows} | {rec['fused_ms']:.3f} ({min(f):.3f}..{max(f):.3f}) | "
                         f"{rec['dense_ms']:.3f} ({min(d):.3f}..{max(d):.3f}) | {rec['fused_ms'] / rec['dense_ms']:.2f}", rec)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("kernel", "prefill"), default=None)
    ap.add_argument("--out", default=None, help="also write the table and one JSON record per row to this file")
    args = ap.parse_args()
    lines, recs = [], []

    def emit(line, rec=None):
        print(line, flush=True)
        lines.append(line)
        if rec is not None:
            recs.append(rec)

    emit(f"device: {torch.cuda.get_device_name(0)}; repeats {args.repeats}, warmup {args.warmup}")
    if args.only in (None, "kernel"):
        bench_kernel(args, emit)
    if args.only in (None, "prefill"):
        bench_prefill(args, emit)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
            for r in recs:
                fh.write(json.dumps(r) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
