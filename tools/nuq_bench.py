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

--select times the step BEFORE the fit: which weights are outliers.  At the gate_proj and q_proj shapes of LLaMA 7B / 13B /
65B, fp16 and fp32: the four order statistics either side of the quartiles by sqllm_select (events around --reps >= 20
calls after a warm-up; achieved bytes/s against passes x matrix bytes) against torch.sort of the flattened matrix on the
same GPU (the only GPU route there was: torch.quantile refuses more than 16 M elements) and np.quantile on the host (what
the reference runs; once per shape; np.quantile is single-threaded whatever the thread count of the process; fp16 is
widened to fp32 first, inside the timed region, because np.quantile of more than 65504 halves returns nan);
nuq.outlier_threshold end to end (host wall time, read-back included); the sensitivity cut + mask (sensitivity_threshold +
sqllm_outlier_mask) against the torch route (topk + the boolean union); and nuq.outlier_config over the seven linears of
one decoder layer.  Three controls say what bounds the select: one streaming read of the same matrix (sqllm_outlier_mask,
count only: the floor of a pass), and the select on two other matrices of the same shape -- keys spread evenly over the
first digit's bins (no skew) and one value everywhere (all 64 lanes of a wave on one LDS counter: the worst skew).  The
clocks are read once at the end.  --out writes the table to a file as well (profiles/select_bench.txt is such a run).

    python tools/nuq_bench.py --select [--reps 20] [--models 7b 13b 65b] [--out profiles/select_bench.txt]
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


MODELS = {"7b": (4096, 11008), "13b": (5120, 13824), "65b": (8192, 22016)}  # hidden, intermediate


def _events_ms(fn, reps):
    """Mean milliseconds of fn() over `reps` back-to-back calls between two events, after two warm-up calls."""
    fn()
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _wall_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def _clocks():
    import shutil
    import subprocess

    exe = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    try:
        out = subprocess.run([exe, "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=60).stdout
        keep = [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln]
        return "; ".join(keep) or "clocks: not reported"
    except Exception as e:  # the tool is optional: the table stands without the note
        return f"clocks: not read ({type(e).__name__})"


def _flat_keys(N, K, dtype, seed):
    """Finite values whose bit patterns are uniform: every bin of the select's first digit is hit alike."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    if dtype == torch.float16:
        bits = torch.randint(0, 0x7c00, (N, K), device="cuda", generator=gen, dtype=torch.int16)
    else:
        bits = torch.randint(0, 0x7f800000, (N, K), device="cuda", generator=gen, dtype=torch.int32)
    x = bits.view(dtype)
    return torch.where(torch.rand(N, K, device="cuda", generator=gen) < 0.5, -x, x)


def select_leg(reps, models, out_path=None):
    import numpy as np

    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"# tools/nuq_bench.py --select --reps {reps} --models {' '.join(models)}: {torch.cuda.get_device_name(0)}, torch {torch.__version__}")
    say("# select / read / cut+mask kernel: mean of the repetitions between two events, after two warm-up calls; torch.sort and the")
    say("# torch mask: the same over max(3, reps / 4); np.quantile: host wall time of one call per quartile (single-threaded)")
    results = []
    for model in models:
        hidden, inter = MODELS[model]
        for name, N, K in (("gate_proj", inter, hidden), ("q_proj", hidden, hidden)):
            for dtype in (torch.float16, torch.float32):
                w, g = synthetic(N, K, 300 + N % 97)
                w = w.to(dtype)
                g = g.to(dtype) if dtype == torch.float16 else g
                n = w.numel()
                ranks = [r for q in (0.25, 0.75) for r in nuq.quantile_ranks(n, q)[:2]]
                idx = torch.tensor(ranks, device="cuda")
                passes = 2 if dtype == torch.float16 else 3

                def sort_route():
                    return torch.sort(w.reshape(-1)).values[idx]

                vals, _ = nuq.order_statistics(w, ranks)
                assert torch.equal(vals, sort_route().float()), (model, name, dtype)  # the same numbers, or the timing means nothing
                sel_ms = _events_ms(lambda: nuq.order_statistics(w, ranks), reps)
                # controls: one streaming read of w, and the select with no skew / with the worst skew in its LDS counters
                one = torch.ones((), dtype=torch.float32, device="cuda")
                read_ms = _events_ms(lambda: nuq._mask_kernel(w, None, None, one, want_mask=False, want_count=True), reps)
                x = _flat_keys(N, K, dtype, 500)
                flat_ms = _events_ms(lambda: nuq.order_statistics(x, ranks), reps)
                x.fill_(0.01)
                const_ms = _events_ms(lambda: nuq.order_statistics(x, ranks), reps)
                del x
                sort_ms = _events_ms(sort_route, max(3, reps // 4))
                thr_ms = _wall_ms(lambda: nuq.outlier_threshold(w, 1.8), max(3, reps // 4))
                wn = w.cpu().numpy()
                t0 = time.perf_counter()
                if wn.dtype == np.float16:  # (np.quantile of this many halves computes its positions in fp16 and returns nan)
                    wn = wn.astype(np.float32)
                q1, q3 = np.quantile(wn, 0.25), np.quantile(wn, 0.75)
                np_ms = (time.perf_counter() - t0) * 1e3
                T = nuq.outlier_threshold(w, 1.8)
                want = max(abs(q1 - 1.8 * (q3 - q1)), abs(q3 + 1.8 * (q3 - q1)))
                assert abs(T - want) <= 1e-5 * want, (T, want)  # (numpy interpolates in fp32 here)
                del wn

                def kernel_mask():
                    return nuq.outlier_mask(w, g, sensitivity=0.05, threshold=T)

                def torch_mask():
                    w32 = w.to(torch.float32)
                    t, t2 = nuq._outlier_masks(w32, g, 0.05, T)
                    return torch.logical_or(t, t2)

                assert torch.equal(kernel_mask(), torch_mask())
                km_ms = _events_ms(kernel_mask, reps)
                tm_ms = _events_ms(torch_mask, max(3, reps // 4))
                gbs = passes * n * w.element_size() / (sel_ms * 1e-3) / 1e9
                r = dict(model=model, shape=name, N=N, K=K, dtype=str(dtype).split(".")[-1], passes=passes, select_ms=round(sel_ms, 4),
                         select_gbs=round(gbs, 1), read_ms=round(read_ms, 4), select_flat_ms=round(flat_ms, 4), select_const_ms=round(const_ms, 4),
                         sort_ms=round(sort_ms, 3), np_quantile_ms=round(np_ms, 1), threshold_ms=round(thr_ms, 3),
                         mask_kernel_ms=round(km_ms, 4), mask_torch_ms=round(tm_ms, 3))
                results.append(r)
                say(f"{model:3s} {name:9s} N={N:5d} K={K:5d} {r['dtype']:7s}: select(4 ranks) {sel_ms:7.3f} ms = {gbs:6.0f} GB/s over {passes} passes | "
                    f"one read {read_ms:6.3f} ms = {n * w.element_size() / read_ms / 1e6:5.0f} GB/s | select, flat keys {flat_ms:7.3f} ms, one value {const_ms:7.3f} ms | "
                    f"torch.sort {sort_ms:8.2f} ms (x{sort_ms / sel_ms:5.1f}) | np.quantile x2 {np_ms:8.0f} ms | outlier_threshold {thr_ms:6.3f} ms | "
                    f"cut+mask kernel {km_ms:6.3f} ms, torch {tm_ms:7.2f} ms (x{tm_ms / km_ms:5.1f})")
                del w, g
                torch.cuda.empty_cache()
        # one decoder layer end to end: thresholds and the outlier share of its seven linears
        sd = {}
        for i, (lname, N, K) in enumerate((("self_attn.q_proj", hidden, hidden), ("self_attn.k_proj", hidden, hidden), ("self_attn.v_proj", hidden, hidden),
                                           ("self_attn.o_proj", hidden, hidden), ("mlp.gate_proj", inter, hidden), ("mlp.up_proj", inter, hidden),
                                           ("mlp.down_proj", hidden, inter))):
            sd[f"model.layers.0.{lname}.weight"] = synthetic(N, K, 400 + i)[0]
        cfg_ms = _wall_ms(lambda: nuq.outlier_config(sd, 1.8), 3)
        results.append(dict(model=model, shape="decoder_layer", outlier_config_ms=round(cfg_ms, 3)))
        say(f"{model:3s} outlier_config of one decoder layer (7 linears, fp16, weights resident): {cfg_ms:8.3f} ms")
        del sd
        torch.cuda.empty_cache()
    say("# " + _clocks())
    say(json.dumps({"select": results}))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--select", action="store_true", help="time outlier selection: sqllm_select / sqllm_outlier_mask against torch.sort, np.quantile, the torch mask")
    ap.add_argument("--models", nargs="+", default=["7b", "13b", "65b"], choices=sorted(MODELS))
    ap.add_argument("--encode", action="store_true", help="time the step after the fit: torch packer against pack.encode_layer")
    ap.add_argument("--bits", type=int, nargs="+", default=[3, 4])
    ap.add_argument("--layers", type=int, default=32, help="decoder layers of the model the projection is for")
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--out", default=None, help="with --select: write the table to this file too")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nuq_bench needs a GPU"
    if a.select:
        return select_leg(max(a.reps, 20), a.models, a.out)
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
