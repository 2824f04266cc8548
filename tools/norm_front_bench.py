"""The two norm fronts of a decoder layer four ways, graph-replayed alternately in ONE process (built like qkv_rope_bench.py).

    python tools/norm_front_bench.py [--models 7b,13b] [--fronts qkv,gate_up] [--bits 3,4] [--rows 1,4,16] [--dtypes fp16,bf16]
                                     [--layers 32] [--reps 5]

Workload: --layers decoder layers with distinct weights, each over its own un-normalised hidden state and its own norm weight.
Models 7b (K = 4096: q/k/v 3 x 4096, gate/up 4096 -> 11008) and 13b (K = 5120: 3 x 5120, 5120 -> 13824), head_dim 128; s0 (dense
only) and s45 + top-10.  Per point, four ways:
  A  the norm as the checkpoints' module writes it in torch (upcast, pow, mean, + eps, rsqrt, mul, downcast, mul weight)
     + the parent's kernel (QuantQKVRopeFused / QuantGatedLUTFused)
  B  torch.nn.functional.rms_norm + the parent's kernel
  C  the norm front: the same module with norm_weight (one kernel per layer)
  P  the parent's kernel alone, on input that is normalised already: C - P is what the prologue costs, A - P and B - P what it replaces
Each way is captured once after an eager warm-up; the four graphs are then replayed alternately, --reps repetitions of 30 replays
each.  One JSON line per point: the median per way and its spread (max - min) in ms per pass over all layers, the differences in us
per layer, whether C beats B by more than the repetitions' spread, and the largest difference between A's and C's first output (a
sanity check, not a test).
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from squeezellm_amd import quant, synth

D, N_POS, EPS = 128, 4096, 1e-6
MODELS = {"7b": (4096, 11008), "13b": (5120, 13824)}
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
ap = argparse.ArgumentParser()
ap.add_argument("--models", default="7b,13b")
ap.add_argument("--fronts", default="qkv,gate_up")
ap.add_argument("--bits", default="3,4")
ap.add_argument("--rows", default="1,4,16")
ap.add_argument("--dtypes", default="fp16,bf16")
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
dev = torch.device("cuda:0")
cos32, sin32 = quant.rope_tables(D, N_POS, device=dev)


def timed(fn, reps=30, warmup=3):
    for _ in range(warmup): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / reps * 1e3


def capture(fn):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side): fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr): fn()
    return gr


def module_norm(h, w):  # as the checkpoints' modules spell it
    v = h.to(torch.float32).pow(2).mean(-1, keepdim=True)
    return w * (h.to(torch.float32) * torch.rsqrt(v + EPS)).to(h.dtype)


for model in args.models.split(","):
    K, I = MODELS[model]
    for front in args.fronts.split(","):
        widths = (K, K, K) if front == "qkv" else (I, I)
        for bits in map(int, args.bits.split(",")):
            for tag, frac, topX in (("s0", 0.0, 0), ("s45+top10", 0.0045, 10)):
                sets = [tuple(synth.make_layer(K, n, bits, sparse_frac=frac, topX=topX, heavy_rows=10 if frac else 0, device=dev, seed=3 * i + j)
                              for j, n in enumerate(widths)) for i in range(args.layers)]
                mods = [tuple(quant.QuantLinearLUT.from_operands(l) for l in t) for t in sets]
                fused = [quant.QuantQKVRopeFused(*m, head_dim=D) if front == "qkv" else quant.QuantGatedLUTFused(*m) for m in mods]
                for rows in map(int, args.rows.split(",")):
                    for dname in args.dtypes.split(","):
                        dt = DT[dname]
                        xs = [(torch.randn((rows, K), device=dev) * (1 + i % 5)).to(dt) for i in range(len(sets))]
                        ws = [(1 + 0.1 * torch.randn(K, device=dev)).to(dt) for _ in sets]
                        xns = [module_norm(x, w) for x, w in zip(xs, ws)]
                        pos = torch.randint(0, N_POS, (rows,), device=dev, dtype=torch.int32)
                        keep = []
                        call = (lambda m, h, **kw: m(h, pos, cos32, sin32, **kw)) if front == "qkv" else (lambda m, h, **kw: m(h, **kw))

                        def run_a():
                            keep.clear()
                            with torch.no_grad():
                                for m, x, w in zip(fused, xs, ws): keep.append(call(m, module_norm(x, w)))

                        def run_b():
                            keep.clear()
                            with torch.no_grad():
                                for m, x, w in zip(fused, xs, ws): keep.append(call(m, torch.nn.functional.rms_norm(x, (K,), w, EPS)))

                        def run_c():
                            keep.clear()
                            with torch.no_grad():
                                for m, x, w in zip(fused, xs, ws): keep.append(call(m, x, norm_weight=w, norm_eps=EPS))

                        def run_p():
                            keep.clear()
                            with torch.no_grad():
                                for m, xn in zip(fused, xns): keep.append(call(m, xn))

                        first = lambda: (keep[-1][0] if front == "qkv" else keep[-1]).float().reshape(-1)  # noqa: E731
                        runs = {"A": run_a, "B": run_b, "C": run_c, "P": run_p}
                        run_a(); a = first(); run_c(); c = first()
                        torch.cuda.synchronize()
                        dev_ac = float((a - c).abs().max())
                        gs = {k: capture(f) for k, f in runs.items()}
                        for g in gs.values(): timed(g.replay, 5, 3)
                        ms = {k: [] for k in gs}
                        order = ["A", "B", "C", "P"]
                        for r in range(args.reps):
                            for k in order[r % 4:] + order[:r % 4]: ms[k].append(timed(gs[k].replay))
                        med = {k: statistics.median(v) for k, v in ms.items()}
                        spread = {k: max(v) - min(v) for k, v in ms.items()}
                        per_layer = lambda d: round(d * 1e3 / len(sets), 2)  # noqa: E731
                        rec = dict(model=model, front=front, bits=bits, sparse=tag, rows=rows, dtype=dname, layers=len(sets), reps=args.reps)
                        for k in order:
                            rec[f"{k}_median_ms"] = round(med[k], 4); rec[f"{k}_spread_ms"] = round(spread[k], 4)
                        rec.update(C_minus_P_us_per_layer=per_layer(med["C"] - med["P"]), A_minus_P_us_per_layer=per_layer(med["A"] - med["P"]),
                                   B_minus_P_us_per_layer=per_layer(med["B"] - med["P"]), C_minus_A_us_per_layer=per_layer(med["C"] - med["A"]),
                                   C_minus_B_us_per_layer=per_layer(med["C"] - med["B"]),
                                   C_beats_B_by_more_than_the_spread=bool(med["B"] - med["C"] > max(spread["B"], spread["C"])),
                                   max_abs_A_minus_C=dev_ac)
                        print(json.dumps(rec), flush=True)
                        del gs, xs, ws, xns; keep.clear()
                del sets, mods, fused
                torch.cuda.empty_cache()
