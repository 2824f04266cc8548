"""A linear followed by a residual add or a ReLU two ways, graph-replayed alternately in ONE process (built like gated_bench.py).

    python tools/epilogue_bench.py [--shapes 7b_o,7b_down,13b_o,13b_down,opt_fc1] [--bits 3,4] [--rows 1,4,16] [--dtypes fp16,bf16]
                                   [--sparse s0,s45+top10] [--layers 32] [--reps 5]

Workload: --layers layers of one shape with distinct weights (32 layers of the 7B o_proj in w4 are 268 MB: more than the 256 MB
Infinity Cache), each over its own activations and its own residual.  The LLaMA shapes (o_proj, down_proj of 7B and 13B) are
followed by `residual + y`, OPT-6.7B's fc1 (4096 -> 16384) by `relu(y)`.  Per point, two ways:
  A  QuantLinearLUTFused, then torch add / relu                      (2 launches per layer: what the class offered before)
  B  QuantLinearLUTFused.forward(x, residual=...) / act = "relu"     (1 launch per layer: sqllm_linear_ep_*)
Each way is captured once after an eager warm-up; the two graphs are then replayed alternately, --reps repetitions of 30 replays
each.  One JSON line per point: the median per way and its spread (max - min) in ms per pass over all layers, B against A in
percent and in us per layer, the eager time of both through the modules (min of 3 runs of 5 passes), and the largest difference
between the two results.
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from squeezellm_amd import quant, synth

# name -> (K, N, what follows the linear)
SHAPES = {"7b_o": (4096, 4096, "add"), "7b_down": (11008, 4096, "add"), "13b_o": (5120, 5120, "add"), "13b_down": (13824, 5120, "add"),
          "opt_fc1": (4096, 16384, "relu")}
SPARSE = {"s0": (0.0, 0), "s45+top10": (0.0045, 10)}
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default=",".join(SHAPES))
ap.add_argument("--bits", default="3,4")
ap.add_argument("--rows", default="1,4,16")
ap.add_argument("--dtypes", default="fp16,bf16")
ap.add_argument("--sparse", default="s0,s45+top10")
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("epilogue_bench.py measures on the GPU: none found (there is no CPU fallback)")
dev = torch.device("cuda:0")


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


for shape in args.shapes.split(","):
    K, N, after = SHAPES[shape]
    for bits in map(int, args.bits.split(",")):
        for tag in args.sparse.split(","):
            frac, topX = SPARSE[tag]
            lays = [synth.make_layer(K, N, bits, sparse_frac=frac, topX=topX, heavy_rows=10 if frac else 0, device=dev, seed=i) for i in range(args.layers)]
            plain = [quant.QuantLinearLUTFused.from_operands(l) for l in lays]
            fused = [quant.QuantLinearLUTFused.from_operands(l) for l in lays]
            if after == "relu":
                for m in fused: m.act = "relu"
            for rows in map(int, args.rows.split(",")):
                for dname in args.dtypes.split(","):
                    dt = DT[dname]
                    xs = [torch.randn((rows, K), device=dev).to(dt) for _ in lays]
                    xin = [x if rows > 1 else x.reshape(1, 1, K) for x in xs]
                    rs = [torch.randn(x.shape[:-1] + (N,), device=dev).to(dt) for x in xin]
                    keep = []

                    def run_a():
                        keep.clear()
                        with torch.no_grad():
                            for m, x, r in zip(plain, xin, rs): keep.append(r + m(x) if after == "add" else torch.relu(m(x)))

                    def run_b():
                        keep.clear()
                        with torch.no_grad():
                            for m, x, r in zip(fused, xin, rs): keep.append(m(x, residual=r) if after == "add" else m(x))

                    runs = {"A": run_a, "B": run_b}
                    eager = {k: min(timed(runs[k], 5, 2) for _ in range(3)) for k in runs}
                    run_a(); a = keep[-1].float(); run_b(); b = keep[-1].float()
                    torch.cuda.synchronize()
                    assert fused[0].last_route == "fused_ep" and plain[0].last_route == "fused"
                    dev_ab = float((a.reshape(-1) - b.reshape(-1)).abs().max())
                    gs = {k: capture(f) for k, f in runs.items()}
                    for g in gs.values(): timed(g.replay, 5, 3)
                    ms = {k: [] for k in gs}
                    for r in range(args.reps):
                        for k in (("A", "B") if r % 2 == 0 else ("B", "A")): ms[k].append(timed(gs[k].replay))
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    rec = dict(shape=shape, K=K, N=N, after=after, bits=bits, sparse=tag, rows=rows, dtype=dname, layers=len(lays), reps=args.reps)
                    for k in ("A", "B"):
                        rec[f"{k}_median_ms"] = round(med[k], 4); rec[f"{k}_spread_ms"] = round(max(ms[k]) - min(ms[k]), 4)
                    rec.update(B_vs_A_pct=round((med["B"] / med["A"] - 1) * 100, 1), B_minus_A_us_per_layer=round((med["B"] - med["A"]) * 1e3 / len(lays), 3),
                               A_eager_ms=round(eager["A"], 4), B_eager_ms=round(eager["B"], 4), max_abs_A_minus_B=dev_ab)
                    print(json.dumps(rec), flush=True)
                    del gs, xs, xin, rs; keep.clear()
            del lays, plain, fused
            torch.cuda.empty_cache()
