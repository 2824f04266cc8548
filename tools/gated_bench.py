"""The gated front of the MLP three ways, graph-replayed alternately in ONE process (built like linear_overhead.py --alternate).

    python tools/gated_bench.py [--models 7b,13b] [--bits 3,4] [--rows 1,4,8] [--dtypes fp16,bf16] [--layers 32] [--reps 5]

Workload: the gate / up pairs of --layers decoder layers with distinct weights (32 pairs of 7B w3 are 1.1 GB: more than the
256 MB Infinity Cache), each pair over its own activations; s0 (dense only) and s45 + top-10.  Per point, three ways:
  A  two QuantLinearLUTFused modules + torch silu, mul                         (4 launches per pair)
  B  the two linears as one sqllm_linear_*_groups launch + torch silu, mul     (3 launches per pair)
  C  QuantGatedLUTFused: the gated kernel                                       (1 launch per pair)
Each way is captured once after an eager warm-up; the three graphs are then replayed alternately, --reps repetitions of 30
replays each.  One JSON line per point: the median per way and its spread (max - min) in ms per pass over all pairs, C against
A and B in percent, and the eager time of A and C through the modules (min of 3 runs of 5 passes).
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from squeezellm_amd import decode, quant, synth

SHAPES = {"7b": (4096, 11008), "13b": (5120, 13824)}
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
ap = argparse.ArgumentParser()
ap.add_argument("--models", default="7b,13b")
ap.add_argument("--bits", default="3,4")
ap.add_argument("--rows", default="1,4,8")
ap.add_argument("--dtypes", default="fp16,bf16")
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
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


for model in args.models.split(","):
    K, N = SHAPES[model]
    for bits in map(int, args.bits.split(",")):
        for tag, frac, topX in (("s0", 0.0, 0), ("s45+top10", 0.0045, 10)):
            pairs = [tuple(synth.make_layer(K, N, bits, sparse_frac=frac, topX=topX, heavy_rows=10 if frac else 0, device=dev, seed=2 * i + j)
                           for j in range(2)) for i in range(args.layers)]
            lin = [tuple(quant.QuantLinearLUTFused.from_operands(l) for l in p) for p in pairs]
            gated = [quant.QuantGatedLUTFused(*(quant.QuantLinearLUT.from_operands(l) for l in p)) for p in pairs]
            for rows in map(int, args.rows.split(",")):
                for dname in args.dtypes.split(","):
                    dt = DT[dname]
                    xs = [torch.randn((rows, K), device=dev).to(dt) for _ in pairs]
                    xin = [x if rows > 1 else x.reshape(1, 1, K) for x in xs]
                    ys = [tuple(torch.empty((rows, N), device=dev, dtype=dt) for _ in range(2)) for _ in pairs]
                    seqs = [decode.OpSequence(list(p), [x if rows > 1 else x.reshape(K)] * 2, list(y), batched=rows > 1, fuse_shared_input=True, linear=True)
                            for p, x, y in zip(pairs, xs, ys)]
                    assert all(s.n_groups == 1 for s in seqs)
                    keep = []

                    def run_a():
                        keep.clear()
                        with torch.no_grad():
                            for (g, u), x in zip(lin, xin): keep.append(F.silu(g(x)) * u(x))

                    def run_b():
                        keep.clear()
                        with torch.no_grad():
                            for s, (yg, yu) in zip(seqs, ys):
                                s.launch(); keep.append(F.silu(yg) * yu)

                    def run_c():
                        keep.clear()
                        with torch.no_grad():
                            for m, x in zip(gated, xin): keep.append(m(x))

                    runs = {"A": run_a, "B": run_b, "C": run_c}
                    eager = {k: min(timed(runs[k], 5, 2) for _ in range(3)) for k in ("A", "C")}
                    run_a(); a = keep[-1].float(); run_c(); c = keep[-1].float(); run_b(); b = keep[-1].float()
                    torch.cuda.synchronize()
                    dev_ab = float((a.reshape(-1) - c.reshape(-1)).abs().max()); dev_bc = float((b.reshape(-1) - c.reshape(-1)).abs().max())
                    gs = {k: capture(f) for k, f in runs.items()}
                    for g in gs.values(): timed(g.replay, 5, 3)
                    ms = {k: [] for k in gs}
                    order = ["A", "B", "C"]
                    for r in range(args.reps):
                        for k in order[r % 3:] + order[:r % 3]: ms[k].append(timed(gs[k].replay))
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    rec = dict(model=model, bits=bits, sparse=tag, rows=rows, dtype=dname, pairs=len(pairs), reps=args.reps)
                    for k in order:
                        rec[f"{k}_median_ms"] = round(med[k], 4); rec[f"{k}_spread_ms"] = round(max(ms[k]) - min(ms[k]), 4)
                    rec.update(C_vs_A_pct=round((med["C"] / med["A"] - 1) * 100, 1), C_vs_B_pct=round((med["C"] / med["B"] - 1) * 100, 1),
                               A_eager_ms=round(eager["A"], 4), C_eager_ms=round(eager["C"], 4), max_abs_A_minus_C=dev_ab, max_abs_B_minus_C=dev_bc)
                    print(json.dumps(rec), flush=True)
                    del gs, seqs, ys, xs, xin; keep.clear()
            del pairs, lin, gated
            torch.cuda.empty_cache()
