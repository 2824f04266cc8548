"""What writing k and v into the KV cache costs, three ways, graph-replayed alternately in ONE process (built like qkv_rope_bench.py).

    python tools/kv_cache_bench.py [--shapes mha,gqa] [--bits 3,4] [--rows 1,4,16] [--dtypes fp16,bf16] [--layers 32] [--reps 5]
    python tools/kv_cache_bench.py --fp8 [...]      # a fourth way, d: the fp8 cache entry, against c

Workload: qkv_rope_bench.py's -- the q / k / v projections of --layers decoder layers with distinct weights, each over its own
activations, K = 4096, head_dim 128, positions drawn per row; shapes mha and gqa; s0 and s45 + top-10 -- and per layer a
preallocated slot-major cache pair [n_slots, H, D] (--slots, 256) with distinct slots drawn per row.  Per point, three ways:
  a  QuantQKVRopeFused alone: the parent entry, k and v returned and left where they are          (1 launch per layer)
  b  the same, and k and v copied into the caches in torch: index_copy_ by slot, twice            (3 launches per layer)
  c  QuantQKVRopeFused with the caches and return_kv=False: the cache entry                       (1 launch per layer)
Each way is captured once after an eager warm-up; the three graphs are then replayed alternately, --reps repetitions of 30
replays each.  One JSON line per point: the median per way and its spread (max - min) in ms per pass over all layers, and in us
per layer c - a (what the scattered stores cost) and b - c (what the fused write saves; negative: it does not pay), with a
sanity check that b's and c's caches hold the same bits.
  d  (--fp8) QuantQKVRopeFused with float8_e4m3fn caches of the same shape, k_scale and v_scale, return_kv=False: the fp8 writer.
     Reported as d - c in us per layer (negative: the fp8 writer is the faster one) and `fp8_slower`.
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from squeezellm_amd import quant, synth

K, D, N_POS = 4096, 128, 4096
SHAPES = {"mha": (4096, 4096, 4096), "gqa": (4096, 1024, 1024)}
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="mha,gqa")
ap.add_argument("--bits", default="3,4")
ap.add_argument("--rows", default="1,4,16")
ap.add_argument("--dtypes", default="fp16,bf16")
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--slots", type=int, default=256)
ap.add_argument("--fp8", action="store_true")
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


for shape in args.shapes.split(","):
    widths = SHAPES[shape]
    H = widths[1] // D
    for bits in map(int, args.bits.split(",")):
        for tag, frac, topX in (("s0", 0.0, 0), ("s45+top10", 0.0045, 10)):
            trios = [tuple(synth.make_layer(K, n, bits, sparse_frac=frac, topX=topX, heavy_rows=10 if frac else 0, device=dev, seed=3 * i + j)
                           for j, n in enumerate(widths)) for i in range(args.layers)]
            fused = [quant.QuantQKVRopeFused(*(quant.QuantLinearLUT.from_operands(l) for l in t), head_dim=D) for t in trios]
            for rows in map(int, args.rows.split(",")):
                for dname in args.dtypes.split(","):
                    dt = DT[dname]
                    xs = [torch.randn((rows, K), device=dev).to(dt) for _ in trios]
                    pos = torch.randint(0, N_POS, (rows,), device=dev, dtype=torch.int32)
                    slots = torch.randperm(args.slots, device=dev)[:rows].to(torch.int32)
                    slots64 = slots.long()
                    caches = {w: [tuple(torch.zeros((args.slots, H, D), device=dev, dtype=dt) for _ in "kv") for _ in trios] for w in "bc"}
                    keep = []

                    def run_a():
                        keep.clear()
                        with torch.no_grad():
                            for m, x in zip(fused, xs): keep.append(m(x, pos, cos32, sin32))

                    def run_b():
                        keep.clear()
                        with torch.no_grad():
                            for m, x, (kc, vc) in zip(fused, xs, caches["b"]):
                                q, k, v = m(x, pos, cos32, sin32)
                                kc.index_copy_(0, slots64, k.view(rows, H, D)); vc.index_copy_(0, slots64, v.view(rows, H, D))
                                keep.append(q)

                    def run_c():
                        keep.clear()
                        with torch.no_grad():
                            for m, x, (kc, vc) in zip(fused, xs, caches["c"]):
                                keep.append(m(x, pos, cos32, sin32, k_cache=kc, v_cache=vc, slots=slots, return_kv=False)[0])

                    caches8 = [tuple(torch.zeros((args.slots, H, D), device=dev, dtype=torch.float8_e4m3fn) for _ in "kv") for _ in trios] if args.fp8 else []

                    def run_d():
                        keep.clear()
                        with torch.no_grad():
                            for m, x, (kc, vc) in zip(fused, xs, caches8):
                                keep.append(m(x, pos, cos32, sin32, k_cache=kc, v_cache=vc, slots=slots, return_kv=False, k_scale=0.0625, v_scale=0.03125)[0])

                    runs = {"a": run_a, "b": run_b, "c": run_c}
                    if args.fp8:
                        runs["d"] = run_d
                        run_d()
                    run_b(); run_c(); torch.cuda.synchronize()
                    same = all(torch.equal(b.view(torch.int16), c.view(torch.int16)) for lb, lc in zip(caches["b"], caches["c"]) for b, c in zip(lb, lc))
                    gs = {k: capture(f) for k, f in runs.items()}
                    for g in gs.values(): timed(g.replay, 5, 3)
                    ms = {k: [] for k in gs}
                    order = list(runs)
                    for r in range(args.reps):
                        for k in order[r % len(order):] + order[:r % len(order)]: ms[k].append(timed(gs[k].replay))
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    rec = dict(shape=shape, bits=bits, sparse=tag, rows=rows, dtype=dname, layers=len(trios), reps=args.reps)
                    for k in order:
                        rec[f"{k}_median_ms"] = round(med[k], 4); rec[f"{k}_spread_ms"] = round(max(ms[k]) - min(ms[k]), 4)
                    rec.update(c_minus_a_us_per_layer=round((med["c"] - med["a"]) * 1e3 / len(trios), 2),
                               b_minus_c_us_per_layer=round((med["b"] - med["c"]) * 1e3 / len(trios), 2),
                               b_minus_a_us_per_layer=round((med["b"] - med["a"]) * 1e3 / len(trios), 2),
                               caches_equal=same)
                    if args.fp8:
                        rec.update(d_minus_c_us_per_layer=round((med["d"] - med["c"]) * 1e3 / len(trios), 2), fp8_slower=med["d"] > med["c"])
                    print(json.dumps(rec), flush=True)
                    del gs, xs, caches, caches8; keep.clear()
            del trios, fused
            torch.cuda.empty_cache()
