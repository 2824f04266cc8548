"""The attention front three ways, graph-replayed alternately in ONE process (built like gated_bench.py / epilogue_bench.py).

    python tools/qkv_rope_bench.py [--shapes mha,gqa] [--bits 3,4] [--rows 1,4,16] [--dtypes fp16,bf16] [--layers 32] [--reps 5]

Workload: the q / k / v projections of --layers decoder layers with distinct weights (32 layers of the 7B w3 shape are 0.6 GB:
more than the 256 MB Infinity Cache), each over its own activations, K = 4096, head_dim 128, positions drawn per row;
shapes mha (N_q = N_k = N_v = 4096) and gqa (N_q = 4096, N_k = N_v = 1024); s0 (dense only) and s45 + top-10.  Per point, three ways:
  A  three QuantLinearLUTFused modules + the rotary step in torch              (3 launches + the torch string per layer)
  B  the three linears as one sqllm_linear_*_groups launch + the same step     (1 launch + the torch string per layer)
  C  QuantQKVRopeFused: the q/k/v kernel                                        (1 launch per layer)
The torch step is the rotate_half form as model code writes it: cos / sin gathered by position from [n_pos, D] tables of the
activations' type, q * cos + rotate_half(q) * sin, the same for k.  Each way is captured once after an eager warm-up; the three
graphs are then replayed alternately, --reps repetitions of 30 replays each.  One JSON line per point: the median per way and
its spread (max - min) in ms per pass over all layers, C against A and B in percent and in us per layer, and the largest
difference between the ways' q outputs (a sanity check, not a test).
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from squeezellm_amd import decode, quant, synth

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


def rotate_half(t):
    return torch.cat((-t[..., D // 2:], t[..., : D // 2]), dim=-1)


def rope_torch(q, k, pos, cos16, sin16):
    c, s = cos16[pos][:, None, :], sin16[pos][:, None, :]
    qh, kh = q.view(q.shape[0], -1, D), k.view(k.shape[0], -1, D)
    return (qh * c + rotate_half(qh) * s).view(q.shape), (kh * c + rotate_half(kh) * s).view(k.shape)


for shape in args.shapes.split(","):
    widths = SHAPES[shape]
    for bits in map(int, args.bits.split(",")):
        for tag, frac, topX in (("s0", 0.0, 0), ("s45+top10", 0.0045, 10)):
            trios = [tuple(synth.make_layer(K, n, bits, sparse_frac=frac, topX=topX, heavy_rows=10 if frac else 0, device=dev, seed=3 * i + j)
                           for j, n in enumerate(widths)) for i in range(args.layers)]
            lin = [tuple(quant.QuantLinearLUTFused.from_operands(l) for l in t) for t in trios]
            fused = [quant.QuantQKVRopeFused(*(quant.QuantLinearLUT.from_operands(l) for l in t), head_dim=D) for t in trios]
            for rows in map(int, args.rows.split(",")):
                for dname in args.dtypes.split(","):
                    dt = DT[dname]
                    cos16, sin16 = (torch.cat((t, t), dim=-1).to(dt) for t in (cos32, sin32))
                    xs = [torch.randn((rows, K), device=dev).to(dt) for _ in trios]
                    pos = torch.randint(0, N_POS, (rows,), device=dev, dtype=torch.int32)
                    pos64 = pos.long()
                    ys = [tuple(torch.empty((rows, n), device=dev, dtype=dt) for n in widths) for _ in trios]
                    seqs = [decode.OpSequence(list(t), [x if rows > 1 else x.reshape(K)] * 3, list(y), batched=rows > 1, fuse_shared_input=True, linear=True)
                            for t, x, y in zip(trios, xs, ys)]
                    assert all(s.n_groups == 1 for s in seqs)
                    keep = []

                    def run_a():
                        keep.clear()
                        with torch.no_grad():
                            for (q, k, v), x in zip(lin, xs): keep.append((*rope_torch(q(x), k(x), pos64, cos16, sin16), v(x)))

                    def run_b():
                        keep.clear()
                        with torch.no_grad():
                            for s, (yq, yk, yv) in zip(seqs, ys):
                                s.launch(); keep.append((*rope_torch(yq, yk, pos64, cos16, sin16), yv))

                    def run_c():
                        keep.clear()
                        with torch.no_grad():
                            for m, x in zip(fused, xs): keep.append(m(x, pos, cos32, sin32))

                    runs = {"A": run_a, "B": run_b, "C": run_c}
                    run_a(); a = keep[-1][0].float(); run_c(); c = keep[-1][0].float(); run_b(); b = keep[-1][0].float()
                    torch.cuda.synchronize()
                    dev_ac = float((a.reshape(-1) - c.reshape(-1)).abs().max()); dev_bc = float((b.reshape(-1) - c.reshape(-1)).abs().max())
                    gs = {k: capture(f) for k, f in runs.items()}
                    for g in gs.values(): timed(g.replay, 5, 3)
                    ms = {k: [] for k in gs}
                    order = ["A", "B", "C"]
                    for r in range(args.reps):
                        for k in order[r % 3:] + order[:r % 3]: ms[k].append(timed(gs[k].replay))
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    rec = dict(shape=shape, bits=bits, sparse=tag, rows=rows, dtype=dname, layers=len(trios), reps=args.reps)
                    for k in order:
                        rec[f"{k}_median_ms"] = round(med[k], 4); rec[f"{k}_spread_ms"] = round(max(ms[k]) - min(ms[k]), 4)
                    rec.update(C_vs_A_pct=round((med["C"] / med["A"] - 1) * 100, 1), C_vs_B_pct=round((med["C"] / med["B"] - 1) * 100, 1),
                               C_minus_A_us_per_layer=round((med["C"] - med["A"]) * 1e3 / len(trios), 2),
                               C_minus_B_us_per_layer=round((med["C"] - med["B"]) * 1e3 / len(trios), 2),
                               max_abs_qA_minus_qC=dev_ac, max_abs_qB_minus_qC=dev_bc)
                    print(json.dumps(rec), flush=True)
                    del gs, seqs, ys, xs; keep.clear()
            del trios, lin, fused
            torch.cuda.empty_cache()
