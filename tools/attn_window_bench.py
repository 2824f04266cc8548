"""Sliding-window decode attention: quant.DecodeAttention(window=W) against the entries without a window, graph-replayed
alternately in ONE process (built like attn_decode_bench.py).

    python tools/attn_window_bench.py [--heads 32/32,32/8] [--rows 1,4,16] [--windows 1024,4096] [--caches 16,fp8] [--layers 2] [--reps 3]

Workload: --layers attention layers with distinct paged caches [rows * 8W / 16 blocks, 16, H_kv, 128] (fp16 queries; 16-bit or
float8_e4m3fn caches) behind a shuffled block table of capacity 8W per row, every row at the same length L in {W/2, W, 2W, 8W}.
Per point, three readings, each one call per layer:
  window  DecodeAttention(window=W) at length L over the table of capacity 8W -- the window entry
  whole   DecodeAttention() at the same L over the same table -- what a caller pays today for attending ALL keys (for L > W the
          wrong answer): the bytes the window saves
  floor   DecodeAttention() at length min(L, W) over the first W / 16 table entries (capacity W) -- the same attended bytes
          without a window: the window entry additionally pays one partly used partition and the device-side lookup of its
          first partition
Each reading is captured once after an eager warm-up; the graphs are replayed alternately, --reps repetitions of 20 replays.
One JSON line per point: median us per call (per layer) and spread per reading, the attended K + V bytes, window / whole,
window / floor, and `window_not_faster_than_whole`.  For L <= W the window result is compared bit for bit with `whole`."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from squeezellm_amd import quant

D, BLOCK = 128, 16
ap = argparse.ArgumentParser()
ap.add_argument("--heads", default="32/32,32/8")
ap.add_argument("--rows", default="1,4,16")
ap.add_argument("--windows", default="1024,4096")
ap.add_argument("--caches", default="16,fp8")
ap.add_argument("--layers", type=int, default=2)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda:0")
dt = torch.float16


def timed(fn, reps=20, warmup=2):
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


print(json.dumps(dict(tool="attn_window_bench", torch=torch.__version__, partition=quant.ATTN_PARTITION, head_dim=D, block=BLOCK,
                      layers=args.layers, reps=args.reps, dtype="fp16")), flush=True)
for heads in args.heads.split(","):
    HQ, H = map(int, heads.split("/"))
    plain = quant.DecodeAttention(HQ, H, D, block_size=BLOCK)
    for rows in map(int, args.rows.split(",")):
        for W in map(int, args.windows.split(",")):
            cap = 8 * W
            att = quant.DecodeAttention(HQ, H, D, block_size=BLOCK, window=W)
            n_blocks = rows * cap // BLOCK
            table = torch.randperm(n_blocks, device=dev).reshape(rows, cap // BLOCK).to(torch.int32)
            qs = [torch.randn((rows, HQ * D), device=dev).to(dt) for _ in range(args.layers)]
            for cache in args.caches.split(","):
                caches, scales = [], []
                for _ in range(args.layers):
                    pair = [torch.randn((n_blocks, BLOCK, H, D), device=dev, dtype=dt) for _ in "kv"]
                    if cache == "fp8":
                        sc = [float(quant.fp8_kv_scale(t.float().abs().max())) for t in pair]
                        pair = [(t.float() / s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn) for t, s in zip(pair, sc)]
                        scales.append(dict(k_scale=sc[0], v_scale=sc[1]))
                    else:
                        scales.append({})
                    caches.append(tuple(quant.kv_cache_view(t, "nhd") for t in pair))
                for L in (W // 2, W, 2 * W, 8 * W):
                    lens = torch.full((rows,), L, dtype=torch.int32, device=dev)
                    lens_floor = torch.full((rows,), min(L, W), dtype=torch.int32, device=dev)
                    table_floor = table[:, :W // BLOCK]
                    keep = []

                    def run_window():
                        keep.clear()
                        with torch.no_grad():
                            for q, (k, v), s in zip(qs, caches, scales): keep.append(att(q, k, v, table, lens, **s))

                    def run_whole():
                        keep.clear()
                        with torch.no_grad():
                            for q, (k, v), s in zip(qs, caches, scales): keep.append(plain(q, k, v, table, lens, **s))

                    def run_floor():
                        keep.clear()
                        with torch.no_grad():
                            for q, (k, v), s in zip(qs, caches, scales): keep.append(plain(q, k, v, table_floor, lens_floor, **s))

                    run_window(); yw = keep[0].clone(); assert att.last_route == "attn_window"
                    run_whole(); ya = keep[0].clone(); assert plain.last_route == "attn_decode"
                    torch.cuda.synchronize()
                    same = bool(torch.equal(yw, ya))
                    assert same == (L <= W), (L, W, same)  # inside the window: the bits of the entry without one; beyond it: another result
                    runs = {"window": run_window, "whole": run_whole, "floor": run_floor}
                    gs = {k: capture(f) for k, f in runs.items()}
                    for g in gs.values(): timed(g.replay, 3, 2)
                    ms = {k: [] for k in gs}
                    order = list(runs)
                    for r in range(args.reps):
                        for k in order[r % 3:] + order[:r % 3]: ms[k].append(timed(gs[k].replay))
                    us = {k: statistics.median(v) * 1e3 / args.layers for k, v in ms.items()}
                    elem = 1 if cache == "fp8" else 2
                    attended = rows * H * min(L, W) * D * elem * 2
                    rec = dict(heads=heads, rows=rows, cache=cache, window=W, capacity=cap, seq_len=L, attended_kv_bytes=attended,
                               whole_kv_bytes=rows * H * L * D * elem * 2, l3_resident=rows * H * L * D * elem * 2 * args.layers <= 256 << 20)
                    for k in order:
                        rec[f"{k}_us"] = round(us[k], 2)
                        rec[f"{k}_spread_us"] = round((max(ms[k]) - min(ms[k])) * 1e3 / args.layers, 2)
                    rec.update(window_over_whole=round(us["window"] / us["whole"], 3), window_over_floor=round(us["window"] / us["floor"], 3),
                               window_TBps=round(attended / us["window"] / 1e6, 3), fit_us=round(2 * 3 + attended / 4.8e6, 2),
                               window_not_faster_than_whole=us["window"] >= us["whole"], equals_whole_bits=same)
                    print(json.dumps(rec), flush=True)
                    del gs; keep.clear()
                del caches
                torch.cuda.empty_cache()
