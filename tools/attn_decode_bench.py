"""Decode attention: quant.DecodeAttention against torch SDPA over the static cache with a length mask, graph-replayed alternately
in ONE process (built like kv_cache_bench.py).

    python tools/attn_decode_bench.py [--heads 32/32,32/8] [--rows 1,4,16] [--lens 128,1024,4096] [--dtypes fp16,bf16] [--layers 4] [--reps 3]
    python tools/attn_decode_bench.py --cache fp8 [...]       # the fp8 KV cache against the 16-bit kernels, the same points

Workload: --layers attention layers with distinct caches and queries, head_dim 128, every row at the same sequence length, in
  * a head-major static cache [rows, H_kv, S = 4096, D] per layer (kv_cache_view "bhsd", static_cache_blocks), and
  * a paged cache [rows * S / 16 blocks, 16, H_kv, D] per layer with a shuffled block table, the same keys.
Per point, three ways, each one call per layer:
  sdpa    torch.nn.functional.scaled_dot_product_attention(q [B, HQ, 1, D], k_cache, v_cache, attn_mask = arange(S) < lens) --
          what an integrator writes without this library; the mask is rebuilt from the device lengths inside the captured
          step (one small kernel), grouped-query attention through torch's own enable_gqa (expanded heads where torch lacks it)
  static  DecodeAttention over the "bhsd" view
  paged   DecodeAttention over the paged cache
Each way is captured once after an eager warm-up; the graphs are replayed alternately, --reps repetitions of 20 replays each.
One JSON line per point: median us per call (per layer) and spread per way; the attended K + V bytes per call; the effective
TB/s of the two kernels' ways; the per-launch fit of DESIGN.md 5, launches x 3 us + bytes / 4.8 TB/s; whether the kernel is
faster than sdpa; and the largest |static - sdpa| as a sanity check.  K + V of all layers at short lengths fit the 256 MiB
Infinity Cache: those points measure on-die reads, and say so (`l3_resident`).

--cache fp8: the ways are static, paged (the 16-bit kernels, as above) and static_fp8, paged_fp8 -- DecodeAttention over the same
keys quantised to float8_e4m3fn caches of the same two layouts (one scale per cache, fp8_kv_scale of the largest magnitude),
no sdpa.  Per point: us per call of the four ways, fp8 / 16-bit per layout, and `fp8_slower` naming the layouts where fp8 lost.
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from squeezellm_amd import quant

D, S, BLOCK = 128, 4096, 16
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
ap = argparse.ArgumentParser()
ap.add_argument("--heads", default="32/32,32/8")
ap.add_argument("--rows", default="1,4,16")
ap.add_argument("--lens", default="128,1024,4096")
ap.add_argument("--dtypes", default="fp16,bf16")
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cache", default="16", choices=["16", "fp8"])
args = ap.parse_args()
dev = torch.device("cuda:0")
sdpa = torch.nn.functional.scaled_dot_product_attention
try:
    sdpa(torch.zeros(1, 2, 1, 8, device=dev), torch.zeros(1, 1, 4, 8, device=dev), torch.zeros(1, 1, 4, 8, device=dev), enable_gqa=True)
    GQA = "enable_gqa"
except TypeError:
    GQA = "expanded"


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


print(json.dumps(dict(tool="attn_decode_bench", torch=torch.__version__, gqa=GQA, partition=quant.ATTN_PARTITION, head_dim=D, S=S, block=BLOCK,
                      layers=args.layers, reps=args.reps)), flush=True)
for heads in args.heads.split(","):
    HQ, H = map(int, heads.split("/"))
    att = quant.DecodeAttention(HQ, H, D)
    for rows in map(int, args.rows.split(",")):
        for dname in args.dtypes.split(","):
            dt = DT[dname]
            # the static caches; the paged ones hold the same keys behind a shuffled table
            statics = [tuple(torch.randn((rows, H, S, D), device=dev).to(dt) for _ in "kv") for _ in range(args.layers)]
            perm = torch.randperm(rows * S // BLOCK, device=dev)
            table = perm.reshape(rows, S // BLOCK).to(torch.int32)
            pageds = []
            for ks, vs in statics:
                pair = []
                for t in (ks, vs):
                    blocks = t.permute(0, 2, 1, 3).reshape(rows * S // BLOCK, BLOCK, H, D)  # [row-major blocks, 16, H, D]
                    p = torch.empty_like(blocks)
                    p[perm] = blocks
                    pair.append(quant.kv_cache_view(p, "nhd"))
                pageds.append(tuple(pair))
            views = [tuple(quant.kv_cache_view(t, "bhsd") for t in pair) for pair in statics]
            sblocks = quant.static_cache_blocks(rows, H, dev)
            qs = [torch.randn((rows, HQ * D), device=dev).to(dt) for _ in range(args.layers)]
            if args.cache == "fp8":  # the same keys as bytes, in both layouts; one scale per cache
                scales = [tuple(float(quant.fp8_kv_scale(t.float().abs().max())) for t in pair) for pair in statics]
                to8 = lambda t, s: (t.float() / s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)  # noqa: E731
                views8 = [tuple(quant.kv_cache_view(to8(t, s), "bhsd") for t, s in zip(pair, sc)) for pair, sc in zip(statics, scales)]
                pageds8 = [tuple(quant.kv_cache_view(to8(t, s), "nhd") for t, s in zip(pair, sc)) for pair, sc in zip(pageds, scales)]
            ar = torch.arange(S, device=dev)
            for n in map(int, args.lens.split(",")):
                lens = torch.full((rows,), n, dtype=torch.int32, device=dev)
                keep = []

                def run_sdpa():
                    keep.clear()
                    with torch.no_grad():
                        for q, (k, v) in zip(qs, statics):
                            mask = (ar[None, :] < lens[:, None])[:, None, None, :]
                            q4 = q.view(rows, HQ, 1, D)
                            if H == HQ:
                                keep.append(sdpa(q4, k, v, attn_mask=mask))
                            elif GQA == "enable_gqa":
                                keep.append(sdpa(q4, k, v, attn_mask=mask, enable_gqa=True))
                            else:
                                g = HQ // H
                                keep.append(sdpa(q4, k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1), attn_mask=mask))

                def run_static():
                    keep.clear()
                    with torch.no_grad():
                        for q, (k, v) in zip(qs, views): keep.append(att(q, k, v, sblocks, lens, block_size=S))

                def run_paged():
                    keep.clear()
                    with torch.no_grad():
                        for q, (k, v) in zip(qs, pageds): keep.append(att(q, k, v, table, lens, block_size=BLOCK))

                def run_static8():
                    keep.clear()
                    with torch.no_grad():
                        for q, (k, v), (ks, vs) in zip(qs, views8, scales): keep.append(att(q, k, v, sblocks, lens, block_size=S, k_scale=ks, v_scale=vs))

                def run_paged8():
                    keep.clear()
                    with torch.no_grad():
                        for q, (k, v), (ks, vs) in zip(qs, pageds8, scales): keep.append(att(q, k, v, table, lens, block_size=BLOCK, k_scale=ks, v_scale=vs))

                if args.cache == "fp8":
                    run_static(); st = keep[0].float(); assert att.last_route == "attn_decode"
                    run_static8(); s8 = keep[0].float(); assert att.last_route == "attn_decode"
                    run_paged8(); p8 = keep[0].float()
                    torch.cuda.synchronize()
                    diff8, same8 = float((s8 - st).abs().max()), bool(torch.equal(s8, p8))
                    runs = {"static": run_static, "paged": run_paged, "static_fp8": run_static8, "paged_fp8": run_paged8}
                    gs = {k: capture(f) for k, f in runs.items()}
                    for g in gs.values(): timed(g.replay, 3, 2)
                    ms = {k: [] for k in gs}
                    order = list(runs)
                    for r in range(args.reps):
                        for k in order[r % 4:] + order[:r % 4]: ms[k].append(timed(gs[k].replay))
                    us = {k: statistics.median(v) * 1e3 / args.layers for k, v in ms.items()}
                    nbytes = rows * H * n * D * 2 * 2
                    rec = dict(heads=heads, rows=rows, dtype=dname, seq_len=n, kv_bytes_16=nbytes, kv_bytes_fp8=nbytes // 2,
                               l3_resident=nbytes * args.layers <= 256 << 20)
                    for k in order:
                        rec[f"{k}_us"] = round(us[k], 2)
                        rec[f"{k}_spread_us"] = round((max(ms[k]) - min(ms[k])) * 1e3 / args.layers, 2)
                    rec.update(static_fp8_over_16=round(us["static_fp8"] / us["static"], 3), paged_fp8_over_16=round(us["paged_fp8"] / us["paged"], 3),
                               fp8_slower=[k for k in ("static", "paged") if us[k + "_fp8"] > us[k]],
                               max_abs_diff_fp8_vs_16=round(diff8, 5), static_fp8_equals_paged_fp8=same8)
                    print(json.dumps(rec), flush=True)
                    del gs; keep.clear()
                    continue
                run_sdpa(); ref = keep[0].reshape(rows, HQ * D).float()
                run_static(); st = keep[0].float(); assert att.last_route == "attn_decode"
                run_paged(); pg = keep[0].float()
                torch.cuda.synchronize()
                diff, same = float((st - ref).abs().max()), bool(torch.equal(st, pg))
                runs = {"sdpa": run_sdpa, "static": run_static, "paged": run_paged}
                gs = {k: capture(f) for k, f in runs.items()}
                for g in gs.values(): timed(g.replay, 3, 2)
                ms = {k: [] for k in gs}
                order = list(runs)
                for r in range(args.reps):
                    for k in order[r % 3:] + order[:r % 3]: ms[k].append(timed(gs[k].replay))
                us = {k: statistics.median(v) * 1e3 / args.layers for k, v in ms.items()}
                nbytes = rows * H * n * D * 2 * 2
                launches = 1 if S <= quant.ATTN_PARTITION else 2
                rec = dict(heads=heads, rows=rows, dtype=dname, seq_len=n, kv_bytes=nbytes, l3_resident=nbytes * args.layers <= 256 << 20)
                for k in order:
                    rec[f"{k}_us"] = round(us[k], 2)
                    rec[f"{k}_spread_us"] = round((max(ms[k]) - min(ms[k])) * 1e3 / args.layers, 2)
                for k in ("static", "paged"):
                    rec[f"{k}_TBps"] = round(nbytes / us[k] / 1e6, 3)
                rec.update(fit_us=round(launches * 3 + nbytes / 4.8e6, 2), static_faster=us["static"] < us["sdpa"], paged_faster=us["paged"] < us["sdpa"],
                           max_abs_diff_vs_sdpa=round(diff, 5), static_equals_paged=same)
                print(json.dumps(rec), flush=True)
                del gs; keep.clear()
            if args.cache == "fp8": del views8, pageds8
            del statics, pageds, views, qs
            torch.cuda.empty_cache()
