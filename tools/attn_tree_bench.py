"""Tree-masked decode attention: quant.DecodeAttention(..., q_len=T, tree_mask=) on the tree kernels against what a caller has
without them, graph-replayed alternately in ONE process per group (built like attn_append_bench.py).

    python tools/attn_tree_bench.py [--heads 32/32,32/8] [--seqs 1,4] [--q-lens 8,16] [--contexts 128,1024,4096]
                                    [--caches 16,fp8] [--layers 4] [--reps 3] [--limit 240]

The driver starts one fresh child process per (heads, sequences, cache type) under its own time limit (--limit seconds) and stops
at the first child that fails or runs out of time; a child (--group) measures its tree x T x context points.

Workload per point: --layers attention layers with distinct caches and queries, fp16, head_dim 128, `seqs` sequences of
`context` keys and T nodes each in a paged cache with a shuffled table.  Two trees: "wide" (parent (t - 1) // 4) and "deep" (two
chains from one root).
  tree      one call with the tree's ancestor masks (quant.tree_masks): K and V read once
  chain     (a) one append call (q_len = T, no mask) on the same operands: the same bytes, another function -- the floor
  paths     (b) one append call per root-to-leaf path, q_len = the path's nodes, over context + that many keys: what a caller does
            today with kernels (the rows of q gathered outside the timed region; K and V read once per path)
  fallback  (c) the module's torch fallback on fp32 copies of the operands, timed eagerly (it synchronises): 5 calls, the median
`tree` with the chain's words is asserted bit-identical to `chain`, and `tree` against `fallback` to 2e-2, before they are timed.
tree, chain and paths are captured once after an eager warm-up; the graphs are replayed alternately, --reps repetitions of 20
replays each.  One JSON line per point: median us per call (per layer) and spread (max - min over the repetitions) per way;
`over_chain`: tree / chain, and whether tree - chain exceeds the chain's own spread; `paths_over_tree`, `tree_wins_paths`.

    python tools/attn_tree_bench.py --nodes 32,64 [--dtypes fp16,bf16] [--contexts 128,1024,4096,16384] [...]

--nodes: the WIDE trees instead, quant.PrefillAttention(..., q_len=T, tree_mask=) on the matrix-core kernels with the keys split
(sqllm_attn_tree64_*), T = the node counts, a child per (type, heads, sequences, cache type).  Contenders, graph-replayed alternately:
  tree64    one call with the tree's int64 ancestor masks (quant.tree_masks(wide=True))
  prefill   PrefillAttention without a mask on a chain of the same T and context: ANOTHER function, the unsplit time yardstick
  sdpa      torch SDPA with the boolean tree mask over K / V gathered from the pages (dequantised for an fp8 cache), gather included
  tree16    the 16-node tree entry (DecodeAttention) at T = 16 on the same context: a per-node reference (`tree16_us` is per call)
`tree64` is asserted against `sdpa` to 2e-2 before they are timed.  Per point: median us per call and spread per contender,
`prefill_over_tree64`, `sdpa_over_tree64`, `tree16_per_node_over_tree64` (us per node of tree16 over us per node of tree64), and
`not_faster`: the contenders whose time minus their own spread does not exceed tree64's.
"""
import argparse, json, os, statistics, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, BLOCK = 128, 16
ap = argparse.ArgumentParser()
ap.add_argument("--heads", default="32/32,32/8")
ap.add_argument("--seqs", default="1,4")
ap.add_argument("--q-lens", default="8,16")
ap.add_argument("--contexts", default="128,1024,4096")
ap.add_argument("--caches", default="16,fp8")
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--limit", type=int, default=240)
ap.add_argument("--nodes", default=None, help="node counts of the wide trees (up to 64): measure sqllm_attn_tree64_* instead")
ap.add_argument("--dtypes", default="fp16,bf16", help="with --nodes")
ap.add_argument("--dtype", default="fp16", help="with --nodes and --group: this child's type")
ap.add_argument("--group", default=None, help="heads,seqs,cache: measure this group in this process")
args = ap.parse_args()

if args.group is None:  # the driver: a fresh child per group, each under its own time limit; trouble ends the run
    for dtype in (args.dtypes.split(",") if args.nodes else ["fp16"]):
      for heads in args.heads.split(","):
        for seqs in args.seqs.split(","):
            for cache in args.caches.split(","):
                cmd = [sys.executable, os.path.abspath(__file__), "--group", f"{heads},{seqs},{cache}", "--q-lens", args.q_lens,
                       "--contexts", args.contexts, "--layers", str(args.layers), "--reps", str(args.reps)]
                if args.nodes:
                    cmd += ["--nodes", args.nodes, "--dtype", dtype]
                try:
                    rc = subprocess.run(cmd, timeout=args.limit).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
                if rc != 0:
                    print(json.dumps(dict(group=f"{heads},{seqs},{cache}", failed=rc)), flush=True)
                    sys.exit(rc)
    sys.exit(0)

import torch  # noqa: E402
from squeezellm_amd import quant  # noqa: E402

heads, seqs, cache = args.group.split(",")
HQ, H = map(int, heads.split("/"))
B, dt, fp8 = int(seqs), (torch.bfloat16 if args.nodes and args.dtype == "bf16" else torch.float16), cache == "fp8"
dev = torch.device("cuda:0")
S = (max(map(int, args.contexts.split(","))) + (64 if args.nodes else 16) + BLOCK - 1) // BLOCK * BLOCK
att = quant.DecodeAttention(HQ, H, D, block_size=BLOCK)
att.append_route = "kernel"


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


def tree_parents(name, T):
    return [-1 if t == 0 else (t - 1) // 4 if name == "wide" else max(t - 2, 0) for t in range(T)]


print(json.dumps(dict(tool="attn_tree_bench", torch=torch.__version__, heads=heads, seqs=B, dtype=args.dtype if args.nodes else "fp16", cache=cache, head_dim=D, S=S, block=BLOCK,
                      layers=args.layers, reps=args.reps)), flush=True)
perm = torch.randperm(B * S // BLOCK, device=dev)
table = perm.reshape(B, S // BLOCK).to(torch.int32)
caches, wide, scales = [], [], []
for _ in range(args.layers):
    kv = [torch.randn((B * S, H, D), device=dev).to(dt) for _ in "kv"]
    if not args.nodes: wide.append(tuple(t.float() for t in kv))
    sc = (None, None)
    if fp8:
        sc = tuple(float(quant.fp8_kv_scale(t.float().abs().max())) for t in kv)
        kv = [(t.float() / s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn) for t, s in zip(kv, sc)]
        if not args.nodes: wide[-1] = tuple(t.float() * s for t, s in zip(kv, sc))
    caches.append(tuple(kv))
    scales.append(sc)
celem = 1 if fp8 else 2
if args.nodes:  # the wide trees: sqllm_attn_tree64_* behind PrefillAttention
    pre = quant.PrefillAttention(HQ, H, D, block_size=BLOCK)
    slots_of = (table.long()[:, :, None] * BLOCK + torch.arange(BLOCK, device=dev)).reshape(B, S)  # [B, S]: the slot of key p
    T16 = 16
    mask16 = quant.tree_masks(torch.tensor([tree_parents("wide", T16)] * B, device=dev))[0]
    q16 = [torch.randn((B * T16, HQ * D), device=dev).to(dt) for _ in range(args.layers)]
    for T in map(int, args.nodes.split(",")):
        qs = [torch.randn((B * T, HQ * D), device=dev).to(dt) for _ in range(args.layers)]
        for name in ("wide", "deep"):
            mask = quant.tree_masks(torch.tensor([tree_parents(name, T)] * B, device=dev), wide=True)[0]
            bits = ((mask[:, :, None] >> torch.arange(T, device=dev)) & 1).bool()  # [B, T, T]
            for ctx in map(int, args.contexts.split(",")):
                L = ctx + T
                seq = torch.full((B,), L, dtype=torch.int32, device=dev)
                seq16 = torch.full((B,), ctx + T16, dtype=torch.int32, device=dev)
                allow = torch.cat([torch.ones((B, T, ctx), dtype=torch.bool, device=dev), bits], dim=2)[:, None]  # [B, 1, T, L]
                rec = dict(dtype=args.dtype, heads=heads, seqs=B, cache=cache, tree=name, nodes=T, context=ctx, kv_bytes_once=B * H * L * D * 2 * celem)
                keep = []

                def run(words=None):
                    keep.clear()
                    with torch.no_grad():
                        for q, (k, v), (ks, vs) in zip(qs, caches, scales):
                            keep.append(pre(q, k, v, table, seq, T, k_scale=ks, v_scale=vs, tree_mask=words))

                def run_tree16():
                    keep.clear()
                    with torch.no_grad():
                        for q, (k, v), (ks, vs) in zip(q16, caches, scales):
                            keep.append(att(q, k, v, table, seq16, k_scale=ks, v_scale=vs, q_len=T16, tree_mask=mask16))

                def run_sdpa():
                    keep.clear()
                    with torch.no_grad():
                        for q, (k, v), (ks, vs) in zip(qs, caches, scales):
                            if fp8:  # (through the bytes: torch has no indexing for float8)
                                kk, vv = ((c.view(torch.uint8)[slots_of[:, :L]].view(torch.float8_e4m3fn).to(dt) * s_).to(dt) for c, s_ in ((k, ks), (v, vs)))
                            else:
                                kk, vv = (c[slots_of[:, :L]] for c in (k, v))  # [B, L, H, D], gathered from the pages
                            kk, vv = (t.permute(0, 2, 1, 3).repeat_interleave(HQ // H, dim=1) for t in (kk, vv))
                            y = torch.nn.functional.scaled_dot_product_attention(q.view(B, T, HQ, D).transpose(1, 2), kk, vv, attn_mask=allow)
                            keep.append(y.transpose(1, 2).reshape(B * T, HQ * D))

                run_sdpa(); ref = keep[0].float().clone()
                run(mask); assert pre.last_route == "attn_tree64"
                torch.cuda.synchronize()
                assert bool(torch.isfinite(keep[0]).all()) and float((keep[0].float() - ref).abs().max()) < 2e-2
                run(); assert pre.last_route == "attn_prefill"
                run_tree16(); assert att.last_route == "attn_tree"
                runs = {"tree64": lambda: run(mask), "prefill": run, "sdpa": run_sdpa, "tree16": run_tree16}
                gs = {k: capture(f) for k, f in runs.items()}
                for g in gs.values(): timed(g.replay, 3, 2)
                ms = {k: [] for k in gs}
                order = list(runs)
                for r in range(args.reps):
                    for k in order[r % 4:] + order[:r % 4]: ms[k].append(timed(gs[k].replay))
                us = {k: statistics.median(v) * 1e3 / args.layers for k, v in ms.items()}
                spread = {k: (max(v) - min(v)) * 1e3 / args.layers for k, v in ms.items()}
                for k in order:
                    rec[f"{k}_us"] = round(us[k], 2)
                    rec[f"{k}_spread_us"] = round(spread[k], 2)
                rec["prefill_over_tree64"] = round(us["prefill"] / us["tree64"], 3)
                rec["sdpa_over_tree64"] = round(us["sdpa"] / us["tree64"], 3)
                rec["tree16_per_node_over_tree64"] = round((us["tree16"] / T16) / (us["tree64"] / T), 3)
                per = dict(us, tree16=us["tree16"] / T16 * T)  # (tree16: scaled to T nodes)
                rec["not_faster"] = [k for k in order[1:] if per[k] - spread[k] <= us["tree64"]]
                del gs; keep.clear()
                print(json.dumps(rec), flush=True)
        del qs
    sys.exit(0)
for T in map(int, args.q_lens.split(",")):
    if B * T > 64:
        continue
    qs = [torch.randn((B * T, HQ * D), device=dev).to(dt) for _ in range(args.layers)]
    for name in ("wide", "deep"):
        par = tree_parents(name, T)
        mask = quant.tree_masks(torch.tensor([par] * B, device=dev))[0]
        chain_words = torch.tensor([[(2 << t) - 1 for t in range(T)]] * B, dtype=torch.int32, device=dev)
        leaves = [t for t in range(T) if t not in par]
        paths = []
        for leaf in leaves:
            p = [leaf]
            while par[p[0]] >= 0: p.insert(0, par[p[0]])
            paths.append(p)
        rows = [torch.tensor([b * T + t for b in range(B) for t in p], device=dev) for p in paths]
        path_qs = [[q[r].contiguous() for r in rows] for q in qs]
        for ctx in map(int, args.contexts.split(",")):
            seq = torch.full((B,), ctx + T, dtype=torch.int32, device=dev)
            path_seq = [torch.full((B,), ctx + len(p), dtype=torch.int32, device=dev) for p in paths]
            nbytes = B * H * (ctx + T) * D * 2 * celem
            rec = dict(heads=heads, seqs=B, cache=cache, tree=name, q_len=T, context=ctx, leaves=len(paths), kv_bytes_once=nbytes)
            keep = []

            def run(words=None):
                keep.clear()
                with torch.no_grad():
                    for q, (k, v), (ks, vs) in zip(qs, caches, scales):
                        keep.append(att(q, k, v, table, seq, k_scale=ks, v_scale=vs, q_len=T, tree_mask=words))

            def run_paths():
                keep.clear()
                with torch.no_grad():
                    for pq, (k, v), (ks, vs) in zip(path_qs, caches, scales):
                        for q, p, s in zip(pq, paths, path_seq): keep.append(att(q, k, v, table, s, k_scale=ks, v_scale=vs, q_len=len(p)))

            def run_fallback():  # fp32 operands are not the kernels': the module's torch path
                with torch.no_grad():
                    return att(qs[0].float(), *wide[0], table, seq, q_len=T, tree_mask=mask)

            run(); ref = [t.clone() for t in keep]; assert att.last_route == "attn_append"
            run(chain_words); assert att.last_route == "attn_tree"
            torch.cuda.synchronize()
            assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(keep, ref)) and bool(torch.isfinite(ref[0]).all())
            run(mask)
            slow = run_fallback(); assert att.last_route == "fallback"
            assert float((keep[0].float() - slow).abs().max()) < 2e-2
            runs = {"tree": lambda: run(mask), "chain": run, "paths": run_paths}
            gs = {k: capture(f) for k, f in runs.items()}
            for g in gs.values(): timed(g.replay, 3, 2)
            ms = {k: [] for k in gs}
            order = list(runs)
            for r in range(args.reps):
                for k in order[r % 3:] + order[:r % 3]: ms[k].append(timed(gs[k].replay))
            us = {k: statistics.median(v) * 1e3 / args.layers for k, v in ms.items()}
            spread = {k: (max(v) - min(v)) * 1e3 / args.layers for k, v in ms.items()}
            for k in order:
                rec[f"{k}_us"] = round(us[k], 2)
                rec[f"{k}_spread_us"] = round(spread[k], 2)
            rec["fallback_us"] = round(statistics.median(timed(run_fallback, 1, 0) for _ in range(5)) * 1e3, 1)
            rec["over_chain"] = round(us["tree"] / us["chain"], 3)
            rec["above_chain_spread"] = bool(us["tree"] - us["chain"] > spread["chain"])
            rec["paths_over_tree"] = round(us["paths"] / us["tree"], 3)
            rec["tree_wins_paths"] = bool(us["paths"] - us["tree"] > spread["paths"])
            del gs; keep.clear()
            print(json.dumps(rec), flush=True)
    del qs
