"""Decode attention for several new tokens per sequence: quant.DecodeAttention(..., q_len=T) on the append kernels against the
EMULATION on the unchanged one-query entries -- batch * T rows, every sequence's table row repeated T times, per-token lengths
(quant.append_as_decode_rows) -- graph-replayed alternately in ONE process per group (built like attn_decode_bench.py).

    python tools/attn_append_bench.py [--heads 32/32,32/8] [--seqs 1,4] [--q-lens 2,4,8,16] [--lens 128,1024,4096]
                                      [--dtypes fp16,bf16] [--caches 16,fp8] [--layers 4] [--reps 3] [--limit 240]

The driver starts one fresh child process per (heads, sequences, dtype, cache type) under its own time limit (--limit seconds) and
stops at the first child that fails or runs out of time; a child (--group) measures its T x keys x layout points.

Workload per point: --layers attention layers with distinct caches and queries, head_dim 128, `seqs` sequences of n keys each
(their T new tokens included) in a cache of S = 4096, as a head-major static cache and as a paged cache with a shuffled table.
  emul    one DecodeAttention call of seqs * T rows over the expanded table and lengths: correct, K and V read T times
  append  one DecodeAttention call with q_len = T: K and V read once per sequence
  route_emul  the module's own "emulate" route, called as `append` is (q_len = T): `emul` plus the expansion of the table and
          the lengths, redone on the device in every call and captured with it -- what a caller of that route pays end to end.
          `emul` is the yardstick of the kernels; `route_emul` against `append` is what DecodeAttention's routing rests on.
All are asserted bit-identical before they are timed.  Each way is captured once after an eager warm-up; the graphs are replayed
alternately, --reps repetitions of 20 replays each.  One JSON line per point: median us per call (per layer) and spread
(max - min over the repetitions) per way and layout; the sequence's K + V bytes counted ONCE; the per-launch fit of DESIGN.md 5,
2 x 3 us + bytes / 4.8 TB/s, and both ways over it; `append_wins`: emul - append > the emulation's own spread.
"""
import argparse, json, os, statistics, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, S, BLOCK = 128, 4096, 16
ap = argparse.ArgumentParser()
ap.add_argument("--heads", default="32/32,32/8")
ap.add_argument("--seqs", default="1,4")
ap.add_argument("--q-lens", default="2,4,8,16")
ap.add_argument("--lens", default="128,1024,4096")
ap.add_argument("--dtypes", default="fp16,bf16")
ap.add_argument("--caches", default="16,fp8")
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--limit", type=int, default=240)
ap.add_argument("--group", default=None, help="heads,seqs,dtype,cache: measure this group in this process")
args = ap.parse_args()

if args.group is None:  # the driver: a fresh child per group, each under its own time limit; trouble ends the run
    for heads in args.heads.split(","):
        for seqs in args.seqs.split(","):
            for dname in args.dtypes.split(","):
                for cache in args.caches.split(","):
                    cmd = [sys.executable, os.path.abspath(__file__), "--group", f"{heads},{seqs},{dname},{cache}", "--q-lens", args.q_lens,
                           "--lens", args.lens, "--layers", str(args.layers), "--reps", str(args.reps)]
                    try:
                        rc = subprocess.run(cmd, timeout=args.limit).returncode
                    except subprocess.TimeoutExpired:
                        rc = 124
                    if rc != 0:
                        print(json.dumps(dict(group=f"{heads},{seqs},{dname},{cache}", failed=rc)), flush=True)
                        sys.exit(rc)
    sys.exit(0)

import torch  # noqa: E402
from squeezellm_amd import quant  # noqa: E402

heads, seqs, dname, cache = args.group.split(",")
HQ, H = map(int, heads.split("/"))
B, dt, fp8 = int(seqs), {"fp16": torch.float16, "bf16": torch.bfloat16}[dname], cache == "fp8"
dev = torch.device("cuda:0")
att = quant.DecodeAttention(HQ, H, D)
att.append_route = "kernel"  # the kernels themselves, not what DecodeAttention's measured routing would pick
att_em = quant.DecodeAttention(HQ, H, D)
att_em.append_route = "emulate"


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


print(json.dumps(dict(tool="attn_append_bench", torch=torch.__version__, heads=heads, seqs=B, dtype=dname, cache=cache, head_dim=D, S=S, block=BLOCK,
                      layers=args.layers, reps=args.reps)), flush=True)
statics = [tuple(torch.randn((B, H, S, D), device=dev).to(dt) for _ in "kv") for _ in range(args.layers)]
perm = torch.randperm(B * S // BLOCK, device=dev)
ptable = perm.reshape(B, S // BLOCK).to(torch.int32)
stable = quant.static_cache_blocks(B, H, dev)
scales = [(None, None)] * args.layers
if fp8:
    scales = [tuple(float(quant.fp8_kv_scale(t.float().abs().max())) for t in pair) for pair in statics]
    statics = [tuple((t.float() / s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn) for t, s in zip(pair, sc)) for pair, sc in zip(statics, scales)]
pageds = []
for pair in statics:
    out = []
    for t in pair:
        blocks = t.view(torch.uint8 if fp8 else dt).permute(0, 2, 1, 3).reshape(B * S // BLOCK, BLOCK, H, D)
        p = torch.empty_like(blocks)
        p[perm] = blocks
        out.append(quant.kv_cache_view(p.view(t.dtype), "nhd"))
    pageds.append(tuple(out))
views = [tuple(quant.kv_cache_view(t, "bhsd") for t in pair) for pair in statics]
layouts = {"static": (views, stable, S), "paged": (pageds, ptable, BLOCK)}
celem = 1 if fp8 else 2
for T in map(int, args.q_lens.split(",")):
    if B * T > 64:
        continue
    qs = [torch.randn((B * T, HQ * D), device=dev).to(dt) for _ in range(args.layers)]
    for n in map(int, args.lens.split(",")):
        seq = torch.full((B,), n, dtype=torch.int32, device=dev)
        rec = dict(heads=heads, seqs=B, q_len=T, dtype=dname, cache=cache, seq_len=n)
        nbytes = B * H * n * D * 2 * celem
        rec.update(kv_bytes_once=nbytes, fit_us=round(2 * 3 + nbytes / 4.8e6, 2))
        for name, (caches, table, bs) in layouts.items():
            table_x, lens_x = quant.append_as_decode_rows(table, seq, T, None, bs)
            table_x = table_x.contiguous()
            keep = []

            def run_emul():
                keep.clear()
                with torch.no_grad():
                    for q, (k, v), (ks, vs) in zip(qs, caches, scales): keep.append(att(q, k, v, table_x, lens_x, block_size=bs, k_scale=ks, v_scale=vs))

            def run_append():
                keep.clear()
                with torch.no_grad():
                    for q, (k, v), (ks, vs) in zip(qs, caches, scales): keep.append(att(q, k, v, table, seq, block_size=bs, k_scale=ks, v_scale=vs, q_len=T))

            def run_route():  # what the module's "emulate" route costs a caller: the expansion redone in every call, inside the graph
                keep.clear()
                with torch.no_grad():
                    for q, (k, v), (ks, vs) in zip(qs, caches, scales): keep.append(att_em(q, k, v, table, seq, block_size=bs, k_scale=ks, v_scale=vs, q_len=T))

            run_emul(); ref = [t.clone() for t in keep]; assert att.last_route == "attn_decode"
            run_route(); assert att_em.last_route == "attn_decode"
            torch.cuda.synchronize()
            assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(keep, ref))
            run_append(); assert att.last_route == "attn_append"
            torch.cuda.synchronize()
            assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(keep, ref)) and bool(torch.isfinite(ref[0]).all())
            runs = {"emul": run_emul, "append": run_append, "route_emul": run_route}
            gs = {k: capture(f) for k, f in runs.items()}
            for g in gs.values(): timed(g.replay, 3, 2)
            ms = {k: [] for k in gs}
            order = list(runs)
            for r in range(args.reps):
                for k in order[r % 3:] + order[:r % 3]: ms[k].append(timed(gs[k].replay))
            us = {k: statistics.median(v) * 1e3 / args.layers for k, v in ms.items()}
            spread = {k: (max(v) - min(v)) * 1e3 / args.layers for k, v in ms.items()}
            for k in order:
                rec[f"{name}_{k}_us"] = round(us[k], 2)
                rec[f"{name}_{k}_spread_us"] = round(spread[k], 2)
                rec[f"{name}_{k}_over_fit"] = round(us[k] / rec["fit_us"], 2)
            rec[f"{name}_emul_over_append"] = round(us["emul"] / us["append"], 3)
            rec[f"{name}_append_wins"] = bool(us["emul"] - us["append"] > spread["emul"])
            rec[f"{name}_route_emul_over_append"] = round(us["route_emul"] / us["append"], 3)
            del gs; keep.clear()
        print(json.dumps(rec), flush=True)
    del qs
