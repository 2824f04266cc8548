"""Prefill attention over the paged KV cache: quant.PrefillAttention (one kernel node on the matrix cores) against what the library
offered before it and against torch, graph-replayed ALTERNATELY in one process, timed by device events around the replays.

    python tools/attn_prefill_bench.py [--heads 32/32,32/8] [--seqs 1,4] [--q-lens 128,512,2048] [--ctx 0,2048]
                                       [--dtypes fp16,bf16] [--reps 7] [--replays 50] > profiles/attn_prefill_bench.txt

Workload per point: `seqs` sequences of T new tokens behind `ctx` prior keys each, head_dim 128, a paged cache of blocks of 16 with
a shuffled table, the new tokens' keys already written (what the attention front leaves).  The contenders:
  prefill      one PrefillAttention call
  loop16       (a) what the library offered before: a loop of T / 16 DecodeAttention(q_len=16) calls over the same cache, chunk c
               with seq_lens = ctx + 16 (c + 1) -- K and V re-read once per 16 tokens, two kernel nodes per chunk
  sdpa         (b) torch scaled_dot_product_attention with the bottom-right causal mask on K / V gathered from the pages to
               contiguous [B, HQ, n, D] tensors (grouped heads expanded), timed WITH the gather and WITHOUT it (sdpa_only)
With --cache fp8 (> profiles/attn_prefill_fp8_bench.txt) the same points compare the two prefill kernels of this library:
  prefill_fp8  one PrefillAttention call over the cache quantised to e4m3fn bytes with k_scale = v_scale = 2^-6
  prefill16    one PrefillAttention call over the DEQUANTISED cache in q's type (exact for a power-of-two scale: the same values)
  fallback     what an fp8 cache took before the kernel: the torch route (append_as_decode_rows and the fallback of DecodeAttention),
               eager, on the smallest points only (the fewest tokens, keys and sequences: it gathers [rows, keys, H, D] in fp32)
prefill_fp8 is checked against prefill16 (at most 2^-6) before anything is timed.
With --window W (> profiles/attn_prefill_window_bench.txt; with either --cache) the points compare, on the same operands:
  window       one PrefillAttention(window=W) call: token t attends the last W keys below its length
  full         the prefill kernel WITHOUT a window: beyond W keys it computes another function -- the time yardstick only
  sdpa         torch scaled_dot_product_attention with a BAND mask on K / V gathered from the pages (an fp8 cache: dequantised in the
               gather), timed with the gather; only where seqs * T * (ctx + T) <= --sdpa-cap (the mask and the scores are dense: the
               larger points would take most of a run), otherwise NOT MEASURED (null)
window is checked against sdpa where that runs (at most 2^-6), and against full on the rows with L <= W (equal bits).  A contender
whose single replay takes long is replayed fewer times per round (at least 3; "replays" in the record); `tiles_ratio` is the
windowed walk's share of the full one by the tile count, min(1, (W + 64 / group) / (ctx + T / 2)).
prefill is checked against loop16 (largest absolute difference printed, at most 2^-6) before anything is timed.  Each contender
is captured once after an eager warm-up; --reps rounds, each replaying every contender --replays times between two events, in
turn.  One JSON line per point: median us and spread (max - min over the rounds) per contender, the causal-trimmed operation count
from the shapes -- 4 * head_dim * (T * ctx + T (T + 1) / 2) per (sequence, query head) -- and prefill's FLOP/s over it.
Needs a GPU: there is no CPU timing."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, BLOCK = 128, 16
ap = argparse.ArgumentParser()
ap.add_argument("--heads", default="32/32,32/8")
ap.add_argument("--seqs", default="1,4")
ap.add_argument("--q-lens", default="128,512,2048")
ap.add_argument("--ctx", default="0,2048")
ap.add_argument("--dtypes", default="fp16,bf16")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--replays", type=int, default=50)
ap.add_argument("--cache", default="16bit", choices=("16bit", "fp8"))
ap.add_argument("--window", type=int, default=None)
ap.add_argument("--sdpa-cap", type=float, default=4 * 2048 * 6144.0)
ap.add_argument("--round-us", type=float, default=60000.0, help="--window: the time one contender may take per round")
args = ap.parse_args()

import torch  # noqa: E402
if not torch.cuda.is_available():
    sys.exit("attn_prefill_bench: no GPU is visible; there is nothing to measure on a CPU")
from squeezellm_amd import quant  # noqa: E402

dev = torch.device("cuda:0")


def capture(fn):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side): fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr): fn()
    return gr


def replay_us(gr, n):
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(n): gr.replay()
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) * 1e3 / n


def fp8_point(rec, q, k_cache, v_cache, table, seq, T, HQ, H, smallest):
    """the --cache fp8 contenders of one point -> rec"""
    S = 2.0 ** -6  # randn reaches about +-4.5: 288 in units of the scale, inside +-448
    k8, v8 = (quant._fp8_bytes(c.float(), S).view(torch.float8_e4m3fn) for c in (k_cache, v_cache))
    k16, v16 = ((c.float() * S).to(q.dtype) for c in (k8, v8))
    att8, att16 = (quant.PrefillAttention(HQ, H, D, block_size=BLOCK) for _ in range(2))
    out_8, out_16 = torch.empty_like(q), torch.empty_like(q)
    runs = {"prefill_fp8": lambda: att8(q, k8, v8, table, seq, T, out=out_8, k_scale=S, v_scale=S),
            "prefill16": lambda: att16(q, k16, v16, table, seq, T, out=out_16)}
    for run in runs.values(): run()
    assert att8.last_route == "attn_prefill" and att16.last_route == "attn_prefill"
    rec["max_abs_diff_vs_prefill16"] = diff = float((out_8.float() - out_16.float()).abs().max())
    assert diff <= 2.0 ** -6, diff
    graphs = {name: capture(run) for name, run in runs.items()}
    for gr in graphs.values(): replay_us(gr, 2)  # warm-up of the replays themselves
    times = {name: [] for name in graphs}
    for _ in range(args.reps):
        for name, gr in graphs.items():  # alternately
            times[name].append(replay_us(gr, args.replays))
    if smallest:  # today's route for an fp8 cache, eager (it synchronises), after one warm-up call
        def fallback():
            tb, ln = quant.append_as_decode_rows(table, seq, T, None, BLOCK)
            return quant._torch_attn_decode(q, k8, v8, tb, ln, BLOCK, HQ, H, D, D ** -0.5, q.dtype, S, S)
        assert float((fallback().float() - out_8.float()).abs().max()) <= 2.0 ** -6
        times["fallback"] = []
        for _ in range(3):
            beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            beg.record(); fallback(); end.record(); end.synchronize()
            times["fallback"].append(beg.elapsed_time(end) * 1e3)
    for name, ts in times.items():
        rec[name + "_us"], rec[name + "_spread_us"] = round(statistics.median(ts), 1), round(max(ts) - min(ts), 1)
    rec["prefill_fp8_tflops"] = round(rec["flops"] / (rec["prefill_fp8_us"] * 1e-6) / 1e12, 2)
    rec["fp8_over_16bit"] = round(rec["prefill_fp8_us"] / rec["prefill16_us"], 3)
    rec["prefill_fp8_faster_than"] = [name for name in times if name != "prefill_fp8" and rec["prefill_fp8_us"] < rec[name + "_us"]]


def window_point(rec, q, k_cache, v_cache, table, seq, T, HQ, H, ctx, Wn):
    """the --window contenders of one point -> rec"""
    B, G, n, S = seq.numel(), HQ // H, ctx + T, 2.0 ** -6
    kw = {}
    if args.cache == "fp8":
        k_cache, v_cache = (quant._fp8_bytes(c.float(), S).view(torch.float8_e4m3fn) for c in (k_cache, v_cache))
        kw = dict(k_scale=S, v_scale=S)
    att_w, att_f = quant.PrefillAttention(HQ, H, D, block_size=BLOCK, window=Wn), quant.PrefillAttention(HQ, H, D, block_size=BLOCK)
    out_w, out_f = torch.empty_like(q), torch.empty_like(q)
    runs = {"window": lambda: att_w(q, k_cache, v_cache, table, seq, T, out=out_w, **kw),
            "full": lambda: att_f(q, k_cache, v_cache, table, seq, T, out=out_f, **kw)}
    for run in runs.values(): run()
    assert att_w.last_route == "attn_prefill_window" and att_f.last_route == "attn_prefill"
    inside = max(0, min(T, Wn - ctx))  # the tokens with L <= W: the first `inside` of every sequence
    if inside:
        assert torch.equal(out_w.view(B, T, -1)[:, :inside].view(torch.int16), out_f.view(B, T, -1)[:, :inside].view(torch.int16))
    if B * T * n <= args.sdpa_cap:
        slot = (table.long()[:, :, None] * BLOCK + torch.arange(BLOCK, device=dev)[None, None, :]).reshape(B, -1)[:, :n]
        mask = torch.ones((T, n), dtype=torch.bool, device=dev).tril(diagonal=ctx).triu(diagonal=ctx - Wn + 1)
        q4 = q.view(B, T, HQ, D).transpose(1, 2)

        def run_sdpa():
            k, v = (((c.view(torch.float8_e4m3fn)[slot].float() * S).to(q.dtype) if kw else c[slot]).permute(0, 2, 1, 3) for c in (k_cache, v_cache))
            if G > 1: k, v = k.repeat_interleave(G, dim=1), v.repeat_interleave(G, dim=1)
            return torch.nn.functional.scaled_dot_product_attention(q4, k, v, attn_mask=mask)
        rec["max_abs_diff_vs_sdpa"] = diff = float((run_sdpa().transpose(1, 2).reshape(B * T, -1).float() - out_w.float()).abs().max())
        assert diff <= 2.0 ** -6, diff
        runs["sdpa"] = run_sdpa
    graphs = {name: capture(run) for name, run in runs.items()}
    replays = {name: int(max(3, min(args.replays, args.round_us / max(replay_us(gr, 2), 1.0)))) for name, gr in graphs.items()}  # (and the warm-up)
    times = {name: [] for name in graphs}
    for _ in range(args.reps):
        for name, gr in graphs.items():  # alternately
            times[name].append(replay_us(gr, replays[name]))
    rec["replays"] = replays
    for name in ("window", "full", "sdpa"):
        ts = times.get(name)
        rec[name + "_us"], rec[name + "_spread_us"] = (round(statistics.median(ts), 1), round(max(ts) - min(ts), 1)) if ts else (None, None)
    rec["tiles_ratio"] = round(min(1.0, (Wn + 64.0 / G) / (ctx + T / 2.0)), 3)
    rec["window_over_full"] = round(rec["window_us"] / rec["full_us"], 3)
    rec["window_faster_than"] = [name for name in ("full", "sdpa") if rec[name + "_us"] is not None and rec["window_us"] < rec[name + "_us"]]


print(json.dumps(dict(tool="attn_prefill_bench", cache=args.cache, window=args.window, torch=torch.__version__, device=torch.cuda.get_device_name(0), head_dim=D, block=BLOCK,
                      reps=args.reps, replays=args.replays)), flush=True)
for heads in args.heads.split(","):
    HQ, H = map(int, heads.split("/"))
    G = HQ // H
    for B in map(int, args.seqs.split(",")):
        for dname in args.dtypes.split(","):
            dt = {"fp16": torch.float16, "bf16": torch.bfloat16}[dname]
            for ctx in map(int, args.ctx.split(",")):
                for T in map(int, args.q_lens.split(",")):
                    n = ctx + T
                    n_blocks = (n + BLOCK - 1) // BLOCK
                    torch.manual_seed(T + ctx)
                    table = torch.randperm(B * n_blocks, device=dev).reshape(B, n_blocks).to(torch.int32)
                    k_cache, v_cache = (torch.randn((B * n_blocks * BLOCK, H, D), device=dev).to(dt) for _ in "kv")
                    q = torch.randn((B * T, HQ * D), device=dev).to(dt)
                    seq = torch.full((B,), n, dtype=torch.int32, device=dev)
                    if args.window is not None:
                        rec = dict(heads=heads, seqs=B, dtype=dname, ctx=ctx, T=T, window=args.window)
                        window_point(rec, q, k_cache, v_cache, table, seq, T, HQ, H, ctx, args.window)
                        print(json.dumps(rec), flush=True)
                        del k_cache, v_cache
                        continue
                    if args.cache == "fp8":
                        rec = dict(heads=heads, seqs=B, dtype=dname, ctx=ctx, T=T, flops=4.0 * D * (T * ctx + T * (T + 1) / 2) * B * HQ)
                        fp8_point(rec, q, k_cache, v_cache, table, seq, T, HQ, H,
                                  (T, ctx, B) == tuple(min(map(int, getattr(args, a).split(","))) for a in ("q_lens", "ctx", "seqs")))
                        print(json.dumps(rec), flush=True)
                        del k_cache, v_cache
                        continue
                    pre, dec = quant.PrefillAttention(HQ, H, D, block_size=BLOCK), quant.DecodeAttention(HQ, H, D, block_size=BLOCK)
                    dec.append_route = "kernel"
                    out_p, out_l = torch.empty_like(q), torch.empty_like(q)
                    # loop16: chunk c holds rows [16 c, 16 c + 16) of every sequence, gathered to [B * 16, W] outside the timed region
                    chunks = T // 16
                    q_c = [q.view(B, T, -1)[:, 16 * c:16 * c + 16].reshape(B * 16, -1).contiguous() for c in range(chunks)]
                    seq_c = [torch.full((B,), ctx + 16 * (c + 1), dtype=torch.int32, device=dev) for c in range(chunks)]
                    out_c = out_l.view(B, T, -1)
                    tmp = [torch.empty_like(q_c[0]) for _ in range(chunks)]

                    def run_prefill():
                        pre(q, k_cache, v_cache, table, seq, T, out=out_p)

                    def run_loop16():
                        for c in range(chunks):
                            dec(q_c[c], k_cache, v_cache, table, seq_c[c], out=tmp[c], q_len=16)

                    slot = (table.long()[:, :, None] * BLOCK + torch.arange(BLOCK, device=dev)[None, None, :]).reshape(B, -1)[:, :n]
                    mask = torch.ones((T, n), dtype=torch.bool, device=dev).tril(diagonal=ctx)
                    q4 = q.view(B, T, HQ, D).transpose(1, 2)
                    kv = {}

                    def gather():
                        for name, cache in (("k", k_cache), ("v", v_cache)):
                            kv[name] = cache[slot].permute(0, 2, 1, 3).repeat_interleave(G, dim=1) if G > 1 else cache[slot].permute(0, 2, 1, 3).contiguous()

                    def run_sdpa_only():
                        return torch.nn.functional.scaled_dot_product_attention(q4, kv["k"], kv["v"], attn_mask=mask)

                    def run_sdpa():
                        gather()
                        return run_sdpa_only()

                    run_prefill(); run_loop16(); gather()
                    assert pre.last_route == "attn_prefill" and dec.last_route == "attn_append"
                    for c in range(chunks):
                        out_c[:, 16 * c:16 * c + 16] = tmp[c].view(B, 16, -1)
                    diff = float((out_p.float() - out_l.float()).abs().max())
                    assert diff <= 2.0 ** -6, diff
                    graphs = {"prefill": capture(run_prefill), "loop16": capture(run_loop16), "sdpa": capture(run_sdpa), "sdpa_only": capture(run_sdpa_only)}
                    for gr in graphs.values(): replay_us(gr, 2)  # warm-up of the replays themselves
                    times = {name: [] for name in graphs}
                    for _ in range(args.reps):
                        for name, gr in graphs.items():  # alternately
                            times[name].append(replay_us(gr, args.replays))
                    flops = 4.0 * D * (T * ctx + T * (T + 1) / 2) * B * HQ
                    rec = dict(heads=heads, seqs=B, dtype=dname, ctx=ctx, T=T, max_abs_diff_vs_loop16=diff, flops=flops)
                    for name, ts in times.items():
                        rec[name + "_us"], rec[name + "_spread_us"] = round(statistics.median(ts), 1), round(max(ts) - min(ts), 1)
                    rec["prefill_tflops"] = round(flops / (rec["prefill_us"] * 1e-6) / 1e12, 2)
                    rec["prefill_faster_than"] = [name for name in ("loop16", "sdpa", "sdpa_only") if rec["prefill_us"] < rec[name + "_us"]]
                    print(json.dumps(rec), flush=True)
                    del graphs, k_cache, v_cache, kv
