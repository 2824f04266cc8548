"""Fused linear vs bare operator, whole 7B model (batch 1, graph replay), by term: dense only, + CSR, + top-X rows.

    python tools/linear_overhead.py [--dtype {fp16,bf16}]
    python tools/linear_overhead.py --alternate R [--drop-in]   # fp16 and bf16 in ONE process, R alternating repetitions

--dtype: the 16-bit type of the fused linear's two ends (default fp16: sqllm_linear_f16; bf16: sqllm_linear_bf16).
--alternate R: per sparse term, both passes are captured over the same layers and replayed alternately, R repetitions of
30 replays each; every repetition is printed, then the medians and the spread (max - min) of each type.
--drop-in (with --alternate): also the bf16 forward a caller gets WITHOUT the fused class -- QuantLinearLUT.forward on
bf16 input, four launches per linear (zeros / x.float() / operator / cast) -- eager and graph-replayed, on the first 8
decoder layers scaled to the model (as bench.py's `drop_in` does for fp16), beside the fused class on the same layers.
"""
import argparse, sys, os, json, time, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from squeezellm_amd import decode, synth
ap = argparse.ArgumentParser()
ap.add_argument("--dtype", choices=("fp16", "bf16"), default="fp16")
ap.add_argument("--alternate", type=int, default=0, metavar="R")
ap.add_argument("--drop-in", action="store_true")
args = ap.parse_args()
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
dev = torch.device("cuda:0")
def timed(fn, reps=30, warmup=3):
    for _ in range(warmup): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / reps * 1e3
def inputs(layers):
    """one fp32 vec per distinct input of a decoder layer (q/k/v share one, gate/up share one)"""
    xin = {}; xs = []
    for i, l in enumerate(layers):
        lname = l["name"].split(".")[-1]
        key = (i // 7, "h" if lname in ("q_proj", "k_proj", "v_proj") else "m" if lname in ("gate_proj", "up_proj") else lname)
        if key not in xin: xin[key] = torch.randn((l["K"],), device=dev)
        xs.append(xin[key])
    return xs
def linear_graph(layers, xs32, dtype):
    x16 = {id(x): x.to(dtype) for x in xs32}
    xs16 = [x16[id(x)] for x in xs32]
    ys16 = [torch.empty(l["N"], device=dev, dtype=dtype) for l in layers]
    seq = decode.OpSequence(layers, xs16, ys16, fuse_shared_input=True, linear=True, fold_topx=os.environ.get("FOLD_TOPX", "1") != "0")
    return seq.graph(), (seq, xs16, ys16)
def drop_in(layers, xs32, scale):
    """QuantLinearLUT.forward (four launches) and QuantLinearLUTFused.forward (one) on bf16 input, eager and replayed"""
    from squeezellm_amd import quant
    x16 = {id(x): x.to(torch.bfloat16).reshape(1, 1, -1) for x in xs32}
    xs16 = [x16[id(x)] for x in xs32]
    def capture(fn):
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side): fn()
        torch.cuda.current_stream(dev).wait_stream(side)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr): fn()
        return gr
    rec = {}
    for tag, cls in (("four_launch", quant.QuantLinearLUT), ("fused_class", quant.QuantLinearLUTFused)):
        mods = [cls.from_operands(l) for l in layers]
        def run():
            with torch.no_grad():
                for m, x in zip(mods, xs16): m(x)
        e = min(timed(run, 5, 2) for _ in range(3)) * scale
        g = capture(run)
        r = min(timed(g.replay, 20, 3) for _ in range(3)) * scale
        rec[tag] = dict(eager_ms=round(e, 4), eager_tokens_per_s=round(1e3 / e, 1), graph_ms=round(r, 4), graph_tokens_per_s=round(1e3 / r, 1))
        del g, mods
    return rec
for bits in (3, 4):
    for frac, topX in ((0.0, 0), (0.0045, 0), (0.0045, 10)):
        layers = synth.make_model("llama-7b", bits, sparse_frac=frac, topX=topX, n_layers=None, device=dev)
        xs32 = inputs(layers)
        if args.alternate:
            gs = {}; keep = []
            for name in ("fp16", "bf16"):
                gs[name], k = linear_graph(layers, xs32, DT[name]); keep.append(k)
            for g in gs.values(): timed(g.replay, 5, 3)
            ms = {"fp16": [], "bf16": []}
            for r in range(args.alternate):
                for name in ("fp16", "bf16") if r % 2 == 0 else ("bf16", "fp16"):
                    ms[name].append(timed(gs[name].replay))
                print(json.dumps(dict(bits=bits, sparse=frac, topX=topX, rep=r, fp16_ms=round(ms["fp16"][-1], 4), bf16_ms=round(ms["bf16"][-1], 4))), flush=True)
            med = {k: statistics.median(v) for k, v in ms.items()}
            rec = dict(bits=bits, sparse=frac, topX=topX, reps=args.alternate, fp16_median_ms=round(med["fp16"], 4), bf16_median_ms=round(med["bf16"], 4),
                       fp16_spread_ms=round(max(ms["fp16"]) - min(ms["fp16"]), 4), bf16_spread_ms=round(max(ms["bf16"]) - min(ms["bf16"]), 4),
                       bf16_over_fp16_pct=round((med["bf16"] / med["fp16"] - 1) * 100, 2))
            del gs, keep
            if args.drop_in:
                n_dec = 8
                rec["bf16_drop_in_first_8_layers_scaled"] = drop_in(layers[:n_dec * 7], xs32[:n_dec * 7], len(layers) / (n_dec * 7))
            print(json.dumps(rec), flush=True)
            del layers, xs32
            torch.cuda.empty_cache()
            continue
        g3, keep = linear_graph(layers, xs32, DT[args.dtype])
        ys32 = [torch.zeros(l["N"], device=dev) for l in layers]
        g4 = decode.OpSequence(layers, xs32, ys32, fuse_shared_input=True).graph()
        a = timed(g3.replay); b = timed(g4.replay); a2 = timed(g3.replay); b2 = timed(g4.replay)
        rec = dict(bits=bits, sparse=frac, topX=topX, linear_ms=round(min(a, a2), 4), op_ms=round(min(b, b2), 4), overhead_pct=round((min(a, a2) / min(b, b2) - 1) * 100, 1))
        if args.dtype != "fp16": rec = dict(dtype=args.dtype, **rec)
        print(json.dumps(rec), flush=True)
        del layers, g3, g4, keep, ys32, xs32
        torch.cuda.empty_cache()
