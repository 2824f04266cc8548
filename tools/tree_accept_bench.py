"""Closing a speculative-decoding step: quant.tree_accept and quant.compact_kv on their kernels (sqllm_tree_accept, sqllm_kv_compact)
against their torch forms (route="torch"), graph-replayed alternately in ONE process per group (built like attn_tree_bench.py).

    python tools/tree_accept_bench.py [--seqs 1,4,16] [--caches 16,fp8] [--nodes 16,64] [--layers 32] [--context 1024]
                                      [--reps 3] [--limit 300]

The driver starts one fresh child process per (cache type, sequences) under its own time limit (--limit seconds) and stops at the
first child that fails or runs out of time; a child (--group) measures its points.

Workload per point: --layers layers of 8 kv heads of 128, a k and a v cache each (2 x layers cache pointers in ONE compact_kv call),
`seqs` sequences of --context keys and T nodes in paged caches with a shuffled table.  Accepted paths of 1, 4 and 8 nodes that are
not their own prefix (path[j] = 2 j + 1: every row moves) and a prefix path of 4 (nothing moves).
  compact        compact_kv(route="kernel"): one kernel node for all caches
  compact_torch  compact_kv(route="torch"): the fixed-shape gather into a temporary and scatter, per cache -- what a caller has
                 without the kernel that a graph can hold (no host synchronisation)
  floor          the project's per-launch fit, 3 us + bytes moved x 2 / 4.8 TB/s (read and write)
  accept / accept_torch   tree_accept on a heap-shaped tree whose deepest path matches, kernel and torch form
Both torch forms are asserted equal to the kernels' results before anything is timed.  One JSON line per point: median us per step
(the whole model, not per layer) and spread (max - min over the repetitions) per contender, `torch_over_kernel`, and `not_faster`:
the kernels whose time plus their own spread is not below the torch form's.
"""
import argparse, json, os, statistics, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, D, BLOCK = 8, 128, 16
ap = argparse.ArgumentParser()
ap.add_argument("--seqs", default="1,4,16")
ap.add_argument("--caches", default="16,fp8")
ap.add_argument("--nodes", default="16,64")
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--context", type=int, default=1024)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--limit", type=int, default=300)
ap.add_argument("--group", default=None, help="cache,seqs: measure this group in this process")
args = ap.parse_args()

if args.group is None:  # the driver: a fresh child per group, each under its own time limit; trouble ends the run
    for cache in args.caches.split(","):
        for seqs in args.seqs.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--group", f"{cache},{seqs}", "--nodes", args.nodes, "--layers", str(args.layers),
                   "--context", str(args.context), "--reps", str(args.reps)]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                print(json.dumps(dict(group=f"{cache},{seqs}", failed=rc)), flush=True)
                sys.exit(rc)
    sys.exit(0)

import torch  # noqa: E402
from squeezellm_amd import quant  # noqa: E402

cache, seqs = args.group.split(",")
B, fp8 = int(seqs), cache == "fp8"
dev = torch.device("cuda:0")
S = (args.context + 64 + BLOCK - 1) // BLOCK * BLOCK


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


def contest(runs):
    """{name: (median us, spread us)} of the captured runs, replayed alternately"""
    gs = {k: capture(f) for k, f in runs.items()}
    for g in gs.values(): timed(g.replay, 3, 2)
    ms, order = {k: [] for k in gs}, list(runs)
    for r in range(args.reps):
        for k in order[r % len(order):] + order[:r % len(order)]: ms[k].append(timed(gs[k].replay))
    return {k: (statistics.median(v) * 1e3, (max(v) - min(v)) * 1e3) for k, v in ms.items()}


print(json.dumps(dict(tool="tree_accept_bench", torch=torch.__version__, cache=cache, seqs=B, kv_heads=H, head_dim=D, S=S, block=BLOCK,
                      layers=args.layers, context=args.context, reps=args.reps)), flush=True)
table = torch.randperm(B * S // BLOCK, device=dev).reshape(B, S // BLOCK).to(torch.int32)
raw = torch.uint8 if fp8 else torch.int16
bufs = [torch.randint(0, 120, (B * S, H, D), device=dev, dtype=torch.int32).to(raw) for _ in range(2 * args.layers)]
caches = [b.view(torch.float8_e4m3fn if fp8 else torch.float16) for b in bufs]
for T in map(int, args.nodes.split(",")):
    seq = torch.full((B,), args.context + T, dtype=torch.int32, device=dev)
    # acceptance: a heap whose deepest path matches
    par = [[(t - 1) // 2 if t else -1 for t in range(T)]] * B
    parents = torch.tensor(par, dtype=torch.int32, device=dev)
    mask = quant.tree_masks(parents, wide=True)[0]
    target = torch.arange(T, dtype=torch.int32, device=dev).repeat(B, 1) + 100
    draft = torch.zeros_like(target)
    t = T - 1
    while t > 0:
        draft[:, t] = 100 + par[0][t]
        t = par[0][t]
    res = {}
    runs = {k: (lambda k=k: res.__setitem__(k, quant.tree_accept(parents, mask, draft, target, seq_lens=seq, route=k))) for k in ("kernel", "torch")}
    for f in runs.values(): f()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(res["kernel"], res["torch"])) and int(res["kernel"][0][0]) == T.bit_length()
    got = contest(runs)
    rec = dict(what="accept", cache=cache, seqs=B, nodes=T, accept_us=round(got["kernel"][0], 2), accept_spread_us=round(got["kernel"][1], 2),
               accept_torch_us=round(got["torch"][0], 2), accept_torch_spread_us=round(got["torch"][1], 2))
    rec["torch_over_kernel"] = round(got["torch"][0] / got["kernel"][0], 2)
    rec["not_faster"] = ["accept"] if got["kernel"][0] + got["kernel"][1] >= got["torch"][0] else []
    print(json.dumps(rec), flush=True)
    for name, nodes in (("move1", [1]), ("move4", [1, 3, 5, 7]), ("move8", [2 * j + 1 for j in range(8)]), ("prefix4", [0, 1, 2, 3])):
        path = torch.full((B, T), -1, dtype=torch.int32, device=dev)
        path[:, :len(nodes)] = torch.tensor(nodes, dtype=torch.int32, device=dev)
        alen = torch.full((B,), len(nodes), dtype=torch.int32, device=dev)
        moved = 0 if name == "prefix4" else len(nodes) * B * len(caches) * H * D * (1 if fp8 else 2)
        runs = {k: (lambda k=k: quant.compact_kv(caches, table, seq, T, path, alen, block_size=BLOCK, route=k)) for k in ("kernel", "torch")}
        # the two forms leave the same bytes, each from the same state (the first pair refilled: replays have made its rows equal)
        for b in bufs[:2]: b.copy_(torch.randint(0, 120, b.shape, device=dev, dtype=torch.int32).to(raw))
        start = [b.clone() for b in bufs]
        ends = {}
        for k, f in runs.items():
            for b, s0 in zip(bufs, start): b.copy_(s0)
            f()
            ends[k] = [b.clone() for b in bufs[:2]]
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(ends["kernel"], ends["torch"])) and (moved == 0) == torch.equal(ends["kernel"][0], start[0])
        del start, ends
        got = contest(runs)
        rec = dict(what="compact", cache=cache, seqs=B, nodes=T, path=name, caches=len(caches), bytes_moved=moved,
                   floor_us=round(3.0 + moved * 2 / 4.8e12 * 1e6, 2), compact_us=round(got["kernel"][0], 2), compact_spread_us=round(got["kernel"][1], 2),
                   compact_torch_us=round(got["torch"][0], 2), compact_torch_spread_us=round(got["torch"][1], 2))
        rec["torch_over_kernel"] = round(got["torch"][0] / got["kernel"][0], 2)
        rec["not_faster"] = ["compact"] if got["kernel"][0] + got["kernel"][1] >= got["torch"][0] else []
        print(json.dumps(rec), flush=True)
