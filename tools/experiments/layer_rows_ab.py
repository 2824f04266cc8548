#!/usr/bin/env python3
"""13B w4 s45 decoder layer at 2 / 8 / 16 / 128 batch rows, microseconds per layer: HIP-graph replay (up to 16 rows, as
bench.py's 13B batch leg) and eager launches (every row count; the host launch path runs on every call).  One JSON line.
For a same-box A/B run it alternately with SQLLM_LIB pointing at each library.

    python tools/experiments/layer_rows_ab.py [rows,rows,...]
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch

import bench
from squeezellm_amd import decode

dev = torch.device("cuda:0")
rows = [int(r) for r in sys.argv[1].split(",")] if len(sys.argv) > 1 else [2, 8, 16, 128]
n_layers = 4
layers = bench.build_layers(bench.CONFIGS["13b-w4-s45"], dev, 0, n_layers)
gen = torch.Generator(device=dev).manual_seed(4321)
sync = torch.cuda.synchronize
out = {"lib": os.environ.get("SQLLM_LIB", "default")}
for B in rows:
    xs, ys = bench.decoder_inputs(layers, dev, gen, batch=B)
    seq = decode.OpSequence(layers, xs, ys, batched=True, fuse_shared_input=True)
    rec = {}
    if B <= 16:
        graph = seq.graph(warmup=1)
        blocks = bench.time_blocks(graph.replay, sync, 20, 3, 5)
        rec["graph_us"] = round(statistics.median(blocks) / 20 / n_layers * 1e6, 2)
        del graph
    for _ in range(3):
        seq.launch()
    sync()
    walls = []
    for _ in range(7):
        t0 = time.perf_counter()
        for _ in range(10):
            seq.launch()
        sync()
        walls.append((time.perf_counter() - t0) / 10 / n_layers * 1e6)
    rec["eager_us"] = round(statistics.median(walls), 2)
    out[f"rows{B}"] = rec
    del xs, ys, seq
print(json.dumps(out), flush=True)
