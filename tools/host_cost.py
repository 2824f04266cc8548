#!/usr/bin/env python3
"""What one operator call costs on the HOST (eager, no graph): microseconds per call of the quant_cuda names, of the
C function behind them called straight through ctypes with everything pre-marshalled (the floor of this binding),
and of QuantLinearLUT.forward (the reference's four launches per linear).  Tiny layer: the kernel is short, the loop
is host-bound, so wall time / calls = host cost per call.

    python tools/host_cost.py

    python tools/host_cost.py --fronts

The front modules' Python path (quant.QuantLinearLUTFused, QuantGatedLUTFused, QuantQKVRopeFused), for comparing two trees:
one instance of each front is sent through every variant it has (fp16 / bf16, rows 1 / 3 / 1, epilogues, norm weights, KV
caches) from fixed seeds and each call's outputs -- for a call with a KV cache the cache contents too -- are printed as one
sha256; then the eager host microseconds per call of six paths at 1 row of fp16 (median of `per_call` runs).  Uses the public
classes only, so the same file runs against an older tree.
"""
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from squeezellm_amd import _lib, quant, quant_cuda, synth  # noqa: E402

dev = torch.device("cuda:0")


def per_call(fn, n=20000):
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t1 = time.perf_counter()  # (host time only: the queue drains afterwards)
    torch.cuda.synchronize()
    return (t1 - t0) / n * 1e6


def ops():
    out = {}
    for tag, sparse, topX in (("dense", 0.0, 0), ("hybrid", 0.0045, 10)):
        lay = synth.make_layer(256, 256, 4, sparse_frac=sparse, topX=topX, device=dev, seed=1)
        x, y = torch.randn(256, device=dev), torch.zeros(256, device=dev)
        if sparse:
            f = lambda: quant_cuda.vecquant4matmul_spmv_hybrid_nuq_perchannel(lay["rows"], lay["cols"], lay["vals"], x, lay["full_rows"],  # noqa: E731
                                                                              lay["full_row_indices"], y, 256, lay["qweight"], lay["lookup_table"])
        else:
            f = lambda: quant_cuda.vecquant4matmul_nuq_perchannel(x, lay["qweight"], y, lay["lookup_table"])  # noqa: E731
        out[f"op_call_{tag}_us"] = round(per_call(f), 2)
        lib = _lib.load()
        op = _lib.SqllmOp(bits=4, batch=0, K=256, N=256)
        op.vec, op.qweight, op.mul, op.lookup_table = x.data_ptr(), lay["qweight"].data_ptr(), y.data_ptr(), lay["lookup_table"].data_ptr()
        if sparse:
            op.rows, op.cols, op.vals, op.nnz = lay["rows"].data_ptr(), lay["cols"].data_ptr(), lay["vals"].data_ptr(), lay["vals"].numel()
            op.full_rows, op.full_row_indices, op.topX = lay["full_rows"].data_ptr(), lay["full_row_indices"].data_ptr(), 10
        stream = torch.cuda.current_stream(dev).cuda_stream
        ref = ctypes.byref(op)
        out[f"c_launch_{tag}_us"] = round(per_call(lambda: lib.sqllm_launch(ref, stream)), 2)
        mod = quant.QuantLinearLUT.from_operands(lay)
        x16 = x.half().reshape(1, 1, -1)
        with torch.no_grad():
            out[f"forward_{tag}_us"] = round(per_call(lambda: mod(x16), n=5000), 2)
    e = torch.empty(256, device=dev)
    out["torch_zero_us"] = round(per_call(lambda: e.zero_()), 2)
    out["torch_empty_launch_floor_us"] = round(per_call(lambda: torch.zeros(256, device=dev), n=5000), 2)
    print(json.dumps(out))


# ---- --fronts ----
K, NQ, NKV, D, SLOTS = 256, 256, 128, 64, 8  # the smallest shapes with CSR and top-X terms in every member and k / v narrower than q


def front_member(N, bits, seed):
    lay = synth.make_layer(K, N, bits, sparse_frac=0.01, topX=3, bias=bool(seed % 2), device=dev, seed=seed)
    m = quant.QuantLinearLUT.from_operands(lay)
    m.__class__ = quant.QuantLinearLUTFused
    return m


def front_modules(bits):
    """-> {front: a fresh module}, the same operands every time"""
    return {"linear": front_member(NQ, bits, 11),
            "gated": quant.QuantGatedLUTFused(front_member(NQ, bits, 12), front_member(NQ, bits, 13)),
            "qkv": quant.QuantQKVRopeFused(front_member(NQ, bits, 14), front_member(NKV, bits, 15), front_member(NKV, bits, 16), D)}


def _rand(shape, seed, dtype, scale=1.0):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(dev).to(dtype)


def front_calls(front, dtype, rows):
    """-> [(variant, call(module) -> the tensors that make the call's result)], in the order that alternates the variants"""
    x = _rand((rows, 1, K), 100 + rows, dtype)
    if front == "linear":
        res = _rand((rows, 1, NQ), 200 + rows, dtype)

        def silu_out(m):
            out = torch.full((rows, 1, NQ), 7.0, dtype=dtype, device=dev)
            m.act = "silu"
            try:
                y = m(x, out=out)
            finally:
                m.act = None
            assert y is out
            return [out]

        return [("plain", lambda m: [m(x)]), ("residual", lambda m: [m(x, residual=res)]), ("silu_out", silu_out), ("plain", lambda m: [m(x)])]
    w1, w2 = _rand((K,), 301, dtype, 0.5) + 1, _rand((K,), 302, dtype, 0.5) + 1
    if front == "gated":
        return [("norm", lambda m: [m(x, w1, 1e-5)]), ("plain", lambda m: [m(x)]), ("norm_other_weight", lambda m: [m(x, w2, 1e-6)])]
    cos, sin = quant.rope_tables(D, 32, device=dev)
    pos = torch.arange(rows, dtype=torch.int32, device=dev) * 5 + 2
    slots = torch.tensor([5, -1, 2][:rows], dtype=torch.int32, device=dev)

    def cached(fp8, **kw):
        def call(m):
            if fp8:
                kc, vc = (torch.full((SLOTS, NKV // D, D), 0x11 * (i + 1), dtype=torch.uint8, device=dev) for i in range(2))
                kw.update(k_scale=0.05, v_scale=0.02)
            else:
                kc, vc = (torch.full((SLOTS, NKV // D, D), 3.0 + i, dtype=dtype, device=dev) for i in range(2))
            outs = m(x, pos, cos, sin, k_cache=kc, v_cache=vc, slots=slots, **kw)
            return [o for o in outs if o is not None] + [kc, vc]
        return call

    return [("plain", lambda m: list(m(x, pos, cos, sin))), ("cache_no_kv", cached(False, return_kv=False)), ("cache_fp8", cached(True)),
            ("plain", lambda m: list(m(x, pos, cos, sin))), ("norm_cache", cached(False, norm_weight=w1, norm_eps=1e-5))]


def sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(str((t.dtype, tuple(t.shape))).encode())
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def fronts(reps=9):
    with torch.no_grad():
        for bits in (3, 4):
            for front, mod in front_modules(bits).items():
                for dtype in (torch.float16, torch.bfloat16):
                    for i, rows in enumerate((1, 3, 1)):
                        for j, (variant, call) in enumerate(front_calls(front, dtype, rows)):
                            print(f"sha256 {front} w{bits} {str(dtype)[6:]} rows={rows}#{i} {variant}#{j}: {sha(call(mod))}")
        mods = front_modules(4)
        x = _rand((1, 1, K), 1, torch.float16)
        res = _rand((1, 1, NQ), 2, torch.float16)
        w = _rand((K,), 3, torch.float16, 0.5) + 1
        cos, sin = quant.rope_tables(D, 32, device=dev)
        pos, slots = torch.tensor([3], dtype=torch.int32, device=dev), torch.tensor([5], dtype=torch.int32, device=dev)
        kc, vc = (torch.zeros((SLOTS, NKV // D, D), dtype=torch.uint8, device=dev) for _ in range(2))
        lin, gated, qkv = mods["linear"], mods["gated"], mods["qkv"]
        paths = {"linear": lambda: lin(x), "linear_residual": lambda: lin(x, residual=res),
                 "gated": lambda: gated(x), "gated_norm": lambda: gated(x, w, 1e-5),
                 "qkv": lambda: qkv(x, pos, cos, sin),
                 "qkv_norm_fp8_cache": lambda: qkv(x, pos, cos, sin, norm_weight=w, norm_eps=1e-5, k_cache=kc, v_cache=vc, slots=slots,
                                                   k_scale=0.05, v_scale=0.02)}
        out = {}
        for name, f in paths.items():
            runs = sorted(per_call(f) for _ in range(reps))
            out[name] = {"median_us": round(statistics.median(runs), 3), "min_us": round(runs[0], 3), "max_us": round(runs[-1], 3)}
        print("host_us " + json.dumps(out))


if __name__ == "__main__":
    fronts() if "--fronts" in sys.argv[1:] else ops()
