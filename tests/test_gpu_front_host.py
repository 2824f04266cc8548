"""One instance of each front module, sent through every variant it has in an order that alternates them -- fp16 / bf16, rows
1 / 3 / 1, epilogues, norm weights, KV caches --, returns for every call the bits a FRESH instance returns for that one call,
the cache contents included: nothing a call writes into the shared, cached descriptor of (device, stream) is left over for the
next call of another variant.  (tests/test_gpu_attn_append.py does the same for DecodeAttention's four kinds.)  Afterwards the
instance holds one descriptor and one non-graph workspace.  K = 256, N = 256 (q, gate, up) and 128 (k, v), head_dim 64, CSR and
top-X terms in every member: the smallest shapes at which a member op has both terms and the widths of q and k / v differ."""
import pytest

gpu_test = pytest.mark.gpu

K, NQ, NKV, D, SLOTS = 256, 256, 128, 64, 8
H = NKV // D


def _layers(gpu, bits):
    from squeezellm_amd import synth

    return [synth.make_layer(K, n, bits, sparse_frac=0.01, topX=3, bias=bool(i % 2), device=gpu, seed=40 + i) for i, n in enumerate((NQ, NQ, NKV, NKV))]


def _module(front, lays):
    """a fresh module over the same operands"""
    from squeezellm_amd import quant

    def member(lay):
        m = quant.QuantLinearLUT.from_operands(lay)
        m.__class__ = quant.QuantLinearLUTFused
        return m

    if front == "linear":
        return member(lays[0])
    if front == "gated":
        return quant.QuantGatedLUTFused(member(lays[0]), member(lays[1]))
    return quant.QuantQKVRopeFused(member(lays[0]), member(lays[2]), member(lays[3]), D)


def _rand(gpu, shape, seed, dtype, scale=1.0):
    import torch

    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).to(gpu).to(dtype)


def _calls(gpu, front, dtype, rows):
    """[(variant, the route it must take, call(module) -> the tensors that make up the call's result)] in the alternating order"""
    import torch

    from squeezellm_amd import quant

    x = _rand(gpu, (rows, 1, K), 100 + rows, dtype)
    if front == "linear":
        res = _rand(gpu, (rows, 1, NQ), 200 + rows, dtype)

        def silu_out(m):
            out = torch.full((rows, 1, NQ), 7.0, dtype=dtype, device=gpu)
            m.act = "silu"
            try:
                assert m(x, out=out) is out
            finally:
                m.act = None
            return [out]

        return [("plain", "fused", lambda m: [m(x)]), ("residual", "fused_ep", lambda m: [m(x, residual=res)]), ("silu + out", "fused_ep", silu_out),
                ("plain", "fused", lambda m: [m(x)])]
    w1, w2 = _rand(gpu, (K,), 301, dtype, 0.5) + 1, _rand(gpu, (K,), 302, dtype, 0.5) + 1
    if front == "gated":
        return [("norm", "gated_norm", lambda m: [m(x, w1, 1e-5)]), ("plain", "gated", lambda m: [m(x)]),
                ("norm, another weight", "gated_norm", lambda m: [m(x, w2, 1e-6)])]
    cos, sin = quant.rope_tables(D, 32, device=gpu)
    pos = torch.tensor([3, 0, 31][:rows], dtype=torch.int32, device=gpu)
    slots = torch.tensor([5, -1, 2][:rows], dtype=torch.int32, device=gpu)

    def cached(fp8, **kw):
        def call(m):
            if fp8:
                kc, vc = (torch.full((SLOTS, H, D), 0x11 * (i + 1), dtype=torch.uint8, device=gpu) for i in range(2))
            else:
                kc, vc = (torch.full((SLOTS, H, D), 3.0 + i, dtype=dtype, device=gpu) for i in range(2))
            outs = m(x, pos, cos, sin, k_cache=kc, v_cache=vc, slots=slots, **kw)
            assert len(outs) == 3 and (outs[1] is None) == (outs[2] is None) == (kw.get("return_kv") is False)
            assert not torch.equal(kc[5], kc[0]) and torch.equal(kc[0], kc[1])  # slot 5 is written, slots nobody names are not
            return [o for o in outs if o is not None] + [kc, vc]
        return call

    plain = ("no cache", "qkv_rope", lambda m: list(m(x, pos, cos, sin)))
    return [plain, ("16-bit cache, return_kv=False", "qkv_rope", cached(False, return_kv=False)),
            ("fp8 cache", "qkv_rope", cached(True, k_scale=0.05, v_scale=0.02)), plain,
            ("norm + cache", "qkv_rope_norm", cached(False, norm_weight=w1, norm_eps=1e-5))]


@gpu_test
@pytest.mark.parametrize("front", ["linear", "gated", "qkv"])
@pytest.mark.parametrize("bits", [3, 4])
def test_one_instance_through_every_variant_returns_what_fresh_instances_return(gpu, bits, front):
    import torch

    lays = _layers(gpu, bits)
    mod = _module(front, lays)
    n = 0
    with torch.no_grad():
        for dtype in (torch.float16, torch.bfloat16):
            for rows in (1, 3, 1):
                for variant, route, call in _calls(gpu, front, dtype, rows):
                    fresh = _module(front, lays)
                    want = call(fresh)
                    got = call(mod)
                    what = f"{front} w{bits} {dtype} rows={rows} {variant}"
                    assert fresh.last_route == route and mod.last_route == route, what
                    assert len(got) == len(want) and all(bool(torch.isfinite(t.float()).all()) for t in want if t.dtype != torch.uint8), what
                    for g, w in zip(got, want):
                        assert g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.view(torch.uint8), w.view(torch.uint8)), what
                    n += 1
    assert n == 6 * {"linear": 4, "gated": 3, "qkv": 5}[front]
    members = {"linear": [], "gated": ["gate", "up"], "qkv": ["q", "k", "v"]}[front]
    for m in [mod] + [getattr(mod, name) for name in members]:
        assert len(m._desc) == 1  # one descriptor per (device, stream), whatever dtypes, row counts and variants arrived
    if front == "linear":
        assert len(mod._ep_desc) == 1
    own = [k for k in mod._ws if k != "retired" and k[1] != "graph"]
    assert len(own) == 1 and own[0][0] == lays[0]["qweight"].device  # one non-graph workspace
    ws = mod._ws[own[0]]
    torch.cuda.synchronize()
    assert not bool(ws.any())  # and every launch left it zero-filled
