"""The host path the three front modules of squeezellm_amd.quant share, without a GPU: the entry table against the header, the
int32 fix-up of positions / slots, and the fallback route of each front on CPU tensors (fp32 input) against the formulas
composed by hand.  (The operators have no CPU path: the members' sums come from a stand-in for QuantLinearLUT.forward, a seeded
fp32 matrix per member; the norm, the rotation, the epilogue, the routing and the cache writes are the module's.  A cache that is
not fp8 has the activations' type, so the "16-bit cache" of the GPU calls is an fp32 one here.)"""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, NQ, NKV, D, SLOTS = 256, 256, 128, 64, 8
H = NKV // D

# the ten dicts the table replaced, two names each
FORMER = ["sqllm_linear", "sqllm_linear_ep", "sqllm_gated", "sqllm_gated_norm", "sqllm_qkv_rope", "sqllm_qkv_rope_norm", "sqllm_qkv_rope_cache",
          "sqllm_qkv_rope_norm_cache", "sqllm_qkv_rope_cache_fp8", "sqllm_qkv_rope_norm_cache_fp8"]
# (norm, cache, fp8) -> what the launch ladder of QuantQKVRopeFused.forward chose
QKV_LADDER = {(False, False, False): "sqllm_qkv_rope", (True, False, False): "sqllm_qkv_rope_norm", (False, True, False): "sqllm_qkv_rope_cache",
              (True, True, False): "sqllm_qkv_rope_norm_cache", (False, True, True): "sqllm_qkv_rope_cache_fp8",
              (True, True, True): "sqllm_qkv_rope_norm_cache_fp8"}


def test_entry_table_holds_the_twenty_declared_names():
    import torch

    from squeezellm_amd import quant

    header = open(os.path.join(ROOT, "include", "sqllm_hip.h")).read()
    declared = set(re.findall(r"\b(sqllm_\w+)\s*\(", header))
    table = quant._FRONT_ENTRY
    assert len(table) == 20 and len(set(table.values())) == 20
    assert sorted(table.values()) == sorted(f"{name}_{sfx}" for name in FORMER for sfx in ("f16", "bf16"))
    assert set(table.values()) <= declared
    assert quant._FRONT_DTYPES == (torch.float16, torch.bfloat16)
    for dtype, sfx in ((torch.float16, "f16"), (torch.bfloat16, "bf16")):
        assert table["linear", False, False, False, dtype] == f"sqllm_linear_{sfx}"
        assert table["linear_ep", False, False, False, dtype] == f"sqllm_linear_ep_{sfx}"
        assert table["gated", False, False, False, dtype] == f"sqllm_gated_{sfx}"
        assert table["gated", True, False, False, dtype] == f"sqllm_gated_norm_{sfx}"
        qkv = {k[1:4]: v for k, v in table.items() if k[0] == "qkv_rope" and k[4] == dtype}
        assert qkv == {k: f"{v}_{sfx}" for k, v in QKV_LADDER.items()}


def test_int32_vector_passes_a_contiguous_int32_vector_through():
    import torch

    from squeezellm_amd.quant import _int32_vector

    t = torch.arange(5, dtype=torch.int32)
    assert _int32_vector(t) is t  # no copy, no kernel: a captured graph follows the caller's tensor
    for src in (torch.arange(5, dtype=torch.int64), torch.arange(10, dtype=torch.int32)[::2], torch.arange(5, dtype=torch.int32).reshape(5, 1),
                torch.arange(10, dtype=torch.int64).reshape(5, 2)[:, :1]):
        got = _int32_vector(src)
        assert got.dtype == torch.int32 and got.dim() == 1 and got.is_contiguous() and got.tolist() == src.reshape(-1).tolist()
        assert got.data_ptr() != src.data_ptr() or src.dim() == 2  # (a [rows, 1] int32 input is viewed, the others are copied)


@pytest.fixture()
def fwd(monkeypatch):
    """the stand-in for QuantLinearLUT.forward: fp32 sums of a seeded matrix per member"""
    import torch

    from squeezellm_amd import quant

    def forward(self, x):
        w = torch.randn(self.outfeatures, self.infeatures, generator=torch.Generator().manual_seed(self.__dict__["seed"])) / 16
        return x.float() @ w.T

    monkeypatch.setattr(quant.QuantLinearLUT, "forward", forward)
    return forward


def _member(N, bits, seed, fused=True):
    from squeezellm_amd import quant, synth

    m = quant.QuantLinearLUT.from_operands(synth.make_layer(K, N, bits, sparse_frac=0.01, topX=3, bias=bool(seed % 2), device="cpu", seed=seed))
    assert m.op_kind(False) == "spmv_hybrid"
    if fused:
        m.__class__ = quant.QuantLinearLUTFused
    m.__dict__["seed"] = seed
    return m


def _x(rows, seed=0):
    import torch

    return torch.randn((rows, 1, K), generator=torch.Generator().manual_seed(100 + rows + seed))


def _norm_weight():
    import torch

    return torch.randn(K, generator=torch.Generator().manual_seed(7)) * 0.5 + 1


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("bits", [3, 4])
def test_linear_fallback_is_the_parent_forward_and_the_torch_epilogue(fwd, bits, rows):
    import torch

    from squeezellm_amd import quant

    m = _member(NQ, bits, 11)
    x = _x(rows)
    s = fwd(m, x)
    assert torch.equal(m(x), s) and m(x).shape == (rows, 1, NQ)
    res = _x(rows, 5)[..., :NQ].contiguous()
    assert torch.equal(m(x, residual=res), quant._torch_epilogue(s, None, res, x.dtype))
    for act in ("relu", "silu", "gelu", "gelu_tanh"):
        m.act = act
        out = torch.full((rows, 1, NQ), 7.0)
        assert m(x, residual=res, out=out) is out and torch.equal(out, quant._torch_epilogue(s, act, res, x.dtype))
        assert torch.equal(m(x), quant._torch_epilogue(s, act, None, x.dtype))
    m.act = None
    assert torch.equal(m(x), s)
    with pytest.raises(ValueError, match="last dimension of x must be 256"):
        m(x[..., :-1], residual=res)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("bits", [3, 4])
def test_gated_fallback_is_silu_gate_times_up_with_and_without_the_norm(fwd, bits, rows, fused):
    import torch
    import torch.nn.functional as F

    from squeezellm_amd import quant

    gate, up = _member(NQ, bits, 12, fused), _member(NQ, bits, 13, fused)
    mod = quant.QuantGatedLUTFused(gate, up)
    x, w = _x(rows), _norm_weight()
    for _ in range(2):  # norm -> no norm -> norm -> no norm on one instance
        xn = quant._torch_rmsnorm(x.reshape(-1, K), w, 1e-5)
        want = (F.silu(fwd(gate, xn).float()) * fwd(up, xn).float()).to(x.dtype).reshape(rows, 1, NQ)
        assert torch.equal(mod(x, w, 1e-5), want) and mod.last_route == "fallback"
        assert torch.equal(mod(x), F.silu(fwd(gate, x)) * fwd(up, x)) and mod(x).shape == (rows, 1, NQ)
    with pytest.raises(ValueError, match="last dimension of x must be 256"):
        mod(x[..., :-1], w[:-1])


def _write_by_hand(cache, slots, rows_):
    for b, s in enumerate(slots.tolist()):
        if 0 <= s < cache.shape[0]:
            cache[s] = rows_[b].reshape(H, D)


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("bits", [3, 4])
def test_qkv_fallback_is_the_rotated_sums_and_the_cache_writes(fwd, bits, rows, norm):
    import torch

    from squeezellm_amd import quant

    q, k, v = _member(NQ, bits, 14), _member(NKV, bits, 15), _member(NKV, bits, 16)
    mod = quant.QuantQKVRopeFused(q, k, v, D)
    x, w = _x(rows), _norm_weight()
    cos, sin = quant.rope_tables(D, 32)
    pos = torch.tensor([3, 0, 31][:rows], dtype=torch.int32)
    slots = torch.tensor([5, -1, 2][:rows], dtype=torch.int64)
    kw = dict(norm_weight=w, norm_eps=1e-5) if norm else {}
    xin = quant._torch_rmsnorm(x.reshape(-1, K), w, 1e-5) if norm else x.reshape(-1, K)
    sq, sk, sv = (fwd(m, xin) for m in (q, k, v))
    oq = quant._torch_rope(sq, pos, cos, sin, D, "half", x.dtype)
    ok32 = quant._torch_rope(sk, pos, cos, sin, D, "half", torch.float32)
    want = [oq.reshape(rows, 1, NQ), ok32.to(x.dtype).reshape(rows, 1, NKV), sv.to(x.dtype).reshape(rows, 1, NKV)]

    def same(got, kv=True):
        assert mod.last_route == "fallback" and len(got) == 3 and torch.equal(got[0], want[0])
        assert (torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])) if kv else (got[1] is None and got[2] is None)

    same(mod(x, pos, cos, sin, **kw))
    # a cache of the activations' type, k and v to the cache alone
    kc, vc = torch.full((SLOTS, H, D), 3.0), torch.full((SLOTS, H, D), 4.0)
    hk, hv = kc.clone(), vc.clone()
    _write_by_hand(hk, slots, want[1].reshape(rows, NKV))
    _write_by_hand(hv, slots, want[2].reshape(rows, NKV))
    same(mod(x, pos, cos, sin, k_cache=kc, v_cache=vc, slots=slots, return_kv=False, **kw), kv=False)
    assert torch.equal(kc, hk) and torch.equal(vc, hv) and not torch.equal(kc, torch.full_like(kc, 3.0))
    # a byte cache with its two scales: the fp32 values before their rounding, encoded once
    kc8, vc8 = torch.full((SLOTS, H, D), 0x11, dtype=torch.uint8), torch.full((SLOTS, H, D), 0x22, dtype=torch.uint8)
    hk8, hv8 = kc8.clone(), vc8.clone()
    _write_by_hand(hk8, slots, quant._fp8_bytes(ok32, 0.05))
    _write_by_hand(hv8, slots, quant._fp8_bytes(sv.float(), 0.02))
    same(mod(x, pos, cos, sin, k_cache=kc8, v_cache=vc8, slots=slots, k_scale=0.05, v_scale=0.02, **kw))
    assert torch.equal(kc8, hk8) and torch.equal(vc8, hv8) and not torch.equal(kc8, torch.full_like(kc8, 0x11))
    same(mod(x, pos, cos, sin, **kw))  # and without a cache again
    with pytest.raises(ValueError, match="last dimension of x must be 256"):  # the width comes first, whatever else is wrong
        mod(x[..., :-1], pos, cos, sin[:, :-1], return_kv=False)
