"""The KV-cache arguments of quant.QuantQKVRopeFused without a GPU: the two helpers (quant.kv_cache_view for both layouts,
quant.static_cache_slots), the fallback route on CPU tensors -- it writes the same elements as indexing by hand and skips
out-of-range slots -- and the argument errors.  (The operators have no CPU path: the members' sums come from a stand-in
for QuantLinearLUT.forward, a seeded fp32 matrix per width; the rotation, the routing and the cache writes are the module's.)"""
import numpy as np
import pytest

from tests import test_gpu_qkv_rope as TQ

K = TQ.K
NQ, NKV, D = 384, 128, 64  # two kv heads
H = NKV // D


@pytest.fixture(autouse=True)
def _sums_on_the_cpu(monkeypatch):
    import torch

    from squeezellm_amd import quant

    def forward(self, x):
        w = torch.randn(self.outfeatures, self.infeatures, generator=torch.Generator().manual_seed(self.outfeatures)) / 32
        return x.float() @ w.T

    monkeypatch.setattr(quant.QuantLinearLUT, "forward", forward)


def _module():
    members = tuple(TQ._layer("cpu", 4, n, False, m) for m, n in enumerate((NQ, NKV, NKV)))
    return TQ._module(members, D, "half")


def _operands(rows):
    import torch

    x = TQ._x("cpu", rows, "float16").float()
    cos, sin = TQ._tables(D)
    return x, torch.tensor(TQ._positions(rows), dtype=torch.int32), torch.from_numpy(cos.copy()), torch.from_numpy(sin.copy())


def test_kv_cache_view_strides_for_both_layouts():
    import torch

    from squeezellm_amd import quant

    c3 = torch.zeros(23, H, D)
    assert quant.kv_cache_view(c3, "nhd") is c3 and quant.kv_cache_view(c3) is c3
    paged = torch.zeros(6, 4, H, D)  # [blocks, block, H, D]: slot = block_index * 4 + offset
    v = quant.kv_cache_view(paged, "nhd")
    assert tuple(v.shape) == (24, H, D) and v.stride() == (H * D, D, 1) and v.data_ptr() == paged.data_ptr()
    v[4 * 3 + 1, 1, 5] = 7.0
    assert paged[3, 1, 1, 5] == 7.0
    # a view of wider allocations keeps their strides: slot_stride and head_stride beyond the minimum
    wide = torch.zeros(23, H + 1, D + 3)[:, :H, 1:1 + D]
    v = quant.kv_cache_view(wide, "nhd")
    assert v.stride() == ((H + 1) * (D + 3), D + 3, 1) and v.storage_offset() == 1
    B, S = 3, 5
    c4 = torch.zeros(B, H, S, D)
    v = quant.kv_cache_view(c4, "bhsd")
    assert tuple(v.shape) == ((B - 1) * H * S + S, H, D) and v.stride() == (D, S * D, 1) and v.data_ptr() == c4.data_ptr()
    for b in range(B):
        for p in range(S):
            v[b * H * S + p] = torch.full((H, D), float(100 * b + p))
    want = (100 * torch.arange(B)[:, None, None, None] + torch.arange(S)[None, None, :, None]).expand(B, H, S, D).float()
    assert torch.equal(c4, want)  # every (b, p) pair has elements of its own, and together they are the whole cache
    # the extent of the view is the cache's: the last slot's last head ends with it
    assert (v.shape[0] - 1) * D + (H - 1) * S * D + D == c4.numel()
    with pytest.raises(ValueError, match="layout"):
        quant.kv_cache_view(c3, "hnd")
    with pytest.raises(ValueError):
        quant.kv_cache_view(torch.zeros(23, H * D), "nhd")
    with pytest.raises(ValueError):
        quant.kv_cache_view(torch.zeros(6, 8, H, D)[:, :4], "nhd")  # blocks that do not lie block * stride(1) apart
    with pytest.raises(ValueError):
        quant.kv_cache_view(c4.transpose(1, 2), "bhsd")
    with pytest.raises(ValueError, match="contiguous"):
        quant.kv_cache_view(torch.zeros(23, H, 2 * D)[:, :, ::2], "nhd")


def test_static_cache_slots():
    import torch

    from squeezellm_amd import quant

    pos = torch.tensor([4, 0, 2, 1], dtype=torch.int32)
    s = quant.static_cache_slots(pos, n_kv_heads=H, max_seq=5)
    assert s.dtype == torch.int32 and s.tolist() == [b * H * 5 + p for b, p in enumerate(pos.tolist())]
    assert quant.static_cache_slots(pos.long().reshape(2, 2), H, 5).tolist() == s.tolist()
    # a position outside [0, max_seq) would be another row's or head's slot: out of range instead, which writes nothing
    assert quant.static_cache_slots(torch.tensor([5, -1, 3]), H, 5).tolist() == [-1, -1, 2 * H * 5 + 3]
    # ... and every slot lies inside the view of kv_cache_view(cache, "bhsd")
    n_slots = quant.kv_cache_view(torch.zeros(4, H, 5, D), "bhsd").shape[0]
    assert 0 <= min(s.tolist()) and max(s.tolist()) < n_slots and quant.static_cache_slots(torch.tensor([0, 0, 0, 4]), H, 5)[-1] == n_slots - 1


@pytest.mark.parametrize("geom", ["nhd", "bhsd", "padded"])
def test_fallback_route_writes_what_indexing_by_hand_writes(geom):
    import torch

    from squeezellm_amd import quant

    rows, S, n_nhd = 5, 4, 11
    mod = _module()
    x, pos, cos, sin = _operands(rows)
    plain = mod(x, pos, cos, sin)
    assert mod.last_route == "fallback"
    if geom == "nhd":
        back = [torch.full((n_nhd, H, D), -7.0) for _ in range(2)]
        views = back
        slots = [n_nhd - 1, 0, -1, 6, n_nhd]
    elif geom == "padded":
        back = [torch.full((n_nhd, H + 2, D + 5), -7.0) for _ in range(2)]
        views = [b[:, 1:1 + H, 2:2 + D] for b in back]
        slots = [n_nhd - 1, 0, -1, 6, n_nhd]
    else:
        back = [torch.full((rows, H, S, D), -7.0) for _ in range(2)]
        views = [quant.kv_cache_view(b, "bhsd") for b in back]
        slots = quant.static_cache_slots(torch.tensor([3, 0, 4, 1, -1]), H, S).tolist()  # rows 2 and 4: positions outside [0, S)
        assert slots[2] == slots[4] == -1
        slots[4] = views[0].shape[0]
    want = [b.clone() for b in back]
    for b, s in enumerate(slots):  # by hand
        if not 0 <= s < views[0].shape[0]:
            continue
        for which in (0, 1):
            row = plain[1 + which][b].reshape(H, D)
            if geom == "nhd":
                want[which][s] = row
            elif geom == "padded":
                want[which][s, 1:1 + H, 2:2 + D] = row
            else:
                want[which][s // (H * S), :, s % (H * S)] = row
    for sl in (torch.tensor(slots, dtype=torch.int32), torch.tensor(slots, dtype=torch.int64)):
        for return_kv in (True, False):
            for b in back:
                b.fill_(-7.0)
            outs = mod(x, pos, cos, sin, k_cache=views[0], v_cache=views[1], slots=sl, return_kv=return_kv)
            assert mod.last_route == "fallback" and torch.equal(outs[0], plain[0])
            if return_kv:
                assert torch.equal(outs[1], plain[1]) and torch.equal(outs[2], plain[2])
            else:
                assert outs[1] is None and outs[2] is None
            for which in (0, 1):
                assert torch.equal(back[which], want[which])
    assert (want[0] != -7.0).sum() == 3 * NKV  # three live rows, and nothing else


def test_argument_errors():
    import torch

    rows = 3
    mod = _module()
    x, pos, cos, sin = _operands(rows)
    kv, vv = torch.zeros(7, H, D), torch.zeros(7, H, D)
    sl = torch.tensor([0, 6, 3], dtype=torch.int32)
    mod(x, pos, cos, sin, k_cache=kv, v_cache=vv, slots=sl)
    for kw in (dict(k_cache=kv), dict(v_cache=vv), dict(slots=sl), dict(k_cache=kv, v_cache=vv), dict(k_cache=kv, slots=sl), dict(v_cache=vv, slots=sl)):
        with pytest.raises(ValueError, match="all three or none"):
            mod(x, pos, cos, sin, **kw)
    with pytest.raises(ValueError, match="return_kv"):
        mod(x, pos, cos, sin, return_kv=False)
    bad = [
        dict(k_cache=kv.half()),  # dtype
        dict(v_cache=vv.double()),
        dict(k_cache=kv[:, :1], v_cache=vv[:, :1]),  # H_kv * head_dim != N_k
        dict(k_cache=kv.reshape(7, 4, 32), v_cache=vv.reshape(7, 4, 32)),  # head_dim
        dict(k_cache=kv.reshape(7, NKV), v_cache=vv.reshape(7, NKV)),  # not 3-D
        dict(k_cache=kv.reshape(1, 7, H, D), v_cache=vv.reshape(1, 7, H, D)),
        dict(v_cache=vv[:5]),  # unequal shapes
        dict(v_cache=torch.zeros(7, 2 * H, D)[:, ::2]),  # unequal strides
        dict(k_cache=torch.zeros(7, H, 2 * D)[:, :, ::2], v_cache=torch.zeros(7, H, 2 * D)[:, :, ::2]),  # stride(-1) != 1
        dict(k_cache=torch.zeros(1, H, D).expand(7, H, D), v_cache=torch.zeros(1, H, D).expand(7, H, D)),  # slot stride 0
        dict(slots=sl[:2]),
        dict(slots=sl.float()),
        dict(slots=[0, 6, 3]),
        dict(k_cache="cache"),
    ]
    for kw in bad:
        args = dict(k_cache=kv, v_cache=vv, slots=sl)
        args.update(kw)
        with pytest.raises(ValueError):
            mod(x, pos, cos, sin, **args)
    # k and v of different widths cannot share a cache geometry
    wide_v = TQ._module(tuple(TQ._layer("cpu", 4, n, False, m) for m, n in enumerate((NQ, NKV, 192))), D, "half")
    with pytest.raises(ValueError, match="one width"):
        wide_v(x, pos, cos, sin, k_cache=kv, v_cache=vv, slots=sl)


def test_the_signature_and_the_parent_call_are_unchanged():
    import inspect

    from squeezellm_amd import quant

    sig = inspect.signature(quant.QuantQKVRopeFused.forward)
    assert list(sig.parameters) == ["self", "x", "positions", "cos", "sin", "norm_weight", "norm_eps", "k_cache", "v_cache", "slots", "return_kv"]
    assert [sig.parameters[n].default for n in ("norm_weight", "norm_eps", "k_cache", "v_cache", "slots", "return_kv")] == [None, 1e-6, None, None, None, True]
    rows = 2
    mod = _module()
    x, pos, cos, sin = _operands(rows)
    outs = mod(x, pos, cos, sin)
    assert len(outs) == 3 and all(o is not None for o in outs) and np.isfinite(outs[1].numpy()).all()
