"""Tree verification up to 64 nodes without a GPU (include/sqllm_hip.h, sqllm_attn_tree64): the torch fallback of
quant.PrefillAttention(..., tree_mask=) on CPU tensors against the fp64 oracle, quant.tree_masks(wide=True), the module's ValueErrors,
the entries' rejections in order (operand pointers are fake, nothing is launched) and the workspace function.  The cases are those of
tests/attn_tree_cases.py in tables of 2 P + 3 + 64 keys; tests/test_gpu_attn_tree64.py shares `build` and `mask_of`."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from squeezellm_amd._lib import ATTN_TREE64_PARTITION as P
from tests import attn_append_cases as A
from tests import attn_decode_cases as C
from tests import attn_tree_cases as K
from tests import test_attn_append_capi_cpu as TA
from tests.test_attn_tree_cpu import MASK, _desc, _operands

E_SHAPE, E_NULL, E_ALIGN, E_OPTION = TA.E_SHAPE, TA.E_NULL, TA.E_ALIGN, TA.E_OPTION
CAPACITY = 2 * P + 3 + 64  # keys a table row must hold
ENTRIES = ["sqllm_attn_tree64_f16", "sqllm_attn_tree64_bf16", "sqllm_attn_tree64_fp8_f16", "sqllm_attn_tree64_fp8_bf16"]


@functools.lru_cache(maxsize=None)
def build(kind, T, D, hq, hk, dt, contexts, capacity=CAPACITY):
    """(base, case): one sequence per context with T nodes behind it, and its expansion into T rows each (for q)"""
    base = C.build(kind, len(contexts), D, hq, hk, dt, 0, tuple(c + T for c in contexts), capacity)
    return base, A.expand(base, T)


def mask_of(words, device=None):
    """[B][T] words of up to 64 bits as the int64 tensor the module takes (bit 63 is the sign)"""
    return torch.tensor([[w - (1 << 64) if w >> 63 else w for w in row] for row in words], dtype=torch.int64, device=device)


def _module(base):
    from squeezellm_amd.quant import PrefillAttention

    return PrefillAttention(base.HQ, base.H, base.D, block_size=base.block_size)


@pytest.mark.parametrize("tree,kind,D,hq,hk,dt", [("heap", "paged", 64, 8, 2, "fp16"), ("no_tree", "padded", 128, 6, 2, "bf16")])
def test_the_torch_fallback_against_the_oracle(tree, kind, D, hq, hk, dt):
    T, contexts = 33, (0, 62, P - 2)
    base, case = build(kind, T, D, hq, hk, dt, contexts)
    words = [K.words(tree, T)] * len(contexts)
    att = _module(base)
    got = att(*_operands(base, case), q_len=T, tree_mask=mask_of(words))
    assert att.last_route == "fallback" and got.shape == (len(contexts) * T, hq * D)
    want, gate = C.reference_of(K.as_decode_case(base, case, words))
    assert np.isfinite(want).all() and C.excess(got.double().numpy(), want, gate) <= 1.0
    assert not torch.equal(got, att(*_operands(base, case), q_len=T))  # (the chain is another function)


@pytest.mark.parametrize("tree", K.TREES[:3])
def test_tree_masks_wide(tree):
    from squeezellm_amd.quant import tree_masks

    T = 40
    par = torch.tensor([K.parents(tree, T)] * 2)
    mask, depth = tree_masks(par, wide=True)
    want = K.words(tree, T)
    assert mask.dtype == torch.int64 and depth.dtype == torch.int32 and mask[0].tolist() == mask[1].tolist() == want
    assert depth[0].tolist() == [bin(w).count("1") - 1 for w in want]
    full, _ = tree_masks(torch.tensor([K.parents("two_chains", 64)]), wide=True)  # (bit 63: the sign of the int64 word)
    assert torch.equal(full, mask_of([K.words("two_chains", 64)]))
    narrow, _ = tree_masks(par[:, :16])  # the default call is what it was
    assert narrow.dtype == torch.int32 and narrow[0].tolist() == K.words(tree, 16)
    for kw in (dict(parents=par[:, :17]), dict(parents=torch.tensor([[-1] * 65]), wide=True)):
        with pytest.raises(ValueError):
            tree_masks(**kw)


def test_module_surface_value_errors():
    from squeezellm_amd.quant import PrefillAttention

    T = 5
    base, case = build("paged", T, 64, 8, 2, "fp16", (0, 4))
    ops = _operands(base, case)
    m = mask_of([K.words("star", T)] * 2)
    att = _module(base)
    for bad in (m[:1], m.to(torch.int32), m.float(), m.tolist(), m.reshape(-1)):
        with pytest.raises(ValueError):
            att(*ops, q_len=T, tree_mask=bad)
    q65 = ops[0][:1].expand(65, -1).contiguous()
    with pytest.raises(ValueError):  # more than 64 nodes
        att(q65, *[t[:1] if i > 2 else t for i, t in enumerate(ops)][1:], q_len=65, tree_mask=torch.ones((1, 65), dtype=torch.int64))
    with pytest.raises(ValueError):  # nothing defines a window together with a tree
        PrefillAttention(8, 2, 64, block_size=16, window=8)(*ops, q_len=T, tree_mask=m)


@pytest.mark.parametrize("entry", ENTRIES)
def test_rejections_before_the_device_is_touched_in_order(entry):
    """the tree entries' order with the wide mask: 2 q_len words per sequence, 8-byte alignment, q_len up to 64 and no limit on
    the rows (the descriptor: 2 sequences of 2 new tokens, mask rows 4 words apart; every call carries a defect)"""
    from squeezellm_amd import _lib

    lib, fp8 = _lib.load(), "fp8" in entry
    S = _lib.SqllmAttnTreeFp8 if fp8 else _lib.SqllmAttnTree
    assert _lib.SIGNATURES[entry] == [ctypes.POINTER(S), ctypes.c_void_p] and lib.sqllm_abi_version() == 1
    fn = getattr(lib, entry)
    nan = float("nan")
    rc = lambda **kw: fn(ctypes.byref(_desc(fp8, **{"mask_stride": 4, **kw})), None)  # noqa: E731
    assert fn(None, None) == E_NULL
    for name in ("q", "workspace", "tree_mask"):
        assert rc(**{name: None, "batch": 0, "mask_stride": 1, "scale": nan}) == E_NULL, name  # NULL comes first
    assert rc(q_lens=None, scale=nan) == E_OPTION  # q_lens may be NULL
    for kw in (dict(q_len=0), dict(batch=-1), dict(mask_stride=3), dict(mask_stride=-5), dict(q_len=65, batch=1, mask_stride=130), dict(batch=65536),
               dict(slot_stride=63), dict(mask_stride=1 << 61)):
        assert rc(scale=nan, out=TA.Q, tree_mask=MASK + 4, **kw) == E_SHAPE, kw  # ... before the scale, the overlap, the alignment
    assert rc(scale=nan, q_len=64, batch=2, mask_stride=128, out=MASK) == E_OPTION  # 128 rows are served: the scale is judged next
    # overlaps: the mask is (2 - 1) * 4 + 4 words, 32 bytes; an unaligned q stands behind them
    ws = _lib.attn_tree64_workspace_bytes(2, 2, 4, 64, 4, 16)
    for mine, size in (("out", 2048), ("workspace", ws)):
        assert rc(**{mine: MASK}) == E_SHAPE and rc(**{mine: MASK + 28, "q": TA.Q + 1}) == E_SHAPE and rc(**{mine: MASK - size + 4, "q": TA.Q + 1}) == E_SHAPE
        assert rc(**{mine: MASK + 32, "q": TA.Q + 1}) == E_ALIGN and rc(**{mine: MASK - size, "q": TA.Q + 1}) == E_ALIGN  # adjacent is fine
    assert rc(tree_mask=MASK + 4) == E_ALIGN and rc(tree_mask=MASK + 2) == E_ALIGN  # 8 bytes, not 4
    if fp8:  # the scales of the cache come last
        assert rc(k_scale=0.0) == E_OPTION and rc(k_scale=0.0, tree_mask=MASK + 4) == E_ALIGN


def test_workspace_bytes():
    from squeezellm_amd import _lib

    f = _lib.attn_tree64_workspace_bytes
    assert f(3, 64, 32, 128, 4, 16) == 3 * 64 * 32 * 1 * 130 * 4  # one partition: asked for all the same
    assert f(2, 33, 6, 64, (2 * P + 3 + 15) // 16, 16) == 2 * 33 * 6 * 3 * 66 * 4
    assert f(1, 1, 1, 64, P // 16 + 1, 16) == 2 * 66 * 4 and f(65535, 64, 8, 128, 1 << 20, 16) == 65535 * 64 * 8 * (1 << 16) * 130 * 4
    assert all(f(*a) == 0 for a in ((0, 1, 1, 64, 1, 16), (1, 0, 1, 64, 1, 16), (1, 1, 1, 64, 0, 16), (1, 1, 1, 64, 1, -1)))
    assert f(1 << 30, 1 << 30, 1 << 30, 128, 1 << 30, 1 << 30) == (1 << 63) - 1  # saturates, and the entries reject such a call
