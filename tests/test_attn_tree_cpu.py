"""The tree-masked decode attention without a GPU (include/sqllm_hip.h, sqllm_attn_tree): the torch fallback on CPU tensors against
the fp64 oracle, quant.tree_masks, the module's ValueErrors, and the entries' rejections in order (operand pointers are fake)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import attn_decode_cases as C
from tests import attn_tree_cases as K
from tests import test_attn_append_capi_cpu as TA

E_SHAPE, E_NULL, E_ALIGN, E_OPTION = TA.E_SHAPE, TA.E_NULL, TA.E_ALIGN, TA.E_OPTION
MASK = 0x330000


def _module(base):
    from squeezellm_amd.quant import DecodeAttention

    return DecodeAttention(base.HQ, base.H, base.D, block_size=base.block_size)


def _operands(base, case):
    i32 = lambda a: torch.from_numpy(np.asarray(a)).to(torch.int32)  # noqa: E731
    return case.q_buf[:, :base.HQ * base.D], C.cache_view(base, base.k_buf), C.cache_view(base, base.v_buf), i32(base.table), i32(base.lens)


@pytest.mark.parametrize("tree,kind,D,hq,hk,dt", [("heap", "paged", 64, 8, 2, "fp16"), ("no_tree", "padded", 128, 6, 2, "bf16")])
def test_the_torch_fallback_against_the_oracle(tree, kind, D, hq, hk, dt):
    T = 5
    seqs = K.context_batches(T)[0]
    base, case = K.build(kind, T, D, hq, hk, dt, seqs)
    words = [K.words(tree, T)] * len(seqs)
    att = _module(base)
    got = att(*_operands(base, case), q_len=T, tree_mask=torch.tensor(words, dtype=torch.int64))
    assert att.last_route == "fallback" and got.shape == (len(seqs) * T, hq * D)
    want, gate = C.reference_of(K.as_decode_case(base, case, words))
    assert np.isfinite(want).all() and C.excess(got.double().numpy(), want, gate) <= 1.0
    assert not torch.equal(got, att(*_operands(base, case), q_len=T))  # (the chain is another function)


@pytest.mark.parametrize("tree", K.TREES[:3] + ("forest",))
def test_tree_masks(tree):
    from squeezellm_amd.quant import tree_masks

    T = 7
    par = [-1, 0, -1, 2, 2, 1, -1] if tree == "forest" else K.parents(tree, T)
    q_lens = [T, 6] if tree == "forest" else None  # (sequence 1: node 6 is padding)
    mask, depth = tree_masks(torch.tensor([par, par]), q_lens)
    want = [1, 3, 4, 12, 20, 35, 64] if tree == "forest" else K.words(tree, T)  # (the forest's closures, worked by hand)
    assert mask.dtype == depth.dtype == torch.int32 and mask[0].tolist() == want
    assert depth[0].tolist() == [bin(w).count("1") - 1 for w in want]
    pad = [T - 1] if q_lens else []
    assert [w for t, w in enumerate(mask[1].tolist()) if t not in pad] == [w for t, w in enumerate(want) if t not in pad]
    assert all(mask[1, t] == 0 and depth[1, t] == 0 for t in pad)
    for bad in ([[0, 0]], [[-1, 1]], [[-2, 0]], [[-1] * 17], [-1, 0]):
        with pytest.raises(ValueError):
            tree_masks(torch.tensor(bad))


def test_module_surface_value_errors():
    from squeezellm_amd.quant import DecodeAttention

    T = 5
    base, case = K.build("paged", T, 64, 8, 2, "fp16", (T, 9))
    ops = _operands(base, case)
    m = torch.tensor([K.words("star", T)] * 2, dtype=torch.int32)
    att = _module(base)
    for kw in (dict(tree_mask=m), dict(q_len=T, tree_mask=m[:1]), dict(q_len=T, tree_mask=m.float()), dict(q_len=T, tree_mask=m.tolist()),
               dict(q_len=T, tree_mask=m.reshape(-1))):
        with pytest.raises(ValueError):
            att(*ops, **kw)
    q17 = ops[0][:1].expand(17, -1).contiguous()
    with pytest.raises(ValueError):  # more than 16 nodes
        att(q17, *[t[:1] if i > 2 else t for i, t in enumerate(ops)][1:], q_len=17, tree_mask=torch.ones((1, 17), dtype=torch.int32))
    with pytest.raises(ValueError):  # nothing defines a window together with a tree
        DecodeAttention(8, 2, 64, block_size=16, window=8)(*ops, q_len=T, tree_mask=m)


def _desc(fp8, **kw):
    """the append tests' descriptor (2 sequences of 2 new tokens), with a mask of rows 2 words apart"""
    from squeezellm_amd import _lib

    a = _lib.SqllmAttnTreeFp8() if fp8 else _lib.SqllmAttnTree()
    src = TA._desc(fp8)
    for name, _ in type(src)._fields_:
        setattr(a, name, getattr(src, name))
    a.tree_mask, a.mask_stride = MASK, 2
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("entry", ["sqllm_attn_tree_f16", "sqllm_attn_tree_bf16", "sqllm_attn_tree_fp8_f16", "sqllm_attn_tree_fp8_bf16"])
def test_rejections_before_the_device_is_touched_in_order(entry):
    """the append entries' order, with the mask among the NULLs, the strides, the overlaps and the alignments (every call below
    carries at least one defect: nothing reaches a launch)"""
    from squeezellm_amd import _lib

    lib, fp8 = _lib.load(), "fp8" in entry
    S = _lib.SqllmAttnTreeFp8 if fp8 else _lib.SqllmAttnTree
    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "sqllm_hip.h")).read()
    assert _lib.SIGNATURES[entry] == [ctypes.POINTER(S), ctypes.c_void_p] and entry + "(" in header
    assert [n for n, _ in S._fields_][-4:] == ["q_lens", "q_len", "tree_mask", "mask_stride"] and S.tree_mask.offset == (160 if fp8 else 152) - 8
    fn = getattr(lib, entry)
    nan = float("nan")
    rc = lambda **kw: fn(ctypes.byref(_desc(fp8, **kw)), None)  # noqa: E731
    assert fn(None, None) == E_NULL
    for name in ("q", "workspace", "tree_mask"):
        assert rc(**{name: None, "batch": 0, "mask_stride": 1, "scale": nan}) == E_NULL, name  # NULL comes first
    assert rc(q_lens=None, scale=nan) == E_OPTION  # q_lens may be NULL
    for kw in (dict(q_len=0), dict(batch=-1), dict(mask_stride=1), dict(mask_stride=-5), dict(q_len=17, batch=1, mask_stride=17), dict(slot_stride=63),
               dict(mask_stride=1 << 61)):
        assert rc(scale=nan, out=TA.Q, tree_mask=MASK + 2, **kw) == E_SHAPE, kw  # ... before the scale, the overlap, the alignment
    assert rc(scale=nan, mask_stride=2, out=MASK) == E_OPTION and rc(scale=nan, mask_stride=1 << 40, out=MASK) == E_OPTION
    # overlaps: the mask is (2 - 1) * 2 + 2 words, 16 bytes; an unaligned q stands behind them
    ws = _lib.attn_decode_workspace_bytes(4, 4, 64, 4, 16)
    for mine, size in (("out", 2048), ("workspace", ws)):
        assert rc(**{mine: MASK}) == E_SHAPE and rc(**{mine: MASK + 12, "q": TA.Q + 1}) == E_SHAPE and rc(**{mine: MASK - size + 4, "q": TA.Q + 1}) == E_SHAPE
        assert rc(**{mine: MASK + 16, "q": TA.Q + 1}) == E_ALIGN and rc(**{mine: MASK - size, "q": TA.Q + 1}) == E_ALIGN  # adjacent is fine
    assert rc(mask_stride=6, out=MASK + 28) == E_SHAPE and rc(mask_stride=6, out=MASK + 32, q=TA.Q + 1) == E_ALIGN  # (6 + 2 words)
    assert rc(tree_mask=MASK + 2) == E_ALIGN and rc(tree_mask=MASK + 1) == E_ALIGN
    if fp8:  # the scales of the cache come last
        assert rc(k_scale=0.0) == E_OPTION and rc(k_scale=0.0, tree_mask=MASK + 2) == E_ALIGN
