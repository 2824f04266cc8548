"""sqllm_tree_accept and sqllm_kv_compact (include/sqllm_hip.h) on a host without a GPU: the symbols, the structs' layouts against
the C compiler's, every rejection with its code -- each returned before the device is touched (operand pointers are fake integers)
-- and the torch fallbacks of quant.tree_accept / quant.compact_kv against the loop references of tests/tree_accept_cases.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import tree_accept_cases as TA

E_SHAPE, E_NULL, E_ALIGN, E_OPTION = -2, -3, -4, -7
BASE = 0x100000  # fake operands, 64 KiB apart; the caches 16 MiB apart


def _accept(**kw):
    from squeezellm_amd import _lib

    a = _lib.SqllmTreeAccept()
    for i, name in enumerate(("parents", "tree_mask", "draft_tokens", "target_tokens", "q_lens", "seq_lens_in", "accept_len", "path", "next_token", "seq_lens_out")):
        setattr(a, name, BASE + i * 0x10000)
    a.stride, a.mask_stride, a.q_len, a.batch = 64, 128, 64, 4
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _compact(**kw):
    from squeezellm_amd import _lib

    c = _lib.SqllmKvCompact()
    caches = kw.pop("caches", [0x1000000 * (i + 1) for i in range(4)])
    if caches is not None:
        c._keep = (ctypes.c_void_p * 4)(*caches)
        c.caches = ctypes.cast(c._keep, ctypes.POINTER(ctypes.c_void_p))
    c.block_table, c.seq_lens, c.q_lens, c.path, c.accept_len = (BASE + i * 0x10000 for i in range(5))
    c.n_caches, c.elem_bytes, c.n_kv_heads, c.head_dim = 4, 2, 2, 64
    c.n_slots, c.block_size, c.max_blocks, c.table_stride, c.q_len, c.batch = 128, 16, 4, 4, 16, 2
    c.slot_stride, c.head_stride, c.path_stride = 128, 64, 16
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_symbols_and_struct_layouts_match_the_c_declarations(tmp_path):
    from squeezellm_amd import _lib

    lib = _lib.load()
    P = ctypes.POINTER
    assert _lib.SIGNATURES["sqllm_tree_accept"] == [P(_lib.SqllmTreeAccept), ctypes.c_void_p] and lib.sqllm_tree_accept.restype is ctypes.c_int
    assert _lib.SIGNATURES["sqllm_kv_compact"] == [P(_lib.SqllmKvCompact), ctypes.c_void_p] and lib.sqllm_kv_compact.restype is ctypes.c_int
    include = os.path.join(os.path.dirname(_lib.HERE), "include")
    assert f"#define SQLLM_KV_COMPACT_MAX_CACHES {_lib.KV_COMPACT_MAX_CACHES} " in open(os.path.join(include, "sqllm_hip.h")).read()
    assert lib.sqllm_abi_version() == 1  # symbols were added, nothing changed
    gcc = shutil.which("gcc")
    assert gcc, "the layouts are checked against the C compiler's"
    structs = (("sqllm_tree_accept_desc", _lib.SqllmTreeAccept), ("sqllm_kv_compact_desc", _lib.SqllmKvCompact))
    body = "".join(f'printf("%zu ", sizeof({c}));\n' + "".join(f'printf("%zu ", offsetof({c}, {n}));\n' for n, _ in S._fields_) for c, S in structs)
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "sqllm_hip.h"\nint main(void){{\n{body}return 0; }}\n')
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", f"-I{include}", str(src), "-o", str(tmp_path / "layout")], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [v for _, S in structs for v in (ctypes.sizeof(S), *(getattr(S, n).offset for n, _ in S._fields_))]


# every call carries at least one defect: nothing here may reach a launch.  A later defect is added to show the order.
REJECTIONS = [
    ("accept", None, E_NULL), ("compact", None, E_NULL),
    *[("accept", {name: None, "q_len": 0}, E_NULL) for name in ("parents", "tree_mask", "draft_tokens", "target_tokens", "accept_len", "path", "next_token")],
    ("accept", {"seq_lens_in": None, "batch": 0}, E_NULL), ("accept", {"seq_lens_out": None}, E_NULL),
    *[("accept", {k: v, "stride": 1, "tree_mask": BASE + 0x10004}, E_SHAPE) for k, v in (("q_len", 0), ("q_len", 65), ("batch", 0), ("batch", 65536))],
    ("accept", {"stride": 63, "path": BASE}, E_SHAPE), ("accept", {"mask_stride": 127}, E_SHAPE), ("accept", {"stride": 1 << 59}, E_SHAPE),
    ("accept", {"path": BASE + 4, "tree_mask": BASE + 0x10004}, E_SHAPE),  # an output inside parents, before the alignment
    ("accept", {"next_token": BASE + 6 * 0x10000 + 8}, E_SHAPE), ("accept", {"seq_lens_out": BASE + 5 * 0x10000 + 4}, E_SHAPE),
    ("accept", {"tree_mask": BASE + 0x10004}, E_ALIGN), ("accept", {"draft_tokens": BASE + 0x20002}, E_ALIGN),
    *[("compact", {name: None, "n_caches": 0}, E_NULL) for name in ("caches", "block_table", "seq_lens", "path", "accept_len")],
    ("compact", {"caches": [0x1000000, 0, 0x3000000, 0x4000000], "head_dim": 96}, E_NULL),
    *[("compact", {k: v, "elem_bytes": 3}, E_SHAPE) for k, v in (("n_caches", 0), ("n_caches", 257), ("n_kv_heads", 0), ("n_slots", 0), ("block_size", 0), ("max_blocks", 0),
                                                                  ("table_stride", 0), ("head_dim", 96), ("q_len", 0), ("q_len", 65), ("batch", 0), ("batch", 65536), ("max_blocks", 5))],
    ("compact", {"elem_bytes": 4, "slot_stride": 1}, E_OPTION), ("compact", {"elem_bytes": 0}, E_OPTION),
    *[("compact", {k: v, "caches": [0x1000000, 0x1000100, 0x3000000, 0x4000000]}, E_SHAPE) for k, v in (("slot_stride", 63), ("head_stride", 63), ("path_stride", 15), ("slot_stride", 1 << 32))],
    ("compact", {"caches": [0x1000000, 0x1000001 + 2 * 16383, 0x3000000, 0x4000000]}, E_SHAPE),  # the last element of one cache in the next, before the alignment
    ("compact", {"caches": [0x1000000, 0x2000000, 0x3000000, BASE + 0x30000 - 2 * 16384 + 2]}, E_SHAPE),  # a cache's last element is path's first word
    ("compact", {"caches": [0x1000000, 0x2000001, 0x3000000, 0x4000000]}, E_ALIGN), ("compact", {"seq_lens": BASE + 0x10002}, E_ALIGN),
]


@pytest.mark.parametrize("entry,defect,code", REJECTIONS)
def test_rejections_before_the_device_is_touched(entry, defect, code):
    from squeezellm_amd import _lib

    fn = getattr(_lib.load(), "sqllm_tree_accept" if entry == "accept" else "sqllm_kv_compact")
    desc = None if defect is None else (_accept if entry == "accept" else _compact)(**defect)
    assert fn(None if desc is None else ctypes.byref(desc), None) == code


def _signed(words):
    return [[w - (1 << 64) if w >> 63 else w for w in row] for row in words]


@pytest.mark.parametrize("tree", TA.TREES)
@pytest.mark.parametrize("T", TA.SIZES)
def test_torch_tree_accept_is_the_loop_reference(tree, T):
    from squeezellm_amd.quant import tree_accept

    par, words, draft, target, q_lens = TA.accept_batch(tree, T)
    seq = [300 + b for b in range(len(par))]
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
    got = tree_accept(i32(par), torch.tensor(_signed(words), dtype=torch.int64), i32(draft), i32(target), i32(q_lens), i32(seq))
    assert [g.tolist() for g in got] == list(TA.accept_ref(par, words, draft, target, q_lens, T, seq))
    with pytest.raises(RuntimeError):
        tree_accept(i32(par), torch.tensor(_signed(words), dtype=torch.int64), i32(draft), i32(target), route="kernel")  # no CPU kernel, no fallback


@pytest.mark.parametrize("kind,dtype", [("paged", torch.bfloat16), ("padded", torch.float8_e4m3fn), ("bhsd", torch.float16)])
def test_torch_compact_kv_is_the_loop_reference(kind, dtype):
    from squeezellm_amd.quant import compact_kv

    T, H, D = 64, 2, 64
    ctx, q_lens, alen, path = TA.compact_batch(T)
    seq = [c + n for c, n in zip(ctx, q_lens)]
    geo = bs, table, n_slots, ss, hs = TA.geometry(kind, len(seq), H, D, 320)
    n = 8 + (n_slots - 1) * ss + (H - 1) * hs + D + 8
    bufs = [torch.from_numpy(TA.pattern(n, c, 1 if dtype == torch.float8_e4m3fn else 2)) for c in range(2)]
    want = [b.numpy().copy() for b in bufs]
    TA.compact_ref(want, 8, geo, H, D, seq, q_lens, T, path, alen)
    views = [b.view(dtype).as_strided((n_slots, H, D), (ss, hs, 1), 8) for b in bufs]
    i32 = lambda x: torch.tensor(np.asarray(x), dtype=torch.int32)  # noqa: E731
    compact_kv(views, i32(table), i32(seq), T, i32(path), i32(alen), block_size=bs, q_lens=i32(q_lens))
    assert all(np.array_equal(b.numpy(), w) for b, w in zip(bufs, want))
    assert not np.array_equal(want[0], TA.pattern(n, 0, want[0].itemsize))  # something moved
