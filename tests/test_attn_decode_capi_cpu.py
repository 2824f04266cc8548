"""C ABI of the decode attention (sqllm_attn_decode_f16 / _bf16, include/sqllm_hip.h) on a host without a GPU: the symbols, the
struct's layout, and every rejection the header lists, in its order -- each returned before the device is touched (operand
pointers are fake integers: nothing dereferences them)."""
import ctypes
import os
import shutil
import subprocess

import pytest

E_SHAPE, E_NULL, E_ALIGN, E_OPTION = -2, -3, -4, -7
FIELDS = ("q", "out", "k_cache", "v_cache", "block_table", "seq_lens", "batch", "n_q_heads", "n_kv_heads", "head_dim", "n_slots",
          "block_size", "max_blocks", "table_stride", "slot_stride", "head_stride", "q_stride", "out_stride", "scale", "workspace")
# worked from the declaration (LP64): six pointers, eight int32, four int64, a float padded to the next pointer
OFFSETS = [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 68, 72, 76, 80, 88, 96, 104, 112, 120]
SIZE = 128
ENTRIES = ("sqllm_attn_decode_f16", "sqllm_attn_decode_bf16")
Q, OUT, K_CACHE, V_CACHE, TABLE, LENS, WS = 0x100000, 0x200000, 0x800000, 0x900000, 0x300000, 0x310000, 0x400000


@pytest.fixture(scope="module")
def lib():
    from squeezellm_amd import _lib

    return _lib.load()


def _desc(**kw):
    """2 rows, 4 query heads over 2 kv heads of 64, a paged cache of 8 blocks of 16 slots, 4 blocks per row"""
    from squeezellm_amd import _lib

    a = _lib.SqllmAttnDecode()
    a.q, a.out, a.k_cache, a.v_cache, a.block_table, a.seq_lens, a.workspace = Q, OUT, K_CACHE, V_CACHE, TABLE, LENS, WS
    a.batch, a.n_q_heads, a.n_kv_heads, a.head_dim = 2, 4, 2, 64
    a.n_slots, a.block_size, a.max_blocks, a.table_stride = 128, 16, 4, 4
    a.slot_stride, a.head_stride, a.q_stride, a.out_stride = 128, 64, 256, 256
    a.scale = 0.125
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbols_signatures_and_header_text(lib):
    from squeezellm_amd import _lib

    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "sqllm_hip.h")).read()
    for name in ENTRIES + ("sqllm_attn_decode_workspace_bytes",):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header
    P = ctypes.POINTER
    assert _lib.SIGNATURES[ENTRIES[0]] == _lib.SIGNATURES[ENTRIES[1]] == [P(_lib.SqllmAttnDecode), ctypes.c_void_p]
    assert _lib.SIGNATURES["sqllm_attn_decode_workspace_bytes"] == [ctypes.c_int32] * 5
    assert lib.sqllm_attn_decode_f16.restype is ctypes.c_int and lib.sqllm_attn_decode_workspace_bytes.restype is ctypes.c_int64
    assert "typedef struct sqllm_attn_decode {" in header and "#define SQLLM_ABI_VERSION 1" in header
    assert f"#define SQLLM_ATTN_PARTITION {_lib.ATTN_PARTITION}\n" in header
    # the contract, in the header's words
    for text in ("block_table[b, p / block_size] * block_size + p % block_size", "block_size = S, max_blocks = 1, block_table[b, 0] = b * H",
                 "not only a power of two", "rounded ONCE to the output type", "not of the other rows, not of the batch size, not of timing",
                 "combined in ascending partition order", "never on device data", "NaN included, the output bits are the same",
                 "Nothing outside the cache extent is ever read", "seq_lens[b] <= 0: the row of out is +0",
                 "seq_lens[b] > max_blocks * block_size", "outside [0, n_slots)", "makes that head's outputs NaN",
                 "of the heads of that kv group NaN", "are not pinned further", "CONTENTS IRRELEVANT",
                 "TWO kernel nodes (partials, then combine), ONE when"):
        assert text in header, text
    assert lib.sqllm_abi_version() == 1  # symbols were added, nothing changed


def test_ctypes_structure_matches_the_c_declaration(tmp_path):
    from squeezellm_amd import _lib

    S = _lib.SqllmAttnDecode
    assert [n for n, _ in S._fields_] == list(FIELDS)
    assert [getattr(S, n).offset for n in FIELDS] == OFFSETS and ctypes.sizeof(S) == SIZE
    gcc = shutil.which("gcc")
    if gcc:  # ... and from the C compiler, where there is one
        include = os.path.join(os.path.dirname(_lib.HERE), "include")
        c = tmp_path / "layout.c"
        c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sqllm_hip.h"\nint main(void){ printf("%zu", sizeof(sqllm_attn_decode));\n'
                     + "".join(f'printf(" %zu", offsetof(sqllm_attn_decode, {n}));\n' for n in FIELDS) + "return 0; }\n")
        exe = tmp_path / "layout"
        subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", f"-I{include}", str(c), "-o", str(exe)], check=True)
        got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
        assert got == [SIZE, *OFFSETS]


def test_workspace_bytes_positive_and_monotone(lib):
    from squeezellm_amd import _lib

    w = _lib.attn_decode_workspace_bytes
    P = _lib.ATTN_PARTITION
    assert w(1, 1, 64, 1, 1) == (64 + 2) * 4 > 0
    assert w(2, 4, 64, 4, 16) == 2 * 4 * 1 * 66 * 4  # 64 keys: one partition
    assert w(2, 4, 64, 17, 16) == 2 * 4 * 2 * 66 * 4  # 272 keys: two
    assert w(1, 32, 128, 1, 4096) == 32 * (4096 // P) * 130 * 4
    base = (3, 8, 64, 40, 16)
    for i in range(5):
        prev = 0
        for f in (1, 2, 3, 5):
            args = list(base)
            args[i] *= f if i != 2 else 1
            if i == 2:
                args[2] = (64, 64, 128, 128)[(1, 2, 3, 5).index(f)]
            cur = w(*args)
            assert cur >= prev > -1 and cur > 0
            prev = cur
    assert w(1, 1, 64, (1 << 31) - 1, (1 << 31) - 1) > 0  # a capacity beyond int32 is clipped, the size does not wrap
    assert w(0, 1, 64, 1, 1) == 0 and w(1, 1, 64, 0, 16) == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_rejections_before_the_device_is_touched_in_order(lib, entry):
    fn = getattr(lib, entry)

    def rc(**kw):
        return fn(ctypes.byref(_desc(**kw)), None)

    # (nothing here may reach a launch: the operands are fake, and on a host with a GPU a launch would run a kernel on them --
    # every call below carries at least one defect)
    assert fn(None, None) == E_NULL
    for name in ("q", "out", "k_cache", "v_cache", "block_table", "seq_lens", "workspace"):
        assert rc(**{name: None}) == E_NULL, name
        assert rc(**{name: None, "batch": 0, "scale": float("nan"), "q": None if name == "q" else Q + 1}) == E_NULL  # NULL comes first
    # counts < 1
    for name in ("batch", "n_q_heads", "n_kv_heads", "head_dim", "n_slots", "block_size", "max_blocks", "table_stride"):
        for v in (0, -1):
            assert rc(**{name: v}) == E_SHAPE, name
            assert rc(**{name: v, "scale": float("inf"), "out": Q, "q": Q + 1}) == E_SHAPE  # ... before the scale, the overlap, the alignment
    # strides
    assert rc(slot_stride=63) == E_SHAPE and rc(head_stride=63) == E_SHAPE and rc(head_stride=0) == E_SHAPE and rc(slot_stride=-128) == E_SHAPE
    assert rc(q_stride=255) == E_SHAPE and rc(out_stride=255) == E_SHAPE and rc(q_stride=64) == E_SHAPE
    assert rc(max_blocks=5) == E_SHAPE  # > table_stride
    assert rc(max_blocks=5, table_stride=5, scale=float("nan")) == E_OPTION  # (fits now: the next check speaks)
    # what the kernel serves
    for kw in (dict(head_dim=32, q_stride=128, out_stride=128), dict(head_dim=256, slot_stride=512, head_stride=256, q_stride=1024, out_stride=1024),
               dict(head_dim=96, slot_stride=192, head_stride=96, q_stride=384, out_stride=384), dict(n_q_heads=3, n_kv_heads=2),
               dict(n_q_heads=18, n_kv_heads=2, q_stride=18 * 64, out_stride=18 * 64), dict(n_q_heads=2, n_kv_heads=4), dict(batch=65)):
        assert rc(**kw) == E_SHAPE, kw
        assert rc(scale=float("nan"), **kw) == E_SHAPE, kw
    for kw in (dict(head_dim=128, slot_stride=256, head_stride=128, q_stride=512, out_stride=512), dict(n_q_heads=16, n_kv_heads=2, q_stride=1024, out_stride=1024),
               dict(n_q_heads=2, n_kv_heads=2), dict(batch=64), dict(block_size=5), dict(block_size=4099, n_slots=1 << 20)):
        assert rc(scale=float("nan"), **kw) == E_OPTION, kw  # served: the call gets as far as the scale
    # the stride / extent limits of sqllm_kv_cache
    far = dict(k_cache=0x10000000000, v_cache=0x7000000000000)
    assert rc(slot_stride=(1 << 32) - 1, scale=float("nan"), **far) == E_OPTION
    assert rc(slot_stride=1 << 32, scale=float("nan"), **far) == E_SHAPE
    assert rc(head_stride=1 << 32, scale=float("nan"), **far) == E_SHAPE
    assert rc(slot_stride=1 << 40, n_slots=1, scale=float("nan"), **far) == E_OPTION  # one slot: never multiplied
    assert rc(head_stride=1 << 62, n_slots=1, n_kv_heads=1, n_q_heads=4, scale=float("nan"), **far) == E_OPTION
    assert rc(q_stride=1 << 62, scale=float("nan")) == E_SHAPE and rc(out_stride=1 << 62, scale=float("nan")) == E_SHAPE
    # the scale
    for v in (float("nan"), float("inf"), float("-inf")):
        assert rc(scale=v) == E_OPTION
        assert rc(scale=v, out=Q, q=Q + 1) == E_OPTION  # ... before the overlap and the alignment
    # overlaps: out (2 rows of 256 elements: 1024 bytes) and the workspace against every input and each other; an unaligned q
    # stands behind them (SQLLM_E_ALIGN is what an admitted overlap candidate comes back with)
    from squeezellm_amd import _lib

    ws = _lib.attn_decode_workspace_bytes(2, 4, 64, 4, 16)
    cache = 2 * (127 * 128 + 64 + 64)
    inputs = {"q": (Q, 1024), "k_cache": (K_CACHE, cache), "v_cache": (V_CACHE, cache), "block_table": (TABLE, 32), "seq_lens": (LENS, 8)}
    for name, (at, size) in inputs.items():
        for mine, my_size in (("out", 1024), ("workspace", ws)):
            q_odd = {} if name == "q" else {"q": Q + 1}
            odd = E_ALIGN if q_odd else None
            assert rc(**{mine: at}) == E_SHAPE, (mine, name)
            assert rc(**{mine: at + size - 2, **q_odd}) == E_SHAPE
            assert rc(**{mine: at - my_size + 2, **q_odd}) == E_SHAPE
            if odd:
                assert rc(**{mine: at + size + (-size) % 4, **q_odd}) == odd  # adjacent is fine
                assert rc(**{mine: at - my_size - (-my_size) % 4 - 4, **q_odd}) == odd
    assert rc(out=WS) == E_SHAPE and rc(out=WS + ws - 2, q=Q + 1) == E_SHAPE and rc(out=WS - 1022, q=Q + 1) == E_SHAPE
    assert rc(out=WS + ws, q=Q + 1) == E_ALIGN and rc(out=WS - 1024, q=Q + 1) == E_ALIGN
    # strided rows widen q's and out's extents; the table's follows table_stride
    assert rc(out_stride=512, workspace=OUT + 1534, q=Q + 1) == E_SHAPE and rc(out_stride=512, workspace=OUT + 1536, q=Q + 1) == E_ALIGN
    assert rc(table_stride=100, out=TABLE + 4 * 104 - 2, q=Q + 1) == E_SHAPE and rc(table_stride=100, out=TABLE + 4 * 104, q=Q + 1) == E_ALIGN
    # alignment, last
    for name in ("q", "out", "k_cache", "v_cache"):
        assert rc(**{name: getattr(_desc(), name) + 1}) == E_ALIGN, name
    assert rc(workspace=WS + 2) == E_ALIGN and rc(workspace=WS + 1) == E_ALIGN


def test_the_source_is_part_of_the_product_build():
    from squeezellm_amd import build as B

    assert "sqllm_attn_decode.hip" in B.SOURCES and B.SOURCES.index("sqllm_attn_decode.hip") < B.SOURCES.index("sqllm_capi.hip")
    assert B.SOURCES[-1] == "sqllm_capi.hip"
