"""C ABI of the decode attention for several new tokens per sequence (sqllm_attn_append_f16 / _bf16 / _fp8_f16 / _fp8_bf16,
include/sqllm_hip.h) on a host without a GPU: the symbols, the structs' layouts (from ctypes and from the C compiler), every
rejection in the documented order -- the sibling's, with q_len among the counts and the unserved shapes and q_lens among the
tensors out and the workspace must not overlap -- each returned before the device is touched (operand pointers are fake
integers: nothing dereferences them), and the launch hooks on the host layer alone: a missing kernel is an error."""
import ctypes
import os
import shutil
import subprocess

import pytest

from tests import helpers as H
from tests import test_attn_decode_capi_cpu as TA

E_SHAPE, E_NULL, E_ALIGN, E_OPTION = -2, -3, -4, -7
ENTRIES = ("sqllm_attn_append_f16", "sqllm_attn_append_bf16")
ENTRIES_FP8 = ("sqllm_attn_append_fp8_f16", "sqllm_attn_append_fp8_bf16")
Q, OUT, K_CACHE, V_CACHE, TABLE, LENS, WS = TA.Q, TA.OUT, TA.K_CACHE, TA.V_CACHE, TA.TABLE, TA.LENS, TA.WS
QLENS = 0x320000
# worked from the declarations (LP64): the sibling's fields at the sibling's offsets, then a pointer and an int32
LAYOUTS = {"sqllm_attn_append": (TA.FIELDS + ("q_lens", "q_len"), TA.OFFSETS + [128, 136], 144),
           "sqllm_attn_append_fp8": (TA.FIELDS + ("k_scale", "v_scale", "q_lens", "q_len"), TA.OFFSETS + [128, 132, 136, 144], 152)}


@pytest.fixture(scope="module")
def lib():
    from squeezellm_amd import _lib

    return _lib.load()


def _desc(fp8=False, **kw):
    """2 sequences of 2 new tokens (4 rows), 4 query heads over 2 kv heads of 64, a paged cache of 8 blocks of 16 slots"""
    from squeezellm_amd import _lib

    a = _lib.SqllmAttnAppendFp8() if fp8 else _lib.SqllmAttnAppend()
    a.q, a.out, a.k_cache, a.v_cache, a.block_table, a.seq_lens, a.workspace = Q, OUT, K_CACHE, V_CACHE, TABLE, LENS, WS
    a.q_lens, a.q_len = QLENS, 2
    a.batch, a.n_q_heads, a.n_kv_heads, a.head_dim = 2, 4, 2, 64
    a.n_slots, a.block_size, a.max_blocks, a.table_stride = 128, 16, 4, 4
    a.slot_stride, a.head_stride, a.q_stride, a.out_stride = 128, 64, 256, 256
    a.scale = 0.125
    if fp8:
        a.k_scale, a.v_scale = 0.5, 4.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbols_signatures_and_header_text(lib):
    from squeezellm_amd import _lib

    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "sqllm_hip.h")).read()
    P = ctypes.POINTER
    for names, S in ((ENTRIES, _lib.SqllmAttnAppend), (ENTRIES_FP8, _lib.SqllmAttnAppendFp8)):
        for name in names:
            assert hasattr(lib, name) and name + "(" in header
            assert _lib.SIGNATURES[name] == [P(S), ctypes.c_void_p] and getattr(lib, name).restype is ctypes.c_int
    assert "typedef struct sqllm_attn_append {" in header and "typedef struct sqllm_attn_append_fp8 {" in header
    assert lib.sqllm_abi_version() == 1  # symbols were added, nothing changed
    for text in ("L(b,t) = seq_lens[b] - (n_b - 1 - t)", "EXACTLY THE BITS", "ONE table row per sequence", "INCLUDING all its new tokens",
                 "makes NaN only the tokens with L > p", "Rows t >= n_b are padding and are +0", "n_b < 0 is treated as 0",
                 "n_b > T makes all T rows of the sequence NaN", "sqllm_attn_decode_workspace_bytes(batch*q_len, ...)",
                 "q_len 1 to 16; batch*q_len <= 64", "prompt-length prefill stays"):
        assert text in header, text


def test_ctypes_structures_match_the_c_declarations(tmp_path):
    from squeezellm_amd import _lib

    for cname, S in (("sqllm_attn_append", _lib.SqllmAttnAppend), ("sqllm_attn_append_fp8", _lib.SqllmAttnAppendFp8)):
        fields, offsets, size = LAYOUTS[cname]
        assert [n for n, _ in S._fields_] == list(fields)
        assert [getattr(S, n).offset for n in fields] == offsets and ctypes.sizeof(S) == size
        gcc = shutil.which("gcc")
        if gcc:  # ... and from the C compiler, where there is one
            include = os.path.join(os.path.dirname(_lib.HERE), "include")
            c = tmp_path / f"{cname}.c"
            c.write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "sqllm_hip.h"\nint main(void){{ printf("%zu", sizeof({cname}));\n'
                         + "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n in fields) + "return 0; }\n")
            exe = tmp_path / cname
            subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", f"-I{include}", str(c), "-o", str(exe)], check=True)
            assert [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()] == [size, *offsets]


@pytest.mark.parametrize("entry", ENTRIES + ENTRIES_FP8)
def test_rejections_before_the_device_is_touched_in_order(lib, entry):
    from squeezellm_amd import _lib

    fn = getattr(lib, entry)
    fp8 = "fp8" in entry
    celem = 1 if fp8 else 2

    def rc(**kw):
        return fn(ctypes.byref(_desc(fp8, **kw)), None)

    # (nothing here may reach a launch: every call below carries at least one defect)
    assert fn(None, None) == E_NULL
    for name in ("q", "out", "k_cache", "v_cache", "block_table", "seq_lens", "workspace"):
        assert rc(**{name: None}) == E_NULL, name
        assert rc(**{name: None, "batch": 0, "q_len": 0, "scale": float("nan")}) == E_NULL  # NULL comes first
    assert rc(q_lens=None, scale=float("nan")) == E_OPTION  # q_lens may be NULL: the call gets as far as the scale
    # counts < 1, q_len among them
    for name in ("batch", "n_q_heads", "n_kv_heads", "head_dim", "n_slots", "block_size", "max_blocks", "table_stride", "q_len"):
        for v in (0, -1):
            assert rc(**{name: v}) == E_SHAPE, name
            assert rc(**{name: v, "scale": float("inf"), "out": Q, "q": Q + 1}) == E_SHAPE  # ... before the scale, the overlap, the alignment
    assert rc(slot_stride=63) == E_SHAPE and rc(head_stride=63) == E_SHAPE and rc(q_stride=255) == E_SHAPE and rc(out_stride=255) == E_SHAPE
    assert rc(max_blocks=5) == E_SHAPE  # > table_stride
    assert rc(max_blocks=5, table_stride=5, scale=float("nan")) == E_OPTION
    # what the kernels serve: the sibling's shapes, q_len 1 to 16, batch * q_len <= 64
    for kw in (dict(head_dim=32, q_stride=128, out_stride=128), dict(n_q_heads=3, n_kv_heads=2), dict(n_q_heads=18, n_kv_heads=2, q_stride=18 * 64, out_stride=18 * 64),
               dict(q_len=17, batch=1), dict(q_len=17, batch=3), dict(q_len=16, batch=5), dict(q_len=2, batch=33), dict(q_len=1, batch=65),
               dict(q_len=(1 << 31) - 1, batch=(1 << 31) - 1)):
        assert rc(**kw) == E_SHAPE, kw
        assert rc(scale=float("nan"), **kw) == E_SHAPE, kw
    for kw in (dict(q_len=16, batch=4), dict(q_len=16, batch=1), dict(q_len=1, batch=64), dict(q_len=2, batch=32), dict(q_len=5, batch=12),
               dict(n_q_heads=16, n_kv_heads=2, q_stride=1024, out_stride=1024), dict(block_size=5)):
        assert rc(scale=float("nan"), **kw) == E_OPTION, kw  # served: the call gets as far as the scale
    # the stride / extent limits of sqllm_kv_cache
    far = dict(k_cache=0x10000000000, v_cache=0x7000000000000)
    assert rc(slot_stride=(1 << 32) - 1, scale=float("nan"), **far) == E_OPTION
    assert rc(slot_stride=1 << 32, scale=float("nan"), **far) == E_SHAPE and rc(head_stride=1 << 32, scale=float("nan"), **far) == E_SHAPE
    assert rc(q_stride=1 << 62, scale=float("nan")) == E_SHAPE and rc(out_stride=1 << 62, scale=float("nan")) == E_SHAPE
    # the scale
    for v in (float("nan"), float("inf"), float("-inf")):
        assert rc(scale=v) == E_OPTION and rc(scale=v, out=Q, q=Q + 1) == E_OPTION  # ... before the overlap and the alignment
    # overlaps: out (4 rows of 256 elements: 2048 bytes) and the workspace (of 4 rows) against every input, q_lens included, and
    # each other; an unaligned q stands behind them
    ws = _lib.attn_decode_workspace_bytes(4, 4, 64, 4, 16)
    assert ws == 2 * _lib.attn_decode_workspace_bytes(2, 4, 64, 4, 16)
    cache = celem * (127 * 128 + 64 + 64)
    inputs = {"q": (Q, 2048), "k_cache": (K_CACHE, cache), "v_cache": (V_CACHE, cache), "block_table": (TABLE, 32), "seq_lens": (LENS, 8),
              "q_lens": (QLENS, 8)}
    for name, (at, size) in inputs.items():
        for mine, my_size in (("out", 2048), ("workspace", ws)):
            q_odd = {} if name == "q" else {"q": Q + 1}
            assert rc(**{mine: at}) == E_SHAPE, (mine, name)
            assert rc(**{mine: at + size - 2, **q_odd}) == E_SHAPE and rc(**{mine: at - my_size + 2, **q_odd}) == E_SHAPE
            if q_odd:
                assert rc(**{mine: at + size + (-size) % 4, **q_odd}) == E_ALIGN  # adjacent is fine
                assert rc(**{mine: at - my_size - (-my_size) % 4 - 4, **q_odd}) == E_ALIGN
    assert rc(out=QLENS, q_lens=None, q=Q + 1) == E_ALIGN  # no q_lens: nothing there to overlap
    assert rc(out=WS) == E_SHAPE and rc(out=WS + ws - 2, q=Q + 1) == E_SHAPE and rc(out=WS + ws, q=Q + 1) == E_ALIGN
    assert rc(workspace=OUT + 2046, q=Q + 1) == E_SHAPE and rc(workspace=OUT + 2048, q=Q + 1) == E_ALIGN  # out has batch * q_len rows
    # alignment, last of the sibling's
    for name in ("q", "out"):
        assert rc(**{name: getattr(_desc(), name) + 1}) == E_ALIGN, name
    assert rc(workspace=WS + 2) == E_ALIGN
    if fp8:
        assert rc(k_cache=K_CACHE + 1, v_cache=V_CACHE + 3, k_scale=0.0) == E_OPTION  # (admitted: the scales speak)
        for s in (0.0, -1.0, float("nan"), float("inf"), 1e-39):
            assert rc(k_scale=s) == E_OPTION and rc(v_scale=s) == E_OPTION, s
            assert rc(k_scale=s, q=Q + 1) == E_ALIGN  # ... behind the alignment
        assert rc(scale=3e38, k_scale=16.0) == E_OPTION
    else:
        assert rc(k_cache=K_CACHE + 1) == E_ALIGN and rc(v_cache=V_CACHE + 1) == E_ALIGN


def test_the_sources_are_part_of_the_product_build():
    from squeezellm_amd import build as B

    for src in ("sqllm_attn_append.hip", "sqllm_attn_append_fp8.hip"):
        assert src in B.SOURCES and B.SOURCES.index(src) < B.SOURCES.index("sqllm_capi.hip")
    assert B.SOURCES[-1] == "sqllm_capi.hip"
    assert os.path.join(B.CSRC, "sqllm_attn.h") in B.HEADERS  # (a changed header makes the library stale)


def test_launch_hooks_on_the_host_layer_alone(tmp_path):
    """a missing kernel is an error, not a fallback; each of the eight entries (the four here, the four one-query ones) reaches the
    slot of its own kind and no other, with the tokens' fields"""
    from squeezellm_amd import build as B

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found: the host layer cannot be built alone")
    native = os.path.join(H.ROOT, "tests", "native")
    exe = str(tmp_path / "attn_hooks")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-DSQLLM_RECORDER_NO_MAIN", f"-I{B.INCLUDE}", f"-I{B.CSRC}",
                        os.path.join(B.CSRC, "sqllm_capi.hip"), os.path.join(native, "launch_recorder.cpp"),
                        os.path.join(native, "attn_hooks.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = {ln.split()[0]: dict(kv.split("=") for kv in ln.split()[1:]) for ln in out.stdout.splitlines()}
    ns = lines["nohook"]["notsupported"]
    assert int(ns) != 0 and all(lines["nohook"][k] == ns for k in ("f16", "bf16", "fp8_f16", "fp8_bf16"))
    assert lines["half"] == {"notsupported": ns, "f16": "0", "fp8_f16": ns, "calls": "1,0"}  # one source left out: its entries fail
    common = dict(rc="0", batch="2", q_len="3", q_lens="320000", n_parts="3", capacity="640", out_stride="260")
    assert lines["f16"] == dict(common, calls="1,0", bf16="0", scale="0.125", v_scale="1")
    assert lines["bf16"] == dict(common, calls="2,0", bf16="1", scale="0.125", v_scale="1")
    assert lines["fp8_f16"] == dict(common, calls="2,1", bf16="0", scale="0.0625", v_scale="4")
    assert lines["fp8_bf16"] == dict(common, calls="2,2", bf16="1", scale="0.0625", v_scale="4")
    assert lines["null_q_lens"] == dict(common, calls="3,2", bf16="0", scale="0.125", v_scale="1", q_len="1", q_lens="0")
    # the four one-query entries: the same steps on their own two slots
    assert lines["nohook_decode"] == {"notsupported": ns, "f16": ns, "bf16": ns, "fp8_f16": ns, "fp8_bf16": ns}
    # exactly one slot filled, each in turn: its f16 and bf16 entry succeed, the other six fail, and only that slot is called
    entries = ("decode_f16", "decode_bf16", "decode_fp8_f16", "decode_fp8_bf16", "append_f16", "append_bf16", "append_fp8_f16", "append_fp8_bf16")
    for k, slot in enumerate(("decode", "decode_fp8", "append", "append_fp8")):
        want = {e: ("0" if e.rsplit("_", 1)[0] == slot else ns) for e in entries}
        assert lines["only_" + slot] == dict(want, notsupported=ns, calls=",".join("2" if i == k else "0" for i in range(4))), slot
    one = dict(common, q_len="0", q_lens="0")  # (no tokens: q_len 0 names the one-query kernels)
    assert lines["decode_f16"] == dict(one, calls="1,0", bf16="0", scale="0.125", v_scale="1")
    assert lines["decode_bf16"] == dict(one, calls="2,0", bf16="1", scale="0.125", v_scale="1")
    assert lines["decode_fp8_f16"] == dict(one, calls="2,1", bf16="0", scale="0.0625", v_scale="4")
    assert lines["decode_fp8_bf16"] == dict(one, calls="2,2", bf16="1", scale="0.0625", v_scale="4")
    assert lines["slots"] == {"decode": "2", "decode_fp8": "2", "append": "3", "append_fp8": "2"}  # nine calls, each in its own slot
