"""C ABI of the attention front that writes k and v into the KV cache (sqllm_qkv_rope_cache_* / sqllm_qkv_rope_norm_cache_*,
include/sqllm_hip.h) on a host without a GPU: the symbols, the struct's layout, and every rejection the header lists -- each
returned before the device is touched (operand pointers are fake 16-byte-aligned integers: nothing dereferences them)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from tests.test_qkv_rope_capi_cpu import _qkv

E_BITS, E_SHAPE, E_NULL, E_ALIGN, E_SPARSE, E_BATCH, E_OPTION, E_GROUP = -1, -2, -3, -4, -5, -6, -7, -8
FIELDS = ("k_cache", "v_cache", "slots", "n_slots", "slot_stride", "head_stride")
# worked from the declaration (LP64): three pointers, an int32 padded to the next int64, two int64
OFFSETS = [0, 8, 16, 24, 32, 40]
SIZE = 48
PLAIN = ("sqllm_qkv_rope_cache_f16", "sqllm_qkv_rope_cache_bf16")
NORM = ("sqllm_qkv_rope_norm_cache_f16", "sqllm_qkv_rope_norm_cache_bf16")
K_CACHE, V_CACHE = 0x800000, 0x900000


@pytest.fixture(scope="module")
def lib():
    from squeezellm_amd import _lib

    return _lib.load()


def _cache(n_slots=4, H=2, D=64):
    """slot-major [n_slots, H, D] for _qkv()'s k and v (128 wide, head_dim 64): an extent of n_slots * 256 bytes"""
    from squeezellm_amd import _lib

    c = _lib.SqllmKvCache()
    c.k_cache, c.v_cache, c.slots = K_CACHE, V_CACHE, 0x230000
    c.n_slots, c.slot_stride, c.head_stride = n_slots, H * D, D
    return c


def _call(lib, entry, r, c):
    from squeezellm_amd import _lib

    fn = getattr(lib, entry)
    if entry in NORM:
        nm = _lib.SqllmRmsNorm(weight=0x300000, eps=1e-6)
        return fn(ctypes.byref(r), ctypes.byref(nm), ctypes.byref(c) if c is not None else None, None)
    return fn(ctypes.byref(r), ctypes.byref(c) if c is not None else None, None)


def test_symbols_signatures_and_header_text(lib):
    from squeezellm_amd import _lib

    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "sqllm_hip.h")).read()
    for name in PLAIN + NORM:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header
        assert getattr(lib, name).restype is ctypes.c_int
    P = ctypes.POINTER
    assert _lib.SIGNATURES[PLAIN[0]] == _lib.SIGNATURES[PLAIN[1]] == [P(_lib.SqllmQkvRope), P(_lib.SqllmKvCache), ctypes.c_void_p]
    assert _lib.SIGNATURES[NORM[0]] == _lib.SIGNATURES[NORM[1]] == [P(_lib.SqllmQkvRope), P(_lib.SqllmRmsNorm), P(_lib.SqllmKvCache),
                                                                   ctypes.c_void_p]
    assert "typedef struct sqllm_kv_cache {" in header and "#define SQLLM_ABI_VERSION 1" in header
    # the contract, in the header's words
    for text in ("stored with the SAME BITS at k_cache[s * slot_stride + h * head_stride + d]", "Offsets are 64-bit",
                 "out_k and out_v may each be NULL in these four entries", "nothing of row b is written to", "Duplicate slots",
                 "slot_stride = H*D, head_stride = D", "slot = b*H*S + p, slot_stride = D", "n_slots = (B-1)*H*S + S",
                 "(n_slots-1)*slot_stride + (H-1)*head_stride + head_dim"):
        assert text in header, text
    assert lib.sqllm_abi_version() == 1  # symbols were added, nothing changed


def test_ctypes_structure_matches_the_c_declaration(tmp_path):
    from squeezellm_amd import _lib

    S = _lib.SqllmKvCache
    assert [n for n, _ in S._fields_] == list(FIELDS)
    assert [getattr(S, n).offset for n in FIELDS] == OFFSETS and ctypes.sizeof(S) == SIZE
    assert S.n_slots.size == 4 and S.slot_stride.size == S.head_stride.size == 8
    gcc = shutil.which("gcc")
    if gcc:  # ... and from the C compiler, where there is one
        include = os.path.join(os.path.dirname(_lib.HERE), "include")
        c = tmp_path / "layout.c"
        c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sqllm_hip.h"\nint main(void){ printf("%zu", sizeof(sqllm_kv_cache));\n'
                     + "".join(f'printf(" %zu", offsetof(sqllm_kv_cache, {n}));\n' for n in FIELDS) + "return 0; }\n")
        exe = tmp_path / "layout"
        subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", f"-I{include}", str(c), "-o", str(exe)], check=True)
        got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
        assert got == [SIZE, *OFFSETS]


@pytest.mark.parametrize("entry", PLAIN + NORM)
def test_rejections_before_the_device_is_touched(lib, entry):
    from squeezellm_amd import _lib

    def rc(edit_r=lambda r: None, edit_c=lambda c: None, cache=True, **kw):
        r, c = _qkv(**kw), _cache()
        edit_r(r)
        edit_c(c)
        return _call(lib, entry, r, c if cache else None)

    def passes(edit_r=lambda r: None, edit_c=lambda c: None, **kw):
        """the edit is NOT rejected by the checks of this entry point, the cache's included: with q's qweight taken away as
        well, the call gets as far as the linear's own validation, which runs behind them, and comes back with ITS code.
        (Nothing here may reach a launch: the operands are fake, and on a host with a GPU a launch would run a kernel on them.)"""
        def no_qweight(r):
            edit_r(r)
            r.q.qweight = None
        return rc(no_qweight, edit_c, **kw) == E_NULL

    # the parent's own rejections come first, in its order: a cache descriptor that is itself to be rejected does not show
    if entry in PLAIN:
        assert getattr(lib, entry)(None, ctypes.byref(_cache()), None) == E_NULL
    else:
        assert getattr(lib, entry)(None, ctypes.byref(_lib.SqllmRmsNorm(weight=0x300000, eps=1e-6)), ctypes.byref(_cache()), None) == E_NULL
        assert getattr(lib, entry)(ctypes.byref(_qkv()), None, ctypes.byref(_cache()), None) == E_NULL
        assert getattr(lib, entry)(ctypes.byref(_qkv()), ctypes.byref(_lib.SqllmRmsNorm(weight=0x300000, eps=-1.0)), None, None) == E_OPTION
    broken = lambda c: setattr(c, "n_slots", 0)  # (SQLLM_E_SHAPE, were it looked at)
    no_slots = lambda c: setattr(c, "slots", None)  # (SQLLM_E_NULL)
    for m in "qkv":
        assert rc(lambda r: setattr(getattr(r, m), "mul", 0x5000), broken) == E_GROUP
    assert rc(lambda r: setattr(r.k, "K", 256), broken) == E_GROUP
    assert rc(lambda r: setattr(r, "layout", 2), broken) == E_OPTION
    for name in ("out_q", "cos", "sin", "positions", "workspace"):
        assert rc(lambda r: setattr(r, name, None), broken) == E_NULL, name
    assert rc(lambda r: setattr(r, "workspace", 0x400008), broken) == E_ALIGN
    assert rc(lambda r: setattr(r, "head_dim", 63), no_slots) == E_SHAPE
    assert rc(lambda r: setattr(r, "n_pos", 0), no_slots) == E_SHAPE
    assert rc(lambda r: setattr(r, "out_k", r.out_q + 510), no_slots) == E_SHAPE
    assert rc(lambda r: setattr(r, "out_v", r.workspace), no_slots) == E_SHAPE

    # everything the linear rejects comes LAST, with the linear's codes: behind the cache's verdict
    def every(name, value):
        def edit(r):
            for m in (r.q, r.k, r.v):
                setattr(m, name, value)
        return edit
    assert rc(every("bits", 5)) == E_BITS and rc(every("bits", 5), no_slots) == E_NULL
    assert rc(every("batch", -2)) == E_BATCH and rc(every("batch", -2), broken) == E_SHAPE
    assert rc(every("K", 100)) == E_SHAPE
    assert rc(lambda r: setattr(r.k, "qweight", r.k.qweight + 4)) == E_ALIGN
    assert rc(lambda r: setattr(r.k, "nnz", -1) or setattr(r.k, "rows", 0x5000)) == E_SPARSE
    assert rc(lambda r: setattr(r.v, "lookup_table", None)) == E_NULL

    # ... except that a NULL out_k / out_v is admitted
    assert passes(lambda r: setattr(r, "out_k", None))
    assert passes(lambda r: setattr(r, "out_v", None))
    assert passes(lambda r: setattr(r, "out_k", None) or setattr(r, "out_v", None))
    assert passes()

    # then the cache's: NULL descriptor or members
    assert rc(cache=False) == E_NULL
    for name in ("k_cache", "v_cache", "slots"):
        assert rc(edit_c=lambda c: setattr(c, name, None)) == E_NULL, name
    # n_slots < 1, or a stride below head_dim
    assert rc(edit_c=lambda c: setattr(c, "n_slots", 0)) == E_SHAPE
    assert rc(edit_c=lambda c: setattr(c, "n_slots", -1)) == E_SHAPE
    assert rc(edit_c=lambda c: setattr(c, "slot_stride", 63)) == E_SHAPE
    assert rc(edit_c=lambda c: setattr(c, "head_stride", 63)) == E_SHAPE
    assert rc(edit_c=lambda c: setattr(c, "head_stride", 0)) == E_SHAPE
    assert rc(edit_c=lambda c: setattr(c, "slot_stride", -128)) == E_SHAPE
    # N_k != N_v, or head_dim no divisor of N_v
    assert rc(Nv=64) == E_SHAPE
    assert rc(Nv=192) == E_SHAPE
    assert passes(Nq=192, Nk=192, Nv=192, edit_c=lambda c: setattr(c, "slot_stride", 192))  # three kv heads: nothing to reject
    assert passes(lambda r: setattr(r, "head_dim", 32), Nk=96, Nv=96)  # three heads of 32, the strides wider than they need be

    # an extent that overlaps the other cache, the workspace, a non-NULL output or vec (4 slots of 256 bytes: 1024 bytes)
    assert rc(edit_c=lambda c: setattr(c, "v_cache", K_CACHE)) == E_SHAPE
    assert rc(edit_c=lambda c: setattr(c, "v_cache", K_CACHE + 1022)) == E_SHAPE
    assert passes(edit_c=lambda c: setattr(c, "v_cache", K_CACHE + 1024))  # adjacent is fine
    assert rc(edit_c=lambda c: setattr(c, "v_cache", K_CACHE - 1022)) == E_SHAPE
    assert passes(edit_c=lambda c: setattr(c, "v_cache", K_CACHE - 1024))
    need = _lib.qkv_rope_workspace_bytes(256, 128, 128, 0)
    for name in ("k_cache", "v_cache"):
        assert rc(edit_c=lambda c: setattr(c, name, 0x400000)) == E_SHAPE  # the workspace
        assert rc(edit_c=lambda c: setattr(c, name, 0x400000 + need - 2)) == E_SHAPE
        assert passes(edit_c=lambda c: setattr(c, name, 0x400000 + need))
        assert rc(edit_c=lambda c: setattr(c, name, 0x400000 - 1022)) == E_SHAPE
        assert passes(edit_c=lambda c: setattr(c, name, 0x400000 - 1024))
        assert rc(edit_c=lambda c: setattr(c, name, 0x100000 + 510)) == E_SHAPE  # out_q: 512 bytes
        assert passes(edit_c=lambda c: setattr(c, name, 0x100000 + 512))
        assert rc(edit_c=lambda c: setattr(c, name, 0x110000 + 254)) == E_SHAPE  # out_k: 256 bytes
        assert rc(edit_c=lambda c: setattr(c, name, 0x120000 - 1022)) == E_SHAPE  # out_v
        assert rc(edit_c=lambda c: setattr(c, name, 0x1000 + 254)) == E_SHAPE  # vec: one row of K = 128
        assert passes(edit_c=lambda c: setattr(c, name, 0x1000 + 256))
    # ... a NULL output has no extent: the cache may lie where it would have been
    assert rc(lambda r: None, lambda c: setattr(c, "k_cache", 0x110000)) == E_SHAPE
    assert passes(lambda r: setattr(r, "out_k", None), lambda c: setattr(c, "k_cache", 0x110000))
    assert passes(lambda r: setattr(r, "out_v", None), lambda c: setattr(c, "v_cache", 0x120000))
    # the extent follows the strides: head-major with S = 4 (slot_stride = D, head_stride = S * D) and 4 slots ends where
    # 3 * 64 + 1 * 256 + 64 elements do
    def head_major(c):
        c.slot_stride, c.head_stride, c.n_slots = 64, 256, 4
    ext = 2 * (3 * 64 + 256 + 64)
    assert rc(edit_c=lambda c: head_major(c) or setattr(c, "v_cache", K_CACHE + ext - 2)) == E_SHAPE
    assert passes(edit_c=lambda c: head_major(c) or setattr(c, "v_cache", K_CACHE + ext))
    # padded strides widen it
    assert rc(edit_c=lambda c: setattr(c, "slot_stride", 1024) or setattr(c, "v_cache", K_CACHE + 2 * (3 * 1024 + 64 + 64) - 2)) == E_SHAPE
    assert passes(edit_c=lambda c: setattr(c, "slot_stride", 1024) or setattr(c, "v_cache", K_CACHE + 2 * (3 * 1024 + 64 + 64)))


@pytest.mark.parametrize("entry", PLAIN)
def test_strides_the_kernel_multiplies_lie_below_2_to_the_32(lib, entry):
    """the 64-bit offsets are sums of 32 x 32 -> 64-bit products: a stride that is ever multiplied must fit 32 bits; one
    that never is (one slot, one head) may be anything"""
    def rc(edit_c):
        r, c = _qkv(), _cache()
        r.q.qweight = None  # (what these checks admit comes back SQLLM_E_NULL from the linear's validation: nothing is launched)
        c.k_cache, c.v_cache = 0x10000000000, 0x7000000000000
        edit_c(c)
        return _call(lib, entry, r, c)

    assert rc(lambda c: None) == E_NULL
    assert rc(lambda c: setattr(c, "slot_stride", (1 << 32) - 1)) == E_NULL
    assert rc(lambda c: setattr(c, "slot_stride", 1 << 32)) == E_SHAPE
    assert rc(lambda c: setattr(c, "head_stride", (1 << 32) - 1)) == E_NULL
    assert rc(lambda c: setattr(c, "head_stride", 1 << 32)) == E_SHAPE
    assert rc(lambda c: setattr(c, "slot_stride", 1 << 40) or setattr(c, "n_slots", 1)) == E_NULL  # one slot: never multiplied
    assert rc(lambda c: setattr(c, "slot_stride", 1 << 62) or setattr(c, "n_slots", 1)) == E_NULL


@pytest.mark.parametrize("entry", ["sqllm_qkv_rope_f16", "sqllm_qkv_rope_bf16", "sqllm_qkv_rope_norm_f16", "sqllm_qkv_rope_norm_bf16"])
def test_the_parent_entries_still_want_out_k_and_out_v(lib, entry):
    from squeezellm_amd import _lib

    for name in ("out_k", "out_v"):
        r = _qkv()
        setattr(r, name, None)
        args = (ctypes.byref(r), ctypes.byref(_lib.SqllmRmsNorm(weight=0x300000, eps=1e-6)), None) if "norm" in entry else (ctypes.byref(r), None)
        assert getattr(lib, entry)(*args) == E_NULL


def test_the_sources_are_part_of_the_product_build():
    from squeezellm_amd import build as B

    for src in ("sqllm_linear_qkv_cache.hip", "sqllm_linear_qkv_norm_cache.hip"):
        assert src in B.SOURCES and B.SOURCES.index(src) < B.SOURCES.index("sqllm_capi.hip")
    assert B.SOURCES[-1] == "sqllm_capi.hip"
    assert os.path.join(B.CSRC, "sqllm_cache_finish.h") in B.HEADERS
