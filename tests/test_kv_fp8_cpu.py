"""The fp8 KV cache on a host without a GPU (include/sqllm_hip.h, sqllm_kv_cache_fp8 / sqllm_attn_decode_fp8): the symbols and
the structs' layout, every rejection of the six entries in the header's order (operand pointers are fake integers: nothing
dereferences them, and every call carries at least one defect, so nothing is ever launched), the encoding the case builder
uses against an integer model of e4m3fn, and the torch fallbacks of the two modules against the oracle of
tests/attn_decode_cases.py over the dequantised bytes -- with that oracle's five mutants, and two new ones that ignore a scale,
failing the same gate at every shape the GPU tests use."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import attn_decode_cases as AC
from tests import kv_fp8_cases as F
from tests import test_attn_decode_capi_cpu as TA
from tests import test_qkv_cache_capi_cpu as TC
from tests.test_qkv_rope_capi_cpu import _qkv

E_BITS, E_SHAPE, E_NULL, E_ALIGN, E_SPARSE, E_BATCH, E_OPTION, E_GROUP = -1, -2, -3, -4, -5, -6, -7, -8
PLAIN = ("sqllm_qkv_rope_cache_fp8_f16", "sqllm_qkv_rope_cache_fp8_bf16")
NORM = ("sqllm_qkv_rope_norm_cache_fp8_f16", "sqllm_qkv_rope_norm_cache_fp8_bf16")
ATTN = ("sqllm_attn_decode_fp8_f16", "sqllm_attn_decode_fp8_bf16")
BAD_SCALES = (0.0, -1.0, float("nan"), float("inf"), float("-inf"), 1e-45, 2e-39)  # (the last two: subnormals whose reciprocal is inf)
K_CACHE, V_CACHE = TC.K_CACHE, TC.V_CACHE


@pytest.fixture(scope="module")
def lib():
    from squeezellm_amd import _lib

    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- the C ABI

def test_symbols_signatures_layout_and_header_text(lib, tmp_path):
    from squeezellm_amd import _lib

    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "sqllm_hip.h")).read()
    P = ctypes.POINTER
    for name in PLAIN + NORM + ATTN:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header
        assert getattr(lib, name).restype is ctypes.c_int
    assert _lib.SIGNATURES[PLAIN[0]] == _lib.SIGNATURES[PLAIN[1]] == [P(_lib.SqllmQkvRope), P(_lib.SqllmKvCacheFp8), ctypes.c_void_p]
    assert _lib.SIGNATURES[NORM[0]] == _lib.SIGNATURES[NORM[1]] == [P(_lib.SqllmQkvRope), P(_lib.SqllmRmsNorm), P(_lib.SqllmKvCacheFp8), ctypes.c_void_p]
    assert _lib.SIGNATURES[ATTN[0]] == _lib.SIGNATURES[ATTN[1]] == [P(_lib.SqllmAttnDecodeFp8), ctypes.c_void_p]
    # the 16-bit structs stay what they are; the new ones are their fields plus the two scales
    assert ctypes.sizeof(_lib.SqllmKvCache) == TC.SIZE and ctypes.sizeof(_lib.SqllmAttnDecode) == TA.SIZE
    layouts = {"sqllm_kv_cache_fp8": (_lib.SqllmKvCacheFp8, TC.FIELDS + ("k_scale", "v_scale"), TC.OFFSETS + [48, 52], 56),
               "sqllm_attn_decode_fp8": (_lib.SqllmAttnDecodeFp8, TA.FIELDS + ("k_scale", "v_scale"), TA.OFFSETS + [128, 132], 136)}
    gcc = shutil.which("gcc")
    for cname, (S, fields, offsets, size) in layouts.items():
        assert [n for n, _ in S._fields_] == list(fields)
        assert [getattr(S, n).offset for n in fields] == offsets and ctypes.sizeof(S) == size
        assert f"typedef struct {cname} {{" in header
        if gcc:  # ... and from the C compiler, where there is one
            include = os.path.join(os.path.dirname(_lib.HERE), "include")
            c = tmp_path / (cname + ".c")
            c.write_text(f'#include <stddef.h>\n#include <stdio.h>\n#include "sqllm_hip.h"\nint main(void){{ printf("%zu", sizeof({cname}));\n'
                         + "".join(f'printf(" %zu", offsetof({cname}, {n}));\n' for n in fields) + "return 0; }\n")
            exe = tmp_path / cname
            subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", f"-I{include}", str(c), "-o", str(exe)], check=True)
            assert [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()] == [size, *offsets]
    for text in ("byte = e4m3_rne(min(max(x * inv, -448), 448))", "NOT the fnuz format", "rounded ONCE, straight to fp8",
                 "ties to even", "subnormals are produced, not flushed", "+-inf saturates to +-448", "NaN stays NaN",
                 "The clamp is explicit in the kernel", "float(k) = k_scale * f32(byte) and float(v) = v_scale * f32(byte)",
                 "folded into the score's scale, rounded once on the host", "which now count BYTES", "aligned to one byte only",
                 "head_stride = head_dim + 3 included", "The order is not the 16-bit kernel's",
                 "not finite, not positive, or whose fp32 reciprocal is not finite", "a scale * k_scale that is not finite",
                 "per-head or per-token scales, e5m2, int8 or 4-bit caches, computing the scales, prefill attention"):
        assert text in header, text
    assert lib.sqllm_abi_version() == 1  # symbols were added, nothing changed


def _cache8(k_scale=0.5, v_scale=0.25, **kw):
    """TC._cache()'s slot-major [4, 2, 64] in bytes: an extent of 4 * 128 = 512 bytes"""
    from squeezellm_amd import _lib

    c = _lib.SqllmKvCacheFp8()
    c.k_cache, c.v_cache, c.slots = K_CACHE, V_CACHE, 0x230000
    c.n_slots, c.slot_stride, c.head_stride = 4, 128, 64
    c.k_scale, c.v_scale = k_scale, v_scale
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _front(lib, entry, r, c):
    from squeezellm_amd import _lib

    fn = getattr(lib, entry)
    cref = ctypes.byref(c) if c is not None else None
    if entry in NORM:
        return fn(ctypes.byref(r), ctypes.byref(_lib.SqllmRmsNorm(weight=0x300000, eps=1e-6)), cref, None)
    return fn(ctypes.byref(r), cref, None)


@pytest.mark.parametrize("entry", PLAIN + NORM)
def test_front_rejections_the_siblings_first_then_the_scales(lib, entry):
    from squeezellm_amd import _lib

    bad = dict(k_scale=float("nan"))  # (SQLLM_E_OPTION, were it looked at: every sibling rejection comes in front of it)

    def rc(edit_r=lambda r: None, c=None, cache=True, **kw):
        r = _qkv(**kw)
        edit_r(r)
        return _front(lib, entry, r, (c if c is not None else _cache8(**bad)) if cache else None)

    # the parent's and the norm's, in their order
    if entry in PLAIN:
        assert getattr(lib, entry)(None, ctypes.byref(_cache8(**bad)), None) == E_NULL
    else:
        assert getattr(lib, entry)(None, ctypes.byref(_lib.SqllmRmsNorm(weight=0x300000, eps=1e-6)), ctypes.byref(_cache8(**bad)), None) == E_NULL
        assert getattr(lib, entry)(ctypes.byref(_qkv()), None, ctypes.byref(_cache8(**bad)), None) == E_NULL
        assert getattr(lib, entry)(ctypes.byref(_qkv()), ctypes.byref(_lib.SqllmRmsNorm(weight=0x300000, eps=-1.0)), None, None) == E_OPTION
    for m in "qkv":
        assert rc(lambda r: setattr(getattr(r, m), "mul", 0x5000)) == E_GROUP
    assert rc(lambda r: setattr(r.k, "K", 256)) == E_GROUP
    assert rc(lambda r: setattr(r, "layout", 2), _cache8(n_slots=0)) == E_OPTION  # (the layout's code, not the scale's: see below)
    for name in ("out_q", "cos", "sin", "positions", "workspace"):
        assert rc(lambda r: setattr(r, name, None)) == E_NULL, name
    assert rc(lambda r: setattr(r, "workspace", 0x400008)) == E_ALIGN
    assert rc(lambda r: setattr(r, "head_dim", 63)) == E_SHAPE and rc(lambda r: setattr(r, "n_pos", 0)) == E_SHAPE
    assert rc(lambda r: setattr(r, "out_k", r.out_q + 510)) == E_SHAPE and rc(lambda r: setattr(r, "out_v", r.workspace)) == E_SHAPE
    # the cache's, with the 16-bit sibling's codes: NULLs, n_slots, strides, widths
    assert rc(cache=False) == E_NULL
    for name in ("k_cache", "v_cache", "slots"):
        assert rc(c=_cache8(**{name: None}, **bad)) == E_NULL, name
    for kw in (dict(n_slots=0), dict(n_slots=-1), dict(slot_stride=63), dict(head_stride=63), dict(head_stride=0), dict(slot_stride=-128)):
        assert rc(c=_cache8(**kw, **bad)) == E_SHAPE, kw
    assert rc(Nv=64) == E_SHAPE and rc(Nv=192) == E_SHAPE
    # strides that are multiplied, and extents: in BYTES now -- 512 per cache where the 16-bit cache had 1024
    far = dict(k_cache=0x10000000000, v_cache=0x7000000000000)
    assert rc(c=_cache8(slot_stride=1 << 32, **far, **bad)) == E_SHAPE and rc(c=_cache8(head_stride=1 << 32, **far, **bad)) == E_SHAPE
    assert rc(c=_cache8(slot_stride=(1 << 32) - 1, **far, **bad)) == E_OPTION  # (admitted: the scale speaks)
    assert rc(c=_cache8(slot_stride=1 << 62, n_slots=1, **far, **bad)) == E_OPTION  # one slot: never multiplied
    assert rc(c=_cache8(v_cache=K_CACHE, **bad)) == E_SHAPE and rc(c=_cache8(v_cache=K_CACHE + 511, **bad)) == E_SHAPE
    assert rc(c=_cache8(v_cache=K_CACHE - 511, **bad)) == E_SHAPE
    assert rc(c=_cache8(v_cache=K_CACHE + 512, **bad)) == E_OPTION and rc(c=_cache8(v_cache=K_CACHE - 512, **bad)) == E_OPTION  # adjacent, odd or not
    assert rc(c=_cache8(v_cache=K_CACHE + 513, k_cache=K_CACHE + 1, **bad)) == E_OPTION  # no alignment rule for bytes
    need = _lib.qkv_rope_workspace_bytes(256, 128, 128, 0)
    for name in ("k_cache", "v_cache"):
        for at, code in ((0x400000, E_SHAPE), (0x400000 + need - 1, E_SHAPE), (0x400000 + need, E_OPTION), (0x400000 - 511, E_SHAPE),
                         (0x400000 - 512, E_OPTION), (0x100000 + 511, E_SHAPE), (0x100000 + 512, E_OPTION), (0x110000 + 255, E_SHAPE),
                         (0x120000 - 511, E_SHAPE), (0x1000 + 255, E_SHAPE), (0x1000 + 256, E_OPTION)):
            assert rc(c=_cache8(**{name: at}, **bad)) == code, (name, hex(at))
    assert rc(lambda r: setattr(r, "out_k", None), _cache8(k_cache=0x110000, **bad)) == E_OPTION  # a NULL output has no extent
    assert rc(c=_cache8(slot_stride=64, head_stride=256, v_cache=K_CACHE + 3 * 64 + 256 + 64 - 1, **bad)) == E_SHAPE  # head-major
    assert rc(c=_cache8(slot_stride=64, head_stride=256, v_cache=K_CACHE + 3 * 64 + 256 + 64, **bad)) == E_OPTION
    assert rc(c=_cache8(slot_stride=131, head_stride=67, v_cache=K_CACHE + 3 * 131 + 67 + 64, **bad)) == E_OPTION  # padded: head_dim + 3

    # everything the linear rejects, with the linear's codes, IN FRONT of the scales
    def every(name, value):
        def edit(r):
            for m in (r.q, r.k, r.v):
                setattr(m, name, value)
        return edit
    assert rc(every("bits", 5)) == E_BITS and rc(every("batch", -2)) == E_BATCH and rc(every("K", 100)) == E_SHAPE
    assert rc(lambda r: setattr(r.k, "qweight", r.k.qweight + 4)) == E_ALIGN
    assert rc(lambda r: setattr(r.k, "nnz", -1) or setattr(r.k, "rows", 0x5000)) == E_SPARSE
    assert rc(lambda r: setattr(r.v, "lookup_table", None)) == E_NULL
    assert rc(lambda r: setattr(r.q, "qweight", None), _cache8()) == E_NULL  # (good scales: what is admitted ends in the linear's validation)

    # then the scales: not finite, not positive, or a reciprocal that is not finite -- with out_k / out_v NULL or not
    for s in BAD_SCALES:
        assert rc(c=_cache8(k_scale=s)) == E_OPTION, s
        assert rc(c=_cache8(v_scale=s)) == E_OPTION, s
        assert rc(lambda r: setattr(r, "out_k", None) or setattr(r, "out_v", None), _cache8(v_scale=s)) == E_OPTION, s


def _attn8(**kw):
    """TA._desc()'s call over byte caches: 128 slots of 2 heads of 64 bytes"""
    from squeezellm_amd import _lib

    a = _lib.SqllmAttnDecodeFp8()
    a.q, a.out, a.k_cache, a.v_cache, a.block_table, a.seq_lens, a.workspace = TA.Q, TA.OUT, TA.K_CACHE, TA.V_CACHE, TA.TABLE, TA.LENS, TA.WS
    a.batch, a.n_q_heads, a.n_kv_heads, a.head_dim = 2, 4, 2, 64
    a.n_slots, a.block_size, a.max_blocks, a.table_stride = 128, 16, 4, 4
    a.slot_stride, a.head_stride, a.q_stride, a.out_stride = 128, 64, 256, 256
    a.scale, a.k_scale, a.v_scale = 0.125, float("nan"), 0.25  # (a defect that is judged LAST: every call here is rejected)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("entry", ATTN)
def test_attention_rejections_the_siblings_first_then_the_scales(lib, entry):
    from squeezellm_amd import _lib

    fn = getattr(lib, entry)

    def rc(**kw):
        return fn(ctypes.byref(_attn8(**kw)), None)

    Q = TA.Q
    assert fn(None, None) == E_NULL
    for name in ("q", "out", "k_cache", "v_cache", "block_table", "seq_lens", "workspace"):
        assert rc(**{name: None}) == E_NULL, name
        assert rc(**{name: None, "batch": 0, "scale": float("nan")}) == E_NULL  # NULL comes first
    for name in ("batch", "n_q_heads", "n_kv_heads", "head_dim", "n_slots", "block_size", "max_blocks", "table_stride"):
        for v in (0, -1):
            assert rc(**{name: v, "scale": float("inf"), "out": Q, "q": Q + 1}) == E_SHAPE, name
    assert rc(slot_stride=63) == E_SHAPE and rc(head_stride=63) == E_SHAPE and rc(head_stride=0) == E_SHAPE and rc(slot_stride=-128) == E_SHAPE
    assert rc(q_stride=255) == E_SHAPE and rc(out_stride=255) == E_SHAPE and rc(max_blocks=5) == E_SHAPE
    for kw in (dict(head_dim=32, q_stride=128, out_stride=128), dict(head_dim=96, slot_stride=192, head_stride=96, q_stride=384, out_stride=384),
               dict(n_q_heads=3, n_kv_heads=2), dict(n_q_heads=18, n_kv_heads=2, q_stride=18 * 64, out_stride=18 * 64), dict(batch=65)):
        assert rc(scale=float("nan"), **kw) == E_SHAPE, kw
    far = dict(k_cache=0x10000000000, v_cache=0x7000000000000)
    assert rc(slot_stride=1 << 32, **far) == E_SHAPE and rc(head_stride=1 << 32, **far) == E_SHAPE
    assert rc(q_stride=1 << 62) == E_SHAPE and rc(out_stride=1 << 62) == E_SHAPE
    assert rc(slot_stride=(1 << 32) - 1, **far) == E_OPTION and rc(slot_stride=1 << 40, n_slots=1, **far) == E_OPTION
    # the call's own scale, in the sibling's place: before the overlaps and the alignment
    for v in (float("nan"), float("inf"), float("-inf")):
        assert rc(scale=v, out=Q, q=Q + 1, k_scale=0.5) == E_OPTION
    # overlaps, the caches' extents in bytes: 127 * 128 + 64 + 64
    ws = _lib.attn_decode_workspace_bytes(2, 4, 64, 4, 16)
    cache = 127 * 128 + 64 + 64
    inputs = {"q": (Q, 1024), "k_cache": (TA.K_CACHE, cache), "v_cache": (TA.V_CACHE, cache), "block_table": (TA.TABLE, 32), "seq_lens": (TA.LENS, 8)}
    for name, (at, size) in inputs.items():
        for mine, my_size in (("out", 1024), ("workspace", ws)):
            q_odd = {} if name == "q" else {"q": Q + 1}
            assert rc(**{mine: at}) == E_SHAPE, (mine, name)
            assert rc(**{mine: at + size - 2, **q_odd}) == E_SHAPE and rc(**{mine: at - my_size + 2, **q_odd}) == E_SHAPE
            if q_odd:
                assert rc(**{mine: at + size + (-size) % 4, **q_odd}) == E_ALIGN  # adjacent is fine: the next check speaks
                assert rc(**{mine: at - my_size - (-my_size) % 4 - 4, **q_odd}) == E_ALIGN
    assert rc(out=TA.WS) == E_SHAPE and rc(out=TA.WS + ws, q=Q + 1) == E_ALIGN
    # alignment: q and out to 2 bytes, the workspace to 4 -- and the caches to ONE
    assert rc(q=Q + 1) == E_ALIGN and rc(out=TA.OUT + 1) == E_ALIGN and rc(workspace=TA.WS + 2) == E_ALIGN
    assert rc(k_cache=TA.K_CACHE + 1, v_cache=TA.V_CACHE + 3) == E_OPTION  # (admitted: the scales speak)
    # then the scales, and last the product
    for s in BAD_SCALES:
        assert rc(k_scale=s) == E_OPTION and rc(k_scale=0.5, v_scale=s) == E_OPTION, s
        assert rc(k_scale=s, q=Q + 1) == E_ALIGN  # ... behind the alignment
    assert rc(scale=3e38, k_scale=16.0) == E_OPTION and rc(scale=-3e38, k_scale=2.0) == E_OPTION  # scale * k_scale overflows fp32


def test_the_sources_are_part_of_the_product_build():
    from squeezellm_amd import build as B

    for src in ("sqllm_linear_qkv_cache_fp8.hip", "sqllm_linear_qkv_norm_cache_fp8.hip", "sqllm_attn_decode_fp8.hip"):
        assert src in B.SOURCES and B.SOURCES.index(src) < B.SOURCES.index("sqllm_capi.hip")
    assert B.SOURCES[-1] == "sqllm_capi.hip"
    assert os.path.join(B.CSRC, "sqllm_cache_fp8_finish.h") in B.HEADERS


# ------------------------------------------------------------------------------------------------------------ the encoding

def _e4m3_values():
    """the 254 finite e4m3fn values by the format's definition (bias 7, subnormals of 2^-9, no infinities), byte -> value"""
    out = {}
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        if e == 15 and m == 7:
            continue
        v = m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
        out[b] = -v if b & 0x80 else v
    return out


def test_the_case_builders_encoding_is_round_to_nearest_even_with_subnormals_and_saturation():
    vals = _e4m3_values()
    assert max(vals.values()) == 448.0 and min(abs(v) for b, v in vals.items() if b & 0x7F) == 2.0 ** -9
    pos = sorted((v, b) for b, v in vals.items() if b < 0x80)
    dec = F.decode(torch.arange(256, dtype=torch.uint8))
    for b, v in vals.items():
        assert float(dec[b]) == v
    assert bool(torch.isnan(dec[0x7F])) and bool(torch.isnan(dec[0xFF]))
    # every representable value, every midpoint (ties to even) and the points on either side of each midpoint
    xs, want = [], []
    for (lo, blo), (hi, bhi) in zip(pos[:-1], pos[1:]):
        mid = (lo + hi) / 2
        even = blo if blo % 2 == 0 else bhi
        for x, b in ((lo, blo), (np.nextafter(np.float32(mid), np.float32(0)), blo), (mid, even), (np.nextafter(np.float32(mid), np.float32(1e9)), bhi)):
            xs.append(float(x))
            want.append(b)
    xs += [448.0, 464.0, 479.9, 480.0, 1e9, float("inf"), 2.0 ** -10, 2.0 ** -11]
    want += [0x7E, 0x7E, 0x7E, 0x7E, 0x7E, 0x7E, 0, 0]  # saturation (464 is the midpoint to the absent 512), the tie to zero
    x = torch.tensor(xs, dtype=torch.float32)
    assert F.encode(x, 1.0).tolist() == want
    assert F.encode(-x, 1.0).tolist() == [b | 0x80 for b in want]
    assert F.encode(x * 3.0, 3.0).tolist()[-8:-2] == [0x7E] * 6
    assert F.encode(torch.tensor([float("nan")]), 1.0).tolist()[0] & 0x7F == 0x7F
    order = F.byte_order(np.array(sorted(vals, key=lambda b: (vals[b], -(b >> 7)))))
    assert (np.diff(order) == 1).all()  # the sign-magnitude order of the encoding is the order of the values


# ---------------------------------------------------------------------------------------- the fallbacks against the oracle

GPU_SHAPES = [(kind, rows, D, HQ, H) for kind in AC.GEOMETRIES + ("paged_single",) for rows in (1, 3, 5) for D in (64, 128) for HQ, H in AC.HEADS]


def _fallback(fc, k_scale=None, v_scale=None, poison_view=None):
    from squeezellm_amd import quant

    c = fc.case
    att = quant.DecodeAttention(c.HQ, c.H, c.D, scale=c.scale, block_size=c.block_size)
    o = att(c.q_buf[:, :c.HQ * c.D], F.cache_view(fc, fc.k_bytes), F.cache_view(fc, fc.v_bytes), torch.from_numpy(c.table),
            torch.from_numpy(c.lens), k_scale=fc.k_scale if k_scale is None else k_scale, v_scale=fc.v_scale if v_scale is None else v_scale)
    assert att.last_route == "fallback"
    return o.double().numpy()


@pytest.mark.parametrize("dtype_name", list(AC.DTYPES))
@pytest.mark.parametrize("kind,rows,D,HQ,H", [s for i, s in enumerate(GPU_SHAPES) if i % 5 == 0])
def test_attention_fallback_passes_the_oracle_over_the_dequantised_bytes(kind, rows, D, HQ, H, dtype_name):
    fc, want, gate = F.reference(kind, rows, D, HQ, H, dtype_name)
    assert fc.k_scale != 1.0 and fc.v_scale != 1.0 and fc.k_scale != fc.v_scale
    assert AC.excess(_fallback(fc), want, gate) <= 1.0
    other = F.fp8_case(kind, rows, D, HQ, H, dtype_name, poison=1)
    assert (other.k_bytes != fc.k_bytes).any() and np.array_equal(_fallback(other), _fallback(fc))  # isolation: the other NaN byte


def test_attention_fallback_with_scales_that_are_no_powers_of_two():
    fc, want, gate = F.reference("padded", 3, 128, 6, 2, "bf16", F.ODD_SCALES)
    assert AC.excess(_fallback(fc), want, gate) <= 1.0


@pytest.mark.parametrize("kind,rows,D,HQ,H", GPU_SHAPES)
def test_every_mutant_fails_the_gate_at_every_shape_the_gpu_tests_use(kind, rows, D, HQ, H):
    """the five mutants of the oracle, over the dequantised bytes, and two of the fp8 contract: an attention that ignores
    k_scale (scores over the raw bytes' values) and one that ignores v_scale"""
    fc, want, gate = F.reference(kind, rows, D, HQ, H, "fp16")
    for m in AC.MUTANTS:
        assert AC.excess(AC.oracle(fc.shadow, m)[0], want, gate) > 1.0, m
    for name in ("k", "v"):  # the shadow with one cache NOT multiplied by its scale
        import copy
        wrong = copy.copy(fc.shadow)
        setattr(wrong, name + "_buf", getattr(fc.shadow, name + "_buf") / getattr(fc, name + "_scale"))
        assert AC.excess(AC.oracle(wrong)[0], want, gate) > 1.0, name


def test_the_fallback_itself_fails_when_it_is_given_the_wrong_scale():
    fc, want, gate = F.reference("paged", 3, 64, 8, 2, "fp16")
    assert AC.excess(_fallback(fc, k_scale=1.0), want, gate) > 1.0 and AC.excess(_fallback(fc, v_scale=1.0), want, gate) > 1.0


# ------------------------------------------------------------------------------------------------------ the module surface

def test_module_arguments_scales_go_with_fp8_caches_and_only_with_them():
    from squeezellm_amd import quant

    fc = F.fp8_case("paged", 1, 64, 2, 2, "fp16")
    c = fc.case
    att = quant.DecodeAttention(c.HQ, c.H, c.D, block_size=c.block_size)
    q, table, lens = c.q_buf[:, :c.HQ * c.D], torch.from_numpy(c.table), torch.from_numpy(c.lens)
    k8, v8 = F.cache_view(fc, fc.k_bytes), F.cache_view(fc, fc.v_bytes)
    k16, v16 = AC.cache_view(c, c.k_buf), AC.cache_view(c, c.v_buf)
    with pytest.raises(ValueError, match="needs both"):
        att(q, k8, v8, table, lens)
    with pytest.raises(ValueError, match="needs both"):
        att(q, k8, v8, table, lens, k_scale=0.5)
    with pytest.raises(ValueError, match="belong to"):
        att(q, k16, v16, table, lens, k_scale=0.5, v_scale=0.5)
    with pytest.raises(ValueError, match="one dtype"):
        att(q, k8, v16, table, lens, k_scale=0.5, v_scale=0.5)
    for s in BAD_SCALES:
        with pytest.raises(ValueError, match="finite and positive"):
            att(q, k8, v8, table, lens, k_scale=s, v_scale=0.5)
    # uint8 views are the same bytes
    a = att(q, k8, v8, table, lens, k_scale=fc.k_scale, v_scale=fc.v_scale)
    b = att(q, k8.view(torch.uint8), v8.view(torch.uint8), table, lens, k_scale=fc.k_scale, v_scale=fc.v_scale)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert quant.fp8_kv_scale(448.0) == 1.0 and float(quant.fp8_kv_scale(torch.tensor(896.0))) == 2.0
    # kv_cache_view takes float8 and uint8 caches in both layouts
    t = torch.zeros((2, 3, 5, 64), dtype=torch.float8_e4m3fn)
    assert quant.kv_cache_view(t, "bhsd").shape == (3 * 5 + 5, 3, 64) and quant.kv_cache_view(t, "bhsd").stride() == (64, 320, 1)
    assert quant.kv_cache_view(t.view(torch.uint8), "nhd").shape == (6, 5, 64)


def test_front_fallback_writes_the_bytes_of_the_contracts_formula_and_wants_its_scales(monkeypatch):
    """the attention front on the CPU (fp32 activations, the torch route; tests/test_qkv_cache_cpu.py's stand-in for the members'
    sums, which have no CPU path): with float8 caches and the two scales -- keyword
    arguments of the module CALL -- the live slots hold e4m3_rne(clamp(x / scale, +-448)) of the fp32 k and v the call returns
    (fp32 outputs: no rounding in between), rows with out-of-range slots write nothing, every other byte keeps its poison"""
    from squeezellm_amd import quant
    from tests import test_qkv_cache_cpu as TCPU

    def sums(self, x):
        w = torch.randn(self.outfeatures, self.infeatures, generator=torch.Generator().manual_seed(self.outfeatures)) / 32
        return x.float() @ w.T

    monkeypatch.setattr(quant.QuantLinearLUT, "forward", sums)
    rows, n_slots = 5, 9
    mod = TCPU._module()
    x, pos, cos, sin = TCPU._operands(rows)
    H, D = TCPU.H, TCPU.D
    slots = torch.tensor([8, 0, -1, 3, n_slots], dtype=torch.int32)
    _, k0, v0 = mod(x, pos, cos, sin)
    ks, vs = float(k0.abs().max()) / 448.0 / 4.0, float(v0.abs().max()) * 2.0 ** 7  # k: the upper two binades saturate; v: all subnormal
    bufs = [torch.full((64 + n_slots * (H * (D + 3) + 5) + 64,), b, dtype=torch.uint8) for b in F.NAN_BYTES]
    views = [b.view(torch.float8_e4m3fn).as_strided((n_slots, H, D), (H * (D + 3) + 5, D + 3, 1), 65) for b in bufs]
    q, k, v = mod(x, pos, cos, sin, k_cache=views[0], v_cache=views[1], slots=slots, k_scale=ks, v_scale=vs)
    assert mod.last_route == "fallback" and k.dtype == torch.float32
    assert float((k.abs() / ks).max()) > 480.0 and float((v.abs() / vs).max()) < 2.0 ** -6 and float((v.abs() / vs).max()) > 2.0 ** -9
    for buf, view, rows32, scale, poison in ((bufs[0], views[0], k, ks, F.NAN_BYTES[0]), (bufs[1], views[1], v, vs, F.NAN_BYTES[1])):
        want = torch.full_like(buf, poison)
        wv = want.as_strided((n_slots, H, D), (H * (D + 3) + 5, D + 3, 1), 65)
        for b, s in enumerate(slots.tolist()):
            if 0 <= s < n_slots:
                wv[s] = F.encode(rows32[b].reshape(H, D), scale)
        assert torch.equal(buf, want)
    q2, none_k, none_v = mod(x, pos, cos, sin, k_cache=views[0].view(torch.uint8), v_cache=views[1].view(torch.uint8), slots=slots, return_kv=False,
                             k_scale=ks, v_scale=vs)  # uint8 views: the same bytes
    assert none_k is None and none_v is None
    with pytest.raises(ValueError, match="needs both"):
        mod(x, pos, cos, sin, k_cache=views[0], v_cache=views[1], slots=slots)
    with pytest.raises(ValueError, match="needs both"):
        mod(x, pos, cos, sin, k_cache=views[0], v_cache=views[1], slots=slots, v_scale=vs)
    with pytest.raises(ValueError, match="belong to"):
        mod(x, pos, cos, sin, k_scale=ks, v_scale=vs)
    with pytest.raises(ValueError, match="belong to"):
        mod(x, pos, cos, sin, k_cache=torch.zeros(n_slots, H, D), v_cache=torch.zeros(n_slots, H, D), slots=slots, k_scale=ks, v_scale=vs)
    for s in BAD_SCALES:
        with pytest.raises(ValueError, match="finite and positive"):
            mod(x, pos, cos, sin, k_cache=views[0], v_cache=views[1], slots=slots, k_scale=ks, v_scale=s)
    assert "_fp8_scales" not in mod.__dict__ and len(mod(x, pos, cos, sin)) == 3  # (a call without scales is the call it always was)
