"""Cases of the decode attention over an fp8 KV cache (include/sqllm_hip.h, sqllm_attn_decode_fp8), built on
tests/attn_decode_cases.py and shared by the CPU and the GPU tests.  No GPU and no library needed here.

  * `fp8_case` -- attn_decode_cases.build(...)'s case with its attended k and v quantised to e4m3fn bytes by the contract's
                  formula, byte = e4m3_rne(clamp(x * (1 / scale), +-448)) with the reciprocal formed once in fp32 -- torch's CPU
                  conversion to float8_e4m3fn rounds to nearest even and keeps subnormals (`encode` below is checked against an
                  integer model of the format in tests/test_kv_fp8_cpu.py).  EVERY unaddressed byte and the guards hold one of
                  the two NaN bytes 0x7f / 0xff (`poison`); the bytes of the attended elements do not depend on it.
  * the shadow -- the same case with k_buf / v_buf as fp64 tensors of the DEQUANTISED values, scale * f32(byte) formed exactly:
                  attn_decode_cases.reference_of(shadow) is the oracle and the gate of the fp8 attention, unchanged.
"""
import copy
import functools
import types

import numpy as np
import torch

from tests import attn_decode_cases as AC

NAN_BYTES = (0x7F, 0xFF)
E4M3_MAX = 448.0
SCALES = (0.0078125, 0.03125)  # k_scale, v_scale: N(0, 1) values reach about +-4.5, i.e. 576 and 144 in units of the scales:
#                                the largest k saturate at 448 (asserted where it matters), v uses the format's upper binades
ODD_SCALES = (0.0113, 0.0271)  # no powers of two: the products scale * f32(byte) round


def encode(x32: torch.Tensor, scale: float) -> torch.Tensor:
    """uint8 bytes of fp32 values by the contract's formula (CPU)"""
    inv = 1.0 / torch.tensor(scale, dtype=torch.float32)
    assert bool(torch.isfinite(inv))
    return (x32.float() * inv).clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def decode(b: torch.Tensor) -> torch.Tensor:
    """fp32 values of e4m3fn bytes (exact; 0x7f and 0xff are NaN)"""
    return b.view(torch.float8_e4m3fn).float()


def byte_order(b):
    """e4m3fn bytes (not NaN) as integers in the order of their values: sign-magnitude to a monotone scale, -0 below +0"""
    b = np.asarray(b, dtype=np.int64)
    return np.where(b >= 0x80, -(b - 0x80) - 1, b)


@functools.lru_cache(maxsize=None)
def fp8_case(kind, rows, D, HQ, H, dtype_name, scales=SCALES, poison=0, lens=None, capacity=None):
    """namespace(case, shadow, k_bytes, v_bytes, k_scale, v_scale): k_bytes / v_bytes are the guarded uint8 buffers, laid out as
    case.k_buf / case.v_buf (the strides now count bytes)"""
    more = () if capacity is None else (capacity,)  # (functools.lru_cache keys on the call: the old cases stay the objects they were)
    return quantise(AC.build(kind, rows, D, HQ, H, dtype_name, 0, lens, *more), scales, poison)


def quantise(case, scales=SCALES, poison=0):
    """fp8_case's namespace for any case of attn_decode_cases (its k_buf / v_buf NaN exactly where nothing is addressed)"""
    k_scale, v_scale = (float(torch.tensor(s, dtype=torch.float32)) for s in scales)
    out = {}
    shadow = copy.copy(case)
    for name, buf, scale in (("k", case.k_buf, k_scale), ("v", case.v_buf, v_scale)):
        live = ~torch.isnan(buf)  # (build() leaves NaN exactly where nothing is addressed)
        b = torch.where(live, encode(torch.where(live, buf, torch.zeros_like(buf)).float(), scale), torch.tensor(NAN_BYTES[poison], dtype=torch.uint8))
        assert bool((torch.isnan(decode(b)) == ~live).all())  # (no addressed byte is a NaN byte)
        out[name] = b
        setattr(shadow, name + "_buf", decode(b).double() * float(scale))  # (fp64: scale * f32(byte) exactly)
    return types.SimpleNamespace(case=case, shadow=shadow, k_bytes=out["k"], v_bytes=out["v"], k_scale=k_scale, v_scale=v_scale)


@functools.lru_cache(maxsize=None)
def reference(kind, rows, D, HQ, H, dtype_name, scales=SCALES, lens=None, capacity=None):
    """(fp8 case, want, gate) -- the oracle over the dequantised bytes, computed once per case and shared"""
    fc = fp8_case(kind, rows, D, HQ, H, dtype_name, scales, 0, lens, *(() if capacity is None else (capacity,)))
    return (fc, *AC.reference_of(fc.shadow))


def cache_view(fc, buf):
    """the [n_slots, H, D] float8_e4m3fn view of an fp8 case's cache inside its guarded uint8 buffer (on whatever device)"""
    c = fc.case
    return buf.view(torch.float8_e4m3fn).as_strided((c.n_slots, c.H, c.D), (c.slot_stride, c.head_stride, 1), AC.GUARD)


# ---- sharp softmax over a byte cache (attn_decode_cases.sharpen) ----

SHARP_C = 512.0  # coordinate 0 of q: exact in fp16 and bf16, and large enough that an offset of 150 keeps coordinate 0 of k inside
#                  +-448 x k_scale = 3.5 at both head_dims (150 / (scale * 512) = 2.35 and 3.32); e4m3 then rounds the offsets to three
#                  bits -- the oracle reads the bytes, and the profiles' conditions are asserted on the shadow's scores


@functools.lru_cache(maxsize=None)
def sharp_reference(kind, D, HQ, H, dtype_name, profile, lens=AC.SHARP_LENS):
    """(fp8 case, want, gate): attn_decode_cases.sharpen(..., c = SHARP_C) quantised, its profile's conditions asserted on the
    shadow's scores; fc.case carries the sharpened q (and 16-bit values nobody reads)"""
    plain = AC.build(kind, len(lens), D, HQ, H, dtype_name, 0, lens)
    sharp = AC.sharpen(plain, profile, SHARP_C)
    assert 150.0 / (plain.scale * SHARP_C) <= E4M3_MAX * SCALES[0]  # the largest offset of a profile does not saturate
    fc = quantise(sharp)
    fc.shadow.q_buf = sharp.q_buf
    want, gate = AC.reference_of(fc.shadow)
    AC.profile_conditions(fc.shadow, profile, want)
    return fc, want, gate


@functools.lru_cache(maxsize=None)
def long_reference(kind, D, HQ, H, dtype_name):
    """(fp8 case, want, gate) of attn_decode_cases.LONG_LENS in tables of LONG keys"""
    return reference(kind, len(AC.LONG_LENS), D, HQ, H, dtype_name, SCALES, AC.LONG_LENS, AC.LONG)
