"""ctypes binding of libsqllm_hip.so (C ABI: include/sqllm_hip.h).

The library is the product; there is NO CPU or PyTorch fallback.  If it has not been built
(`python -m squeezellm_amd.build`) loading raises, and every operator call raises with it.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_int, c_int32, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
# SQLLM_LIB: measurement aid -- load a variant build of the same library (tools/ab_libs.sh) instead
LIB_PATH = os.environ.get("SQLLM_LIB") or os.path.join(HERE, "libsqllm_hip.so")


class SqllmOp(ctypes.Structure):
    """struct sqllm_op (include/sqllm_hip.h)."""

    _fields_ = [
        ("bits", c_int32),
        ("batch", c_int32),
        ("K", c_int32),
        ("N", c_int32),
        ("vec", c_void_p),
        ("qweight", c_void_p),
        ("mul", c_void_p),
        ("lookup_table", c_void_p),
        ("rows", c_void_p),
        ("cols", c_void_p),
        ("vals", c_void_p),
        ("nnz", c_int32),
        ("topX", c_int32),
        ("full_rows", c_void_p),
        ("full_row_indices", c_void_p),
    ]


class SqllmLinear(ctypes.Structure):
    """struct sqllm_linear (include/sqllm_hip.h): op.vec / op.mul carry fp16 pointers."""

    _fields_ = [("op", SqllmOp), ("bias", c_void_p), ("workspace", c_void_p)]


class SqllmGated(ctypes.Structure):
    """struct sqllm_gated (include/sqllm_hip.h): gate and up share op.vec (fp16 / bf16); their op.mul stay NULL."""

    _fields_ = [("gate", SqllmOp), ("up", SqllmOp), ("bias_gate", c_void_p), ("bias_up", c_void_p), ("out", c_void_p),
                ("workspace", c_void_p), ("act", c_int32)]


ACT_SILU = 0  # SQLLM_ACT_SILU
ACT_IDENTITY = 1  # SQLLM_ACT_IDENTITY ... the epilogue's codes (sqllm_linear_ep_*; the gated pair takes SiLU only)
ACT_RELU = 2
ACT_GELU = 3
ACT_GELU_TANH = 4


class SqllmLinearEp(ctypes.Structure):
    """struct sqllm_linear_ep (include/sqllm_hip.h): a fused linear, the residual (or NULL; may be lin.op.mul) and the activation code."""

    _fields_ = [("lin", SqllmLinear), ("residual", c_void_p), ("act", c_int32)]


ROPE_HALF, ROPE_INTERLEAVED = 0, 1  # SQLLM_ROPE_*


class SqllmRmsNorm(ctypes.Structure):
    """struct sqllm_rmsnorm (include/sqllm_hip.h): the norm weight (16-bit [K], the type of x) and eps of a norm front."""

    _fields_ = [("weight", c_void_p), ("eps", ctypes.c_float)]


class SqllmKvCache(ctypes.Structure):
    """struct sqllm_kv_cache (include/sqllm_hip.h): where the cache entries of the attention front store k and v -- element
    [slots[b] * slot_stride + head * head_stride + d] of each cache, strides in elements."""

    _fields_ = [("k_cache", c_void_p), ("v_cache", c_void_p), ("slots", c_void_p), ("n_slots", ctypes.c_int32),
                ("slot_stride", ctypes.c_int64), ("head_stride", ctypes.c_int64)]


ATTN_PARTITION = 256  # SQLLM_ATTN_PARTITION: keys per partition of the decode attention


class SqllmAttnDecode(ctypes.Structure):
    """struct sqllm_attn_decode (include/sqllm_hip.h): one query per row over the KV cache of sqllm_kv_cache's layout -- key p
    of row b in slot block_table[b, p / block_size] * block_size + p % block_size; strides in elements."""

    _fields_ = [("q", c_void_p), ("out", c_void_p), ("k_cache", c_void_p), ("v_cache", c_void_p), ("block_table", c_void_p),
                ("seq_lens", c_void_p), ("batch", c_int32), ("n_q_heads", c_int32), ("n_kv_heads", c_int32), ("head_dim", c_int32),
                ("n_slots", c_int32), ("block_size", c_int32), ("max_blocks", c_int32), ("table_stride", c_int32),
                ("slot_stride", ctypes.c_int64), ("head_stride", ctypes.c_int64), ("q_stride", ctypes.c_int64),
                ("out_stride", ctypes.c_int64), ("scale", ctypes.c_float), ("workspace", c_void_p)]


class SqllmKvCacheFp8(ctypes.Structure):
    """struct sqllm_kv_cache_fp8 (include/sqllm_hip.h): sqllm_kv_cache for caches of 1-byte e4m3fn elements -- strides in bytes,
    one fp32 scale per cache."""

    _fields_ = SqllmKvCache._fields_ + [("k_scale", ctypes.c_float), ("v_scale", ctypes.c_float)]


class SqllmAttnDecodeFp8(ctypes.Structure):
    """struct sqllm_attn_decode_fp8 (include/sqllm_hip.h): sqllm_attn_decode over caches of 1-byte e4m3fn elements -- the caches'
    strides in bytes, the scales the front was given."""

    _fields_ = SqllmAttnDecode._fields_ + [("k_scale", ctypes.c_float), ("v_scale", ctypes.c_float)]


class SqllmAttnAppend(ctypes.Structure):
    """struct sqllm_attn_append (include/sqllm_hip.h): sqllm_attn_decode for q_len new tokens per sequence -- batch counts
    sequences, q and out have batch * q_len rows, q_lens (or NULL) the real tokens of each sequence."""

    _fields_ = SqllmAttnDecode._fields_ + [("q_lens", c_void_p), ("q_len", c_int32)]


class SqllmAttnAppendFp8(ctypes.Structure):
    """struct sqllm_attn_append_fp8 (include/sqllm_hip.h): sqllm_attn_decode_fp8 followed by the same two fields."""

    _fields_ = SqllmAttnDecodeFp8._fields_ + [("q_lens", c_void_p), ("q_len", c_int32)]


class SqllmQkvRope(ctypes.Structure):
    """struct sqllm_qkv_rope (include/sqllm_hip.h): q, k and v share op.vec (fp16 / bf16); their op.mul stay NULL."""

    _fields_ = [("q", SqllmOp), ("k", SqllmOp), ("v", SqllmOp), ("bias_q", c_void_p), ("bias_k", c_void_p), ("bias_v", c_void_p),
                ("out_q", c_void_p), ("out_k", c_void_p), ("out_v", c_void_p), ("cos", c_void_p), ("sin", c_void_p),
                ("positions", c_void_p), ("n_pos", c_int32), ("head_dim", c_int32), ("layout", c_int32), ("workspace", c_void_p)]


class SqllmPlan(ctypes.Structure):
    """struct sqllm_plan (include/sqllm_hip.h)."""

    _fields_ = [(n, c_int32) for n in (
        "col_tiles", "k_slices", "groups_per_wave", "dense_blocks", "csr_blocks", "topx_blocks", "grid_x", "grid_y")]


class SqllmNuq(ctypes.Structure):
    """struct sqllm_nuq (include/sqllm_hip.h): one exact weighted k-means fit per row."""

    _fields_ = [("bits", c_int32), ("N", c_int32), ("K", c_int32), ("values", c_void_p), ("weights", c_void_p),
                ("centroids", c_void_p), ("cost", c_void_p)]


class SqllmDequant(ctypes.Structure):
    """struct sqllm_dequant_desc (include/sqllm_hip.h): op.vec / op.mul / op.batch are ignored."""

    _fields_ = [("op", SqllmOp), ("out", c_void_p), ("ld", ctypes.c_int64), ("out_dtype", c_int32)]


class SqllmEncode(ctypes.Structure):
    """struct sqllm_encode_desc (include/sqllm_hip.h): weight + codebooks (+ mask) -> qweight (+ rows)."""

    _fields_ = [("bits", c_int32), ("K", c_int32), ("N", c_int32), ("weight_dtype", c_int32), ("weight", c_void_p),
                ("ld", ctypes.c_int64), ("lookup_table", c_void_p), ("mask", c_void_p), ("qweight", c_void_p), ("rows", c_void_p)]


SELECT_MAX_RANKS = 8  # SQLLM_SELECT_MAX_RANKS


class SqllmSelect(ctypes.Structure):
    """struct sqllm_select_desc (include/sqllm_hip.h): up to 8 exact order statistics of a matrix."""

    _fields_ = [("dtype", c_int32), ("n_ranks", c_int32), ("values", c_void_p), ("rows", ctypes.c_int64), ("cols", ctypes.c_int64),
                ("ld", ctypes.c_int64), ("ranks", ctypes.c_int64 * SELECT_MAX_RANKS), ("out", c_void_p), ("less", c_void_p)]


class SqllmOutlier(ctypes.Structure):
    """struct sqllm_outlier_desc (include/sqllm_hip.h): weight (+ gradient) and device thresholds -> byte mask, count."""

    _fields_ = [("weight_dtype", c_int32), ("grad_dtype", c_int32), ("K", c_int32), ("N", c_int32), ("weight", c_void_p),
                ("ld_w", ctypes.c_int64), ("gradient", c_void_p), ("ld_g", ctypes.c_int64), ("g_threshold", c_void_p),
                ("w_threshold", c_void_p), ("mask", c_void_p), ("count", c_void_p)]


DTYPE_F32, DTYPE_F16 = 0, 1  # SQLLM_DTYPE_*
DTYPE_BF16 = 3  # (sqllm_dequant's out_dtype only; 2 is unassigned)

P = c_void_p  # every device pointer crosses as void*

_DENSE = [P, P, P, P, c_int, c_int, P]
_DENSE_B = [P, P, P, P, c_int, c_int, c_int, c_int, P]
_SPMV = [P, P, P, P, P, c_int, P, P, c_int, c_int, c_int, P]
_SPMV_B = [P, P, P, P, P, c_int, P, P, c_int, c_int, c_int, c_int, c_int, P]
_HYB = [P, P, P, P, P, P, P, c_int, P, P, c_int, c_int, c_int, c_int, P]
_HYB_B = [P, P, P, P, P, P, P, c_int, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P]
_BAL = [P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, P]

# every symbol include/sqllm_hip.h declares -> argtypes (restype is int unless noted)
SIGNATURES = {
    "sqllm_launch": [POINTER(SqllmOp), P],
    "sqllm_launch_sequence": [POINTER(SqllmOp), c_int32, P, POINTER(c_int32)],
    "sqllm_profile_sequence": [POINTER(SqllmOp), c_int32, P, c_int32, POINTER(ctypes.c_float)],
    "sqllm_launch_group": [POINTER(SqllmOp), c_int32, P],
    "sqllm_launch_groups": [POINTER(SqllmOp), POINTER(c_int32), c_int32, P, POINTER(c_int32)],
    "sqllm_profile_groups": [POINTER(SqllmOp), POINTER(c_int32), c_int32, P, c_int32, POINTER(ctypes.c_float)],
    "sqllm_workspace_bytes": [POINTER(SqllmOp), c_int32],
    "sqllm_launch_ws": [POINTER(SqllmOp), P, ctypes.c_int64, P],
    "sqllm_launch_group_ws": [POINTER(SqllmOp), c_int32, P, ctypes.c_int64, P],
    "sqllm_launch_groups_ws": [POINTER(SqllmOp), POINTER(c_int32), c_int32, P, ctypes.c_int64, P, POINTER(c_int32)],
    "sqllm_profile_groups_ws": [POINTER(SqllmOp), POINTER(c_int32), c_int32, P, ctypes.c_int64, P, c_int32, POINTER(ctypes.c_float)],
    "sqllm_linear_workspace_bytes": [POINTER(SqllmOp)],
    "sqllm_linear_f16": [POINTER(SqllmLinear), P],
    "sqllm_linear_f16_groups": [POINTER(SqllmLinear), POINTER(c_int32), c_int32, P, POINTER(c_int32)],
    "sqllm_linear_bf16": [POINTER(SqllmLinear), P],
    "sqllm_linear_bf16_groups": [POINTER(SqllmLinear), POINTER(c_int32), c_int32, P, POINTER(c_int32)],
    "sqllm_gated_workspace_bytes": [POINTER(SqllmOp)],
    "sqllm_gated_f16": [POINTER(SqllmGated), P],
    "sqllm_gated_bf16": [POINTER(SqllmGated), P],
    "sqllm_linear_ep_f16": [POINTER(SqllmLinearEp), P],
    "sqllm_linear_ep_bf16": [POINTER(SqllmLinearEp), P],
    "sqllm_qkv_rope_workspace_bytes": [POINTER(SqllmOp), POINTER(SqllmOp), POINTER(SqllmOp)],
    "sqllm_qkv_rope_f16": [POINTER(SqllmQkvRope), P],
    "sqllm_qkv_rope_bf16": [POINTER(SqllmQkvRope), P],
    "sqllm_gated_norm_f16": [POINTER(SqllmGated), POINTER(SqllmRmsNorm), P],
    "sqllm_gated_norm_bf16": [POINTER(SqllmGated), POINTER(SqllmRmsNorm), P],
    "sqllm_qkv_rope_norm_f16": [POINTER(SqllmQkvRope), POINTER(SqllmRmsNorm), P],
    "sqllm_qkv_rope_norm_bf16": [POINTER(SqllmQkvRope), POINTER(SqllmRmsNorm), P],
    "sqllm_qkv_rope_cache_f16": [POINTER(SqllmQkvRope), POINTER(SqllmKvCache), P],
    "sqllm_qkv_rope_cache_bf16": [POINTER(SqllmQkvRope), POINTER(SqllmKvCache), P],
    "sqllm_qkv_rope_norm_cache_f16": [POINTER(SqllmQkvRope), POINTER(SqllmRmsNorm), POINTER(SqllmKvCache), P],
    "sqllm_qkv_rope_norm_cache_bf16": [POINTER(SqllmQkvRope), POINTER(SqllmRmsNorm), POINTER(SqllmKvCache), P],
    "sqllm_attn_decode_workspace_bytes": [c_int32, c_int32, c_int32, c_int32, c_int32],
    "sqllm_attn_decode_f16": [POINTER(SqllmAttnDecode), P],
    "sqllm_attn_decode_bf16": [POINTER(SqllmAttnDecode), P],
    "sqllm_qkv_rope_cache_fp8_f16": [POINTER(SqllmQkvRope), POINTER(SqllmKvCacheFp8), P],
    "sqllm_qkv_rope_cache_fp8_bf16": [POINTER(SqllmQkvRope), POINTER(SqllmKvCacheFp8), P],
    "sqllm_qkv_rope_norm_cache_fp8_f16": [POINTER(SqllmQkvRope), POINTER(SqllmRmsNorm), POINTER(SqllmKvCacheFp8), P],
    "sqllm_qkv_rope_norm_cache_fp8_bf16": [POINTER(SqllmQkvRope), POINTER(SqllmRmsNorm), POINTER(SqllmKvCacheFp8), P],
    "sqllm_attn_decode_fp8_f16": [POINTER(SqllmAttnDecodeFp8), P],
    "sqllm_attn_decode_fp8_bf16": [POINTER(SqllmAttnDecodeFp8), P],
    "sqllm_attn_append_f16": [POINTER(SqllmAttnAppend), P],
    "sqllm_attn_append_bf16": [POINTER(SqllmAttnAppend), P],
    "sqllm_attn_append_fp8_f16": [POINTER(SqllmAttnAppendFp8), P],
    "sqllm_attn_append_fp8_bf16": [POINTER(SqllmAttnAppendFp8), P],
    "sqllm_attn_window_workspace_bytes": [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32],
    "sqllm_attn_decode_window_f16": [POINTER(SqllmAttnDecode), c_int32, P],
    "sqllm_attn_decode_window_bf16": [POINTER(SqllmAttnDecode), c_int32, P],
    "sqllm_attn_decode_window_fp8_f16": [POINTER(SqllmAttnDecodeFp8), c_int32, P],
    "sqllm_attn_decode_window_fp8_bf16": [POINTER(SqllmAttnDecodeFp8), c_int32, P],
    "sqllm_abi_version": [],
    "sqllm_error_string": [c_int],
    "sqllm_set_option": [c_char_p, c_int],
    "sqllm_get_option": [c_char_p, POINTER(c_int)],
    "sqllm_plan_query": [POINTER(SqllmOp), POINTER(SqllmPlan)],
    "sqllm_nuq_workspace_bytes": [POINTER(SqllmNuq)],
    "sqllm_nuq_fit": [POINTER(SqllmNuq), P, ctypes.c_int64, P],
    "sqllm_dequant": [POINTER(SqllmDequant), P],
    "sqllm_encode": [POINTER(SqllmEncode), P],
    "sqllm_encode_csr": [POINTER(SqllmEncode), P, P, c_int32, P],
    "sqllm_select_workspace_bytes": [POINTER(SqllmSelect)],
    "sqllm_select": [POINTER(SqllmSelect), P, ctypes.c_int64, P],
    "sqllm_outlier_mask": [POINTER(SqllmOutlier), P],
}
for _b in (3, 4):
    SIGNATURES[f"sqllm_vecquant{_b}matmul_nuq_perchannel"] = _DENSE
    SIGNATURES[f"sqllm_vecquant{_b}matmul_nuq_perchannel_batched"] = _DENSE_B
    SIGNATURES[f"sqllm_vecquant{_b}matmul_spmv_nuq_perchannel"] = _SPMV
    SIGNATURES[f"sqllm_vecquant{_b}matmul_spmv_nuq_perchannel_batched"] = _SPMV_B
    SIGNATURES[f"sqllm_vecquant{_b}matmul_spmv_hybrid_nuq_perchannel"] = _HYB
    SIGNATURES[f"sqllm_vecquant{_b}matmul_spmv_hybrid_nuq_perchannel_batched"] = _HYB_B
    SIGNATURES[f"sqllm_vecquant{_b}matmul_spmv_balanced_nuq_perchannel"] = _BAL

_lib = None


def load() -> ctypes.CDLL:
    """dlopen the library once and attach prototypes.  Raises if it is missing: by design."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own libamdhip64; it must be the HIP runtime this library binds to
    # (device pointers and streams come from torch), so it has to be loaded first
    import torch  # noqa: F401

    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -m squeezellm_amd.build). "
            "There is no CPU/PyTorch fallback for the quant_cuda operators."
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        if os.environ.get("SQLLM_LIB") and not hasattr(lib, name):
            continue  # (measurement aid: an older build of the library under SQLLM_LIB lacks the newer entry points)
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.argtypes = argtypes
        fn.restype = (c_char_p if name == "sqllm_error_string" else
                      ctypes.c_int64 if name in ("sqllm_linear_workspace_bytes", "sqllm_workspace_bytes", "sqllm_nuq_workspace_bytes",
                                               "sqllm_select_workspace_bytes", "sqllm_gated_workspace_bytes",
                                               "sqllm_qkv_rope_workspace_bytes", "sqllm_attn_decode_workspace_bytes",
                                               "sqllm_attn_window_workspace_bytes") else c_int)
    if lib.sqllm_abi_version() != 1:
        raise RuntimeError(f"libsqllm_hip.so ABI {lib.sqllm_abi_version()} != 1 expected by this package")
    _lib = lib
    # SQLLM_OPTIONS="name=value,..." (measurement aid): library options applied to the current device at load
    for item in filter(None, os.environ.get("SQLLM_OPTIONS", "").split(",")):
        name, _, value = item.partition("=")
        rc = lib.sqllm_set_option(name.strip().encode(), int(value))
        if rc != 0:
            raise RuntimeError(f"SQLLM_OPTIONS: {item!r} rejected ({rc})")
    return lib


def error_string(code: int) -> str:
    return load().sqllm_error_string(int(code)).decode()


def check(code: int, what: str) -> None:
    if code != 0:
        kind = ValueError if code < 0 else RuntimeError
        raise kind(f"{what}: {error_string(code)} (code {code})")


option_epoch = 0  # bumped by every set_option: sizes cached on the Python side (quant_cuda's workspace needs) are per epoch


def set_option(name: str, value: int) -> None:
    global option_epoch
    check(load().sqllm_set_option(name.encode(), int(value)), f"sqllm_set_option({name})")
    option_epoch += 1


def get_option(name: str) -> int:
    v = c_int(0)
    check(load().sqllm_get_option(name.encode(), ctypes.byref(v)), f"sqllm_get_option({name})")
    return v.value


def linear_workspace_bytes(N: int, batch: int = 0) -> int:
    """Bytes of zero-filled device memory one fused linear of this shape needs (no GPU needed)."""
    op = SqllmOp(N=N, batch=batch)
    return int(load().sqllm_linear_workspace_bytes(ctypes.byref(op)))


def gated_workspace_bytes(N: int, batch: int = 0) -> int:
    """Bytes of zero-filled device memory one gated pair of this shape needs (no GPU needed)."""
    op = SqllmOp(N=N, batch=batch)
    return int(load().sqllm_gated_workspace_bytes(ctypes.byref(op)))


def qkv_rope_workspace_bytes(n_q: int, n_k: int, n_v: int, batch: int = 0) -> int:
    """Bytes of zero-filled device memory one q/k/v rotary launch of these widths needs (no GPU needed)."""
    ops = [SqllmOp(N=n, batch=batch) for n in (n_q, n_k, n_v)]
    return int(load().sqllm_qkv_rope_workspace_bytes(*[ctypes.byref(o) for o in ops]))


def attn_decode_workspace_bytes(batch: int, n_q_heads: int, head_dim: int, max_blocks: int, block_size: int) -> int:
    """Bytes of device memory (contents irrelevant) one decode attention of these shapes needs (no GPU needed)."""
    return int(load().sqllm_attn_decode_workspace_bytes(batch, n_q_heads, head_dim, max_blocks, block_size))


def attn_window_workspace_bytes(batch: int, n_q_heads: int, head_dim: int, max_blocks: int, block_size: int, window: int) -> int:
    """Bytes of device memory (contents irrelevant) one sliding-window decode attention of these shapes needs (no GPU needed)."""
    return int(load().sqllm_attn_window_workspace_bytes(batch, n_q_heads, head_dim, max_blocks, block_size, window))


def workspace_bytes(bits: int, K: int, N: int, batch: int, nnz: int = 0, topX: int = 0, n_ops: int = 1) -> int:
    """Bytes of caller workspace a batched op (or a group of `n_ops` such ops over one vec) can use (no GPU needed)."""
    ops = (SqllmOp * n_ops)()
    for op in ops:
        op.bits, op.batch, op.K, op.N, op.nnz, op.topX = bits, batch, K, N, nnz, topX
        op.vec = op.qweight = op.mul = op.lookup_table = 16  # (sizing looks at shapes and at which pointers are non-NULL)
        if nnz:
            op.rows = op.cols = op.vals = 16
        if topX:
            op.full_rows = op.full_row_indices = 16
    return int(load().sqllm_workspace_bytes(ops, n_ops))


def plan_query(bits: int, K: int, N: int, batch: int = 0, nnz: int = 0, topX: int = 0) -> dict:
    """Launch geometry the library would use (no GPU needed)."""
    op = SqllmOp(bits=bits, batch=batch, K=K, N=N, nnz=nnz, topX=topX)
    # planning only looks at shapes and at whether the sparse pointers are non-NULL
    if nnz:
        op.rows = op.cols = op.vals = 1
    if topX:
        op.full_rows = op.full_row_indices = 1
    plan = SqllmPlan()
    check(load().sqllm_plan_query(ctypes.byref(op), ctypes.byref(plan)), "sqllm_plan_query")
    return {n: getattr(plan, n) for n, _ in SqllmPlan._fields_}


def nuq_workspace_bytes(bits: int, N: int, K: int) -> int:
    """Bytes of device workspace one sqllm_nuq_fit of these shapes needs (no GPU needed); raises on bad shapes."""
    d = SqllmNuq(bits=bits, N=N, K=K)
    n = int(load().sqllm_nuq_workspace_bytes(ctypes.byref(d)))
    check(n if n < 0 else 0, "sqllm_nuq_workspace_bytes")
    return n


def select_workspace_bytes(dtype: int, n_ranks: int, rows: int, cols: int, ld: int | None = None) -> int:
    """Bytes of device workspace one sqllm_select of these shapes needs (no GPU needed); raises on bad shapes."""
    d = SqllmSelect(dtype=dtype, n_ranks=n_ranks, rows=rows, cols=cols, ld=cols if ld is None else ld)
    n = int(load().sqllm_select_workspace_bytes(ctypes.byref(d)))
    check(n if n < 0 else 0, "sqllm_select_workspace_bytes")
    return n
