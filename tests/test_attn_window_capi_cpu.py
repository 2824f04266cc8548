"""C ABI of the sliding-window decode attention (sqllm_attn_decode_window_f16 / _bf16 / _fp8_f16 / _fp8_bf16 and
sqllm_attn_window_workspace_bytes, include/sqllm_hip.h) on a host without a GPU: the symbols and their signatures, the window
among the counts in the documented order -- returned before the device is touched (operand pointers are fake integers: nothing
dereferences them) --, the size function, and the launch hooks on the host layer alone: a missing window kernel is an error,
never the kernels without a window."""
import ctypes
import os
import shutil
import subprocess

import pytest

from tests import attn_window_cases as WC
from tests import helpers as H
from tests import test_attn_decode_capi_cpu as TA

E_SHAPE, E_NULL, E_ALIGN, E_OPTION = -2, -3, -4, -7
ENTRIES = ("sqllm_attn_decode_window_f16", "sqllm_attn_decode_window_bf16")
ENTRIES_FP8 = ("sqllm_attn_decode_window_fp8_f16", "sqllm_attn_decode_window_fp8_bf16")
INT32_MAX = (1 << 31) - 1


@pytest.fixture(scope="module")
def lib():
    from squeezellm_amd import _lib

    return _lib.load()


def _desc(fp8=False, **kw):
    from squeezellm_amd import _lib

    a = _lib.SqllmAttnDecodeFp8() if fp8 else _lib.SqllmAttnDecode()
    for name, _ in _lib.SqllmAttnDecode._fields_:
        setattr(a, name, getattr(TA._desc(), name))
    if fp8:
        a.k_scale, a.v_scale = 0.5, 4.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_symbols_signatures_and_header_text(lib):
    from squeezellm_amd import _lib

    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "sqllm_hip.h")).read()
    P = ctypes.POINTER
    for names, S in ((ENTRIES, _lib.SqllmAttnDecode), (ENTRIES_FP8, _lib.SqllmAttnDecodeFp8)):
        for name in names:
            assert hasattr(lib, name) and name + "(" in header
            assert _lib.SIGNATURES[name] == [P(S), ctypes.c_int32, ctypes.c_void_p] and getattr(lib, name).restype is ctypes.c_int
    assert hasattr(lib, "sqllm_attn_window_workspace_bytes") and "sqllm_attn_window_workspace_bytes(" in header
    assert _lib.SIGNATURES["sqllm_attn_window_workspace_bytes"] == [ctypes.c_int32] * 6
    assert lib.sqllm_attn_window_workspace_bytes.restype is ctypes.c_int64
    assert lib.sqllm_abi_version() == 1  # symbols were added, nothing changed
    for text in ("lo = max(0, L - window)", "kv_idx > q_idx - sliding_window", "ABSOLUTE key ranges [256 i, 256 i + 256)",
                 "a row with L <= window holds EXACTLY THE BITS", "advanced by lo / block_size entries", "never\n *     make a row NaN",
                 "free or reuse the\n *     blocks behind the window", "ceil(window / block_size) + 1 physical", "A USED table entry outside [0, n_slots)",
                 "win_parts = min(n_parts, (window - 1 + 255) / 256 + 1)", "RELATIVE partition", "ONE when win_parts == 1",
                 "window < 1 counts among the counts", "hipErrorNotSupported, never with the kernels above"):
        assert text in header, text


@pytest.mark.parametrize("entry", ENTRIES + ENTRIES_FP8)
def test_the_window_is_a_count_in_the_siblings_order(lib, entry):
    fn = getattr(lib, entry)
    fp8 = "fp8" in entry

    def rc(window, **kw):
        return fn(ctypes.byref(_desc(fp8, **kw)), window, None)

    # (nothing here may reach a launch: every call below carries at least one defect)
    assert fn(None, 4, None) == E_NULL and fn(None, 0, None) == E_NULL
    for name in ("q", "out", "k_cache", "v_cache", "block_table", "seq_lens", "workspace"):
        assert rc(0, **{name: None}) == E_NULL and rc(-1, **{name: None, "scale": float("nan")}) == E_NULL, name  # NULL comes first
    for w in (0, -1, -INT32_MAX - 1):
        assert rc(w) == E_SHAPE
        assert rc(w, scale=float("inf"), out=TA.Q, q=TA.Q + 1) == E_SHAPE  # ... before the scale, the overlap, the alignment
    for name in ("batch", "n_q_heads", "n_kv_heads", "head_dim", "n_slots", "block_size", "max_blocks", "table_stride"):
        assert rc(4, **{name: 0}) == E_SHAPE, name
    for w in (1, 4, 64, 65, INT32_MAX):  # served: the call gets as far as the scale
        assert rc(w, scale=float("nan")) == E_OPTION
    assert rc(4, head_dim=32, q_stride=128, out_stride=128, scale=float("nan")) == E_SHAPE and rc(4, batch=65) == E_SHAPE
    assert rc(4, q=TA.Q + 1) == E_ALIGN and rc(4, workspace=TA.WS + 2) == E_ALIGN
    # the workspace that must not overlap is the windowed one: 40 blocks of 16 keys are 3 partitions, a window of 4 touches 2
    from squeezellm_amd import _lib

    big = dict(max_blocks=40, table_stride=40, n_slots=1024)
    ws_w, ws_all = _lib.attn_window_workspace_bytes(2, 4, 64, 40, 16, 4), _lib.attn_decode_workspace_bytes(2, 4, 64, 40, 16)
    assert ws_w * 3 == ws_all * 2
    assert rc(4, workspace=TA.OUT - ws_w + 2, q=TA.Q + 1, **big) == E_SHAPE and rc(4, workspace=TA.OUT - ws_w, q=TA.Q + 1, **big) == E_ALIGN
    assert rc(INT32_MAX, workspace=TA.OUT - ws_w, q=TA.Q + 1, **big) == E_SHAPE  # (three partitions: it reaches out)
    if fp8:
        assert rc(4, k_scale=0.0) == E_OPTION and rc(0, k_scale=0.0) == E_SHAPE


def test_the_size_function(lib):
    from squeezellm_amd import _lib

    for batch, hq, D, mb, bs in ((2, 4, 64, 40, 16), (64, 32, 128, 2048, 16), (1, 8, 128, 1, 515), (3, 6, 64, 105, 5), (1, 1, 64, 1 << 27, 16),
                                 (64, 65535, 128, INT32_MAX, INT32_MAX)):
        whole = _lib.attn_decode_workspace_bytes(batch, hq, D, mb, bs)
        for W in (1, 2, 100, 256, 257, 258, 640, 4096, 1 << 20, INT32_MAX - 1, INT32_MAX):
            got = _lib.attn_window_workspace_bytes(batch, hq, D, mb, bs, W)
            assert got == batch * hq * WC.win_parts(mb, bs, W) * (D + 2) * 4, (batch, hq, D, mb, bs, W)
            assert 0 < got <= whole
        assert _lib.attn_window_workspace_bytes(batch, hq, D, mb, bs, INT32_MAX) == whole
    assert [WC.win_parts(40, 16, W) for W in (100, 640, 1)] == [2, 3, 1]
    for bad in ((0, 4, 64, 4, 16, 4), (2, 4, 64, 4, 16, 0), (2, 4, 64, 4, 16, -1), (2, 4, 64, 0, 16, 4)):
        assert _lib.attn_window_workspace_bytes(*bad) == 0


def test_the_sources_are_part_of_the_product_build():
    from squeezellm_amd import build as B

    for src in ("sqllm_attn_window.hip", "sqllm_attn_window_fp8.hip"):
        assert src in B.SOURCES and B.SOURCES.index(src) < B.SOURCES.index("sqllm_capi.hip")
    assert B.SOURCES[-1] == "sqllm_capi.hip"


def test_launch_hooks_on_the_host_layer_alone(tmp_path):
    """a missing window kernel is an error, not a fallback onto the kernels without a window; each entry reaches the slot of its
    cache type and no other, with the window and win_parts of the host fields"""
    from squeezellm_amd import build as B

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found: the host layer cannot be built alone")
    native = os.path.join(H.ROOT, "tests", "native")
    exe = str(tmp_path / "attn_window_hooks")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-DSQLLM_RECORDER_NO_MAIN", f"-I{B.INCLUDE}", f"-I{B.CSRC}",
                        os.path.join(B.CSRC, "sqllm_capi.hip"), os.path.join(native, "launch_recorder.cpp"),
                        os.path.join(native, "attn_window_hooks.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = {ln.split()[0]: dict(kv.split("=") for kv in ln.split()[1:]) for ln in out.stdout.splitlines()}
    ns = lines["nohook"]["notsupported"]
    failed = {"notsupported": ns, "f16": ns, "bf16": ns, "fp8_f16": ns, "fp8_bf16": ns}
    assert int(ns) != 0 and lines["nohook"] == failed
    assert lines["plainhooks"] == dict(failed, plain="0")  # the four slots without a window are filled: still an error, none is called
    assert lines["only_window"] == dict(failed, f16="0", bf16="0", calls="2,0", plain="0")
    assert lines["only_window_fp8"] == dict(failed, fp8_f16="0", fp8_bf16="0", calls="0,2", plain="0")
    assert lines["eight"] == {"failed": "0", "calls": "0,0", "plain": "8", "window": "0", "n_parts": "3"}
    common = dict(rc="0", plain="0", batch="2", q_len="0", capacity="640")
    assert lines["f16"] == dict(common, calls="1,0", window="100", n_parts="2", bf16="0", fp8="0", scale="0.125", v_scale="1")
    assert lines["bf16"] == dict(common, calls="2,0", window="640", n_parts="3", bf16="1", fp8="0", scale="0.125", v_scale="1")
    assert lines["fp8_f16"] == dict(common, calls="2,1", window="1", n_parts="1", bf16="0", fp8="1", scale="0.0625", v_scale="4")
    assert lines["fp8_bf16"] == dict(common, calls="2,2", window=str(INT32_MAX), n_parts="3", bf16="1", fp8="1", scale="0.0625", v_scale="4")
    assert lines["window0"] == {"rc": str(E_SHAPE)} and lines["windowneg"] == {"rc": str(E_SHAPE)}
    assert lines["window1nan"] == {"rc": str(E_OPTION)} and lines["nullq"] == {"rc": str(E_NULL), "calls": "2,2"}
