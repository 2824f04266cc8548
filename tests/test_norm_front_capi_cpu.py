"""C ABI of the norm fronts (sqllm_gated_norm_f16 / _bf16, sqllm_qkv_rope_norm_f16 / _bf16, include/sqllm_hip.h) on a host
without a GPU: the symbols, the struct, every rejection the header lists -- each returned before the device is touched
(operand pointers are fake 16-byte-aligned integers: nothing dereferences them) --, the parent entries' rejections
inherited with their codes, the parent entries themselves untouched, and, on the host layer linked against recording
launchers (tests/native/launch_recorder.cpp + tests/native/norm_front_hooks.cpp), the launch hooks: a missing kernel is an
error, and each entry reaches its own hook with the norm's weight and eps."""
import ctypes
import os
import shutil
import subprocess

import pytest

from tests import helpers as H
from tests.test_gated_capi_cpu import _gated
from tests.test_qkv_rope_capi_cpu import _qkv

E_BITS, E_SHAPE, E_NULL, E_ALIGN, E_SPARSE, E_BATCH, E_OPTION, E_GROUP = -1, -2, -3, -4, -5, -6, -7, -8
ENTRIES = [("sqllm_gated_norm_f16", "sqllm_gated_f16", "gated"), ("sqllm_gated_norm_bf16", "sqllm_gated_bf16", "gated"),
           ("sqllm_qkv_rope_norm_f16", "sqllm_qkv_rope_f16", "qkv"), ("sqllm_qkv_rope_norm_bf16", "sqllm_qkv_rope_bf16", "qkv")]
WEIGHT = 0x300000  # clear of every operand of _gated() and _qkv()


@pytest.fixture(scope="module")
def lib():
    from squeezellm_amd import _lib

    return _lib.load()


def _norm(weight=WEIGHT, eps=1e-6):
    from squeezellm_amd import _lib

    return _lib.SqllmRmsNorm(weight=weight, eps=eps)


def test_symbols_struct_and_header(lib):
    from squeezellm_amd import _lib

    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "sqllm_hip.h")).read()
    for name, _, _ in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header
        assert len(_lib.SIGNATURES[name]) == 3
    assert "typedef struct sqllm_rmsnorm" in header
    # pointer, float, padded to the pointer's alignment
    assert ctypes.sizeof(_lib.SqllmRmsNorm) == 16 and _lib.SqllmRmsNorm.weight.offset == 0 and _lib.SqllmRmsNorm.eps.offset == 8
    assert lib.sqllm_abi_version() == 1  # symbols were added; the existing structs and symbols are as they were
    assert ctypes.sizeof(_lib.SqllmGated) == 2 * 96 + 4 * 8 + 8 and ctypes.sizeof(_lib.SqllmQkvRope) == 384
    # the header says what the issue asks it to say
    for phrase in ("NEVER rounded to 16 bits", "depends on the order above", "rounds x * r to 16 bits", "in ascending k"):
        assert phrase in header, phrase


@pytest.mark.parametrize("entry,parent,kind", ENTRIES)
def test_the_norm_descriptor_is_checked_first(lib, entry, parent, kind):
    fn = getattr(lib, entry)
    d = _gated() if kind == "gated" else _qkv()
    assert fn(ctypes.byref(d), None, None) == E_NULL  # no norm descriptor
    assert fn(ctypes.byref(d), ctypes.byref(_norm(weight=None)), None) == E_NULL
    assert fn(None, ctypes.byref(_norm()), None) == E_NULL  # no parent descriptor
    for eps in (-1e-6, -0.0 - 1.0, float("nan"), float("inf"), -float("inf")):
        assert fn(ctypes.byref(d), ctypes.byref(_norm(eps=eps)), None) == E_OPTION, eps
    # ... ahead of the parent's own checks: a descriptor the parent rejects, with a bad eps, reports the eps
    d.workspace = None
    assert fn(ctypes.byref(d), ctypes.byref(_norm(eps=-1.0)), None) == E_OPTION
    assert fn(ctypes.byref(d), ctypes.byref(_norm()), None) == E_NULL


@pytest.mark.parametrize("entry,parent,kind", ENTRIES)
def test_a_weight_that_overlaps_an_output_or_the_workspace(lib, entry, parent, kind):
    from squeezellm_amd import _lib

    fn = getattr(lib, entry)

    def rc(weight, batch=0):
        d = _gated(batch=batch) if kind == "gated" else _qkv(batch=batch)
        return fn(ctypes.byref(d), ctypes.byref(_norm(weight=weight)), None)

    K = 128  # the weight is 2 K = 256 bytes
    if kind == "gated":
        outs = [(0x3000, 2 * 128)]
        ws = (0x40000, _lib.gated_workspace_bytes(128, 0))
    else:
        outs = [(0x100000, 2 * 256), (0x110000, 2 * 128), (0x120000, 2 * 128)]
        ws = (0x400000, _lib.qkv_rope_workspace_bytes(256, 128, 128, 0))
    for a0, n in outs + [ws]:
        assert rc(a0) == E_SHAPE                 # starts where the range starts
        assert rc(a0 + n - 2) == E_SHAPE         # starts on its last element
        assert rc(a0 - 2 * K + 2) == E_SHAPE     # ends on its first element
    # several rows: the ranges grow with the batch
    a0, n = outs[-1]
    assert rc(a0 + 5 * n - 2, batch=5) == E_SHAPE


@pytest.mark.parametrize("entry,parent,kind", ENTRIES)
def test_the_parents_rejections_are_inherited_with_their_codes(lib, entry, parent, kind):
    fn, pfn = getattr(lib, entry), getattr(lib, parent)
    make = _gated if kind == "gated" else _qkv
    first = "gate" if kind == "gated" else "q"
    second = "up" if kind == "gated" else "k"

    def member(which, name, value):
        return lambda d: setattr(getattr(d, which), name, value)

    def every(name, value):
        def edit(d):
            for w in (("gate", "up") if kind == "gated" else ("q", "k", "v")):
                setattr(getattr(d, w), name, value)
        return edit

    edits = [
        (member(first, "mul", 0x5000), E_GROUP), (member(second, "vec", 0x1100), E_GROUP), (member(second, "K", 256), E_GROUP),
        (member(second, "bits", 3), E_GROUP), (member(second, "batch", 2), E_GROUP),
        (lambda d: setattr(d, "workspace", None), E_NULL), (lambda d: setattr(d, "workspace", d.workspace + 8), E_ALIGN),
        (every("bits", 2), E_BITS), (every("bits", 5), E_BITS), (every("K", 100), E_SHAPE), (every("K", 0), E_SHAPE),
        (every("batch", -2), E_BATCH), (every("vec", None), E_NULL), (member(first, "qweight", None), E_NULL),
        (member(second, "lookup_table", None), E_NULL), (member(second, "qweight", 0x12004), E_ALIGN),
        (lambda d: setattr(getattr(d, second), "nnz", -1) or setattr(getattr(d, second), "rows", 0x5000), E_SPARSE),
        (lambda d: setattr(getattr(d, second), "nnz", 7) or setattr(getattr(d, second), "rows", 0x5000), E_NULL),
        (lambda d: setattr(getattr(d, first), "topX", 3) or setattr(getattr(d, first), "full_rows", 0x6000), E_NULL),
    ]
    if kind == "gated":
        edits += [(lambda d: setattr(d, "act", 1), E_OPTION), (member("up", "N", 256), E_GROUP), (lambda d: setattr(d, "out", None), E_NULL),
                  (every("N", 126), E_SHAPE)]
    else:
        edits += [(lambda d: setattr(d, "layout", 2), E_OPTION), (lambda d: setattr(d, "head_dim", 63), E_SHAPE),
                  (lambda d: setattr(d, "head_dim", 48), E_SHAPE), (lambda d: setattr(d, "n_pos", 0), E_SHAPE),
                  (lambda d: setattr(d, "out_k", None), E_NULL), (lambda d: setattr(d, "cos", None), E_NULL),
                  (lambda d: setattr(d, "positions", None), E_NULL), (lambda d: setattr(d, "out_k", d.out_q + 2), E_SHAPE),
                  (lambda d: setattr(d, "out_v", d.workspace), E_SHAPE)]
    for i, (edit, code) in enumerate(edits):
        d = make()
        edit(d)
        assert pfn(ctypes.byref(d), None) == code, i            # the parent entry, as it ever did
        assert fn(ctypes.byref(d), ctypes.byref(_norm()), None) == code, i  # the norm entry: the same code
    # the 63-contribution limit, per member, from the planner
    d = make(K=64 * 1024)
    m = getattr(d, second)
    m.rows, m.cols, m.vals, m.nnz = 0x5000, 0x6000, 0x7000, 1000
    assert pfn(ctypes.byref(d), None) == E_SHAPE and fn(ctypes.byref(d), ctypes.byref(_norm(weight=0x30000000)), None) == E_SHAPE


def test_the_sources_are_part_of_the_product_build():
    from squeezellm_amd import build as B

    for src in ("sqllm_linear_gated_norm.hip", "sqllm_linear_qkv_norm.hip"):
        assert src in B.SOURCES and B.SOURCES.index(src) < B.SOURCES.index("sqllm_capi.hip")
    assert B.SOURCES[-1] == "sqllm_capi.hip"
    for h in ("sqllm_norm_front.h", "sqllm_pair_finish.h", "sqllm_rope_finish.h"):
        assert os.path.join(B.CSRC, h) in B.HEADERS  # (a changed header makes the library stale)


def test_launch_hooks_on_the_recording_host_layer(tmp_path):
    """a missing kernel is an error, not a fallback; each entry reaches its own hook; the norm hooks get weight and eps"""
    from squeezellm_amd import build as B

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found: the recording host layer cannot be built")
    native = os.path.join(H.ROOT, "tests", "native")
    exe = str(tmp_path / "norm_front_hooks")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-DSQLLM_RECORDER_NO_MAIN", f"-I{B.INCLUDE}", f"-I{B.CSRC}",
                        os.path.join(B.CSRC, "sqllm_capi.hip"), os.path.join(native, "launch_recorder.cpp"),
                        os.path.join(native, "norm_front_hooks.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = {ln.split()[0]: dict(kv.split("=") for kv in ln.split()[1:]) for ln in out.stdout.splitlines()}
    ns = lines["nohook"]["notsupported"]
    assert int(ns) != 0
    assert all(lines["nohook"][k] == ns for k in ("gated", "gated_norm", "qkv", "qkv_norm"))
    # the parents' kernels linked in, the norm fronts' not: the norm entries still fail, and launch nothing
    p = lines["parenthooks"]
    assert (p["gated"], p["qkv"], p["gated_norm"], p["qkv_norm"]) == ("0", "0", ns, ns) and p["calls"] == "1,1,0,0"
    assert lines["gated"] == {"rc": "0", "calls": "1,0,0,0", "n_seg": "2"}
    assert lines["qkv"] == {"rc": "0", "calls": "1,1,1,0", "n_seg": "3"}
    for name, calls, n_seg in (("gated_norm", "1,0,1,0", "2"), ("qkv_norm", "1,1,1,1", "3")):
        f = lines[name]
        assert (f["rc"], f["calls"], f["n_seg"]) == ("0", calls, n_seg)
        assert int(f["weight"], 16) == 0x300000 and float(f["eps"]) == pytest.approx(1e-5, rel=1e-6)
        assert int(f["x"], 16) == 0x1000 and f["same_pair"] == "1"  # the parent's launch arguments, the parent's workspace layout
    # the table of nine kinds.  Nothing registered: every one of the 18 front entries is an error
    assert len(lines["nohook_all"]) == 18 and all(v == ns for v in lines["nohook_all"].values())
    # recording launchers in all nine slots: each entry reaches the slot of its own kind and no other, with its descriptors' fields
    KINDS = ("gated", "gated_norm", "ep", "qkv", "qkv_norm", "qkv_cache", "qkv_norm_cache", "qkv_cache_fp8", "qkv_norm_cache_fp8")
    entry_of = {"gated": "sqllm_gated", "gated_norm": "sqllm_gated_norm", "ep": "sqllm_linear_ep", "qkv": "sqllm_qkv_rope",
                "qkv_norm": "sqllm_qkv_rope_norm", "qkv_cache": "sqllm_qkv_rope_cache", "qkv_norm_cache": "sqllm_qkv_rope_norm_cache",
                "qkv_cache_fp8": "sqllm_qkv_rope_cache_fp8", "qkv_norm_cache_fp8": "sqllm_qkv_rope_norm_cache_fp8"}
    reached = {k: v for k, v in lines.items() if k.startswith("reach:")}
    assert sorted(reached) == sorted(f"reach:{entry_of[kind]}_{t}" for kind in KINDS for t in ("f16", "bf16"))
    assert set(lines["nohook_all"]) == {k[len("reach:"):] for k in reached}
    for i, kind in enumerate(KINDS):
        for t in ("f16", "bf16"):
            f = reached[f"reach:{entry_of[kind]}_{t}"]
            assert f["rc"] == "0" and int(f["kind"]) == i, (kind, t, f)
            assert f["calls"] == ",".join("1" if j == i else "0" for j in range(9)), (kind, t, f["calls"])
            gated, qkv, norm, cache, fp8 = kind.startswith("gated"), kind.startswith("qkv"), "norm" in kind, "cache" in kind, "fp8" in kind
            assert f["n_seg"] == ("2" if gated else "3" if qkv else "1") and int(f["x"], 16) == 0x1000
            assert (f["pair"], f["has_qkv"], f["has_vn"], f["has_kc"]) == tuple(str(int(b)) for b in (gated, qkv, norm, cache))
            # the epilogue's residual and activation code (SQLLM_ACT_GELU = 3), nowhere else
            assert (int(f["residual"], 16), f["act"]) == ((0x500000, "3") if kind == "ep" else (0, "0"))
            if norm:  # VecNorm
                assert int(f["weight"], 16) == 0x300000 and float(f["eps"]) == pytest.approx(1e-5, rel=1e-6)
            if qkv:  # QkvRope
                assert (f["pair_q"], f["pair_k"], f["n_pos"], f["head_dim"], f["interleaved"]) == ("1", "1", "16", "64", "0")
                assert [int(f[k], 16) for k in ("cos", "sin", "positions")] == [0x200000, 0x210000, 0x220000]
            if cache:  # KvCache
                assert [int(f[k], 16) for k in ("k_cache", "v_cache", "slots")] == [0x800000, 0x900000, 0x230000]
                assert (f["n_slots"], f["slot_stride"], f["head_stride"], f["write_out"]) == ("8", "128", "64", "11")
                assert (f["fp8"], f["scales_ok"]) == (("1", "1") if fp8 else ("0", "0"))
            if fp8:  # k_scale 0.5, v_scale 4: the reciprocals
                assert (float(f["inv_k"]), float(f["inv_v"])) == (2.0, 0.25)
