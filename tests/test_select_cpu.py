"""CPU tests of the outlier-selection boundary (sqllm_select / sqllm_select_workspace_bytes / sqllm_outlier_mask,
include/sqllm_hip.h): the symbols are declared and exported, the ctypes structures match the C declarations, bad arguments
are rejected before the device is touched, the workspace is sized without a GPU, the kernels compile for gfx950 without
scratch or spills -- and the host arithmetic of nuq (quantile positions, the torch route of outlier_mask) is right."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from squeezellm_amd import build as B
from tests import helpers as H

HEADER = os.path.join(H.ROOT, "include", "sqllm_hip.h")
E_SHAPE, E_NULL, E_ALIGN = -2, -3, -4
NAMES = ("sqllm_select_workspace_bytes", "sqllm_select", "sqllm_outlier_mask")


def test_select_symbols_are_declared_and_exported():
    from squeezellm_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint64_t\s+sqllm_select_workspace_bytes\s*\(\s*const\s+sqllm_select_desc\s*\*\s*\w+\s*\)\s*;", src)
    assert re.search(r"\bint\s+sqllm_select\s*\(\s*const\s+sqllm_select_desc\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*,"
                     r"\s*sqllm_stream_t\s+\w+\s*\)\s*;", src)
    assert re.search(r"\bint\s+sqllm_outlier_mask\s*\(\s*const\s+sqllm_outlier_desc\s*\*\s*\w+\s*,\s*sqllm_stream_t\s+\w+\s*\)\s*;", src)
    assert re.search(r"#define\s+SQLLM_SELECT_MAX_RANKS\s+8\b", src) and _lib.SELECT_MAX_RANKS == 8
    assert re.search(r"#define\s+SQLLM_ABI_VERSION\s+1\b", src)  # the addition is additive
    lib = _lib.load()
    assert "sqllm_select.hip" in B.SOURCES and B.SOURCES[-1] == "sqllm_capi.hip"  # (build_ablation slices on the last one)
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\bT " + name + "$", syms, flags=re.M)
    assert lib.sqllm_select_workspace_bytes.restype is ctypes.c_int64


SEL_FIELDS = ("dtype", "n_ranks", "values", "rows", "cols", "ld", "ranks", "out", "less")
SEL_OFFSETS = [0, 4, 8, 16, 24, 32, 40, 104, 112]  # LP64: 2 x int32, a pointer, 3 x int64, int64[8], two pointers: 120 bytes
OUT_FIELDS = ("weight_dtype", "grad_dtype", "K", "N", "weight", "ld_w", "gradient", "ld_g", "g_threshold", "w_threshold", "mask", "count")
OUT_OFFSETS = [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72]  # 4 x int32, then eight 8-byte members: 80 bytes


def test_ctypes_structures_match_the_c_declarations(tmp_path):
    from squeezellm_amd import _lib

    S, O = _lib.SqllmSelect, _lib.SqllmOutlier
    assert [n for n, _ in S._fields_] == list(SEL_FIELDS) and [n for n, _ in O._fields_] == list(OUT_FIELDS)
    assert [getattr(S, n).offset for n in SEL_FIELDS] == SEL_OFFSETS and ctypes.sizeof(S) == 120
    assert [getattr(O, n).offset for n in OUT_FIELDS] == OUT_OFFSETS and ctypes.sizeof(O) == 80
    assert S.ranks.size == 64 and S.ld.size == 8 and O.ld_g.size == 8 and O.N.size == 4
    gcc = shutil.which("gcc")
    if gcc:  # ... and from the C compiler, where there is one
        c = tmp_path / "layout.c"
        c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sqllm_hip.h"\nint main(void){ printf("%zu", sizeof(sqllm_select_desc));\n'
                     + "".join(f'printf(" %zu", offsetof(sqllm_select_desc, {n}));\n' for n in SEL_FIELDS)
                     + 'printf(" %zu", sizeof(sqllm_outlier_desc));\n'
                     + "".join(f'printf(" %zu", offsetof(sqllm_outlier_desc, {n}));\n' for n in OUT_FIELDS) + "return 0; }\n")
        exe = tmp_path / "layout"
        subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", f"-I{os.path.dirname(HEADER)}", str(c), "-o", str(exe)], check=True)
        got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
        assert got == [120, *SEL_OFFSETS, 80, *OUT_OFFSETS]


def _sel(_lib, ranks=(3,), **kw):
    """A select descriptor that passes every check (dummy device pointers: a rejected call launches nothing)."""
    d = _lib.SqllmSelect(dtype=_lib.DTYPE_F32, n_ranks=len(ranks), values=64, rows=4, cols=32, ld=32, out=16, less=None)
    for i, r in enumerate(ranks):
        d.ranks[i] = r
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_select_rejections_before_the_device_is_touched():
    from squeezellm_amd import _lib

    lib = _lib.load()
    big = 1 << 24

    def sel(ws=256, ws_bytes=big, **kw):
        return lib.sqllm_select(ctypes.byref(_sel(_lib, **kw)), ws, ws_bytes, None)

    def size(**kw):
        return lib.sqllm_select_workspace_bytes(ctypes.byref(_sel(_lib, **kw)))

    assert lib.sqllm_select(None, 256, big, None) == E_NULL and lib.sqllm_select_workspace_bytes(None) == E_NULL
    assert sel(values=None) == E_NULL and sel(out=None) == E_NULL and sel(ws=None) == E_NULL
    for both in (sel, size):
        for dt in (-1, 2, 7):
            assert both(dtype=dt) == E_SHAPE
        assert both(n_ranks=0) == E_SHAPE and both(n_ranks=9) == E_SHAPE and both(n_ranks=-1) == E_SHAPE
        # a rank outside [0, rows * cols)
        assert both(ranks=(128,)) == E_SHAPE and both(ranks=(-1,)) == E_SHAPE and both(ranks=(0, 5, 127, 1 << 40)) == E_SHAPE
        # cols and ld: multiples of 4 (fp32) / 8 (fp16), ld >= cols; rows, cols >= 1
        assert both(cols=30) == E_SHAPE and both(cols=28, ld=30) == E_SHAPE and both(ld=28) == E_SHAPE and both(ld=0) == E_SHAPE
        assert both(dtype=_lib.DTYPE_F16, cols=28, ld=32) == E_SHAPE and both(dtype=_lib.DTYPE_F16, cols=24, ld=28) == E_SHAPE
        assert both(rows=0) == E_SHAPE and both(cols=0, ld=0) == E_SHAPE and both(rows=-4) == E_SHAPE
        assert both(rows=1 << 30, cols=1 << 10, ld=1 << 10) == E_SHAPE  # rows * cols = 2^40
    assert size(rows=1 << 29, cols=1 << 10, ld=1 << 10) > 0
    need = size()
    assert sel(ws_bytes=need - 1) == E_SHAPE and sel(ws_bytes=0) == E_SHAPE
    for p in (8, 20, 4, 33):
        assert sel(values=p) == E_ALIGN
    assert b"NULL" in lib.sqllm_error_string(E_NULL)


def test_select_workspace_is_sized_without_a_gpu():
    from squeezellm_amd import _lib

    sizes = [_lib.select_workspace_bytes(_lib.DTYPE_F32, n, 4096, 11008) for n in range(1, 9)]
    assert all(b > a > 0 for a, b in zip(sizes, sizes[1:]))  # one histogram per live prefix: grows with n_ranks
    assert sizes[-1] < 1 << 20
    # the shape does not matter, the pass count (fp16: two, fp32: three) does
    assert _lib.select_workspace_bytes(_lib.DTYPE_F32, 4, 1, 4) == sizes[3]
    assert 0 < _lib.select_workspace_bytes(_lib.DTYPE_F16, 4, 4096, 11008) < sizes[3]
    assert _lib.select_workspace_bytes(_lib.DTYPE_F32, 2, 64, 96, ld=104) == sizes[1]
    with pytest.raises(ValueError):
        _lib.select_workspace_bytes(_lib.DTYPE_F32, 9, 4, 32)
    with pytest.raises(ValueError):
        _lib.select_workspace_bytes(_lib.DTYPE_F16, 1, 4, 36)


def _out(_lib, **kw):
    d = _lib.SqllmOutlier(weight_dtype=_lib.DTYPE_F16, grad_dtype=_lib.DTYPE_F32, K=128, N=6, weight=64, ld_w=128, gradient=256, ld_g=128,
                          g_threshold=16, w_threshold=32, mask=8, count=24)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_outlier_mask_rejections_before_the_device_is_touched():
    from squeezellm_amd import _lib

    lib = _lib.load()

    def om(**kw):
        return lib.sqllm_outlier_mask(ctypes.byref(_out(_lib, **kw)), None)

    assert lib.sqllm_outlier_mask(None, None) == E_NULL
    assert om(weight=None) == E_NULL
    assert om(g_threshold=None) == E_NULL and om(gradient=None) == E_NULL  # a gradient without its threshold, and the reverse
    assert om(mask=None, count=None) == E_NULL
    for bad in (dict(K=0), dict(K=-32), dict(K=100, ld_w=104, ld_g=104), dict(N=0), dict(N=-1)):
        assert om(**bad) == E_SHAPE, bad
    for dt in (-1, 2, 7):
        assert om(weight_dtype=dt) == E_SHAPE and om(grad_dtype=dt) == E_SHAPE
    # ld: >= K, a multiple of 8 elements for fp16 and of 4 for fp32, per operand
    assert om(ld_w=120) == E_SHAPE and om(ld_w=0) == E_SHAPE and om(ld_w=132) == E_SHAPE
    assert om(ld_g=120) == E_SHAPE and om(ld_g=130) == E_SHAPE and om(ld_g=-128) == E_SHAPE
    assert om(ld_w=130, weight_dtype=_lib.DTYPE_F32) == E_SHAPE
    # N * K < 2^40, the select's bound (the kernel's partial counts are 32-bit)
    assert om(N=1 << 20, K=1 << 20, ld_w=1 << 20, ld_g=1 << 20) == E_SHAPE
    assert om(N=1 << 19, K=1 << 20, ld_w=1 << 20, ld_g=1 << 20, weight=None) == E_NULL  # (a shape that passes reaches the pointer checks)
    for p in (8, 20, 4, 33):
        assert om(weight=p) == E_ALIGN and om(gradient=p) == E_ALIGN
    assert om(mask=12) == E_ALIGN and om(count=12) == E_ALIGN and om(g_threshold=18) == E_ALIGN and om(w_threshold=6) == E_ALIGN


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("asm_select") / "s.s"
    cmd = [hipcc, f"--offload-arch={B.ARCH}", *[f for f in B.FLAGS if f != "-fPIC"], "-S", "--cuda-device-only",
           f"-I{B.INCLUDE}", f"-I{B.CSRC}", os.path.join(B.CSRC, "sqllm_select.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


def test_select_kernels_use_no_scratch_and_do_not_spill(asm):
    meta = re.findall(r"\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(_ZN5sqllm\d+sqllm_\w+).*?\.private_segment_fixed_size:\s+(\d+).*?"
                      r"\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", asm, re.S)
    names = [m[1] for m in meta]
    # the histogram kernel per {fp16, fp32} x {first digit, later digit}; the pick kernel; the mask kernel per operand type
    hist = {re.search(r"select_hist_kernelILb([01])ELb([01])E", n).groups() for n in names if "select_hist_kernelI" in n}
    mask = {re.search(r"outlier_mask_kernelILb([01])ELb([01])E", n).groups() for n in names if "outlier_mask_kernelI" in n}
    both = {(a, b) for a in "01" for b in "01"}
    assert hist == both and mask == both and sum("select_pick_kernel" in n for n in names) == 1 and len(meta) == 9
    for lds, name, scratch, sspill, vgpr, vspill in meta:
        assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, (name, scratch, sspill, vspill)
        assert int(vgpr) <= 64, (name, vgpr)
        if "select_hist" in name:
            assert int(lds) == 8 * 2048 * 4, (name, lds)  # eight histograms of 2048 counters: two workgroups per CU


@pytest.mark.parametrize("n", [1, 2, 5, 128, 41120, 2 ** 24 + 3])
def test_quantile_ranks_are_numpys_linear_method(n):
    from squeezellm_amd import nuq

    x = np.arange(n)
    for q in (0, 0.25, 0.5, 0.75, 1):
        lo, hi, g = nuq.quantile_ranks(n, q)
        assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1 and 0.0 <= g < 1.0 and (hi > lo or g == 0.0)
        assert lo + g == np.quantile(x, q), (n, q)


def test_cpu_tensors_keep_the_torch_route_and_have_no_select():
    import torch

    from squeezellm_amd import nuq

    gen = torch.Generator().manual_seed(11)
    w = torch.randn(24, 64, generator=gen)
    w[w == 0] = 0.5
    g = torch.rand(24, 64, generator=gen) ** 4
    for wt in (w, w.half()):
        for sens, thres in ((2.0, None), (0.0, 1.5), (2.0, 1.5), (0.01, 1.5)):
            m = nuq.outlier_mask(wt, g, sensitivity=sens, threshold=thres)
            dense, out = nuq.remove_outliers(wt, g, sensitivity=sens, threshold=thres)
            assert m.dtype == torch.bool and torch.equal(m, out != 0) and torch.equal(m, dense == 0) and m.any() and not m.all()
    with pytest.raises(ValueError, match="CUDA"):
        nuq.order_statistics(w, [0])
    with pytest.raises(ValueError, match="CUDA"):
        nuq.quantiles(w, [0.5])
    with pytest.raises(ValueError, match="CUDA"):
        nuq.sensitivity_threshold(g, 2.0)
    assert nuq.sensitivity_threshold(g, 0.01) is None  # num == 0: no cut, on any device
    with pytest.raises(ValueError, match="mutually exclusive"):
        nuq.quantize_state_dict({}, {}, 4, outlier_config={"outlier_config": []}, outlier_range=1.8)
