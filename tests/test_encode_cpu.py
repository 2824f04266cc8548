"""CPU tests of the encode direction's C boundary (sqllm_encode / sqllm_encode_csr, include/sqllm_hip.h): the symbols are
declared and exported, bad arguments are rejected before the device is touched, the ctypes descriptor matches the C
declaration, the kernels compile for gfx950 without scratch or spills (hipcc cross-compiles without a GPU) -- and
nuq.outlier_mask is the mask remove_outliers applies."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from squeezellm_amd import build as B
from tests import helpers as H

HEADER = os.path.join(H.ROOT, "include", "sqllm_hip.h")
E_BITS, E_SHAPE, E_NULL, E_ALIGN, E_SPARSE = -1, -2, -3, -4, -5


def test_encode_symbols_are_declared_and_exported():
    from squeezellm_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+sqllm_encode\s*\(\s*const\s+sqllm_encode_desc\s*\*\s*\w+\s*,\s*sqllm_stream_t\s+\w+\s*\)\s*;", src)
    assert re.search(r"\bint\s+sqllm_encode_csr\s*\(\s*const\s+sqllm_encode_desc\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*,"
                     r"\s*int32_t\s+\w+\s*,\s*sqllm_stream_t\s+\w+\s*\)\s*;", src)
    assert re.search(r"#define\s+SQLLM_ABI_VERSION\s+1\b", src)  # the addition is additive
    lib = _lib.load()
    assert "sqllm_encode.hip" in B.SOURCES
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in ("sqllm_encode", "sqllm_encode_csr"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\bT " + name + "$", syms, flags=re.M)


def _desc(_lib, **kw):
    """A descriptor that passes every check (dummy device pointers: nothing is launched by a rejected call)."""
    d = _lib.SqllmEncode(bits=4, K=128, N=64, weight_dtype=_lib.DTYPE_F16, weight=64, ld=128, lookup_table=32, mask=None,
                         qweight=128, rows=None)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_rejections_before_the_device_is_touched():
    from squeezellm_amd import _lib

    lib = _lib.load()

    def enc(**kw):
        return lib.sqllm_encode(ctypes.byref(_desc(_lib, **kw)), None)

    def csr(cols=16, vals=16, nnz=5, **kw):
        kw = dict(dict(mask=8, rows=4), **kw)
        return lib.sqllm_encode_csr(ctypes.byref(_desc(_lib, **kw)), cols, vals, nnz, None)

    assert lib.sqllm_encode(None, None) == E_NULL and lib.sqllm_encode_csr(None, 16, 16, 5, None) == E_NULL
    for both in (enc, csr):
        assert both(weight=None) == E_NULL and both(lookup_table=None) == E_NULL and both(qweight=None) == E_NULL
        for bits in (0, 2, 5, 8):
            assert both(bits=bits) == E_BITS
        # K / N: positive, K % 32 == 0, N % 4 == 0
        for bad in (dict(K=0), dict(K=-32), dict(K=100, ld=104), dict(N=0), dict(N=-4), dict(N=66)):
            assert both(**bad) == E_SHAPE, bad
        # ld: >= K, a multiple of 8 elements for fp16 and of 4 for fp32
        assert both(ld=120) == E_SHAPE and both(ld=0) == E_SHAPE and both(ld=-128) == E_SHAPE
        assert both(ld=132) == E_SHAPE and both(ld=129) == E_SHAPE
        assert both(ld=130, weight_dtype=_lib.DTYPE_F32) == E_SHAPE
        for dt in (-1, 2, 7):
            assert both(weight_dtype=dt) == E_SHAPE
        # alignment: weight and qweight, 16 bytes
        for p in (8, 20, 4, 33):
            assert both(weight=p) == E_ALIGN and both(qweight=p) == E_ALIGN
        assert both(mask=12, rows=4) == E_ALIGN  # the mask is read 8 bytes at a time
        assert both(mask=8, rows=None) == E_NULL  # rows goes with a mask
    # sqllm_encode_csr: the mask, rows, cols and vals are all required
    assert csr(mask=None) == E_NULL and csr(cols=None) == E_NULL and csr(vals=None) == E_NULL
    assert csr(nnz=-1) == E_SPARSE
    assert b"NULL" in lib.sqllm_error_string(E_NULL)


def test_ctypes_descriptor_matches_the_c_declaration(tmp_path):
    from squeezellm_amd import _lib

    # worked from the declaration (LP64): 4 x int32 (16), weight (8) at 16, ld (int64) at 24, then four pointers: 64 bytes
    D = _lib.SqllmEncode
    fields = ("bits", "K", "N", "weight_dtype", "weight", "ld", "lookup_table", "mask", "qweight", "rows")
    assert [n for n, _ in D._fields_] == list(fields)
    assert [getattr(D, n).offset for n in fields] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56] and ctypes.sizeof(D) == 64
    assert D.ld.size == 8 and D.weight_dtype.size == 4
    # ... and from the C compiler, where there is one
    gcc = shutil.which("gcc")
    if gcc:
        c = tmp_path / "layout.c"
        c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sqllm_hip.h"\nint main(void){ printf("%zu", sizeof(sqllm_encode_desc));\n'
                     + "".join(f'printf(" %zu", offsetof(sqllm_encode_desc, {n}));\n' for n in fields) + "return 0; }\n")
        exe = tmp_path / "layout"
        subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", f"-I{os.path.dirname(HEADER)}", str(c), "-o", str(exe)], check=True)
        got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(v) for v in got] == [64, 0, 4, 8, 12, 16, 24, 32, 40, 48, 56]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("asm_encode") / "e.s"
    cmd = [hipcc, f"--offload-arch={B.ARCH}", *[f for f in B.FLAGS if f != "-fPIC"], "-S", "--cuda-device-only",
           f"-I{B.INCLUDE}", f"-I{B.CSRC}", os.path.join(B.CSRC, "sqllm_encode.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


def test_encode_kernels_use_no_scratch_and_do_not_spill(asm):
    meta = re.findall(r"\.name:\s+(_ZN5sqllm\d+sqllm_encode\w+).*?\.private_segment_fixed_size:\s+(\d+).*?"
                      r"\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", asm, re.S)
    names = [m[0] for m in meta]
    # {3, 4} bits x {fp16, fp32} weights; the scan; the CSR kernel per weight type
    enc = {re.search(r"encode_kernelILi([34])ELb([01])E", n).groups() for n in names if "encode_kernelI" in n}
    assert enc == {(b, f) for b in "34" for f in "01"}
    assert sum("encode_scan_kernel" in n for n in names) == 1 and sum("encode_csr_kernelI" in n for n in names) == 2
    assert len(meta) == 7
    for name, scratch, sspill, vgpr, vspill in meta:
        assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, (name, scratch, sspill, vspill)
        assert int(vgpr) <= 64, (name, vgpr)  # eight waves per SIMD stay possible


def test_outlier_mask_is_the_mask_remove_outliers_applies():
    import torch

    from squeezellm_amd import nuq

    gen = torch.Generator().manual_seed(5)
    w = torch.randn(24, 64, generator=gen)
    w[w == 0] = 0.5  # no zero weights: the outlier matrix then shows the mask
    g = torch.rand(24, 64, generator=gen) ** 4
    # sensitivity only; threshold only; both; num == 0 (0.01 % of 1536 entries), alone and with a threshold
    for sens, thres in ((2.0, None), (0.0, 1.5), (2.0, 1.5), (0.01, None), (0.01, 1.5)):
        m = nuq.outlier_mask(w, g, sensitivity=sens, threshold=thres)
        dense, out = nuq.remove_outliers(w, g, sensitivity=sens, threshold=thres)
        assert m.dtype == torch.bool and m.shape == w.shape
        assert torch.equal(m, out != 0) and torch.equal(m, dense == 0)
        assert torch.equal(torch.where(m, w, torch.zeros_like(w)), out) and torch.equal(torch.where(m, torch.zeros_like(w), w), dense)
        if sens == 0.01 and thres is None:
            assert not m.any()
        else:
            assert m.any() and not m.all()
    both, only_s, only_t = (nuq.outlier_mask(w, g, sensitivity=s, threshold=t) for s, t in ((2.0, 1.5), (2.0, None), (0.0, 1.5)))
    assert torch.equal(both, only_s | only_t) and int((only_s & ~only_t).sum()) > 0 and int((only_t & ~only_s).sum()) > 0
    assert not nuq.outlier_mask(w).any()  # neither given: nothing is an outlier
    # a masked zero weight leaves no outlier, but it is in the mask; fp16 weights are widened first
    w2 = torch.tensor([[0.0, 1.0, -2.0, 0.25]]).half()
    g2 = torch.tensor([[9.0, 0.0, 0.0, 8.0]])
    m2 = nuq.outlier_mask(w2, g2, sensitivity=75.0)  # num = 3: the third largest gradient is 0, two entries lie above it
    assert m2.tolist() == [[True, False, False, True]]
    assert nuq.remove_outliers(w2, g2, sensitivity=75.0)[1].tolist() == [[0.0, 0.0, 0.0, 0.25]]
    with pytest.raises(ValueError, match="gradient"):
        nuq.outlier_mask(w, None, sensitivity=1.0)
