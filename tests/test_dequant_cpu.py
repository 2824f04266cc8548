"""CPU tests of the dense export's C boundary (sqllm_dequant, include/sqllm_hip.h): the symbol is declared and exported,
bad arguments are rejected before the device is touched, the ctypes descriptor matches the C declaration, and the
kernels compile for gfx950 without scratch or spills (hipcc cross-compiles without a GPU)."""
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


def test_sqllm_dequant_is_declared_and_exported():
    from squeezellm_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+sqllm_dequant\s*\(\s*const\s+sqllm_dequant_desc\s*\*\s*\w+\s*,\s*sqllm_stream_t\s+\w+\s*\)\s*;", src)
    assert re.search(r"#define\s+SQLLM_DTYPE_F32\s+0\b", src) and re.search(r"#define\s+SQLLM_DTYPE_F16\s+1\b", src)
    assert re.search(r"#define\s+SQLLM_ABI_VERSION\s+1\b", src)  # the addition is additive
    lib = _lib.load()
    assert hasattr(lib, "sqllm_dequant") and "sqllm_dequant" in _lib.SIGNATURES
    assert "sqllm_dequant.hip" in B.SOURCES
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT sqllm_dequant$", syms, flags=re.M)


def _desc(_lib, **kw):
    """A descriptor that passes every check (dummy device pointers: nothing is launched by a rejected call)."""
    d = _lib.SqllmDequant()
    d.op.bits, d.op.K, d.op.N = 4, 128, 64
    d.op.qweight = d.op.lookup_table = 32
    d.out, d.ld, d.out_dtype = 64, 128, _lib.DTYPE_F16
    for k, v in kw.items():
        if hasattr(d, k):
            setattr(d, k, v)
        else:
            setattr(d.op, k, v)
    return d


def test_rejections_before_the_device_is_touched():
    from squeezellm_amd import _lib

    lib = _lib.load()

    def rc(**kw):
        return lib.sqllm_dequant(ctypes.byref(_desc(_lib, **kw)), None)

    assert lib.sqllm_dequant(None, None) == E_NULL
    assert rc(out=None) == E_NULL
    assert rc(qweight=None) == E_NULL
    assert rc(lookup_table=None) == E_NULL
    for bits in (0, 2, 5, 8):
        assert rc(bits=bits) == E_BITS
    # K / N: positive, K % 32 == 0, N % 4 == 0
    for bad in (dict(K=0), dict(K=-32), dict(K=100, ld=104), dict(N=0), dict(N=-4), dict(N=66)):
        assert rc(**bad) == E_SHAPE, bad
    # ld: >= K, a multiple of 8 elements for fp16 and of 4 for fp32
    assert rc(ld=120) == E_SHAPE and rc(ld=0) == E_SHAPE and rc(ld=-128) == E_SHAPE
    assert rc(ld=132) == E_SHAPE and rc(ld=129) == E_SHAPE
    assert rc(ld=132, out_dtype=_lib.DTYPE_F32, K=100) == E_SHAPE  # (K first)
    assert rc(ld=130, out_dtype=_lib.DTYPE_F32) == E_SHAPE
    for dt in (-1, 2, 7):
        assert rc(out_dtype=dt) == E_SHAPE
    # alignment: qweight and out, 16 bytes
    for p in (8, 20, 4, 33):
        assert rc(qweight=p) == E_ALIGN and rc(out=p) == E_ALIGN
    # sparse operands, as sqllm_launch checks them
    assert rc(rows=16, nnz=-1) == E_SPARSE
    assert rc(rows=16, nnz=5) == E_NULL  # cols / vals missing
    assert rc(rows=16, nnz=5, cols=16) == E_NULL
    assert rc(full_rows=16, topX=-1) == E_SPARSE
    assert rc(full_rows=16, topX=3) == E_NULL  # indices missing
    # vec, mul and batch are ignored
    assert rc(bits=5, vec=None, mul=None, batch=-7) == E_BITS
    assert b"NULL" in lib.sqllm_error_string(E_NULL)


def test_ctypes_descriptor_matches_the_c_declaration(tmp_path):
    from squeezellm_amd import _lib

    # worked from the declaration (LP64): sqllm_op = 4 x int32 (16) + 7 pointers (56) + 2 x int32 (8) + 2 pointers (16) = 96;
    # then out (8) at 96, ld (int64) at 104, out_dtype (int32) at 112, padded to the 8-byte alignment: 120
    D = _lib.SqllmDequant
    assert ctypes.sizeof(_lib.SqllmOp) == 96
    assert (D.op.offset, D.out.offset, D.ld.offset, D.out_dtype.offset, ctypes.sizeof(D)) == (0, 96, 104, 112, 120)
    assert D.ld.size == 8 and D.out_dtype.size == 4
    # ... and from the C compiler, where there is one
    gcc = shutil.which("gcc")
    if gcc:
        c = tmp_path / "layout.c"
        c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sqllm_hip.h"\nint main(void){ printf("%zu %zu %zu %zu\\n", '
                     "sizeof(sqllm_dequant_desc), offsetof(sqllm_dequant_desc, out), offsetof(sqllm_dequant_desc, ld), "
                     "offsetof(sqllm_dequant_desc, out_dtype)); return 0; }\n")
        exe = tmp_path / "layout"
        subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", f"-I{os.path.dirname(HEADER)}", str(c), "-o", str(exe)], check=True)
        got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
        assert [int(v) for v in got] == [120, 96, 104, 112]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("asm_dequant") / "d.s"
    cmd = [hipcc, f"--offload-arch={B.ARCH}", *[f for f in B.FLAGS if f != "-fPIC"], "-S", "--cuda-device-only",
           f"-I{B.INCLUDE}", f"-I{B.CSRC}", os.path.join(B.CSRC, "sqllm_dequant.hip"), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


def test_dequant_kernels_use_no_scratch_and_do_not_spill(asm):
    prefix = "_ZN5sqllm20sqllm_dequant_kernel"
    meta = re.findall(r"\.name:\s+(" + prefix + r"\w+).*?\.private_segment_fixed_size:\s+(\d+).*?"
                      r"\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", asm, re.S)
    assert len(meta) == 4  # {3, 4} bits x {fp16, fp32} output
    assert {re.search(r"kernelILi([34])ELb([01])E", m[0]).groups() for m in meta} == {("3", "0"), ("3", "1"), ("4", "0"), ("4", "1")}
    for name, scratch, sspill, vgpr, vspill in meta:
        assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, (name, scratch, sspill, vspill)
        assert int(vgpr) <= 64, (name, vgpr)  # eight waves per SIMD stay possible: LDS, not registers, sets the occupancy
    bodies = re.findall(r"^(" + prefix + r"\w+):.*?^\.Lfunc_end", asm, re.S | re.M)
    assert len(bodies) == 4
