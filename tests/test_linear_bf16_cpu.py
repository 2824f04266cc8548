"""CPU tests of the bf16 surface of the C ABI (include/sqllm_hip.h: sqllm_linear_bf16, sqllm_linear_bf16_groups,
SQLLM_DTYPE_BF16 for sqllm_dequant): the symbols are declared and exported, bad arguments are rejected before the device
is touched with the codes of the fp16 entry points, and the new kernels -- csrc/sqllm_linear_bf16.hip and the bf16 kernel
of csrc/sqllm_dequant.hip -- compile for gfx950 within the register budgets of their fp16 counterparts (hipcc
cross-compiles without a GPU)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from squeezellm_amd import build as B
from tests import helpers as H

HEADER = os.path.join(H.ROOT, "include", "sqllm_hip.h")
E_BITS, E_SHAPE, E_NULL, E_ALIGN, E_GROUP = -1, -2, -3, -4, -8


def test_header_declares_the_bf16_entry_points_and_dtype():
    from squeezellm_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+sqllm_linear_bf16\s*\(\s*const\s+sqllm_linear\s*\*\s*\w+\s*,\s*sqllm_stream_t\s+\w+\s*\)\s*;", src)
    assert re.search(r"\bint\s+sqllm_linear_bf16_groups\s*\(\s*const\s+sqllm_linear\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,"
                     r"\s*sqllm_stream_t\s+\w+\s*,\s*int32_t\s*\*\s*\w+\s*\)\s*;", src)
    assert re.search(r"#define\s+SQLLM_DTYPE_BF16\s+3\b", src)
    assert re.search(r"#define\s+SQLLM_ABI_VERSION\s+1\b", src)  # additive
    assert _lib.DTYPE_BF16 == 3
    lib = _lib.load()
    for name in ("sqllm_linear_bf16", "sqllm_linear_bf16_groups"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.SIGNATURES["sqllm_linear_bf16"] == _lib.SIGNATURES["sqllm_linear_f16"]
    assert _lib.SIGNATURES["sqllm_linear_bf16_groups"] == _lib.SIGNATURES["sqllm_linear_f16_groups"]
    assert "sqllm_linear_bf16.hip" in B.SOURCES and B.SOURCES.index("sqllm_linear_bf16.hip") < B.SOURCES.index("sqllm_capi.hip")
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT sqllm_linear_bf16$", syms, flags=re.M) and re.search(r"\bT sqllm_linear_bf16_groups$", syms, flags=re.M)


def _lin(_lib):
    lin = _lib.SqllmLinear()
    lin.op.bits, lin.op.K, lin.op.N = 4, 128, 128
    lin.op.vec = lin.op.qweight = lin.op.mul = lin.op.lookup_table = 16
    return lin


def test_linear_bf16_rejects_what_linear_f16_rejects():
    from squeezellm_amd import _lib

    lib = _lib.load()
    assert lib.sqllm_linear_bf16(None, None) == E_NULL
    for ws, bits in ((None, 4), (8, 4), (20, 4), (16, 2), (16, 5)):  # NULL / misaligned workspace; then the op's own checks
        lin = _lin(_lib)
        lin.workspace, lin.op.bits = ws, bits
        want = lib.sqllm_linear_f16(ctypes.byref(lin), None)
        assert want < 0
        assert lib.sqllm_linear_bf16(ctypes.byref(lin), None) == want, (ws, bits)
        sizes = (ctypes.c_int32 * 1)(1)
        done = ctypes.c_int32(-1)
        assert lib.sqllm_linear_bf16_groups(ctypes.byref(lin), sizes, 1, None, ctypes.byref(done)) == want and done.value == 0
    lin = _lin(_lib)
    assert lib.sqllm_linear_bf16(ctypes.byref(lin), None) == E_NULL  # no workspace
    lin.workspace = 8
    assert lib.sqllm_linear_bf16(ctypes.byref(lin), None) == E_ALIGN
    lin.workspace, lin.op.K = 16, 100
    assert lib.sqllm_linear_bf16(ctypes.byref(lin), None) == E_SHAPE


def test_linear_bf16_groups_of_zero_or_more_than_four_members():
    from squeezellm_amd import _lib

    lib = _lib.load()
    lins = (_lib.SqllmLinear * 5)()
    for i in range(5):
        lins[i].op.bits, lins[i].op.K, lins[i].op.N = 4, 128, 128
        lins[i].op.vec = lins[i].op.qweight = lins[i].op.mul = lins[i].op.lookup_table = 16
        lins[i].workspace = 16
    for size in (0, 5):
        sizes = (ctypes.c_int32 * 1)(size)
        done = ctypes.c_int32(-1)
        assert lib.sqllm_linear_bf16_groups(lins, sizes, 1, None, ctypes.byref(done)) == E_GROUP and done.value == 0
        done = ctypes.c_int32(-1)
        assert lib.sqllm_linear_f16_groups(lins, sizes, 1, None, ctypes.byref(done)) == E_GROUP and done.value == 0  # the same code
    assert lib.sqllm_linear_bf16_groups(None, None, 0, None, None) == 0
    assert lib.sqllm_linear_bf16_groups(None, None, 1, None, None) == E_NULL


def test_dequant_knows_dtype_3():
    from squeezellm_amd import _lib

    lib = _lib.load()

    def rc(**kw):
        d = _lib.SqllmDequant()
        d.op.bits, d.op.K, d.op.N = 4, 128, 64
        d.op.qweight = d.op.lookup_table = 32
        d.out, d.ld, d.out_dtype = 64, 128, _lib.DTYPE_BF16
        for k, v in kw.items():
            setattr(d, k, v)
        return lib.sqllm_dequant(ctypes.byref(d), None)

    # an unknown dtype is E_SHAPE before the alignment is looked at: E_ALIGN shows that 3 is known
    assert rc(out=8) == E_ALIGN and rc(out=20) == E_ALIGN
    assert rc(out=8, out_dtype=2) == E_SHAPE and rc(out=8, out_dtype=4) == E_SHAPE
    # fp16's rules for the leading dimension: >= K, a multiple of 8
    assert rc(ld=132) == E_SHAPE and rc(ld=120) == E_SHAPE and rc(ld=129) == E_SHAPE
    assert rc(ld=136, out=8) == E_ALIGN  # (136 passes the shape checks)
    assert rc(out=None) == E_NULL


# ---- generated code ----

def _compile(tmp_path_factory, src, tag):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp(tag) / "k.s"
    cmd = [hipcc, f"--offload-arch={B.ARCH}", *[f for f in B.FLAGS if f != "-fPIC"], "-S", "--cuda-device-only",
           f"-I{B.INCLUDE}", f"-I{B.CSRC}", os.path.join(B.CSRC, src), "-o", str(out)]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


@pytest.fixture(scope="module")
def asm_linear(tmp_path_factory):
    return _compile(tmp_path_factory, "sqllm_linear_bf16.hip", "asm_linear_bf16")


@pytest.fixture(scope="module")
def asm_dequant(tmp_path_factory):
    return _compile(tmp_path_factory, "sqllm_dequant.hip", "asm_dequant_bf16")


def _meta(asm, prefix):
    return re.findall(r"\.name:\s+(" + prefix + r"\w+).*?\.private_segment_fixed_size:\s+(\d+).*?"
                      r"\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", asm, re.S)


def _bodies(asm, prefix):
    return {m.group(1): m.group(0).split("\n") for m in re.finditer(r"^(" + prefix + r"\w+):.*?^\.Lfunc_end", asm, re.S | re.M)}


LINEAR = "_ZN5sqllm24sqllm_linear_bf16_kernel"


def test_linear_bf16_kernels_instantiations_registers_and_memory_instructions(asm_linear):
    meta = _meta(asm_linear, LINEAR)
    assert len(meta) == 8  # {3, 4} bits x batch tile {1, 2, 4, 8}
    assert {re.search(r"kernelILi([34])ELi(\d)E", m[0]).groups() for m in meta} == {(b, t) for b in "34" for t in "1248"}
    assert not re.search(r"sqllm_fused_matvec", asm_linear)  # a kernel of its own name, no further instantiation of the fp16 one
    for name, scratch, sspill, vgpr, vspill in meta:
        assert int(scratch) == 0 and int(vspill) == 0, (name, scratch, vspill)
        bits, bt = re.search(r"kernelILi([34])ELi(\d)E", name).groups()
        # the limits tests/test_codegen_cpu.py applies to the fp16 linear tiles: four 8-wave workgroups per CU for the one-row
        # tiles and the 4-bit 2-row tile, two for the rest
        limit = 64 if (bt == "1" or (bits == "4" and bt == "2")) else 128
        assert int(vgpr) <= limit, (name, vgpr)
    bodies = _bodies(asm_linear, LINEAR)
    assert len(bodies) == 8
    for name, body in bodies.items():
        flat = [l.strip() for l in body if re.match(r"\s+flat_", l)]
        assert not flat, f"{name}: {flat[:3]}"
        assert sum("v_cvt_pk_bf16_f32" in l for l in body) >= 1, name  # the output is rounded by the hardware conversion
        assert not [l for l in body if "v_cvt_f16_f32" in l or "v_cvt_f32_f16" in l], name  # ... and nothing in it is fp16


def test_dequant_bf16_kernels(asm_dequant):
    prefix = "_ZN5sqllm25sqllm_dequant_bf16_kernel"
    meta = _meta(asm_dequant, prefix)
    assert {re.search(r"kernelILi([34])E", m[0]).group(1) for m in meta} == {"3", "4"} and len(meta) == 2
    for name, scratch, sspill, vgpr, vspill in meta:
        assert int(scratch) == 0 and int(sspill) == 0 and int(vspill) == 0, (name, scratch, sspill, vspill)
        assert int(vgpr) <= 64, (name, vgpr)
    bodies = _bodies(asm_dequant, prefix)
    assert len(bodies) == 2
    for name, body in bodies.items():
        assert sum("v_cvt_pk_bf16_f32" in l for l in body) >= 4, name  # eight values per lane, two per conversion
        assert [l for l in body if re.search(r"global_store_dwordx4", l)], name  # the 16-byte store of eight bf16
