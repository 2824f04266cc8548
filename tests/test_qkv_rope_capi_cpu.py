"""C ABI of the attention front (sqllm_qkv_rope_f16 / sqllm_qkv_rope_bf16, include/sqllm_hip.h) on a host without a GPU: the
symbols, the struct's layout, the size of the workspace, and every rejection the header lists -- each returned before the
device is touched (operand pointers are fake 16-byte-aligned integers: nothing dereferences them)."""
import ctypes
import os
import shutil
import subprocess

import pytest

E_BITS, E_SHAPE, E_NULL, E_ALIGN, E_SPARSE, E_BATCH, E_OPTION, E_GROUP = -1, -2, -3, -4, -5, -6, -7, -8
FIELDS = ("q", "k", "v", "bias_q", "bias_k", "bias_v", "out_q", "out_k", "out_v", "cos", "sin", "positions", "n_pos", "head_dim",
          "layout", "workspace")
# worked from the declaration (LP64): three sqllm_op of 96 bytes, nine pointers, three int32 padded to the next pointer
OFFSETS = [0, 96, 192, 288, 296, 304, 312, 320, 328, 336, 344, 352, 360, 364, 368, 376]
SIZE = 384


@pytest.fixture(scope="module")
def lib():
    from squeezellm_amd import _lib

    return _lib.load()


def _qkv(batch=0, K=128, Nq=256, Nk=128, Nv=128, bits=4, D=64):
    """a descriptor that passes every check up to the launch -- never handed over unedited: see `passes` below"""
    from squeezellm_amd import _lib

    r = _lib.SqllmQkvRope()
    for i, (op, N) in enumerate(((r.q, Nq), (r.k, Nk), (r.v, Nv))):
        op.bits, op.batch, op.K, op.N = bits, batch, K, N
        op.vec, op.qweight, op.lookup_table = 0x1000, 0x20000 + 0x10000 * i, 0x24000 + 0x10000 * i
    r.out_q, r.out_k, r.out_v = 0x100000, 0x110000, 0x120000
    r.cos, r.sin, r.positions = 0x200000, 0x210000, 0x220000
    r.n_pos, r.head_dim, r.layout = 16, D, _lib.ROPE_HALF
    r.workspace = 0x400000
    return r


def test_symbols_and_binding(lib):
    from squeezellm_amd import _lib

    header = open(os.path.join(os.path.dirname(_lib.HERE), "include", "sqllm_hip.h")).read()
    for name in ("sqllm_qkv_rope_workspace_bytes", "sqllm_qkv_rope_f16", "sqllm_qkv_rope_bf16"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header
    assert lib.sqllm_qkv_rope_workspace_bytes.restype is ctypes.c_int64
    assert "#define SQLLM_ROPE_HALF 0" in header and "#define SQLLM_ROPE_INTERLEAVED 1" in header
    assert (_lib.ROPE_HALF, _lib.ROPE_INTERLEAVED) == (0, 1)
    assert lib.sqllm_abi_version() == 1  # symbols were added, nothing changed


def test_ctypes_structure_matches_the_c_declaration(tmp_path):
    from squeezellm_amd import _lib

    S = _lib.SqllmQkvRope
    assert ctypes.sizeof(_lib.SqllmOp) == 96
    assert [n for n, _ in S._fields_] == list(FIELDS)
    assert [getattr(S, n).offset for n in FIELDS] == OFFSETS and ctypes.sizeof(S) == SIZE
    assert S.n_pos.size == S.head_dim.size == S.layout.size == 4
    gcc = shutil.which("gcc")
    if gcc:  # ... and from the C compiler, where there is one
        include = os.path.join(os.path.dirname(_lib.HERE), "include")
        c = tmp_path / "layout.c"
        c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sqllm_hip.h"\nint main(void){ printf("%zu", sizeof(sqllm_qkv_rope));\n'
                     + "".join(f'printf(" %zu", offsetof(sqllm_qkv_rope, {n}));\n' for n in FIELDS) + "return 0; }\n")
        exe = tmp_path / "layout"
        subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", f"-I{include}", str(c), "-o", str(exe)], check=True)
        got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
        assert got == [SIZE, *OFFSETS]


@pytest.mark.parametrize("widths", [(8, 8, 4), (456, 456, 132), (384, 128, 128), (4096, 1024, 1024)])
@pytest.mark.parametrize("batch", [-1, 0, 1, 2, 5, 8, 19])
def test_workspace_is_three_accumulator_planes_and_two_pair_planes(lib, widths, batch):
    from squeezellm_amd import _lib

    ops = [_lib.SqllmOp(N=n, batch=batch) for n in widths]
    lin = [int(lib.sqllm_linear_workspace_bytes(ctypes.byref(o))) for o in ops]
    pair = [(8 * max(batch, 1) * (n // 2) + 15) // 16 * 16 for n in widths[:2]]  # [batch, N / 2] 64-bit words, rounded up as the planes are
    got = int(lib.sqllm_qkv_rope_workspace_bytes(*[ctypes.byref(o) for o in ops]))
    assert got == sum(lin) + sum(pair) == _lib.qkv_rope_workspace_bytes(*widths, batch)
    assert all(b % 16 == 0 for b in lin + pair)  # every plane starts 16-byte aligned


def test_workspace_of_nothing_is_zero(lib):
    from squeezellm_amd import _lib

    op = ctypes.byref(_lib.SqllmOp(N=64, batch=4))
    assert lib.sqllm_qkv_rope_workspace_bytes(None, op, op) == 0
    assert lib.sqllm_qkv_rope_workspace_bytes(op, op, None) == 0
    assert lib.sqllm_qkv_rope_workspace_bytes(op, ctypes.byref(_lib.SqllmOp(N=0, batch=4)), op) == 0


@pytest.mark.parametrize("entry", ["sqllm_qkv_rope_f16", "sqllm_qkv_rope_bf16"])
def test_rejections_before_the_device_is_touched(lib, entry):
    from squeezellm_amd import _lib

    fn = getattr(lib, entry)

    def rc(edit, **kw):
        r = _qkv(**kw)
        edit(r)
        return fn(ctypes.byref(r), None)

    def passes(edit, **kw):
        """`edit` is NOT rejected by the checks of this entry point: with q's qweight taken away as well, the call gets as far as
        the linear's own validation, which runs behind them, and comes back with ITS code.  (Nothing here may reach a launch:
        the operands are fake, and on a host with a GPU a launch would run a kernel on them.)"""
        def both(r):
            edit(r)
            r.q.qweight = None
        return rc(both, **kw) == E_NULL

    assert fn(None, None) == E_NULL
    # a member with an output of its own; members that differ in vec / K / bits / batch (N may differ)
    for m in "qkv":
        assert rc(lambda r: setattr(getattr(r, m), "mul", 0x5000)) == E_GROUP
    for m in "kv":
        assert rc(lambda r: setattr(getattr(r, m), "vec", 0x1100)) == E_GROUP
        assert rc(lambda r: setattr(getattr(r, m), "K", 256)) == E_GROUP
        assert rc(lambda r: setattr(getattr(r, m), "bits", 3)) == E_GROUP
        assert rc(lambda r: setattr(getattr(r, m), "batch", 2)) == E_GROUP
    assert rc(lambda r: setattr(r.q, "batch", 5)) == E_GROUP
    # head_dim odd, < 2, or no divisor of N_q or N_k; no positions in the tables
    assert rc(lambda r: setattr(r, "head_dim", 63)) == E_SHAPE
    assert rc(lambda r: setattr(r, "head_dim", 1)) == E_SHAPE
    assert rc(lambda r: setattr(r, "head_dim", 0)) == E_SHAPE
    assert rc(lambda r: setattr(r, "head_dim", -2)) == E_SHAPE
    assert rc(lambda r: setattr(r, "head_dim", 256)) == E_SHAPE  # divides N_q, not N_k
    assert rc(lambda r: setattr(r, "head_dim", 24)) == E_SHAPE
    assert passes(lambda r: None, Nq=192)  # three heads: nothing to reject
    assert rc(lambda r: None, Nq=160) == E_SHAPE  # 160 / 64
    assert rc(lambda r: None, Nk=96) == E_SHAPE
    assert rc(lambda r: setattr(r, "n_pos", 0)) == E_SHAPE
    assert rc(lambda r: setattr(r, "n_pos", -3)) == E_SHAPE
    # v's width is free of head_dim
    assert passes(lambda r: None, Nv=68)
    for name in ("out_q", "out_k", "out_v", "cos", "sin", "positions", "workspace"):
        assert rc(lambda r: setattr(r, name, None)) == E_NULL, name
    assert rc(lambda r: setattr(r, "workspace", 0x400008)) == E_ALIGN
    assert rc(lambda r: setattr(r, "layout", 2)) == E_OPTION
    assert rc(lambda r: setattr(r, "layout", -1)) == E_OPTION
    assert passes(lambda r: setattr(r, "layout", _lib.ROPE_INTERLEAVED))

    # outputs that overlap each other or the workspace (batch 0 = one row: out_q is 512 bytes, out_k and out_v 256)
    assert rc(lambda r: setattr(r, "out_k", r.out_q)) == E_SHAPE
    assert rc(lambda r: setattr(r, "out_k", r.out_q + 510)) == E_SHAPE
    assert passes(lambda r: setattr(r, "out_k", r.out_q + 512))  # adjacent is fine
    assert rc(lambda r: setattr(r, "out_v", r.out_k + 16)) == E_SHAPE
    assert rc(lambda r: setattr(r, "out_v", r.out_q - 128)) == E_SHAPE
    need = _lib.qkv_rope_workspace_bytes(256, 128, 128, 0)
    assert rc(lambda r: setattr(r, "out_q", r.workspace)) == E_SHAPE
    assert rc(lambda r: setattr(r, "out_v", r.workspace + need - 2)) == E_SHAPE
    assert passes(lambda r: setattr(r, "out_v", r.workspace + need))
    assert rc(lambda r: setattr(r, "out_k", r.workspace - 254)) == E_SHAPE
    assert passes(lambda r: setattr(r, "out_k", r.workspace - 256))

    # everything the linear rejects, with the linear's codes (the same edit on all members, so that the group stays a group)
    def every(name, value):
        def edit(r):
            for m in (r.q, r.k, r.v):
                setattr(m, name, value)
        return edit

    assert rc(every("bits", 2)) == E_BITS
    assert rc(every("bits", 5)) == E_BITS
    assert rc(every("K", 100)) == E_SHAPE
    assert rc(every("K", 0)) == E_SHAPE
    assert rc(lambda r: setattr(r.v, "N", 126)) == E_SHAPE
    assert rc(every("batch", -2)) == E_BATCH
    assert rc(every("vec", None)) == E_NULL
    assert rc(lambda r: setattr(r.q, "qweight", None)) == E_NULL
    assert rc(lambda r: setattr(r.v, "lookup_table", None)) == E_NULL
    assert rc(lambda r: setattr(r.k, "qweight", r.k.qweight + 4)) == E_ALIGN
    assert rc(lambda r: setattr(r.k, "nnz", -1) or setattr(r.k, "rows", 0x5000)) == E_SPARSE
    assert rc(lambda r: setattr(r.v, "nnz", 7) or setattr(r.v, "rows", 0x5000)) == E_NULL  # cols / vals missing
    assert rc(lambda r: setattr(r.q, "topX", 3) or setattr(r.q, "full_rows", 0x6000)) == E_NULL  # indices missing


def test_the_limits_of_the_division_free_index_arithmetic(lib):
    """c / head_dim is a 32-bit multiply-high (exact up to N * head_dim = 2^32) and the batch row comes out of b * N by an
    fp32 multiply (b * N below 2^31, at most 2^20 rows): beyond those, SQLLM_E_SHAPE"""
    fn = lib.sqllm_qkv_rope_f16
    r = _qkv(Nq=1 << 20, Nk=1 << 13, D=1 << 13)  # N_q * D = 2^33
    r.out_k, r.out_v, r.workspace = 0x10000000, 0x11000000, 0x40000000
    assert fn(ctypes.byref(r), None) == E_SHAPE
    r = _qkv(batch=1 << 15, Nq=1 << 16, Nk=128, D=64)  # batch * N_q = 2^31
    r.out_q, r.out_k, r.out_v, r.workspace = 0x100000000, 0x300000000, 0x400000000, 0x1000000000
    assert fn(ctypes.byref(r), None) == E_SHAPE


def test_the_63_contribution_limit_applies_per_member(lib):
    """the linear's SQLLM_E_SHAPE from the planner, for a group whose k member alone has a CSR term (cf. test_gated_capi_cpu)"""
    K = 64 * 1024  # K / 1024 + 2 = 66 possible chunks per row
    r = _qkv(K=K)
    r.k.rows, r.k.cols, r.k.vals, r.k.nnz = 0x5000, 0x6000, 0x7000, 1000
    assert lib.sqllm_qkv_rope_f16(ctypes.byref(r), None) == E_SHAPE
    assert lib.sqllm_qkv_rope_bf16(ctypes.byref(r), None) == E_SHAPE


def test_the_source_is_part_of_the_product_build():
    from squeezellm_amd import build as B

    assert "sqllm_linear_qkv.hip" in B.SOURCES
    assert B.SOURCES.index("sqllm_linear_qkv.hip") < B.SOURCES.index("sqllm_capi.hip") == len(B.SOURCES) - 1
