"""C ABI of the gated fused linear (sqllm_gated_f16 / sqllm_gated_bf16, include/sqllm_hip.h) on a host without a GPU: the
symbols, the size of the workspace, and every rejection the header lists -- each returned before the device is touched
(operand pointers are fake 16-byte-aligned integers: nothing dereferences them)."""
import ctypes

import pytest

E_BITS, E_SHAPE, E_NULL, E_ALIGN, E_SPARSE, E_BATCH, E_OPTION, E_GROUP = -1, -2, -3, -4, -5, -6, -7, -8


@pytest.fixture(scope="module")
def lib():
    from squeezellm_amd import _lib

    return _lib.load()


def _gated(batch=0, K=128, N=128, bits=4):
    """a descriptor that passes every check up to the launch"""
    from squeezellm_amd import _lib

    g = _lib.SqllmGated()
    for op in (g.gate, g.up):
        op.bits, op.batch, op.K, op.N = bits, batch, K, N
        op.vec, op.qweight, op.lookup_table = 0x1000, 0x2000, 0x4000
    g.up.qweight, g.up.lookup_table = 0x12000, 0x14000
    g.out, g.workspace, g.act = 0x3000, 0x40000, _lib.ACT_SILU
    return g


def test_symbols_and_binding(lib):
    from squeezellm_amd import _lib

    for name in ("sqllm_gated_workspace_bytes", "sqllm_gated_f16", "sqllm_gated_bf16"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.sqllm_gated_workspace_bytes.restype is ctypes.c_int64
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib.HERE), "include", "sqllm_hip.h")).read()
    assert "#define SQLLM_ACT_SILU 0" in header and _lib.ACT_SILU == 0
    # the struct as the header lays it out: two ops, two biases, out, workspace, act (padded to the pointers' alignment)
    assert ctypes.sizeof(_lib.SqllmGated) == 2 * ctypes.sizeof(_lib.SqllmOp) + 4 * 8 + 8
    assert _lib.SqllmGated.up.offset == ctypes.sizeof(_lib.SqllmOp) and _lib.SqllmGated.act.offset == 2 * ctypes.sizeof(_lib.SqllmOp) + 32


@pytest.mark.parametrize("N", [4, 68, 456, 11008])
@pytest.mark.parametrize("batch", [-1, 0, 1, 2, 5, 8, 19])
def test_workspace_is_two_accumulator_planes_and_the_pair_plane(lib, N, batch):
    from squeezellm_amd import _lib

    op = _lib.SqllmOp(N=N, batch=batch)
    lin = int(lib.sqllm_linear_workspace_bytes(ctypes.byref(op)))
    pair = (8 * max(batch, 1) * N + 15) // 16 * 16  # rounded up as sqllm_linear_workspace_bytes rounds
    assert int(lib.sqllm_gated_workspace_bytes(ctypes.byref(op))) == 2 * lin + pair == _lib.gated_workspace_bytes(N, batch)
    assert lin % 16 == 0  # the second plane and the pair plane start 16-byte aligned


def test_workspace_of_nothing_is_zero(lib):
    from squeezellm_amd import _lib

    assert lib.sqllm_gated_workspace_bytes(None) == 0
    assert lib.sqllm_gated_workspace_bytes(ctypes.byref(_lib.SqllmOp(N=0, batch=4))) == 0


@pytest.mark.parametrize("entry", ["sqllm_gated_f16", "sqllm_gated_bf16"])
def test_rejections_before_the_device_is_touched(lib, entry):
    fn = getattr(lib, entry)

    def rc(edit):
        g = _gated()
        edit(g)
        return fn(ctypes.byref(g), None)

    assert fn(None, None) == E_NULL
    assert rc(lambda g: setattr(g, "act", 1)) == E_OPTION
    assert rc(lambda g: setattr(g, "act", -1)) == E_OPTION
    # a member with an output of its own; members that differ in vec / K / N / bits / batch
    assert rc(lambda g: setattr(g.gate, "mul", 0x5000)) == E_GROUP
    assert rc(lambda g: setattr(g.up, "mul", 0x5000)) == E_GROUP
    assert rc(lambda g: setattr(g.up, "vec", 0x1100)) == E_GROUP
    assert rc(lambda g: setattr(g.up, "K", 256)) == E_GROUP
    assert rc(lambda g: setattr(g.up, "N", 256)) == E_GROUP
    assert rc(lambda g: setattr(g.gate, "N", 64)) == E_GROUP
    assert rc(lambda g: setattr(g.up, "bits", 3)) == E_GROUP
    assert rc(lambda g: setattr(g.up, "batch", 2)) == E_GROUP
    assert rc(lambda g: setattr(g.gate, "batch", 5)) == E_GROUP
    assert rc(lambda g: setattr(g, "out", None)) == E_NULL
    assert rc(lambda g: setattr(g, "workspace", None)) == E_NULL
    assert rc(lambda g: setattr(g, "workspace", 0x40008)) == E_ALIGN

    # everything the linear rejects, with the linear's codes (the same edit on both members, so that the pair stays a pair)
    def both(name, value):
        def edit(g):
            setattr(g.gate, name, value)
            setattr(g.up, name, value)
        return edit

    assert rc(both("bits", 2)) == E_BITS
    assert rc(both("bits", 5)) == E_BITS
    assert rc(both("K", 100)) == E_SHAPE
    assert rc(both("N", 126)) == E_SHAPE
    assert rc(both("K", 0)) == E_SHAPE
    assert rc(both("batch", -2)) == E_BATCH
    assert rc(both("vec", None)) == E_NULL
    assert rc(lambda g: setattr(g.gate, "qweight", None)) == E_NULL
    assert rc(lambda g: setattr(g.up, "lookup_table", None)) == E_NULL
    assert rc(lambda g: setattr(g.up, "qweight", 0x12004)) == E_ALIGN
    assert rc(lambda g: setattr(g.up, "nnz", -1) or setattr(g.up, "rows", 0x5000)) == E_SPARSE
    assert rc(lambda g: setattr(g.up, "nnz", 7) or setattr(g.up, "rows", 0x5000)) == E_NULL  # cols / vals missing
    assert rc(lambda g: setattr(g.gate, "topX", 3) or setattr(g.gate, "full_rows", 0x6000)) == E_NULL  # indices missing


def test_the_63_contribution_limit_applies_per_member(lib):
    """K so long that a column's K slices and the CSR chunks its row can be spread over exceed the 6-bit count: the
    linear's SQLLM_E_SHAPE, from the planner, for a pair whose up member alone has a CSR term"""
    from squeezellm_amd import _lib

    K = 64 * 1024  # K / 1024 + 2 = 66 possible chunks per row
    lin = _lib.SqllmLinear()
    o = lin.op
    o.bits, o.K, o.N, o.vec, o.qweight, o.mul, o.lookup_table = 4, K, 128, 0x1000, 0x2000, 0x3000, 0x4000
    o.rows, o.cols, o.vals, o.nnz = 0x5000, 0x6000, 0x7000, 1000
    lin.workspace = 0x40000
    assert lib.sqllm_linear_f16(ctypes.byref(lin), None) == E_SHAPE
    g = _gated(K=K)
    g.up.rows, g.up.cols, g.up.vals, g.up.nnz = 0x5000, 0x6000, 0x7000, 1000
    assert lib.sqllm_gated_f16(ctypes.byref(g), None) == E_SHAPE
    assert lib.sqllm_gated_bf16(ctypes.byref(g), None) == E_SHAPE
