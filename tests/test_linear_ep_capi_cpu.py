"""C ABI of the fused linear with an epilogue (sqllm_linear_ep_f16 / sqllm_linear_ep_bf16, include/sqllm_hip.h) on a host
without a GPU: the symbols, the struct, the constants, and every rejection the header lists -- each returned before the
device is touched (operand pointers are fake 16-byte-aligned integers: nothing dereferences them).

Nothing here reaches a launch.  That a residual passes the epilogue's own checks is shown by a descriptor whose LINEAR is
invalid in a way that is checked afterwards (bits = 5): it returns the linear's code, where a bad residual or act returns
the epilogue's."""
import ctypes

import pytest

E_BITS, E_SHAPE, E_NULL, E_ALIGN, E_SPARSE, E_BATCH, E_OPTION, E_GROUP = -1, -2, -3, -4, -5, -6, -7, -8
ENTRIES = ["sqllm_linear_ep_f16", "sqllm_linear_ep_bf16"]
MUL = 0x30000


@pytest.fixture(scope="module")
def lib():
    from squeezellm_amd import _lib

    return _lib.load()


def _ep(batch=0, K=128, N=128, bits=5, residual=None, act=None):
    """a descriptor that passes every check of the epilogue and every check of the linear but one: bits (5, checked by the
    linear's validation, after the epilogue's own) -- so that no call of this file gets as far as a launch"""
    from squeezellm_amd import _lib

    e = _lib.SqllmLinearEp()
    o = e.lin.op
    o.bits, o.batch, o.K, o.N = bits, batch, K, N
    o.vec, o.qweight, o.lookup_table, o.mul = 0x1000, 0x2000, 0x4000, MUL
    e.lin.workspace = 0x40000
    e.residual, e.act = residual, _lib.ACT_RELU if act is None else act
    return e


def test_symbols_struct_and_constants(lib):
    from squeezellm_amd import _lib

    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name][0]._type_ is _lib.SqllmLinearEp
        assert getattr(lib, name).restype is ctypes.c_int
    header = open(_lib.os.path.join(_lib.os.path.dirname(_lib.HERE), "include", "sqllm_hip.h")).read()
    for name, value in (("SILU", 0), ("IDENTITY", 1), ("RELU", 2), ("GELU", 3), ("GELU_TANH", 4)):
        assert f"#define SQLLM_ACT_{name} {value}\n" in header and getattr(_lib, f"ACT_{name}") == value
    assert "int sqllm_linear_ep_f16(const sqllm_linear_ep*" in header and "int sqllm_linear_ep_bf16(const sqllm_linear_ep*" in header
    # the struct as the header lays it out: the linear, the residual pointer, act (padded to the pointers' alignment)
    lin = ctypes.sizeof(_lib.SqllmLinear)
    assert lin % 8 == 0
    assert ctypes.sizeof(_lib.SqllmLinearEp) == lin + 8 + 8
    assert _lib.SqllmLinearEp.lin.offset == 0 and _lib.SqllmLinearEp.residual.offset == lin and _lib.SqllmLinearEp.act.offset == lin + 8


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_epilogues_own_rejections(lib, entry):
    fn = getattr(lib, entry)
    assert fn(None, None) == E_NULL
    for act in (-1, 5, 6, 1 << 20, -(1 << 31)):
        assert fn(ctypes.byref(_ep(act=act)), None) == E_OPTION
        assert fn(ctypes.byref(_ep(act=act, bits=4, residual=MUL + 2)), None) == E_OPTION  # (before the residual is looked at)
    # a residual that overlaps the output [batch, N] x 2 bytes without being it
    for batch, N in ((0, 128), (1, 128), (5, 128), (9, 456)):
        nbytes = 2 * max(batch, 1) * N
        for r in (MUL + 2, MUL - 2, MUL + nbytes - 2, MUL - nbytes + 2, MUL + 2 * N):
            if abs(r - MUL) < nbytes:
                assert fn(ctypes.byref(_ep(batch=batch, N=N, residual=r)), None) == E_SHAPE, (batch, N, r - MUL)


@pytest.mark.parametrize("entry", ENTRIES)
def test_residuals_that_get_past_the_epilogues_checks(lib, entry):
    """NULL, the output itself, vec (K == N), and ranges that end where the output begins or begin where it ends: the
    call goes on to the linear's validation, which returns ITS code for bits = 5; so does every activation code"""
    from squeezellm_amd import _lib

    fn = getattr(lib, entry)
    for batch in (0, 1, 5):
        nbytes = 2 * max(batch, 1) * 128
        for r in (None, MUL, 0x1000, MUL + nbytes, MUL - nbytes, 0x7F0000):
            assert fn(ctypes.byref(_ep(batch=batch, residual=r)), None) == E_BITS, (batch, r)
    for act in (_lib.ACT_SILU, _lib.ACT_IDENTITY, _lib.ACT_RELU, _lib.ACT_GELU, _lib.ACT_GELU_TANH):
        assert fn(ctypes.byref(_ep(act=act, residual=MUL)), None) == E_BITS


@pytest.mark.parametrize("entry", ENTRIES)
def test_everything_the_linear_rejects_with_its_codes(lib, entry):
    fn = getattr(lib, entry)
    plain = getattr(lib, entry.replace("_ep", ""))

    def rc(edit, **kw):
        e = _ep(bits=4, **kw)
        edit(e)
        assert plain(ctypes.byref(e.lin), None) == fn(ctypes.byref(e), None)  # the plain linear's code for the same descriptor
        return fn(ctypes.byref(e), None)

    for residual in (None, MUL):
        assert rc(lambda e: setattr(e.lin.op, "bits", 2), residual=residual) == E_BITS
        assert rc(lambda e: setattr(e.lin.op, "bits", 5), residual=residual) == E_BITS
        assert rc(lambda e: setattr(e.lin.op, "K", 100), residual=residual) == E_SHAPE
        assert rc(lambda e: setattr(e.lin.op, "N", 126), residual=residual) == E_SHAPE
        assert rc(lambda e: setattr(e.lin.op, "K", 0), residual=residual) == E_SHAPE
        assert rc(lambda e: setattr(e.lin.op, "N", 0), residual=residual) == E_SHAPE
        assert rc(lambda e: setattr(e.lin.op, "N", -4), residual=residual) == E_SHAPE
        assert rc(lambda e: setattr(e.lin.op, "batch", -2), residual=residual) == E_BATCH
        assert rc(lambda e: setattr(e.lin.op, "vec", None), residual=residual) == E_NULL
        assert rc(lambda e: setattr(e.lin.op, "mul", None), residual=residual) == E_NULL
        assert rc(lambda e: setattr(e.lin.op, "qweight", None), residual=residual) == E_NULL
        assert rc(lambda e: setattr(e.lin.op, "lookup_table", None), residual=residual) == E_NULL
        assert rc(lambda e: setattr(e.lin.op, "qweight", 0x2004), residual=residual) == E_ALIGN
        assert rc(lambda e: setattr(e.lin, "workspace", None), residual=residual) == E_NULL
        assert rc(lambda e: setattr(e.lin, "workspace", 0x40008), residual=residual) == E_ALIGN
        assert rc(lambda e: setattr(e.lin.op, "nnz", -1) or setattr(e.lin.op, "rows", 0x5000), residual=residual) == E_SPARSE
        assert rc(lambda e: setattr(e.lin.op, "nnz", 7) or setattr(e.lin.op, "rows", 0x5000), residual=residual) == E_NULL
        assert rc(lambda e: setattr(e.lin.op, "topX", 3) or setattr(e.lin.op, "full_rows", 0x6000), residual=residual) == E_NULL


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_63_contribution_limit_is_the_linears(lib, entry):
    """K so long that a column's K slices and the CSR chunks its row can be spread over exceed the 6-bit count: the
    linear's SQLLM_E_SHAPE, from the planner -- the last check before a launch"""
    e = _ep(K=64 * 1024, bits=4, residual=MUL)
    o = e.lin.op
    o.rows, o.cols, o.vals, o.nnz = 0x5000, 0x6000, 0x7000, 1000
    assert getattr(lib, entry)(ctypes.byref(e), None) == E_SHAPE


@pytest.mark.parametrize("entry", ["sqllm_gated_f16", "sqllm_gated_bf16"])
def test_the_gated_pair_still_takes_silu_only(lib, entry):
    from squeezellm_amd import _lib

    g = _lib.SqllmGated()
    for op in (g.gate, g.up):
        op.bits, op.batch, op.K, op.N = 5, 0, 128, 128  # (bits = 5: SiLU gets as far as the linear's validation, no further)
        op.vec, op.qweight, op.lookup_table = 0x1000, 0x2000, 0x4000
    g.out, g.workspace = 0x3000, 0x40000
    for act in (_lib.ACT_IDENTITY, _lib.ACT_RELU, _lib.ACT_GELU, _lib.ACT_GELU_TANH):
        g.act = act
        assert getattr(lib, entry)(ctypes.byref(g), None) == E_OPTION
    g.act = _lib.ACT_SILU
    assert getattr(lib, entry)(ctypes.byref(g), None) == E_BITS
