"""Tests of the attention front that writes k and v straight into the KV cache (sqllm_qkv_rope_cache_* /
sqllm_qkv_rope_norm_cache_* behind quant.QuantQKVRopeFused's k_cache / v_cache / slots).  Operands and helpers are those of
tests/test_gpu_qkv_rope.py, by import; K = 1024.

The PARENT entry (sqllm_qkv_rope_* / sqllm_qkv_rope_norm_*) is pinned to the fp64 oracle there and in
tests/test_gpu_norm_front.py: it is not the code under test here.  The contract is "the same bits, somewhere else as
well", so the main test runs the parent on the same operands and compares as int16: the outputs, every addressed cache
element, and EVERY other element of an allocation that surrounds the caches with guards, which must still hold the
per-element distinct 16-bit pattern it was given.  One test checks cache contents against the oracle directly, with that
file's own tolerance functions, so that this file does not rest on the parent alone.

Cache geometries: "nhd" slot-major contiguous, 23 slots; "bhsd" head-major static [B, H, S, D] with S = 5 through
quant.kv_cache_view; "padded" a slot-major view with both strides beyond their minimum, cut out of a larger tensor.  Slots are
non-monotonic, include 0 and n_slots - 1, and from three rows up one -1 and one n_slots, whose rows must write nothing."""
import ctypes

import numpy as np
import pytest

from tests import test_gpu_qkv_rope as TQ
from tests.test_gpu_qkv_rope import K, N_POS

gpu_test = pytest.mark.gpu
# (N_q, N_k, N_v, D): ragged last tile, pairs within a lane group | D no power of two, pairs and heads straddling tile
# boundaries | one kv head, partner a tile away | two kv heads
SHAPES = {"d8": (456, 456, 456, 8), "d24": (456, 456, 456, 24), "d128": (384, 128, 128, 128), "d64": (384, 128, 128, 64)}
CONFIGS = TQ.CONFIGS  # both layouts where that file runs both
N_SLOTS, S, GUARD = 23, 5, 64
GEOMS = ("nhd", "bhsd", "padded")


def _members(device, bits, kind, shape):
    return tuple(TQ._layer(device, bits, n, sp, m) for m, (n, sp) in enumerate(zip(SHAPES[shape][:3], TQ.KINDS[kind])))


def _order(rows):
    """a fixed shuffle of range(rows) that starts with the last and the first: non-monotonic from two rows up"""
    rest = list(np.random.default_rng(rows).permutation(np.arange(1, rows - 1))) if rows > 2 else []
    return ([rows - 1, 0] + [int(v) for v in rest])[:rows]


class Cache:
    """k and v caches of one geometry inside guard-padded allocations that hold a per-element distinct 16-bit pattern; the
    slots of `rows` rows; and the expected contents, as int16, after rows `out_k` / `out_v` were written"""

    def __init__(self, gpu, geom, rows, N, D, dtype):
        import torch

        from squeezellm_amd import quant

        H = N // D
        self.H, self.D, self.rows = H, D, rows
        if geom == "nhd":
            self.n_slots, self.ss, self.hs, self.off = N_SLOTS, H * D, D, GUARD
            total = GUARD + N_SLOTS * H * D + GUARD
            mid = _order(N_SLOTS)  # the last, the first, then the others shuffled: distinct
            valid = mid[:rows]
        elif geom == "padded":
            self.n_slots, self.hs = N_SLOTS, D + 3
            self.ss = (H + 1) * self.hs + 5
            self.off = GUARD + 1
            total = GUARD + N_SLOTS * self.ss + GUARD
            valid = _order(N_SLOTS)[:rows]
        else:  # head-major static: row i lives in batch entry order[i] of the cache, at sequence position p_i
            B = rows
            self.n_slots, self.ss, self.hs, self.off = (B - 1) * H * S + S, D, S * D, GUARD
            total = GUARD + B * H * S * D + GUARD
            ps = [S - 1, 0] + [int(v) for v in np.random.default_rng(7).integers(0, S, max(rows - 2, 0))]
            order = _order(rows) if rows > 1 else [0]
            valid = [b * H * S + p for b, p in zip(order, ps[:rows])]
        assert total <= 65536  # the pattern is distinct per element
        slots = list(valid)
        if rows >= 3:  # two rows whose slots are out of range, one on either side
            slots[2], slots[rows - 1] = -1, self.n_slots
        self.slots = slots
        assert rows < 2 or sorted(slots) != slots
        assert (self.n_slots - 1 in slots) and (rows < 2 or 0 in slots)
        live = [s for s in slots if 0 <= s < self.n_slots]
        assert len(set(live)) == len(live)
        dt = getattr(torch, dtype)
        base = torch.arange(total, dtype=torch.int32)
        self.pattern = [((base * 3 + add) % 65536 - 32768).to(torch.int16) for add in (1, 40001)]  # k, v: distinct per element, distinct from each other
        self.backing = [p.clone().to(gpu).view(dt) for p in self.pattern]
        self.t_slots = torch.tensor(slots, dtype=torch.int32, device=gpu)
        self.views = []
        for b in self.backing:
            if geom == "bhsd":
                c4 = b[GUARD:total - GUARD].view(rows, H, S, D)
                v = quant.kv_cache_view(c4, "bhsd")
            else:
                v = b.as_strided((self.n_slots, H, D), (self.ss, self.hs, 1), self.off)
                if geom == "nhd":
                    assert v.is_contiguous() and quant.kv_cache_view(v, "nhd") is v
            assert tuple(v.shape) == (self.n_slots, H, D) and v.stride() == (self.ss, self.hs, 1) and v.storage_offset() == self.off
            self.views.append(v)

    def reset(self):
        for b, p in zip(self.backing, self.pattern):
            b.view(p.dtype).copy_(p)

    def index(self, slots=None):
        """flat element offsets [live rows, H * D] into a backing allocation, and which rows are live"""
        s = np.asarray(self.slots if slots is None else slots)
        live = (s >= 0) & (s < self.n_slots)
        at = (self.off + s[live][:, None, None] * self.ss + np.arange(self.H)[None, :, None] * self.hs + np.arange(self.D)[None, None, :])
        return at.reshape(int(live.sum()), -1), live

    def expected(self, which, out, slots=None, start=None):
        """the allocation as int16 numpy after `out` [rows, N] (a 16-bit tensor) went to the slots"""
        import torch

        want = (self.pattern[which] if start is None else start).clone().numpy()
        at, live = self.index(slots)
        want[at] = out.reshape(len(live), -1).view(torch.int16).cpu().numpy()[live]
        return want

    def got(self, which):
        import torch

        return self.backing[which].view(torch.int16).cpu().numpy()

    def rows_of(self, which, slots=None):
        """the cache's rows of the live slots as a 16-bit tensor [live rows, N], and which rows are live"""
        import torch

        at, live = self.index(slots)
        return self.backing[which].cpu()[torch.from_numpy(at)], live

    def check(self, outs_parent, what, slots=None):
        for which, name in ((0, "k"), (1, "v")):
            got, want = self.got(which), self.expected(which, outs_parent[1 + which], slots)
            assert np.array_equal(got, want), f"{what}: {name}_cache differs from the parent's out_{name} / its pattern at {(got != want).sum()} elements"


def _norm_weight(gpu, dtype):
    import torch

    g = torch.Generator().manual_seed(5)
    return (1.0 + 0.25 * torch.randn(K, generator=g)).to(getattr(torch, dtype)).to(gpu)


def _eq16(a, b):
    import torch

    return torch.equal(a.view(torch.int16), b.view(torch.int16))


# ---- 1. equals the parent ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 2, 5, 8, 19])
@pytest.mark.parametrize("kind", ["dense", "hybrid", "mixed"])
@pytest.mark.parametrize("bits", [3, 4])
def test_cache_entries_equal_the_parent_bit_for_bit_and_write_nothing_else(gpu, bits, kind, rows, dtype):
    """every shape class and layout (CONFIGS) x every cache geometry per case, the plain entry on all of them and the norm
    entry on one geometry per configuration (in turn): out_q, out_k, out_v equal the parent's as int16, every addressed cache
    element equals the parent's out_k / out_v element, every other element of the guard-padded allocations keeps its pattern
    (rows with out-of-range slots have written nothing), and the workspace is all zero afterwards"""
    x = TQ._x(gpu, rows, dtype)
    pos = TQ._positions(rows)
    g = _norm_weight(gpu, dtype)
    for ci, (shape, layout) in enumerate(CONFIGS):
        Nq, Nk, Nv, D = SHAPES[shape]
        members = _members(gpu, bits, kind, shape)
        mod = TQ._module(members, D, layout)
        tp, tc, ts = TQ._dev(gpu, pos, *TQ._tables(D))
        xin = x if rows > 1 else x.reshape(1, 1, K)
        for gi, geom in enumerate(GEOMS):
            c = Cache(gpu, geom, rows, Nk, D, dtype)
            for norm in ((False, True) if gi == ci % 3 else (False,)):
                kw = dict(norm_weight=g, norm_eps=1e-5) if norm else {}
                parent = mod(xin, tp, tc, ts, **kw)
                route = "qkv_rope_norm" if norm else "qkv_rope"
                assert mod.last_route == route
                for rep in range(2):  # the second call runs on the workspace the first one left behind
                    c.reset()
                    outs = mod(xin, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=c.t_slots, **kw)
                    assert mod.last_route == route  # (`last_route` gains nothing new)
                    what = f"{shape} {layout} {geom} norm={norm} call {rep}"
                    for o, p, name in zip(outs, parent, "qkv"):
                        assert o.shape == p.shape and _eq16(o, p), f"{what}: out_{name}"
                    c.check(parent, what)
        TQ._clean(mod)


# ---- 2. the oracle, directly ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("geom", GEOMS)
def test_cache_contents_against_the_oracle(gpu, geom, dtype):
    """what the live rows left in the caches, against the fp64 oracle with tests/test_gpu_qkv_rope.py's own tolerances: k
    rotated (_rotated), v plain (_plain)"""
    rows, shape, layout, bits = 5, "d24", "half", 4
    Nq, Nk, Nv, D = SHAPES[shape]
    members = _members(gpu, bits, "hybrid", shape)
    x = TQ._x(gpu, rows, dtype)
    TQ._in_range(members, x)
    sums = TQ._sums(members, x, rows, dtype)
    pos = TQ._positions(rows)
    cos, sin = TQ._tables(D)
    mod = TQ._module(members, D, layout)
    tp, tc, ts = TQ._dev(gpu, pos, cos, sin)
    c = Cache(gpu, geom, rows, Nk, D, dtype)
    q, none_k, none_v = mod(x, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=c.t_slots, return_kv=False)
    assert none_k is None and none_v is None
    TQ._inside(q, *TQ._rotated(sums[0], pos, cos, sin, D, layout, dtype), "q")
    for which, (exact, tol) in enumerate((TQ._rotated(sums[1], pos, cos, sin, D, layout, dtype), TQ._plain(sums[2], dtype))):
        got, live = c.rows_of(which)
        assert live.sum() == rows - 2
        TQ._inside(got, exact[live], tol[live], "kv"[which] + "_cache")
    TQ._clean(mod)


# ---- 3. return_kv=False ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 5, 19])
@pytest.mark.parametrize("bits", [3, 4])
def test_without_outputs_the_caches_are_filled_identically_and_nothing_else_is_touched(gpu, bits, rows, dtype):
    """return_kv=False passes NULL out_k / out_v: (q, None, None) comes back, q and both caches hold what the call with outputs
    gives, and the guard-padded allocations around the caches are otherwise untouched; plain and norm entries"""
    x = TQ._x(gpu, rows, dtype)
    pos = TQ._positions(rows)
    g = _norm_weight(gpu, dtype)
    for (shape, layout), geom in zip((("d8", "interleaved"), ("d24", "half"), ("d128", "half"), ("d64", "half")), GEOMS + ("bhsd",)):
        Nq, Nk, Nv, D = SHAPES[shape]
        members = _members(gpu, bits, "mixed", shape)
        mod = TQ._module(members, D, layout)
        tp, tc, ts = TQ._dev(gpu, pos, *TQ._tables(D))
        c = Cache(gpu, geom, rows, Nk, D, dtype)
        for kw in ({}, dict(norm_weight=g, norm_eps=1e-5)):
            with_outs = mod(x, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=c.t_slots, **kw)
            c.check(with_outs, f"{shape} {geom} with outputs")
            c.reset()
            outs = mod(x, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=c.t_slots, return_kv=False, **kw)
            assert isinstance(outs, tuple) and len(outs) == 3 and outs[1] is None and outs[2] is None and _eq16(outs[0], with_outs[0])
            c.check(with_outs, f"{shape} {geom} without outputs")
            c.reset()
        TQ._clean(mod)


# ---- 4. position and slot are independent ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("layout", ["half", "interleaved"])
def test_a_position_outside_the_tables_puts_the_nan_row_into_k_cache_only(gpu, layout, dtype):
    """positions -1 and n_pos with VALID slots: k_cache receives the NaN rows the output receives, v_cache's rows are finite;
    and a valid position with an out-of-range slot writes nothing while its outputs are as ever"""
    import torch

    rows, shape = 5, "d8"
    Nq, Nk, Nv, D = SHAPES[shape]
    members = _members(gpu, 4, "mixed", shape)
    x = TQ._x(gpu, rows, dtype)
    pos = [3, -1, 0, N_POS, N_POS - 1]
    mod = TQ._module(members, D, layout)
    tp, tc, ts = TQ._dev(gpu, pos, *TQ._tables(D))
    c = Cache(gpu, "nhd", rows, Nk, D, dtype)
    slots = [N_SLOTS - 1, 4, -1, 0, 9]  # rows 1 and 3 (bad positions) have valid slots; row 2 (a good position) has none
    t_slots = torch.tensor(slots, dtype=torch.int32, device=gpu)
    parent = mod(x, tp, tc, ts)
    outs = mod(x, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=t_slots)
    for o, p in zip(outs, parent):
        assert _eq16(o, p)
    c.check(parent, "nan rows", slots)
    kc, vc = c.views[0].float().cpu(), c.views[1].float().cpu()
    assert torch.isnan(kc[4]).all() and torch.isnan(kc[0]).all() and torch.isfinite(kc[N_SLOTS - 1]).all() and torch.isfinite(kc[9]).all()
    assert torch.isfinite(vc[[4, 0, N_SLOTS - 1, 9]]).all()
    assert torch.isfinite(outs[0][2].float()).all() and torch.isfinite(outs[1][2].float()).all()
    TQ._clean(mod)


# ---- 5. capture ----

@gpu_test
@pytest.mark.parametrize("return_kv", [True, False])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_captured_call_is_one_kernel_node_and_follows_slots_and_positions(gpu, dtype, return_kv):
    """after one eager call, a captured forward with a cache is ONE kernel node; a replay after slots.add_(1) and
    positions.add_(1) writes the next slot with the next rotation, and the previous slot keeps its values"""
    import torch

    hip = ctypes.CDLL("libamdhip64.so")

    def node_types(g):
        raw = ctypes.c_void_p(g.raw_cuda_graph())
        n = ctypes.c_size_t(0)
        assert hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) == 0
        nodes = (ctypes.c_void_p * n.value)()
        assert hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) == 0
        out = []
        for nd in nodes:
            ty = ctypes.c_int(-1)
            assert hip.hipGraphNodeGetType(ctypes.c_void_p(nd), ctypes.byref(ty)) == 0
            out.append(ty.value)
        return out

    rows, shape, layout = 2, "d64", "half"
    Nq, Nk, Nv, D = SHAPES[shape]
    members = _members(gpu, 4, "hybrid", shape)
    mod = TQ._module(members, D, layout, fused_members=True)
    x = TQ._x(gpu, rows, dtype)
    cos, sin = TQ._tables(D)
    pos, slots = [4, 9], [6, 17]
    tp, tc, ts = TQ._dev(gpu, pos, cos, sin)
    c = Cache(gpu, "nhd", rows, Nk, D, dtype)
    t_slots = torch.tensor(slots, dtype=torch.int32, device=gpu)
    parents = []
    for step in range(3):  # what the parent gives at the three steps
        tpi = torch.tensor([p + step for p in pos], dtype=torch.int32, device=gpu)
        parents.append([o.clone() for o in mod(x, tpi, tc, ts)])
    assert not _eq16(parents[0][1], parents[1][1])
    outs = []

    def run():
        outs.clear()
        with torch.no_grad():
            outs.extend(mod(x, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=t_slots, return_kv=return_kv))

    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        run()
    assert node_types(g) == [0]  # hipGraphNodeTypeKernel: the q/k/v kernel and nothing else
    g.instantiate()
    c.reset()
    start = [p.clone() for p in c.pattern]
    for step in range(3):
        if step:
            t_slots.add_(1)  # in place: the graph holds the tensors' addresses
            tp.add_(1)
        g.replay()
        torch.cuda.synchronize()
        now = [s + step for s in slots]
        for which in (0, 1):
            want = c.expected(which, parents[step][1 + which], now, start[which])  # (the earlier steps' slots keep their values)
            assert np.array_equal(c.got(which), want), (step, which)
            start[which] = torch.from_numpy(want)
        assert _eq16(outs[0], parents[step][0])
        if return_kv:
            assert _eq16(outs[1], parents[step][1]) and _eq16(outs[2], parents[step][2])
        else:
            assert outs[1] is None and outs[2] is None
    TQ._clean(mod)


# ---- 6. the C ABI, directly ----

@gpu_test
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("layout", ["half", "interleaved"])
def test_c_abi_directly(gpu, layout, dtype, norm):
    """the descriptors filled in by hand from the layers' raw operands (CSR and top-X rows passed separately, not folded), a
    workspace zero-filled once, launches on it: a slot-major cache with out_k / out_v, then a head-major cache with the strides
    given by hand and NULL out_k / out_v; against the parent entry called the same way"""
    import torch

    from squeezellm_amd import _lib, quant_cuda

    rows, shape = 5, "d24"
    Nq, Nk, Nv, D = SHAPES[shape]
    H = Nk // D
    members = _members(gpu, 3, "mixed", shape)
    x = TQ._x(gpu, rows, dtype)
    cos, sin = TQ._tables(D)
    pos = TQ._positions(rows)
    tp, tc, ts = TQ._dev(gpu, pos, cos, sin)
    r = _lib.SqllmQkvRope()
    outs = []
    for op, name, (lay, _, _, _) in zip((r.q, r.k, r.v), "qkv", members):
        op.bits, op.batch, op.K, op.N = lay["bits"], rows, K, lay["N"]
        op.vec, op.qweight, op.lookup_table = x.data_ptr(), lay["qweight"].data_ptr(), lay["lookup_table"].data_ptr()
        if lay["vals"] is not None:
            op.rows, op.cols, op.vals, op.nnz = lay["rows"].data_ptr(), lay["cols"].data_ptr(), lay["vals"].data_ptr(), lay["vals"].numel()
            op.full_rows, op.full_row_indices, op.topX = lay["full_rows"].data_ptr(), lay["full_row_indices"].data_ptr(), lay["full_rows"].shape[1]
        setattr(r, "bias_" + name, lay["bias"].data_ptr())
        outs.append(torch.empty((rows, lay["N"]), dtype=x.dtype, device=gpu))
        setattr(r, "out_" + name, outs[-1].data_ptr())
    r.cos, r.sin, r.positions = tc.data_ptr(), ts.data_ptr(), tp.data_ptr()
    r.n_pos, r.head_dim, r.layout = N_POS, D, _lib.ROPE_INTERLEAVED if layout == "interleaved" else _lib.ROPE_HALF
    need = _lib.qkv_rope_workspace_bytes(Nq, Nk, Nv, rows)
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=gpu)
    ws[need:] = 0xA5  # a guard behind the workspace
    r.workspace = ws.data_ptr()
    dev = x.get_device()
    stream = quant_cuda._raw_stream(dev)
    lib = _lib.load()
    sfx = "f16" if dtype == "float16" else "bf16"
    g = _norm_weight(gpu, dtype)
    nm = _lib.SqllmRmsNorm(weight=g.data_ptr(), eps=1e-5)
    if norm:
        parent_fn = lambda: getattr(lib, "sqllm_qkv_rope_norm_" + sfx)(ctypes.byref(r), ctypes.byref(nm), stream)  # noqa: E731
        cache_fn = lambda kc: getattr(lib, "sqllm_qkv_rope_norm_cache_" + sfx)(ctypes.byref(r), ctypes.byref(nm), ctypes.byref(kc), stream)  # noqa: E731
    else:
        parent_fn = lambda: getattr(lib, "sqllm_qkv_rope_" + sfx)(ctypes.byref(r), stream)  # noqa: E731
        cache_fn = lambda kc: getattr(lib, "sqllm_qkv_rope_cache_" + sfx)(ctypes.byref(r), ctypes.byref(kc), stream)  # noqa: E731
    assert parent_fn() == 0
    torch.cuda.synchronize()
    parent = [o.clone() for o in outs]
    assert int(ws[:need].count_nonzero()) == 0
    for geom in ("nhd", "bhsd"):
        c = Cache(gpu, geom, rows, Nk, D, dtype)
        kc = _lib.SqllmKvCache()
        kc.k_cache = c.backing[0].data_ptr() + 2 * c.off
        kc.v_cache = c.backing[1].data_ptr() + 2 * c.off
        kc.slots, kc.n_slots = c.t_slots.data_ptr(), c.n_slots
        if geom == "nhd":
            kc.slot_stride, kc.head_stride = H * D, D
        else:
            kc.slot_stride, kc.head_stride, kc.n_slots = D, S * D, (rows - 1) * H * S + S
            r.out_k = r.out_v = None
        for o in outs:
            o.zero_()
        assert cache_fn(kc) == 0
        torch.cuda.synchronize()
        assert _eq16(outs[0], parent[0])
        if geom == "nhd":
            assert _eq16(outs[1], parent[1]) and _eq16(outs[2], parent[2])
        else:
            assert int(outs[1].view(torch.int16).count_nonzero()) == 0 and int(outs[2].view(torch.int16).count_nonzero()) == 0
        c.check(parent, geom)
        assert int(ws[:need].count_nonzero()) == 0 and bool((ws[need:] == 0xA5).all())


# ---- 7. the module's surface, the torch routes ----

@gpu_test
def test_module_surface(gpu):
    """the argument errors, int64 slots, leading dimensions"""
    import torch

    shape, layout, dtype, rows = "d64", "half", "float16", 8
    Nq, Nk, Nv, D = SHAPES[shape]
    members = _members(gpu, 4, "dense", shape)
    mod = TQ._module(members, D, layout)
    x = TQ._x(gpu, rows, dtype)
    pos = TQ._positions(rows)
    tp, tc, ts = TQ._dev(gpu, pos, *TQ._tables(D))
    c = Cache(gpu, "nhd", rows, Nk, D, dtype)
    kv, vv, sl = c.views[0], c.views[1], c.t_slots
    parent = mod(x, tp, tc, ts)
    outs = mod(x.reshape(2, 4, K), tp.reshape(2, 4), tc, ts, k_cache=kv, v_cache=vv, slots=sl.reshape(2, 4).long())  # int64 slots
    assert [tuple(o.shape) for o in outs] == [(2, 4, n) for n in (Nq, Nk, Nv)]
    for o, p in zip(outs, parent):
        assert _eq16(o.reshape(rows, -1), p)
    c.check(parent, "int64 slots")
    c.reset()
    for kw in (dict(k_cache=kv), dict(v_cache=vv), dict(slots=sl), dict(k_cache=kv, v_cache=vv), dict(k_cache=kv, slots=sl), dict(v_cache=vv, slots=sl)):
        with pytest.raises(ValueError, match="all three or none"):
            mod(x, tp, tc, ts, **kw)
    with pytest.raises(ValueError, match="return_kv"):
        mod(x, tp, tc, ts, return_kv=False)
    bad = {
        "dtype": dict(k_cache=kv.view(torch.bfloat16)),
        "device": dict(v_cache=vv.cpu()),
        "shape: heads": dict(k_cache=kv[:, :1], v_cache=vv[:, :1]),
        "shape: head_dim": dict(k_cache=kv.reshape(N_SLOTS, 4, 32), v_cache=vv.reshape(N_SLOTS, 4, 32)),
        "shape: 2-D": dict(k_cache=kv.reshape(N_SLOTS, Nk), v_cache=vv.reshape(N_SLOTS, Nk)),
        "shape: unequal": dict(v_cache=vv[:5]),
        "strides: last": dict(k_cache=kv.transpose(1, 2).contiguous().transpose(1, 2), v_cache=vv.transpose(1, 2).contiguous().transpose(1, 2)),
        "strides: unequal": dict(v_cache=torch.empty((N_SLOTS, 2 * Nk // D, D), dtype=x.dtype, device=gpu)[:, ::2]),
        "slots: count": dict(slots=sl[:3]),
        "slots: dtype": dict(slots=sl.float()),
        "slots: device": dict(slots=sl.cpu()),
    }
    for name, kw in bad.items():
        args = dict(k_cache=kv, v_cache=vv, slots=sl)
        args.update(kw)
        with pytest.raises(ValueError):
            mod(x, tp, tc, ts, **args)
        assert np.array_equal(c.got(0), c.pattern[0].numpy()) and np.array_equal(c.got(1), c.pattern[1].numpy()), name
    TQ._clean(mod)


@gpu_test
@pytest.mark.parametrize("geom", GEOMS)
def test_fp32_fallback_makes_the_same_writes(gpu, geom):
    """fp32 activations: the operator path and the rotation in torch -- the caches receive the rows the call returns, bit for
    bit, rows with out-of-range slots write nothing, and what they hold is inside the fallback's tolerance (eps = 2^-24)"""
    import torch

    shape, layout, rows = "d24", "half", 5
    Nq, Nk, Nv, D = SHAPES[shape]
    members = _members(gpu, 4, "mixed", shape)
    mod = TQ._module(members, D, layout)
    x = TQ._x(gpu, rows, "float16").float()
    sums = [TQ.BF._exact(npl, x, k) for _, npl, _, k in members]
    cos, sin = TQ._tables(D)
    pos = TQ._positions(rows)
    tp, tc, ts = TQ._dev(gpu, pos, cos, sin)
    c = Cache(gpu, geom, rows, Nk, D, "float16")  # (16-bit slots of pattern; the fp32 caches are separate tensors below)
    at, live = c.index()
    total = c.backing[0].numel()
    flat = [torch.full((total,), -7.0, dtype=torch.float32, device=gpu) for _ in range(2)]
    views = [f.as_strided((c.n_slots, c.H, D), (c.ss, c.hs, 1), c.off) for f in flat]
    outs = mod(x, tp, tc, ts, k_cache=views[0], v_cache=views[1], slots=c.t_slots)
    assert mod.last_route == "fallback"
    TQ._check(outs, sums, pos, cos, sin, D, layout, "float32")
    for which in (0, 1):
        want = np.full(total, -7.0, np.float32)
        want[at] = outs[1 + which].cpu().numpy()[live]
        assert np.array_equal(flat[which].cpu().numpy(), want)
    q2, k2, v2 = mod(x, tp, tc, ts, k_cache=views[0], v_cache=views[1], slots=c.t_slots, return_kv=False)
    assert k2 is None and v2 is None  # (q is not compared bit for bit: the fp32 operators add in arrival order)
    TQ._inside(q2, *TQ._rotated(sums[0], pos, cos, sin, D, layout, "float32"), "q without outputs")
    for which in (0, 1):  # ... and k and v went to the caches again, inside the same tolerance
        got = flat[which].cpu()[torch.from_numpy(at)]
        exact, tol = TQ._rotated(sums[1], pos, cos, sin, D, layout, "float32") if which == 0 else TQ._plain(sums[2], "float32")
        TQ._inside(got, exact[live], tol[live], "kv"[which] + "_cache without outputs")
        rest = np.ones(total, bool)
        rest[at.reshape(-1)] = False
        assert (flat[which].cpu().numpy()[rest] == -7.0).all()


@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
def test_dense_route_makes_the_same_writes(gpu, dtype):
    """dense_min_rows = 4 on q, 5 rows: the dense route's k and v (pinned with its own tolerance in
    tests/test_gpu_qkv_rope.py: the call without a cache gives the same bits) go to the caches bit for bit, out-of-range slots
    skipped; and k_cache is inside that route's tolerance of the oracle"""
    shape, layout, rows = "d24", "half", 5
    Nq, Nk, Nv, D = SHAPES[shape]
    members = _members(gpu, 4, "mixed", shape)
    mod = TQ._module(members, D, layout, fused_members=True)
    mod.q.dense_min_rows = 4
    x = TQ._x(gpu, rows, dtype)
    sums = TQ._sums(members, x, rows, dtype)
    cos, sin = TQ._tables(D)
    pos = TQ._positions(rows)
    tp, tc, ts = TQ._dev(gpu, pos, cos, sin)
    plain = mod(x, tp, tc, ts)
    assert mod.last_route == "dense"
    for geom in GEOMS:
        c = Cache(gpu, geom, rows, Nk, D, dtype)
        outs = mod(x, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=c.t_slots)
        assert mod.last_route == "dense"
        for o, p in zip(outs, plain):
            assert _eq16(o, p)
        c.check(plain, f"dense {geom}")
        # the parent route's tolerance (tests/test_gpu_qkv_rope.py: test_dense_route_from_dense_min_rows), on the caches
        for which, i in ((0, 1), (1, 2)):
            _, npl, mag, _ = members[i]
            gemm = K * 2.0 ** -24 * TQ.BF._abs_sum(npl, mag, x)
            if i == 1:
                exact, tol = TQ._rotated(sums[i], pos, cos, sin, D, layout, dtype)
                lo, hi = TQ._split(gemm, D, layout)
                cc, sn = np.abs(TQ._at(cos, pos)).astype(np.float64), np.abs(TQ._at(sin, pos)).astype(np.float64)
                tol = tol + TQ._merge(lo * cc + hi * sn, hi * cc + lo * sn, layout)
            else:
                exact, tol = TQ._plain(sums[i], dtype)
                tol = tol + gemm
            got, live = c.rows_of(which)
            TQ._inside(got, exact[live], tol[live], "kv"[which] + "_cache")
        c.reset()
        q2, k2, v2 = mod(x, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=c.t_slots, return_kv=False)
        assert k2 is None and v2 is None and _eq16(q2, plain[0])
        c.check(plain, f"dense {geom} without outputs")
    outs3 = mod(x[:3].contiguous(), tp[:3].contiguous(), tc, ts)
    assert mod.last_route == "qkv_rope" and len(outs3) == 3
    TQ._clean(mod)


# ---- 8. run to run ----

@gpu_test
@pytest.mark.parametrize("dtype", ["float16", "bfloat16"])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("bits", [3, 4])
def test_two_runs_are_bit_identical_cache_included(gpu, bits, rows, dtype):
    """hybrid members (CSR rows held by several waves of a chunk; which column of a pair finishes first differs from run to run)"""
    import torch

    x = TQ._x(gpu, rows, dtype)
    pos = TQ._positions(rows)
    for (shape, layout), geom in zip((("d8", "half"), ("d128", "interleaved"), ("d24", "half")), GEOMS):
        Nq, Nk, Nv, D = SHAPES[shape]
        members = _members(gpu, bits, "hybrid", shape)
        tp, tc, ts = TQ._dev(gpu, pos, *TQ._tables(D))
        mod = TQ._module(members, D, layout)
        c = Cache(gpu, geom, rows, Nk, D, dtype)
        runs = []
        for _ in range(4):
            c.reset()
            outs = mod(x, tp, tc, ts, k_cache=c.views[0], v_cache=c.views[1], slots=c.t_slots)
            torch.cuda.synchronize()
            runs.append(([o.clone() for o in outs], c.got(0), c.got(1)))
        for r in runs[1:]:
            assert all(_eq16(a, b) for a, b in zip(r[0], runs[0][0])) and np.array_equal(r[1], runs[0][1]) and np.array_equal(r[2], runs[0][2])
        c.check(runs[0][0], f"{shape} {geom}")
        TQ._clean(mod)
