"""The encode direction on the GPU (sqllm_encode / sqllm_encode_csr and pack.encode_layer on top of them): bit for bit
against the reference packer's own output (tests/golden/pack2_*.npz) and against the torch route
(nuq.assign_indices + pack.pack_layer, run on CPU tensors), round trip through the dense export, through the operator,
and captured.  Every output buffer is pre-filled with a sentinel (qweight 0x5A5A5A5A, rows / cols -1, vals NaN), so an
element the kernels skip fails the comparison; cols / vals carry four guard elements the kernels must leave alone."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import helpers as H

pytestmark = pytest.mark.gpu

oracle = H.oracle
GUARD = 4


def encode_raw(gpu, w, lut, bits, mask, pad=0):
    """Straight through the C ABI into sentinel-filled buffers.  w: numpy [N, K] fp16 / fp32 (copied into an [N, K + pad]
    buffer and passed as a view with ld = K + pad), mask: numpy bool [N, K] or None.
    Returns (qweight, rows, cols, vals) as numpy, the last three None without a mask."""
    import torch

    from squeezellm_amd import _lib

    lib = _lib.load()
    N, K = w.shape
    buf = torch.full((N, K + pad), 7.0, dtype=torch.from_numpy(w).dtype, device=gpu)  # (the pad holds finite junk far from any codebook)
    buf[:, :K] = torch.from_numpy(w).to(gpu)
    lt = torch.from_numpy(lut).to(gpu)
    q = torch.full((K // 32 * bits, N), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
    d = _lib.SqllmEncode(bits=bits, K=K, N=N, weight_dtype=_lib.DTYPE_F16 if w.dtype == np.float16 else _lib.DTYPE_F32,
                         weight=buf.data_ptr(), ld=K + pad, lookup_table=lt.data_ptr(), qweight=q.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    if mask is None:
        assert lib.sqllm_encode(ctypes.byref(d), stream) == 0
        torch.cuda.synchronize()
        return q.cpu().numpy(), None, None, None
    mt = torch.from_numpy(mask).to(gpu)
    rows = torch.full((N + 1,), -1, dtype=torch.int32, device=gpu)
    d.mask, d.rows = mt.data_ptr(), rows.data_ptr()
    assert lib.sqllm_encode(ctypes.byref(d), stream) == 0
    nnz = int(rows[N].item())
    assert 0 <= nnz <= N * K
    cols = torch.full((nnz + GUARD,), -1, dtype=torch.int32, device=gpu)
    vals = torch.full((nnz + GUARD,), float("nan"), dtype=torch.float32, device=gpu)
    assert lib.sqllm_encode_csr(ctypes.byref(d), cols.data_ptr(), vals.data_ptr(), nnz, stream) == 0
    torch.cuda.synchronize()
    cols, vals = cols.cpu().numpy(), vals.cpu().numpy()
    assert (cols[nnz:] == -1).all() and np.isnan(vals[nnz:]).all()  # nothing beyond nnz is touched
    assert torch.equal(buf[:, K:], torch.full_like(buf[:, K:], 7.0))
    return q.cpu().numpy(), rows.cpu().numpy(), cols[:nnz], vals[:nnz]


def torch_route(w, lut, bits, mask, topX=0, device="cpu"):
    """The reference: nuq.assign_indices + pack.pack_layer on torch tensors, as nuq.quantize_linear chained them.  On CPU
    tensors, except where top-X rows are extracted: which of several rows with EQUAL outlier counts torch.topk picks is
    not specified and differs between the CPU and the GPU, and encode_layer runs extract_topx_rows where quantize_linear
    always ran it, on the GPU."""
    import torch

    from squeezellm_amd import nuq, pack

    w32, lt = torch.from_numpy(w).to(device=device, dtype=torch.float32), torch.from_numpy(lut).to(device)
    if mask is None:
        lay = pack.pack_layer(nuq.assign_indices(w32, lt), lt, bits)
    else:
        mt = torch.from_numpy(mask).to(device)
        lay = pack.pack_layer(nuq.assign_indices(w32 * ~mt, lt), lt, bits, w32 * mt, topX=topX)
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in lay.items()}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# pinned to the reference packer
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture(name):
    z = np.load(os.path.join(H.GOLDEN, name + ".npz"))
    f = {k: z[k] for k in z.files}
    lut, idx, outl = f["lut"], f["idx_nk"].astype(np.int64), f["outliers_nk"]
    w = np.take_along_axis(lut, idx, axis=1)
    f["weight"] = np.where(outl != 0, outl, w).astype(np.float32)
    f["mask"] = outl != 0
    return f


@pytest.mark.parametrize("name", ["pack2_w4_dense", "pack2_w3_dense"])
def test_dense_fixture_bit_for_bit(gpu, name):
    f = fixture(name)
    bits = int(f["bits"])
    assert not f["mask"].any()
    q, _, _, _ = encode_raw(gpu, f["weight"], f["lut"], bits, None)
    assert same_bits(q, f["qweight"])
    # ... and the same through an all-false mask
    q, rows, cols, vals = encode_raw(gpu, f["weight"], f["lut"], bits, f["mask"])
    assert same_bits(q, f["qweight"]) and (rows == 0).all() and cols.size == 0 and vals.size == 0


@pytest.mark.parametrize("name", ["pack2_w4_sparse", "pack2_w3_sparse_balanced"])
def test_sparse_fixture_bit_for_bit(gpu, name):
    f = fixture(name)
    bits, N = int(f["bits"]), int(f["N"])
    counts = np.diff(f["rows"])
    assert counts[11] == 0 and counts[7] > 60 and f["mask"][13, 5]  # the empty row, the heavy row, the vanishing outlier
    q, rows, cols, vals = encode_raw(gpu, f["weight"], f["lut"], bits, f["mask"])
    assert same_bits(rows, f["rows"]) and same_bits(cols, f["cols"]) and same_bits(vals, f["vals"])
    idx = oracle.unpack_indices(q, bits).T  # [N, K]
    zero_idx = np.abs(f["lut"]).argmin(axis=1)
    want = np.where(f["mask"], zero_idx[:, None], f["idx_nk"])
    assert np.array_equal(idx, want)
    assert zero_idx[3] == 0 and f["lut"][3, 0] == -f["lut"][3, 1]  # the |tie| channel takes the lower index


# ---------------------------------------------------------------------------------------------------------------------
# against the torch route
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(bits, K, N, dtype, kind):
    """Seeded weights, codebooks and mask.  Channel 1's codebook is dyadic and symmetric ((j - E/2 + 1/2) / 64: two
    entries tie for the zero-nearest), and its first weights sit exactly midway between neighbouring entries (the tie
    rule of the index).  kind: "none" (no mask), "false" (a mask of zeros), "mixed" (2 % random, row 2 fully masked
    -- with K = 544 more outliers than a 512-wide chunk holds -- masked zero weights and a masked weight equal to the
    zero-nearest entry)."""
    E = 1 << bits
    rng = np.random.default_rng(bits * 100000 + K * 100 + N + (dtype == "float16") * 7 + len(kind))
    lut = np.sort(rng.normal(0, 0.02, (N, E)).astype(np.float32), axis=1)
    lut[1] = (np.arange(E, dtype=np.float32) - E / 2 + 0.5) / 64
    w = rng.normal(0, 0.02, (N, K)).astype(np.float32)
    mid = (lut[1, :-1] + lut[1, 1:]) / 2  # multiples of 1 / 128: exact in fp16 and midway in fp32
    w[1, :E - 1] = mid
    w[1, E - 1] = 0.0  # midway between the two zero-nearest entries
    w = w.astype(np.dtype(dtype))
    mask = None
    if kind != "none":
        mask = np.zeros((N, K), bool)
    if kind == "mixed":
        mask = rng.random((N, K)) < 0.02
        mask[1, :E] = False  # (the tie positions keep their own index)
        mask[2] = True
        w[2, 3] = 0.0
        w[2, K - 1] = -0.0
        w[0, 7] = 0.0
        mask[0, 7] = True
        z = lut[np.arange(N), np.abs(lut).argmin(axis=1)]
        w[1, 20] = z[1]  # (-1 / 128: exact in fp16) a masked weight equal to the zero-nearest entry: no outlier
        mask[1, 20] = True
        w[3, K - 2] = np.dtype(dtype).type(z[3])
        mask[3, K - 2] = True  # (fp32: vanishes; fp16: the rounded z leaves a tiny outlier -- either way the torch route decides)
        mask[N - 1, K - 1] = True
        mask[N - 1, 0] = True
    return w, lut, mask, torch_route(w, lut, bits, mask)


# K = 32: one 3-bit group (straddlers at k = 10 and 21); 544: a whole 512-chunk and a 32-wide tail; N = 4, 68, 128: a
# partial channel tile, one full tile plus 4, two full tiles; pad: ld = K + 8
SHAPES = [(32, 4, 0), (32, 68, 8), (544, 4, 8), (544, 68, 0), (544, 128, 8)]


@pytest.mark.parametrize("kind", ["none", "false", "mixed"])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("K,N,pad", SHAPES)
@pytest.mark.parametrize("bits", [3, 4])
def test_bit_for_bit_against_the_torch_route(gpu, bits, K, N, pad, dtype, kind):
    w, lut, mask, want = random_case(bits, K, N, dtype, kind)
    q, rows, cols, vals = encode_raw(gpu, w, lut, bits, mask, pad=pad)
    assert same_bits(q, want["qweight"])
    if kind == "none":
        assert want["rows"] is None and rows is None
        return
    assert same_bits(rows, want["rows"]) and same_bits(cols, want["cols"]) and same_bits(vals, want["vals"])
    if kind == "false":
        assert (rows == 0).all() and cols.size == 0
    else:
        counts = np.diff(rows)
        assert counts[2] == K - 2 and counts.sum() == rows[N] == cols.size  # the fully masked row, less its two zeros
        idx = oracle.unpack_indices(q, bits).T
        assert idx[1, 20] == (1 << bits) // 2 - 1 and not ((cols[rows[1]:rows[2]]) == 20).any()
    # the tie rule: midway between entries j and j + 1 the index is j
    idx = oracle.unpack_indices(q, bits).T
    E = 1 << bits
    assert idx[1, :E - 1].tolist() == list(range(E - 1)) and idx[1, E - 1] == E // 2 - 1


@pytest.mark.parametrize("topX", [0, 3])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("K,N", [(32, 68), (544, 68)])
@pytest.mark.parametrize("bits", [3, 4])
def test_encode_layer_returns_what_pack_layer_returns(gpu, bits, K, N, dtype, topX):
    import torch

    from squeezellm_amd import pack

    w, lut, mask, _ = random_case(bits, K, N, dtype, "mixed")
    want = torch_route(w, lut, bits, mask, topX=topX, device=gpu if topX else "cpu")
    wt = torch.from_numpy(w).to(gpu)
    bias = torch.arange(N, dtype=torch.float32, device=gpu)
    lay = pack.encode_layer(wt, torch.from_numpy(lut).to(gpu), bits, torch.from_numpy(mask).to(gpu), topX=topX, bias=bias)
    assert list(lay) == list(want) and (lay["bits"], lay["K"], lay["N"]) == (bits, K, N) and lay["bias"] is bias
    for key in ("qweight", "lookup_table", "rows", "cols", "vals", "full_rows", "full_row_indices"):
        if want[key] is None:
            assert lay[key] is None, key
        else:
            assert lay[key].is_cuda and same_bits(lay[key].cpu().numpy(), want[key]), key
    assert (lay["full_rows"] is not None) == (topX > 0)
    # a strided view is read in place, a layout the kernel cannot read is copied: the same operands either way
    big = torch.zeros((N, K + 8), dtype=wt.dtype, device=gpu)
    big[:, :K] = wt
    for view in (big[:, :K], wt.t().contiguous().t()):
        again = pack.encode_layer(view, torch.from_numpy(lut).to(gpu), bits, torch.from_numpy(mask).to(gpu), topX=topX)
        assert all(same_bits(again[k].cpu().numpy(), want[k]) for k in ("qweight", "rows", "cols", "vals"))
    # no mask: the dense operands alone
    dense = pack.encode_layer(wt, torch.from_numpy(lut).to(gpu), bits)
    assert dense["rows"] is None and dense["cols"] is None and dense["vals"] is None and dense["full_rows"] is None
    assert same_bits(dense["qweight"].cpu().numpy(), torch_route(w, lut, bits, None)["qweight"])


def test_encode_layer_rejects_what_it_cannot_take(gpu):
    import torch

    from squeezellm_amd import pack

    w = torch.zeros(8, 64, device=gpu)
    lut = torch.zeros(8, 16, device=gpu)
    with pytest.raises(ValueError, match="CUDA"):
        pack.encode_layer(w.cpu(), lut.cpu(), 4)
    with pytest.raises(ValueError, match="lookup_table"):
        pack.encode_layer(w, lut, 3)
    with pytest.raises(ValueError, match="mask"):
        pack.encode_layer(w, lut, 4, torch.zeros(8, 32, dtype=torch.bool, device=gpu))
    bad = w.clone()
    bad[1, 3] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        pack.encode_layer(bad, lut, 4)
    with pytest.raises(ValueError, match="sqllm_encode"):
        pack.encode_layer(torch.zeros(6, 64, device=gpu), torch.zeros(6, 16, device=gpu), 4)  # N % 4


# ---------------------------------------------------------------------------------------------------------------------
# round trip, the product, capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16"])
@pytest.mark.parametrize("bits", [3, 4])
def test_round_trip_through_the_dense_export(gpu, bits, dtype):
    import torch

    from squeezellm_amd import decode, nuq, pack

    K, N = 544, 68
    w, lut, mask, _ = random_case(bits, K, N, dtype, "mixed")
    lay = pack.encode_layer(torch.from_numpy(w).to(gpu), torch.from_numpy(lut).to(gpu), bits, torch.from_numpy(mask).to(gpu))
    got = decode.dequantize_layer(lay, dtype=torch.float32).cpu().numpy()
    w32 = w.astype(np.float32)
    idx = nuq.assign_indices(torch.from_numpy(w32), torch.from_numpy(lut)).numpy().astype(np.int64)
    off = ~mask
    assert same_bits(got[off], np.take_along_axis(lut, idx, axis=1)[off])
    # on the mask: z_n + fl32(w - z_n), two fp32 roundings of values no larger than |w| + |z_n|; no outlier: z_n itself
    z = lut[np.arange(N), np.abs(lut).argmin(axis=1)][:, None] * np.ones((1, K), np.float32)
    outlier = mask & (w32 != 0) & ((w32 - z) != 0)
    assert outlier.sum() == lay["vals"].numel() > K
    err = np.abs(got.astype(np.float64) - w32.astype(np.float64))
    bound = 2.0 ** -23 * (np.abs(w32.astype(np.float64)) + np.abs(z.astype(np.float64)))
    assert (err[outlier] <= bound[outlier]).all(), float((err[outlier] / bound[outlier]).max())
    rest = mask & ~outlier
    assert rest.any() and same_bits(got[rest], z[rest])


@pytest.mark.parametrize("bits", [3, 4])
def test_encoded_layer_through_the_hybrid_operator(gpu, bits):
    import torch

    from squeezellm_amd import pack, quant_cuda

    K, N = 544, 68
    w, lut, mask, _ = random_case(bits, K, N, "float16", "mixed")
    want = torch_route(w, lut, bits, mask, topX=3, device=gpu)  # the same layer packed by pack_layer
    lay = pack.encode_layer(torch.from_numpy(w).to(gpu), torch.from_numpy(lut).to(gpu), bits, torch.from_numpy(mask).to(gpu), topX=3)
    rng = np.random.default_rng(bits)
    x = rng.normal(size=K).astype(np.float16).astype(np.float32)
    mul = rng.normal(0, 0.5, size=N).astype(np.float32)
    yt = torch.from_numpy(mul).to(gpu)
    H.call_op(quant_cuda, lay, torch.from_numpy(x).to(gpu), yt, "hybrid", False)
    torch.cuda.synchronize()
    ref = H.oracle_ref(want, x, mul, "hybrid")
    assert H.rel_err(yt.cpu().numpy(), ref) <= 2e-5  # tests/test_gpu_parity.py: fp32 outputs against the fp64 oracle


def test_capture_holds_no_allocation_nodes_and_replays(gpu):
    import torch

    from squeezellm_amd import _lib

    lib = _lib.load()
    hip = ctypes.CDLL("libamdhip64.so")
    bits, K, N = 3, 544, 68
    w, lut, mask, want = random_case(bits, K, N, "float16", "mixed")
    nnz = int(want["rows"][N])
    wt, lt, mt = torch.from_numpy(w).to(gpu), torch.from_numpy(lut).to(gpu), torch.from_numpy(mask).to(gpu)
    q = torch.empty((K // 32 * bits, N), dtype=torch.int32, device=gpu)
    rows = torch.empty(N + 1, dtype=torch.int32, device=gpu)
    cols = torch.empty(nnz, dtype=torch.int32, device=gpu)
    vals = torch.empty(nnz, dtype=torch.float32, device=gpu)
    d = _lib.SqllmEncode(bits=bits, K=K, N=N, weight_dtype=_lib.DTYPE_F16, weight=wt.data_ptr(), ld=K, lookup_table=lt.data_ptr(),
                         mask=mt.data_ptr(), qweight=q.data_ptr(), rows=rows.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream  # eagerly once: the code objects are loaded outside the capture
    assert lib.sqllm_encode(ctypes.byref(d), stream) == 0 and lib.sqllm_encode_csr(ctypes.byref(d), cols.data_ptr(), vals.data_ptr(), nnz, stream) == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(g):
        stream = torch.cuda.current_stream().cuda_stream
        rc = (lib.sqllm_encode(ctypes.byref(d), stream), lib.sqllm_encode_csr(ctypes.byref(d), cols.data_ptr(), vals.data_ptr(), nnz, stream))
    assert rc == (0, 0)
    raw = ctypes.c_void_p(g.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) == 0
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(raw, nodes, ctypes.byref(n)) == 0
    types = []
    for nd in nodes:
        ty = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(nd), ctypes.byref(ty)) == 0
        types.append(ty.value)
    # fill, encode, scan + the CSR kernel: kernel (0) and memset (2) nodes only -- no MemAlloc (10) / MemFree (11)
    assert len(types) == 4 and set(types) <= {0, 2} and types.count(0) >= 3, types
    g.instantiate()
    for _ in range(2):  # rows is overwritten, not accumulated into: a second replay gives the same
        q.fill_(0x5A5A5A5A)
        rows.fill_(-1)
        cols.fill_(-1)
        vals.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for got, key in ((q, "qweight"), (rows, "rows"), (cols, "cols"), (vals, "vals")):
            assert same_bits(got.cpu().numpy(), want[key]), key
