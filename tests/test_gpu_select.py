"""Outlier selection on the GPU (sqllm_select / sqllm_outlier_mask and what nuq builds on them): exact order statistics
against np.sort, the mask bit for bit against the torch union of nuq._outlier_masks, captured, and end to end through
quantize_state_dict and the command line.  Expectations are computed with numpy / torch in the test.  Outputs carry guard
elements the kernels must leave alone, and the workspace is filled with 0xFF before every raw call."""
import ctypes
import functools
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 3


def select_raw(gpu, x, ranks, pad=0):
    """Straight through the C ABI.  x: numpy [rows, cols] fp16 / fp32, copied into a [rows, cols + pad] buffer whose pad
    alternates +inf and -1e30 (fp16: -6e4) and is checked untouched.  Returns (out fp32, less int64) as numpy."""
    import torch

    from squeezellm_amd import _lib

    lib = _lib.load()
    rows, cols = x.shape
    tdt = torch.from_numpy(x).dtype
    buf = torch.empty((rows, cols + pad), dtype=tdt, device=gpu)
    if pad:
        junk = torch.tensor([float("inf"), -1e30 if x.dtype == np.float32 else -6e4], dtype=tdt, device=gpu).repeat(pad // 2)
        buf[:, cols:] = junk
    buf[:, :cols] = torch.from_numpy(x).to(gpu)
    n = len(ranks)
    dt = _lib.DTYPE_F16 if x.dtype == np.float16 else _lib.DTYPE_F32
    out = torch.full((n + GUARD,), float("nan"), dtype=torch.float32, device=gpu)
    less = torch.full((n + GUARD,), -7, dtype=torch.int64, device=gpu)
    ws = torch.full((_lib.select_workspace_bytes(dt, n, rows, cols, cols + pad),), 0xFF, dtype=torch.uint8, device=gpu)
    d = _lib.SqllmSelect(dtype=dt, n_ranks=n, values=buf.data_ptr(), rows=rows, cols=cols, ld=cols + pad, out=out.data_ptr(), less=less.data_ptr())
    for i, r in enumerate(ranks):
        d.ranks[i] = int(r)
    assert lib.sqllm_select(ctypes.byref(d), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    o, l = out.cpu().numpy(), less.cpu().numpy()
    assert np.isnan(o[n:]).all() and (l[n:] == -7).all()
    if pad:
        assert torch.equal(buf[:, cols:], junk.expand(rows, pad))
    return o[:n], l[:n]


def check_ranks(gpu, x, ranks, pad=0):
    """out by value (and +0.0 for a zero) and less against numpy, eight ranks per call."""
    flat = np.sort(x.astype(np.float32), axis=None)
    ranks = list(ranks)
    for i0 in range(0, len(ranks), 8):
        part = ranks[i0:i0 + 8]
        out, less = select_raw(gpu, x, part, pad=pad)
        want = flat[part]
        assert np.array_equal(out, want), (part, out, want)
        assert not np.signbit(out[out == 0]).any()
        assert np.array_equal(less, np.searchsorted(flat, want, side="left")), (part, less)


@functools.lru_cache(maxsize=None)
def gauss(rows, cols, dtype, seed=0):
    return (0.02 * np.random.default_rng(seed).standard_normal((rows, cols))).astype(np.dtype(dtype))


def quartile_neighbours(n):
    from squeezellm_amd import nuq

    return [r for q in (0.25, 0.75) for r in nuq.quantile_ranks(n, q)[:2]]


# ---------------------------------------------------------------------------------------------------------------------
# 1. exact order statistics and `less`
# ---------------------------------------------------------------------------------------------------------------------
def test_every_rank_of_a_small_matrix(gpu):
    x = gauss(4, 32, "float32", 1)
    order = np.random.default_rng(2).permutation(128).tolist()  # unsorted
    order.append(order[5])
    order[5] = order[2]  # a repeated rank within one call; the one it displaced goes last, in a call of its own
    assert sorted(set(order)) == list(range(128)) and len(order) == 129
    check_ranks(gpu, x, order)


def test_padded_rows_are_never_read(gpu):
    x = gauss(64, 96, "float32", 3)
    n = x.size
    check_ranks(gpu, x, [0, n - 1, n // 2, 1, n - 2, 4097, 77, n // 3], pad=8)


def test_fp16_matrix(gpu):
    x = gauss(257, 160, "float16", 4)
    n = x.size
    check_ranks(gpu, x, [0, n - 1, *quartile_neighbours(n), n // 2, 12345, 1, n - 2, 3, n // 7])


def test_gaussian_weights_at_the_quartiles(gpu):
    x = gauss(1024, 1024, "float32", 5)
    n = x.size
    check_ranks(gpu, x, [0, n - 1, *quartile_neighbours(n)])


# ---------------------------------------------------------------------------------------------------------------------
# 2. adversarial keys
# ---------------------------------------------------------------------------------------------------------------------
def adversarial(kind, rows, cols):
    n = rows * cols
    rng = np.random.default_rng(rows + len(kind))
    if kind == "equal":
        return np.full((rows, cols), 0.37, np.float32)
    if kind == "two":
        return np.where(rng.random((rows, cols)) < 0.3, np.float32(-1.5), np.float32(2.25)).astype(np.float32)
    if kind == "last_digit":  # 1.0 + i ulp, i < 256: only the lowest digit of the key differs
        return (np.float32(1.0).view(np.uint32) + (rng.permutation(n) % 256).astype(np.uint32)).view(np.float32).reshape(rows, cols)
    if kind == "ties":
        return rng.integers(0, 8, (rows, cols)).astype(np.float32)
    if kind == "specials":
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1e-38, -1.1e-38, float(np.float16(6e-8)), -float(np.float16(6e-8)), float(np.float16(5.9e-5)),
                         np.inf, -np.inf, 1.0, -1.0, 3.4e38, -3.4e38], np.float32)
        return pool[rng.integers(0, pool.size, (rows, cols))]
    if kind == "negative":
        return -np.abs(gauss(rows, cols, "float32", 9)) - np.float32(1e-6)
    raise AssertionError(kind)


@pytest.mark.parametrize("rows,cols", [(8, 64), (300, 256)])
@pytest.mark.parametrize("kind", ["equal", "two", "last_digit", "ties", "specials", "negative"])
def test_adversarial_keys(gpu, kind, rows, cols):
    x = adversarial(kind, rows, cols)
    n = x.size
    with np.errstate(all="ignore"):
        check_ranks(gpu, x, [0, n - 1, n // 2, n // 2 - 1, *quartile_neighbours(n), n // 3, 1, n - 2, (n * 3) // 10 - 1, (n * 3) // 10, 7])
    if kind == "specials":
        with np.errstate(all="ignore"):
            h = x.astype(np.float16)  # +-inf, +-0, fp16 subnormals and overflowed values as halves
        check_ranks(gpu, h, [0, n - 1, n // 2, n // 2 - 1, n // 3, 1, n - 2, n // 5])


# ---------------------------------------------------------------------------------------------------------------------
# 3. reproducible and self-initialising
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_two_runs_are_byte_identical(gpu, dtype):
    x = gauss(300, 256, dtype, 6)
    n = x.size
    ranks = [0, n - 1, *quartile_neighbours(n), n // 2, n // 2]
    a, b = select_raw(gpu, x, ranks), select_raw(gpu, x, ranks)  # (each with its workspace filled with 0xFF, guards checked)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    check_ranks(gpu, x, ranks)


# ---------------------------------------------------------------------------------------------------------------------
# 4. past torch.quantile's limit
# ---------------------------------------------------------------------------------------------------------------------
def test_a_matrix_torch_quantile_refuses(gpu):
    import torch

    from squeezellm_amd import nuq

    gen = torch.Generator(device=gpu).manual_seed(7)
    x = (0.02 * torch.randn((4096, 4352), generator=gen, device=gpu)).half()
    n = x.numel()
    assert n > 16_000_000
    ranks = quartile_neighbours(n)
    vals, less = nuq.order_statistics(x, ranks)
    flat = torch.sort(x.reshape(-1)).values
    want = flat[torch.tensor(ranks, device=gpu)].float()
    assert torch.equal(vals, want)
    assert torch.equal(less, torch.searchsorted(flat, want.half(), right=False))


# ---------------------------------------------------------------------------------------------------------------------
# 5. capture
# ---------------------------------------------------------------------------------------------------------------------
def test_select_then_mask_captured_in_one_graph(gpu):
    import torch

    from squeezellm_amd import _lib

    lib = _lib.load()
    hip = ctypes.CDLL("libamdhip64.so")
    N, K = 260, 160
    w = torch.from_numpy(gauss(N, K, "float16", 8)).to(gpu)
    g = torch.from_numpy(gauss(N, K, "float32", 9) ** 2).to(gpu)
    n = N * K
    num = int(n * 0.45 / 100)
    out = torch.empty(1, dtype=torch.float32, device=gpu)
    mask = torch.empty((N, K), dtype=torch.bool, device=gpu)
    count = torch.empty(1, dtype=torch.int64, device=gpu)
    wt = torch.tensor([0.05], dtype=torch.float32, device=gpu)
    ws = torch.empty(_lib.select_workspace_bytes(_lib.DTYPE_F32, 1, N, K), dtype=torch.uint8, device=gpu)
    ds = _lib.SqllmSelect(dtype=_lib.DTYPE_F32, n_ranks=1, values=g.data_ptr(), rows=N, cols=K, ld=K, out=out.data_ptr())
    ds.ranks[0] = n - num
    dm = _lib.SqllmOutlier(weight_dtype=_lib.DTYPE_F16, grad_dtype=_lib.DTYPE_F32, K=K, N=N, weight=w.data_ptr(), ld_w=K, gradient=g.data_ptr(),
                           ld_g=K, g_threshold=out.data_ptr(), w_threshold=wt.data_ptr(), mask=mask.data_ptr(), count=count.data_ptr())

    def enqueue():
        stream = torch.cuda.current_stream().cuda_stream
        return lib.sqllm_select(ctypes.byref(ds), ws.data_ptr(), ws.numel(), stream), lib.sqllm_outlier_mask(ctypes.byref(dm), stream)

    assert enqueue() == (0, 0)  # eagerly once: the code objects are loaded outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        rc = enqueue()
    assert rc == (0, 0)
    raw = ctypes.c_void_p(graph.raw_cuda_graph())
    cnt = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, ctypes.byref(cnt)) == 0
    nodes = (ctypes.c_void_p * cnt.value)()
    assert hip.hipGraphGetNodes(raw, nodes, ctypes.byref(cnt)) == 0
    types = []
    for nd in nodes:
        ty = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(nd), ctypes.byref(ty)) == 0
        types.append(ty.value)
    # select: a fill and 2 x 3 kernels (fp32); the mask: a fill and one kernel -- kernel (0) and memset (2) nodes only
    assert len(types) == 9 and set(types) <= {0, 2} and types.count(0) == 7, types
    graph.instantiate()

    def expect():
        thres = g.reshape(-1).topk(num).values[-1]
        m = (g > thres) | (w.float() >= 0.05) | (w.float() <= -0.05)
        return thres, m

    for step in range(2):
        if step == 1:  # the input changes in place: the replay answers for the new input
            g.mul_(torch.from_numpy(np.random.default_rng(10).random((N, K)).astype(np.float32)).to(gpu))
            w.neg_()
        out.fill_(float("nan"))
        mask.fill_(True)
        count.fill_(-1)
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        thres, m = expect()
        assert out[0].item() == thres.item() and torch.equal(mask, m) and count.item() == int(m.sum()) > num // 2


# ---------------------------------------------------------------------------------------------------------------------
# 6. quantiles and thresholds
# ---------------------------------------------------------------------------------------------------------------------
QSHAPES = [(4, 32, "float32"), (64, 96, "float32"), (257, 160, "float16"), (1024, 1024, "float32"), (257, 160, "float32"), (64, 96, "float16")]


@pytest.mark.parametrize("rows,cols,dtype", QSHAPES)
def test_quantiles_and_the_outlier_threshold(gpu, rows, cols, dtype):
    import torch

    from squeezellm_amd import nuq

    x = gauss(rows, cols, dtype, 11)
    t = torch.from_numpy(x).to(gpu)
    x64 = x.astype(np.float64)
    flat = np.sort(x64, axis=None)
    qs = (0.0, 0.25, 0.5, 0.75, 1.0, 0.123)
    got = nuq.quantiles(t, qs)
    for q, v in zip(qs, got):
        lo, hi, _ = nuq.quantile_ranks(x.size, q)
        want = np.quantile(x64, q)
        # two fp64 evaluations of one lerp between the same two exact order statistics
        assert isinstance(v, float) and abs(v - want) <= 1e-14 * max(abs(flat[lo]), abs(flat[hi])), (q, v, want)
    for r in (1.0, 1.8, 3.0):
        q1 = np.quantile(x64, 0.25)
        q3 = np.quantile(x64, 0.75)
        minimum = q1 - r * (q3 - q1)
        maximum = q3 + r * (q3 - q1)
        want = max(abs(minimum), abs(maximum))
        T = nuq.outlier_threshold(t, r)
        assert isinstance(T, float) and abs(T - want) <= 1e-13 * want, (r, T, want)  # (1 + 2 r) amplifies the 1e-14 of each quartile
    with pytest.raises(ValueError):
        nuq.order_statistics(t[:, :12], [0])  # not contiguous
    with pytest.raises(ValueError):
        nuq.order_statistics(t, [x.size])


# ---------------------------------------------------------------------------------------------------------------------
# 7. the sensitivity cut
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["squares", "zeros"])
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_sensitivity_cut_is_topk(gpu, dtype, kind):
    import torch

    from squeezellm_amd import nuq

    g = gauss(257, 160, "float32", 12).astype(np.float64) ** 2 * 2500
    if kind == "zeros":
        g[np.random.default_rng(13).random(g.shape) < 0.6] = 0.0
    gt = torch.from_numpy(g.astype(np.dtype(dtype))).to(gpu)
    for pct in (0.05, 0.45, 5.0, 50.0):
        num = int(gt.numel() * pct / 100)
        want = gt.float().reshape(-1).topk(num).values[-1]
        got = nuq.sensitivity_threshold(gt, pct)
        assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (pct, got.item(), want.item())
    assert nuq.sensitivity_threshold(gt, 0.002) is None  # num == 0


# ---------------------------------------------------------------------------------------------------------------------
# 8. the mask kernel
# ---------------------------------------------------------------------------------------------------------------------
def mask_raw(gpu, w, g, g_thres, w_thres, pad_w=0, pad_g=0, want_mask=True):
    """Straight through the C ABI: w / g numpy [N, K] (g may be None), thresholds floats or None.  Returns (mask uint8
    numpy or None, count)."""
    import torch

    from squeezellm_amd import _lib

    lib = _lib.load()
    N, K = w.shape

    def padded(a, pad):
        buf = torch.full((N, K + pad), 1e4, dtype=torch.from_numpy(a).dtype, device=gpu)  # (the pad would be an outlier)
        buf[:, :K] = torch.from_numpy(a).to(gpu)
        return buf

    wb = padded(w, pad_w)
    gb = None if g is None else padded(g, pad_g)
    gt = None if g is None else torch.tensor([g_thres], dtype=torch.float32, device=gpu)
    wt = None if w_thres is None else torch.tensor([w_thres], dtype=torch.float32, device=gpu)
    mask = torch.full((N * K + 8,), 0x5A, dtype=torch.uint8, device=gpu) if want_mask else None
    count = torch.full((2,), -5, dtype=torch.int64, device=gpu)
    f16 = lambda a: _lib.DTYPE_F16 if a.dtype == np.float16 else _lib.DTYPE_F32
    d = _lib.SqllmOutlier(weight_dtype=f16(w), grad_dtype=0 if g is None else f16(g), K=K, N=N, weight=wb.data_ptr(), ld_w=K + pad_w,
                          gradient=None if g is None else gb.data_ptr(), ld_g=0 if g is None else K + pad_g,
                          g_threshold=None if g is None else gt.data_ptr(), w_threshold=None if wt is None else wt.data_ptr(),
                          mask=None if mask is None else mask.data_ptr(), count=count.data_ptr())
    assert lib.sqllm_outlier_mask(ctypes.byref(d), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert count[1].item() == -5
    if mask is None:
        return None, count[0].item()
    m = mask.cpu().numpy()
    assert (m[N * K:] == 0x5A).all()
    return m[:N * K].reshape(N, K), count[0].item()


@pytest.mark.parametrize("steps", ["gradient", "threshold", "both"])
@pytest.mark.parametrize("gdtype", ["float32", "float16"])
@pytest.mark.parametrize("wdtype", ["float32", "float16"])
@pytest.mark.parametrize("N,K,pad_w,pad_g", [(4, 32, 0, 0), (260, 160, 8, 16)])
def test_mask_kernel_is_the_torch_union(gpu, N, K, pad_w, pad_g, wdtype, gdtype, steps):
    import torch

    from squeezellm_amd import nuq

    w = gauss(N, K, wdtype, 14)
    g = (gauss(N, K, "float32", 15).astype(np.float64) ** 2 * 2500).astype(np.dtype(gdtype))
    # thresholds that ARE elements: > for the gradient, >= / <= for the weight
    g_thres = float(np.sort(g, axis=None)[-max(2, g.size // 50)])
    w_thres = float(np.sort(np.abs(w), axis=None)[-max(2, w.size // 40)])
    use_g, use_t = steps != "threshold", steps != "gradient"
    wt, gtens = torch.from_numpy(w).to(gpu), torch.from_numpy(g).to(gpu)
    # the specification: the two masks of _outlier_masks, with the cut given instead of found
    g32 = gtens.float()
    t = (g32 > g_thres) if use_g else None
    left = wt.float() if t is None else wt.float() * ~t
    t2 = torch.logical_or(left >= w_thres, left <= -w_thres) if use_t else None
    want = t if t2 is None else t2 if t is None else torch.logical_or(t, t2)
    got, count = mask_raw(gpu, w, g if use_g else None, g_thres, w_thres if use_t else None, pad_w, pad_g)
    assert set(np.unique(got)) <= {0, 1} and np.array_equal(got.astype(bool), want.cpu().numpy())
    assert count == int(want.sum()) > 0
    if use_g:
        assert 1 <= int((g32 > g_thres).sum()) < max(2, g.size // 50)
        if not use_t:
            assert not got[g == g.dtype.type(g_thres)].any()  # the element equal to the cut is not above it
    if use_t:
        assert got[np.abs(w) == np.abs(w).dtype.type(w_thres)].all()  # ... and the weight equal to the threshold is in
    _, count_only = mask_raw(gpu, w, g if use_g else None, g_thres, w_thres if use_t else None, pad_w, pad_g, want_mask=False)
    assert count_only == count
    # the same through nuq.outlier_mask (which finds the cut itself): the torch route on CPU tensors is the reference
    sens = 2.0 if use_g else 0.0
    m = nuq.outlier_mask(wt, gtens if use_g else None, sensitivity=sens, threshold=w_thres if use_t else None)
    ref = nuq.outlier_mask(wt.cpu(), gtens.cpu() if use_g else None, sensitivity=sens, threshold=w_thres if use_t else None)
    assert m.dtype == torch.bool and m.is_cuda and torch.equal(m.cpu(), ref)
    big = torch.zeros((N, K + 8), dtype=wt.dtype, device=gpu)
    big[:, :K] = wt
    assert torch.equal(nuq.outlier_mask(big[:, :K], gtens if use_g else None, sensitivity=sens, threshold=w_thres if use_t else None).cpu(), ref)
    if use_t:
        # a Python float fp32 cannot hold (outlier_threshold's fp64 T is one): a hair above / below an existing |w|, and
        # halfway to the next fp32.  torch rounds the float to fp32 before it compares; the kernel route must round alike.
        e = np.float32(w_thres)
        for thr in (float(e) * (1 + 1e-9), float(e) * (1 - 1e-9), (float(e) + float(np.nextafter(e, np.float32(np.inf)))) / 2):
            assert float(np.float32(thr)) != thr
            m = nuq.outlier_mask(wt, gtens if use_g else None, sensitivity=sens, threshold=thr)
            ref = nuq.outlier_mask(wt.cpu(), gtens.cpu() if use_g else None, sensitivity=sens, threshold=thr)
            assert torch.equal(m.cpu(), ref), thr


# ---------------------------------------------------------------------------------------------------------------------
# 9. end to end
# ---------------------------------------------------------------------------------------------------------------------
LLAMA = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")
OPT = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "fc1", "fc2")


def synthetic(kind):
    import torch

    rng = np.random.default_rng(len(kind))
    prefix, mods = ("model.layers", LLAMA) if kind == "llama" else ("model.decoder.layers", OPT)
    sd, gd = {}, {}
    for li in range(2):
        for m in mods:
            N, K = (256, 128) if m.endswith(("gate_proj", "up_proj", "fc1")) else (128, 256) if m.endswith(("down_proj", "fc2")) else (128, 128)
            w = 0.02 * rng.standard_normal((N, K))
            w[rng.random((N, K)) < 0.002] *= 8  # a heavy tail: threshold outliers exist
            sd[f"{prefix}.{li}.{m}.weight"] = torch.from_numpy(w.astype(np.float16))
            gd[f"{prefix}.{li}.{m}.weight"] = torch.from_numpy((rng.standard_normal((N, K)) ** 2).astype(np.float32))
    sd["lm_head.weight"] = torch.from_numpy(rng.standard_normal((8, 128)).astype(np.float16))
    return sd, gd


def same_state_dicts(a, b):
    import torch

    assert list(a) == list(b)
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("kind", ["llama", "opt"])
def test_end_to_end(gpu, kind, tmp_path):
    import torch

    from squeezellm_amd import nuq

    sd, gd = synthetic(kind)
    cfg = nuq.outlier_config(sd, 1.8)
    mods = LLAMA if kind == "llama" else OPT
    short = {"llama": ["q", "k", "v", "o", "gate", "up", "down"], "opt": ["q", "k", "v", "o", "up", "down"]}[kind]
    assert list(cfg) == ["outlier_threshold", "outlier_config"] and len(cfg["outlier_config"]) == 2
    total = outliers = 0
    for li, layer in enumerate(cfg["outlier_config"]):
        assert list(layer) == short
        for m, s in zip(mods, short):
            w = sd[[k for k in sd if f".{li}.{m}." in k][0]].numpy().astype(np.float64)
            q1, q3 = np.quantile(w, 0.25), np.quantile(w, 0.75)
            want = max(abs(q1 - 1.8 * (q3 - q1)), abs(q3 + 1.8 * (q3 - q1)))
            assert type(layer[s]) is float and abs(layer[s] - want) <= 1e-13 * want
            total += w.size
            outliers += int((np.abs(w.astype(np.float32)) >= np.float32(layer[s])).sum())
    assert cfg["outlier_threshold"] == round(outliers / total * 100, 2) and 0 < outliers < total // 20
    assert json.loads(json.dumps(cfg)) == cfg

    direct = nuq.quantize_state_dict(sd, gd, 3, sensitivity=0.45, outlier_range=1.8)
    via_cfg = nuq.quantize_state_dict(sd, gd, 3, sensitivity=0.45, outlier_config=cfg)
    same_state_dicts(direct, via_cfg)
    assert any(k.endswith(".vals") and v.numel() > 0 for k, v in direct.items())  # dense-and-sparse
    with pytest.raises(ValueError, match="mutually exclusive"):
        nuq.quantize_state_dict(sd, gd, 3, outlier_config=cfg, outlier_range=1.8)

    # the command line: --range writes the same checkpoint, --write-outlier-config the same JSON (alone, and on the way)
    torch.save(sd, tmp_path / "sd.pt")
    torch.save(gd, tmp_path / "g.pt")
    assert nuq.main(["--model", str(tmp_path / "sd.pt"), "--range", "1.8", "--write-outlier-config", str(tmp_path / "cfg.json")]) == 0
    assert json.load(open(tmp_path / "cfg.json")) == cfg and not (tmp_path / "sq.pt").exists()
    assert nuq.main(["--model", str(tmp_path / "sd.pt"), "--gradient", str(tmp_path / "g.pt"), "--bits", "3", "--range", "1.8",
                     "--sensitivity", "0.45", "--out", str(tmp_path / "sq.pt"), "--write-outlier-config", str(tmp_path / "cfg2.json")]) == 0
    same_state_dicts(torch.load(tmp_path / "sq.pt"), {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in direct.items()})
    assert json.load(open(tmp_path / "cfg2.json")) == cfg
    with pytest.raises(SystemExit):
        nuq.main(["--model", str(tmp_path / "sd.pt"), "--range", "1.8", "--outlier-config", str(tmp_path / "cfg.json"), "--gradient", "g", "--bits", "3", "--out", "o"])
