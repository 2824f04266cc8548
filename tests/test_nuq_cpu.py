"""CPU tests of offline quantisation (squeezellm_amd.nuq, csrc/sqllm_nuq.hip): the brute-force oracle the GPU tests
hold the kernel to, the fixture the sklearn comparison uses, outlier extraction against a literal restatement of the
reference's squeezellm/outliers.py, the argument checks of sqllm_nuq_fit (no GPU needed) and the kernel's code."""
import ctypes
import importlib.util
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as H

GOLDEN_SCRIPT = os.path.join(H.GOLDEN, "make_nuq_golden.py")
GOLDEN = os.path.join(H.GOLDEN, "nuq_sklearn.npz")


def golden_module():
    spec = importlib.util.spec_from_file_location("make_nuq_golden", GOLDEN_SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------------------------------
# the oracle: O(k K^2) fp64 dynamic programming over every split point (no monotonicity shortcut, no merging of equal
# values), then the cost of the partition it finds summed directly around its centroids
# ---------------------------------------------------------------------------------------------------------------------
def effective_weights(w):
    w = np.asarray(w, np.float64)
    return np.ones_like(w) if w.sum() == 0 else w


def range_centroid(x, w):
    return (w * x).sum() / w.sum() if w.sum() > 0 else x.mean()


def partition_cost(x, w, cuts):
    """(cost, centroids) of the contiguous ranges [cuts[r], cuts[r+1]) of a sorted row."""
    cents, total = [], 0.0
    for a, b in zip(cuts[:-1], cuts[1:]):
        c = range_centroid(x[a:b], w[a:b])
        cents.append(c)
        total += (w[a:b] * (x[a:b] - c) ** 2).sum()
    return total, np.array(cents)


def brute_force_fit(x, w, k):
    """Sorted row x, weights w (>= 0; all zero = unit weights), k ranges -> (cost, centroids fp64, cuts)."""
    x = np.asarray(x, np.float64)
    w = effective_weights(w)
    K = x.size
    assert K >= k and np.all(np.diff(x) >= 0)
    W, S, Q = (np.concatenate([[0.0], np.cumsum(a)]) for a in (w, w * x, w * x * x))
    dW = W[None, :] - W[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        C = (Q[None, :] - Q[:, None]) - (S[None, :] - S[:, None]) ** 2 / dW
    C = np.where(dW > 0, np.maximum(C, 0.0), 0.0)
    m, i = np.meshgrid(np.arange(K + 1), np.arange(K + 1), indexing="ij")
    C[m >= i] = np.inf  # C[m, i]: range [m, i), non-empty
    D = C[0].copy()  # level 1
    args = []
    for _ in range(2, k + 1):
        T = D[:, None] + C
        a = T.argmin(axis=0)
        D = T[a, np.arange(K + 1)]
        args.append(a)
    cuts = [K]
    for a in reversed(args):
        cuts.append(int(a[cuts[-1]]))
    cuts.append(0)
    cuts = cuts[::-1]
    cost, cents = partition_cost(x, w, cuts)
    return cost, cents, cuts


def exhaustive_fit(x, w, k):
    """Every assignment of every element to one of k labels (contiguity not assumed): the minimum cost."""
    x = np.asarray(x, np.float64)
    w = effective_weights(w)
    best = np.inf
    for lab in itertools.product(range(k), repeat=x.size):
        lab = np.array(lab)
        tot = 0.0
        for j in range(k):
            sel = lab == j
            if sel.any():
                c = range_centroid(x[sel], w[sel])
                tot += (w[sel] * (x[sel] - c) ** 2).sum()
        best = min(best, tot)
    return best


def test_oracle_matches_exhaustive_search_on_tiny_rows():
    rng = np.random.default_rng(1)
    for trial in range(12):
        K, k = (7, 3) if trial % 2 else (6, 2)
        x = np.sort(rng.standard_t(3, K))
        if trial % 3 == 0:
            x[2] = x[3] = x[4]  # equal values
            x = np.sort(x)
        w = rng.lognormal(0, 2, K)
        if trial % 4 == 1:
            w[:3] = 0.0  # a zero-weight stretch
        if trial == 5:
            w[:] = 0.0  # unit-weight fallback
        cost, cents, cuts = brute_force_fit(x, w, k)
        assert np.all(np.diff(cents) > 0) and len(cuts) == k + 1
        ex = exhaustive_fit(x, w, k)
        assert cost == pytest.approx(ex, rel=1e-12, abs=1e-15), (trial, cost, ex)


def test_oracle_rows_with_few_distinct_values_cost_nothing():
    x = np.array([0.0, 0.0, 1.0, 1.0, 1.0, 2.0, 2.0, 2.0, 2.0, 2.0])
    cost, cents, _ = brute_force_fit(x, np.ones(10), 8)
    assert cost == 0.0 and set(cents) == {0.0, 1.0, 2.0}


def test_fixture_regenerates():
    g = golden_module()
    d = np.load(GOLDEN)
    assert int(d["seed"]) == g.SEED and tuple(d["Ks"]) == g.KS and int(d["rows_per_k"]) == g.ROWS_PER_K
    for K in g.KS:
        x, sw = g.make_rows(g.SEED, K)
        assert x.shape == sw.shape == (g.ROWS_PER_K, K) and x.dtype == np.float32
        np.testing.assert_allclose(g.checksum(x, sw), d[f"checksum_K{K}"], rtol=1e-12)
        assert np.all(x.astype(np.float16).astype(np.float32) == x)  # fp16-born
        assert (sw[g.ZERO_WEIGHT_ROW] == 0).all() and (sw[0] > 0).all()
        for r in g.OUTLIER_ROWS:
            assert (x[r] == 0).sum() >= K * 5 // 1000 and (sw[r][x[r] == 0] == 0).all()
        for bits in (3, 4):
            sse = d[f"sse_w{bits}_K{K}"]
            assert sse.shape == (g.ROWS_PER_K,) and np.all(np.isfinite(sse)) and np.all(sse > 0)
    # the exact optimum of a fixture row is never above sklearn's (the bar the GPU test holds the kernel to)
    x, sw = g.make_rows(g.SEED, 256)
    for bits in (3, 4):
        for r in range(g.ROWS_PER_K):
            o = np.argsort(x[r], kind="stable")
            cost, _, _ = brute_force_fit(x[r][o], sw[r][o], 1 << bits)
            assert cost <= d[f"sse_w{bits}_K256"][r] * (1 + 1e-9)


# ---------------------------------------------------------------------------------------------------------------------
# outlier extraction: a literal restatement of squeezellm/outliers.py for one module
# ---------------------------------------------------------------------------------------------------------------------
def reference_remove_outliers(weight, gradient, sensitivity, thres):
    outlier_weights = None
    weight = weight.to(torch.float)
    if sensitivity != 0:  # remove_outliers_by_sensitivity._body
        gweight = gradient.to(torch.float)
        num_outliers = int(gweight.numel() * sensitivity / 100)
        t_thres = gweight.reshape(-1).topk(k=num_outliers).values[-1]
        t = gweight > t_thres
        outlier_weights = weight * t
        weight = weight * ~t
    if thres is not None:  # remove_outliers_by_threshold._body
        t = torch.logical_or(weight >= thres, weight <= -thres)
        ow = weight * t
        weight = weight * ~t
        outlier_weights = (0 if outlier_weights is None else outlier_weights) + ow
    return weight, outlier_weights


def test_remove_outliers_follows_the_reference():
    from squeezellm_amd import nuq

    gen = torch.Generator().manual_seed(3)
    w = (0.02 * torch.randn(64, 96, generator=gen)).half()
    g = torch.rand(64, 96, generator=gen) ** 4
    # ties at the sensitivity threshold: entries equal to the num-th largest gradient stay (strictly greater goes)
    g.view(-1)[:40] = 2.0
    for sens, thres in ((0.45, None), (1.0, None), (0.0, 0.03), (0.45, 0.03), (5.0, 0.04), (0.45, 0.0)):
        dense, out = nuq.remove_outliers(w, g, sensitivity=sens, threshold=thres)
        rd, ro = reference_remove_outliers(w, g, sens, thres)
        assert torch.equal(dense, rd) and torch.equal(out, ro), (sens, thres)
        assert torch.equal(dense + out, w.float())
    # 0.45 % of 6144 = 27 < 40 tied maxima: the threshold is 2.0 itself and nothing is strictly above it
    dense, out = nuq.remove_outliers(w, g, sensitivity=0.45)
    assert int((out != 0).sum()) == 0
    # 1 %: 61 entries; the 40 tied 2.0s are > the 61st largest
    dense, out = nuq.remove_outliers(w, g, sensitivity=1.0)
    assert int((g > 1.99).logical_and(w != 0).logical_and(out == 0).sum()) == 0
    # >= on the magnitude threshold: an entry exactly at it goes
    w2 = torch.tensor([[0.5, -0.5, 0.375, -0.25, 0.0, 1.0]])
    dense, out = nuq.remove_outliers(w2, threshold=0.5)
    assert out.tolist() == [[0.5, -0.5, 0.0, 0.0, 0.0, 1.0]] and dense.tolist() == [[0.0, 0.0, 0.375, -0.25, 0.0, 0.0]]
    # order: sensitivity first, then the threshold on what is left (a sensitivity outlier is not counted twice)
    g2 = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 9.0]])
    dense, out = nuq.remove_outliers(w2, g2, sensitivity=34.0, threshold=0.5)  # num = 2: 2nd largest gradient is 0
    rd, ro = reference_remove_outliers(w2, g2, 34.0, 0.5)
    assert torch.equal(out, ro) and torch.equal(dense, rd) and out.tolist() == [[0.5, -0.5, 0.0, 0.0, 0.0, 1.0]]
    # num == 0: no sensitivity outliers (the reference's topk(k=0) would raise)
    dense, out = nuq.remove_outliers(w2, g2, sensitivity=1.0)
    assert torch.equal(dense, w2) and not out.any()


def test_assign_indices_takes_the_first_nearest_centroid():
    from squeezellm_amd import nuq

    lut = torch.tensor([[-1.0, 0.0, 0.0, 1.0, 1.0, 2.0, 3.0, 4.0]])
    w = torch.tensor([[-5.0, -0.5, 0.0, 0.4, 0.5, 0.9, 1.0, 2.5, 9.0]])
    idx = nuq.assign_indices(w, lut)
    assert idx.dtype == torch.uint8 and idx.tolist() == [[0, 0, 1, 1, 1, 3, 3, 5, 7]]
    assert int(idx[0, 2]) == int(lut.abs().argmin())  # the index pack.outliers_to_csr takes for a removed outlier


def test_quantize_state_dict_picks_the_decoder_linears():
    from squeezellm_amd import nuq

    sd = {"model.embed_tokens.weight": torch.zeros(8, 4), "model.layers.0.self_attn.q_proj.weight": torch.zeros(4, 4),
          "model.layers.3.mlp.down_proj.weight": torch.zeros(4, 4), "model.layers.0.input_layernorm.weight": torch.zeros(4),
          "lm_head.weight": torch.zeros(8, 4), "model.decoder.layers.1.fc1.weight": torch.zeros(4, 4)}
    assert nuq.default_names(sd) == ["model.layers.0.self_attn.q_proj", "model.layers.3.mlp.down_proj", "model.decoder.layers.1.fc1"]
    assert [nuq._short_name(n) for n in nuq.default_names(sd)] == ["q", "down", "up"]


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI: arguments checked before the device is touched (the library loads without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
def test_nuq_fit_rejects_bad_arguments_before_touching_the_device():
    from squeezellm_amd import _lib

    lib = _lib.load()
    d = _lib.SqllmNuq(bits=4, N=3, K=64, values=16, weights=None, centroids=16, cost=None)
    need = lib.sqllm_nuq_workspace_bytes(ctypes.byref(d))
    assert need > 0 and need == _lib.nuq_workspace_bytes(4, 3, 64)
    assert _lib.nuq_workspace_bytes(4, 4096, 64) == _lib.nuq_workspace_bytes(4, 1024, 64) > need  # slots are capped
    assert lib.sqllm_nuq_fit(None, 16, need, None) == -3
    assert lib.sqllm_nuq_fit(ctypes.byref(d), None, need, None) == -3  # SQLLM_E_NULL: workspace
    assert lib.sqllm_nuq_fit(ctypes.byref(d), 16, need - 1, None) == -2  # SQLLM_E_SHAPE: short workspace
    for field, value, code in (("bits", 2, -1), ("bits", 5, -1), ("K", 15, -2), ("K", 65536, -2), ("N", 0, -2),
                               ("values", None, -3), ("centroids", None, -3)):
        bad = _lib.SqllmNuq(bits=4, N=3, K=64, values=16, weights=None, centroids=16, cost=None)
        setattr(bad, field, value)
        assert lib.sqllm_nuq_fit(ctypes.byref(bad), 16, 1 << 40, None) == code, (field, value)
        if field in ("bits", "K", "N"):
            assert lib.sqllm_nuq_workspace_bytes(ctypes.byref(bad)) == code
    d3 = _lib.SqllmNuq(bits=3, N=1, K=8, values=16, centroids=16)
    assert lib.sqllm_nuq_fit(ctypes.byref(d3), 16, 0, None) == -2  # K == 2^bits is fine, a zero workspace is short
    with pytest.raises(ValueError):
        _lib.nuq_workspace_bytes(3, 1, 7)


def test_fit_lut_refuses_cpu_tensors_and_non_finite_input():
    from squeezellm_amd import nuq

    with pytest.raises(ValueError, match="CUDA"):
        nuq.fit_lut(torch.zeros(4, 64), None, 4)
    with pytest.raises(ValueError):
        nuq.fit_lut(torch.zeros(4, 64), None, 5)


def test_nuq_kernel_has_no_scratch_and_no_vector_spills(tmp_path):
    """The fit kernel keeps everything in registers, LDS and the caller's workspace."""
    from squeezellm_amd import build as B

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = tmp_path / "nuq.s"
    subprocess.run([hipcc, f"--offload-arch={B.ARCH}", *[f for f in B.FLAGS if f != "-fPIC"], "-S", "--cuda-device-only",
                    f"-I{B.INCLUDE}", f"-I{B.CSRC}", os.path.join(B.CSRC, "sqllm_nuq.hip"), "-o", str(out)], check=True, capture_output=True)
    asm = out.read_text()
    kernels = re.findall(r"\.name:\s+(_Z\w*nuq_fit_kernel\w*)", asm)
    assert len(kernels) == 2, kernels  # 3- and 4-bit
    for key in ("private_segment_fixed_size", "vgpr_spill_count"):
        vals = [int(v) for v in re.findall(rf"\.{key}:\s+(\d+)", asm)]
        assert vals and all(v == 0 for v in vals), (key, vals)
    assert "scratch_" not in "\n".join(l for l in asm.splitlines() if not l.lstrip().startswith((".", ";")))
    assert "sqllm_nuq.hip" in B.SOURCES
