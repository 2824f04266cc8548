#!/usr/bin/env python3
"""Generate tests/golden/nuq_sklearn.npz: what the reference's per-row k-means (quantization/nuq.py:50-58, sklearn KMeans
with sample weights) reaches on seeded rows, as the bar the exact fit of squeezellm_amd.nuq must meet or beat.

The rows are NOT stored: `make_rows` regenerates them from the seed (tests/test_nuq_cpu.py checks that they still do,
through the stored checksums), so the fixture stays a few KB.  sklearn is called directly with nuq.py's settings
(n_clusters=2**bits, random_state=0, n_init="auto", max_iter=50); no reference code is involved.

    python tests/golden/make_nuq_golden.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "nuq_sklearn.npz")
SEED = 20240611
KS = (256, 1024, 4096)
ROWS_PER_K = 8
OUTLIER_ROWS = (2, 5)  # 0.5 % of their largest-magnitude weights zeroed (as outlier extraction leaves them)
ZERO_WEIGHT_ROW = 7    # all sample weights 0: fitted with unit weights (nuq.py:174-175)


def make_rows(seed=SEED, K=256, n=ROWS_PER_K):
    """(values fp32 [n, K], sample weights fp32 [n, K]) of one K: heavy-tailed fp16-rounded weights (Student t, 3
    degrees of freedom), log-normal squared-gradient weights masked by (value != 0), as nuq.py:172-173 forms them."""
    rng = np.random.default_rng([seed, K])
    x = (0.02 * rng.standard_t(3, size=(n, K))).astype(np.float16).astype(np.float32)
    g = rng.lognormal(mean=-12.0, sigma=2.0, size=(n, K)).astype(np.float32)
    for r in OUTLIER_ROWS:
        top = np.argsort(-np.abs(x[r]), kind="stable")[: max(1, K * 5 // 1000)]
        x[r, top] = 0.0
    g[ZERO_WEIGHT_ROW] = 0.0
    return x, g * (x != 0)


def effective_weights(sw):
    """nuq.py:174-175: a row whose weights sum to 0 is fitted with unit weights."""
    sw = sw.astype(np.float64)
    out = sw.copy()
    out[sw.sum(axis=1) == 0] = 1.0
    return out


def weighted_sse(x, sw, centroids):
    """Per-row sum of w * (x - nearest centroid)^2 in fp64 (the objective both fits minimise)."""
    x64, c = x.astype(np.float64), np.asarray(centroids, np.float64)
    d = (x64[:, :, None] - c[:, None, :]) ** 2
    return (effective_weights(sw) * d.min(axis=2)).sum(axis=1)


def checksum(x, sw):
    return np.array([x.astype(np.float64).sum(), np.abs(x.astype(np.float64)).sum(), sw.astype(np.float64).sum()])


def sklearn_fit(x, sw, bits):
    from sklearn.cluster import KMeans

    w = effective_weights(sw)
    cents = np.zeros((x.shape[0], 1 << bits))
    for r in range(x.shape[0]):
        km = KMeans(n_clusters=1 << bits, random_state=0, n_init="auto", max_iter=50).fit(x[r].reshape(-1, 1), sample_weight=w[r])
        cents[r] = km.cluster_centers_.reshape(-1)
    return cents


def main():
    import sklearn

    out = dict(seed=np.int64(SEED), Ks=np.array(KS), rows_per_k=np.int64(ROWS_PER_K), sklearn_version=np.array(sklearn.__version__))
    for K in KS:
        x, sw = make_rows(SEED, K)
        out[f"checksum_K{K}"] = checksum(x, sw)
        for bits in (3, 4):
            out[f"sse_w{bits}_K{K}"] = weighted_sse(x, sw, sklearn_fit(x, sw, bits))
    np.savez(OUT, **out)
    print(f"wrote {OUT}")


if __name__ == "__main__":
    main()
