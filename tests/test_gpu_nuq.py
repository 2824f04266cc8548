"""Offline quantisation on the GPU (squeezellm_amd.nuq, csrc/sqllm_nuq.hip): the kernel's per-row optimum against the
brute-force oracle of tests/test_nuq_cpu.py (edge rows included, workspace poisoned with NaN first), the optimum against
sklearn's k-means on the fixture rows (the reference's quantization/nuq.py settings), the index rule, and the whole
route weight + Fisher diagonal -> operands -> QuantLinearLUT forward / checkpoint."""
import ctypes
import json

import numpy as np
import pytest
import torch

from tests.test_nuq_cpu import brute_force_fit, effective_weights, golden_module

pytestmark = pytest.mark.gpu


def _edge_rows(K, k, rng):
    """Rows (values fp32 ascending, weights fp32) of every kind sqllm_nuq_fit promises something about."""
    rows = []
    x = np.sort((0.02 * rng.standard_t(3, K)).astype(np.float16).astype(np.float32))
    g = rng.lognormal(-12, 2, K).astype(np.float32)
    rows.append((x, g))                                  # heavy tails, fp16 duplicates
    rows.append((x, np.zeros(K, np.float32)))            # weights sum to 0: unit weights
    g2 = g.copy()
    g2[: K // 3] = 0.0
    rows.append((x, g2))                                 # a zero-weight stretch (ranges of zero total weight)
    few = np.sort(rng.choice(np.float32([-0.5, 0.0, 0.25, 1.0]), K)).astype(np.float32)
    rows.append((few, rng.lognormal(0, 1, K).astype(np.float32)))  # 4 distinct values < k
    rows.append((np.full(K, 0.125, np.float32), g))     # constant row
    xs = np.sort(rng.normal(0, 1, K).astype(np.float32))
    rows.append((xs, rng.lognormal(0, 3, K).astype(np.float32)))   # continuous, widely spread weights
    zero_out = x.copy()
    zero_out[np.argsort(-np.abs(zero_out))[: max(1, K // 200)]] = 0.0
    zero_out = np.sort(zero_out)
    rows.append((zero_out, g * (zero_out != 0)))         # outliers removed: zeros of weight 0
    big = np.sort(rng.normal(0, 3e4, K).astype(np.float32))
    rows.append((big, rng.lognormal(5, 2, K).astype(np.float32)))  # large magnitudes
    return rows


def _fit(bits, x, w, use_weights=True, poison=True):
    """sqllm_nuq_fit straight through the C ABI on a NaN-filled workspace."""
    from squeezellm_amd import _lib

    lib = _lib.load()
    N, K = x.shape
    dev = torch.device("cuda:0")
    xv = torch.from_numpy(x).to(dev).contiguous()
    wv = torch.from_numpy(w).to(dev).contiguous() if use_weights else None
    lut = torch.full((N, 1 << bits), float("nan"), dtype=torch.float32, device=dev)
    cost = torch.full((N,), float("nan"), dtype=torch.float64, device=dev)
    need = _lib.nuq_workspace_bytes(bits, N, K)
    ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
    if poison:  # (the conftest poisoner knows only the decode workspaces: this one is filled here)
        ws.fill_(float("nan"))
    d = _lib.SqllmNuq(bits=bits, N=N, K=K, values=xv.data_ptr(), weights=None if wv is None else wv.data_ptr(),
                      centroids=lut.data_ptr(), cost=cost.data_ptr())
    _lib.check(lib.sqllm_nuq_fit(ctypes.byref(d), ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream), "fit")
    torch.cuda.synchronize()
    return lut.cpu().numpy(), cost.cpu().numpy()


def _close(c, o, x, w):
    """Costs agree to 1e-9 relative; a cost that is rounding noise of the row's energy (an exact fit) counts as 0."""
    energy = (effective_weights(w) * x.astype(np.float64) ** 2).sum()
    return abs(c - o) <= 1e-9 * o + 1e-12 * energy


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("K", [16, 100, 256, 1024])
def test_cost_matches_the_brute_force_oracle(gpu, bits, K):
    k = 1 << bits
    rng = np.random.default_rng(K * 10 + bits)
    rows = _edge_rows(K, k, rng)
    x = np.stack([r[0] for r in rows])
    w = np.stack([r[1] for r in rows])
    lut, cost = _fit(bits, x, w)
    assert np.all(np.isfinite(lut)) and np.all(np.isfinite(cost))
    assert np.all(np.diff(lut, axis=1) >= 0)
    for r in range(x.shape[0]):
        o, ocents, _ = brute_force_fit(x[r], w[r], k)
        assert _close(cost[r], o, x[r], w[r]), (r, cost[r], o)
        # the LUT achieves that cost (nearest-centroid assignment can only do better than the ranges it came from)
        we = effective_weights(w[r])
        sse = (we * ((x[r, :, None].astype(np.float64) - lut[r][None, :].astype(np.float64)) ** 2).min(axis=1)).sum()
        assert sse <= cost[r] * (1 + 1e-5) + 1e-12 * (we * x[r].astype(np.float64) ** 2).sum(), (r, sse, cost[r])
        distinct = np.unique(x[r])
        if distinct.size <= k:  # fewer distinct values than centroids: each value is a centroid, the rest repeats
            assert set(lut[r].tolist()) == set(distinct.tolist()) and cost[r] == 0.0
    # weights = NULL is unit weights
    lut1, cost1 = _fit(bits, x[:1], w[:1], use_weights=False)
    o1, _, _ = brute_force_fit(x[0], np.ones(K), k)
    assert _close(cost1[0], o1, x[0], np.ones(K))


def test_many_rows_share_the_persistent_slots(gpu):
    """More rows than workgroups: every row is fitted, and a row's result does not depend on its neighbours."""
    rng = np.random.default_rng(7)
    N, K = 1500, 128
    x = np.sort((0.02 * rng.standard_t(3, (N, K))).astype(np.float16).astype(np.float32), axis=1)
    w = rng.lognormal(-12, 2, (N, K)).astype(np.float32)
    lut, cost = _fit(4, x, w)
    lut2, cost2 = _fit(4, x[-7:], w[-7:])
    assert np.array_equal(lut[-7:], lut2) and np.array_equal(cost[-7:], cost2)
    for r in (0, 1023, 1024, N - 1):
        o, _, _ = brute_force_fit(x[r], w[r], 16)
        assert _close(cost[r], o, x[r], w[r]), r


def test_never_worse_than_sklearn_on_the_fixture(gpu):
    from squeezellm_amd import nuq

    gm = golden_module()
    d = np.load(gm.OUT)
    for bits in (3, 4):
        ratios = {}
        for K in gm.KS:
            x, sw = gm.make_rows(gm.SEED, K)
            lut, idx, cost = nuq.fit_lut(torch.from_numpy(x).cuda(), torch.from_numpy(sw).cuda(), bits)
            sse = gm.weighted_sse(x, sw, lut.cpu().numpy())
            ratios[K] = sse / d[f"sse_w{bits}_K{K}"]
            assert np.all(sse <= d[f"sse_w{bits}_K{K}"] * (1 + 1e-6)), (bits, K, ratios[K])
        geo = float(np.exp(np.log(ratios[4096]).mean()))
        print(f"w{bits}: exact / sklearn weighted SSE, K = 4096: geometric mean {geo:.4f}, rows {np.round(ratios[4096], 4)}")
        assert geo <= 0.97, (bits, geo)


@pytest.mark.parametrize("bits", [3, 4])
def test_indices_follow_the_argmin_rule_and_outliers_sit_on_the_zero_centroid(gpu, bits):
    from squeezellm_amd import nuq, pack

    gen = torch.Generator(device="cuda").manual_seed(bits)
    N, K = 96, 256
    w = (0.02 * torch.randn(N, K, device="cuda", generator=gen)).half()
    g = torch.rand(N, K, device="cuda", generator=gen) ** 6
    lay = nuq.quantize_linear(w, g, bits, sensitivity=0.45)
    lut = lay["lookup_table"]
    idx = pack.unpack_qweight(lay["qweight"], bits).t().long()  # [N, K]
    dense, outliers = nuq.remove_outliers(w, g, 0.45)
    dist = (dense[:, :, None] - lut[:, None, :]).abs()  # fp32, as the rule is stated
    mind = dist.min(dim=2).values
    assert torch.equal(dist.gather(2, idx[:, :, None]).squeeze(2), mind)
    first = torch.where(dist == mind[:, :, None], torch.arange(1 << bits, device="cuda"), 1 << bits).min(dim=2).values
    assert torch.equal(idx, first)
    at = outliers != 0
    assert int(at.sum()) > 0
    zero_idx = lut.abs().argmin(dim=1)
    assert torch.equal(idx[at], zero_idx[:, None].expand(N, K)[at])
    # the CSR holds exactly outlier - that centroid
    _, _, vals = pack.outliers_to_csr(outliers, lut)
    assert vals.numel() == lay["vals"].numel()


@pytest.mark.parametrize("bits", [3, 4])
@pytest.mark.parametrize("sens,topX", [(0.0, 0), (0.45, 0), (0.45, 10), (0.0, 10)])
def test_quantized_linear_matches_its_dequantised_weight(gpu, bits, sens, topX):
    from squeezellm_amd import nuq
    from squeezellm_amd.quant import QuantLinearLUT

    gen = torch.Generator(device="cuda").manual_seed(100 * bits + topX)
    torch.manual_seed(100 * bits + topX)
    N, K = 384, 512
    w = (0.02 * torch.distributions.StudentT(3.0).sample((N, K)).cuda()).half()
    g = torch.rand(N, K, device="cuda", generator=gen) ** 8
    bias = torch.randn(N, device="cuda", generator=gen) * 0.01
    lay = nuq.quantize_linear(w, g, bits, sensitivity=sens, topX=topX, bias=bias)
    mod = QuantLinearLUT.from_operands(lay)
    dense, outliers = nuq.remove_outliers(w, g, sens)
    _, idx, _ = nuq.fit_lut(dense, g, bits)
    # LUT[idx] + the CSR, which holds outlier - (centroid nearest 0) where the dense part holds that centroid: at an
    # outlier position the layer's weight is the outlier itself
    wdq = torch.where(outliers != 0, outliers, lay["lookup_table"].gather(1, idx.long()))  # [N, K]
    if sens:
        assert lay["vals"] is not None and (topX == 0 or lay["full_rows"] is not None)
    x = torch.randn(3, 1, K, device="cuda", generator=gen).half()
    y = mod(x)
    torch.cuda.synchronize()
    ref = x.double() @ wdq.double().t() + bias.double()
    err = float((y.double() - ref).abs().max() / ref.abs().max())
    assert y.shape == (3, 1, N) and err <= 2e-3, (bits, sens, topX, err)
    # and the dequantised weight is a fit of w (the LUT spans the row)
    assert float((wdq - w.float()).abs().max()) <= float(w.float().abs().max())


def test_quantize_state_dict_round_trips_through_the_checkpoint(gpu, tmp_path):
    from squeezellm_amd import checkpoint, nuq

    torch.manual_seed(0)
    H, I = 128, 320
    shapes = {"self_attn.q_proj": (H, H), "self_attn.k_proj": (H, H), "self_attn.v_proj": (H, H), "self_attn.o_proj": (H, H),
              "mlp.gate_proj": (I, H), "mlp.up_proj": (I, H), "mlp.down_proj": (H, I)}
    model_sd = {"model.embed_tokens.weight": torch.randn(64, H).half(), "model.norm.weight": torch.ones(H).half(),
                "lm_head.weight": torch.randn(64, H).half()}
    grad_sd = {}
    for l in range(2):
        model_sd[f"model.layers.{l}.input_layernorm.weight"] = torch.ones(H).half()
        for n, s in shapes.items():
            model_sd[f"model.layers.{l}.{n}.weight"] = (0.02 * torch.distributions.StudentT(3.0).sample(s)).half()
            grad_sd[f"model.layers.{l}.{n}.weight"] = torch.rand(s) ** 6
    cfg = {"outlier_threshold": 0.1,
           "outlier_config": [{"q": 0.08, "k": 0.08, "v": 0.09, "o": 0.1, "gate": 0.07, "up": 0.07, "down": 0.1}] * 2}
    sd = nuq.quantize_state_dict(model_sd, grad_sd, 3, sensitivity=0.45, outlier_config=cfg, topX=4)
    path = tmp_path / "sq.pt"
    torch.save(sd, path)
    for key in ("model.embed_tokens.weight", "model.norm.weight", "lm_head.weight", "model.layers.1.input_layernorm.weight"):
        assert torch.equal(sd[key], model_sd[key])
    assert not any(k.endswith("_proj.weight") for k in sd)
    layers = checkpoint.load_layers(str(path), device="cuda")
    assert len(layers) == 14 and list(layers)[:2] == ["model.layers.0.self_attn.q_proj", "model.layers.0.self_attn.k_proj"]
    name = "model.layers.1.mlp.down_proj"
    direct = nuq.quantize_linear(model_sd[f"{name}.weight"].cuda(), grad_sd[f"{name}.weight"].cuda(), 3, sensitivity=0.45,
                                 threshold=0.1)
    got = layers[name]
    assert (got["K"], got["N"], got["bits"]) == (I, H, 3)
    for f in ("qweight", "lookup_table", "rows", "cols", "vals"):
        assert torch.equal(got[f], direct[f]), f
    # the command line writes the same checkpoint
    torch.save(model_sd, tmp_path / "m.pt")
    torch.save(grad_sd, tmp_path / "g.pt")
    (tmp_path / "cfg.json").write_text(json.dumps(cfg))
    assert nuq.main(["--model", str(tmp_path / "m.pt"), "--gradient", str(tmp_path / "g.pt"), "--bits", "3", "--out",
                     str(tmp_path / "cli.pt"), "--sensitivity", "0.45", "--outlier-config", str(tmp_path / "cfg.json"),
                     "--topx", "4"]) == 0
    cli = torch.load(tmp_path / "cli.pt")
    assert sorted(cli) == sorted(sd) and all(torch.equal(cli[k], sd[k]) if isinstance(sd[k], torch.Tensor) else cli[k] == sd[k] for k in sd)


def test_fit_lut_rejects_non_finite_input(gpu):
    from squeezellm_amd import nuq

    w = torch.zeros(4, 64, device="cuda")
    w[1, 3] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        nuq.fit_lut(w, None, 4)
    g = torch.ones(4, 64, device="cuda")
    g[0, 0] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        nuq.fit_lut(torch.zeros(4, 64, device="cuda"), g, 3)
