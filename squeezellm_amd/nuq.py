"""Making a SqueezeLLM checkpoint on the GPU: outlier extraction, optimal Fisher-weighted lookup tables, packing.

The reference's route is quantization/nuq.py (one sklearn KMeans per output channel on the CPU: Lloyd from a k-means++
start, a local optimum) followed by quantization/pack.py.  Here the codebooks are the EXACT optimum of the same
objective, sum over a row of g * (w - c)^2 with g the Fisher diagonal, computed per row by the HIP kernel behind
sqllm_nuq_fit (csrc/sqllm_nuq.hip); torch does the plumbing around it (sorting, the outlier mask), sqllm_encode
(csrc/sqllm_encode.hip, through pack.encode_layer) turns weight + codebooks + mask into the packed operands, and
squeezellm_amd.checkpoint writes the checkpoint.

    python -m squeezellm_amd.nuq --model sd.pt --gradient g.pt --bits 4 --out sq.pt \\
        [--sensitivity 0.05] [--outlier-config cfg.json] [--topx 0]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import re
import sys

import torch

from . import _lib, checkpoint, pack

# short module names of the reference's outlier configs (squeezellm/model_parse.py get_module_names) by linear name
_SHORT = {"q_proj": "q", "k_proj": "k", "v_proj": "v", "o_proj": "o", "out_proj": "o", "gate_proj": "gate",
          "up_proj": "up", "fc1": "up", "down_proj": "down", "fc2": "down"}
WORKSPACE_BUDGET = 1 << 30  # bytes of kernel workspace one chunk of rows may use


def _outlier_masks(w: torch.Tensor, gradient: torch.Tensor | None, sensitivity: float, threshold: float | None):
    """The two boolean masks remove_outliers applies one after the other (None: that step does nothing): the
    sensitivity outliers, then the threshold outliers of what the first step left."""
    t = t2 = None
    if sensitivity:
        if gradient is None:
            raise ValueError("sensitivity-based outliers need the gradient")
        g = gradient.to(torch.float32)
        num = int(g.numel() * sensitivity / 100)
        if num > 0:
            thres = g.reshape(-1).topk(k=num).values[-1]
            t = g > thres
    if threshold is not None:
        left = w if t is None else w * ~t
        t2 = torch.logical_or(left >= threshold, left <= -threshold)
    return t, t2


def outlier_mask(weight: torch.Tensor, gradient: torch.Tensor | None = None, sensitivity: float = 0.0,
                 threshold: float | None = None) -> torch.Tensor:
    """The boolean mask [N, K] of the positions remove_outliers takes out of the dense part (True = outlier candidate;
    a candidate whose weight is 0 leaves no outlier behind) -- what pack.encode_layer takes as `mask`."""
    w = weight.to(torch.float32)
    t, t2 = _outlier_masks(w, gradient, sensitivity, threshold)
    if t is None and t2 is None:
        return torch.zeros(w.shape, dtype=torch.bool, device=w.device)
    if t is None or t2 is None:
        return t if t2 is None else t2
    return torch.logical_or(t, t2)


def remove_outliers(weight: torch.Tensor, gradient: torch.Tensor | None = None, sensitivity: float = 0.0,
                    threshold: float | None = None):
    """Split a weight into (dense, outliers), both fp32 of its shape, as squeezellm/outliers.py does for one module:
    first the `sensitivity` percent of entries with the largest gradient (the threshold is the num-th largest gradient
    and only entries STRICTLY above it go: outliers.py:15-18), then, on what is left, every entry with
    w >= threshold or w <= -threshold (outliers.py:51-54); the second set adds to the first.  num == 0 means no
    sensitivity outliers (the reference would fail there).  outlier_mask returns the positions alone."""
    w = weight.to(torch.float32)
    outliers = torch.zeros_like(w)
    t, t2 = _outlier_masks(w, gradient, sensitivity, threshold)
    if t is not None:
        outliers = w * t
        w = w * ~t
    if t2 is not None:
        outliers = outliers + w * t2
        w = w * ~t2
    return w, outliers


def _check_finite(name, t):
    if t is not None and not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} holds non-finite values")


def fit_lut(weight: torch.Tensor, gradient: torch.Tensor | None = None, bits: int = 4):
    """Per-row optimal lookup tables of a weight [N, K] (a CUDA tensor): returns (lookup_table fp32 [N, 2**bits]
    ascending, idx uint8 [N, K], cost fp64 [N]).  The sample weights are gradient * (weight != 0) (nuq.py:172-173),
    ones without a gradient; a row whose weights sum to 0 is fitted with unit weights.  idx is the first j that
    minimises |w - lut_j| in fp32 -- the rule pack.outliers_to_csr uses to find the zero-nearest centroid."""
    lut, cost, w = _fit_codebooks(weight, gradient, bits)
    return lut, assign_indices(w, lut), cost


def _fit_codebooks(weight: torch.Tensor, gradient: torch.Tensor | None, bits: int):
    """fit_lut without the index matrix: (lookup_table, cost, the weight as contiguous fp32)."""
    if bits not in (3, 4):
        raise ValueError("bits must be 3 or 4")
    if weight.dim() != 2 or not weight.is_cuda:
        raise ValueError("fit_lut takes a 2-D CUDA tensor (there is no CPU path)")
    w = weight.to(torch.float32).contiguous()
    _check_finite("weight", w)
    if gradient is not None:
        if gradient.shape != weight.shape:
            raise ValueError(f"gradient {tuple(gradient.shape)} does not match weight {tuple(weight.shape)}")
        g = gradient.to(device=w.device, dtype=torch.float32)
        _check_finite("gradient", g)
        if bool((g < 0).any()):
            raise ValueError("gradient (a Fisher diagonal) must be non-negative")
        sw = (g * (w != 0)).contiguous()
    else:
        sw = None
    N, K = w.shape
    k = 1 << bits
    lib = _lib.load()
    lut = torch.empty((N, k), dtype=torch.float32, device=w.device)
    cost = torch.empty(N, dtype=torch.float64, device=w.device)
    per_slot = _lib.nuq_workspace_bytes(bits, 1, K)
    chunk = max(1, min(N, 8192, WORKSPACE_BUDGET // per_slot))
    ws = torch.empty(_lib.nuq_workspace_bytes(bits, chunk, K), dtype=torch.uint8, device=w.device)
    stream = torch.cuda.current_stream(w.device).cuda_stream
    with torch.cuda.device(w.device):
        for r0 in range(0, N, chunk):
            r1 = min(N, r0 + chunk)
            vals, order = torch.sort(w[r0:r1], dim=1)
            wts = None if sw is None else torch.gather(sw[r0:r1], 1, order).contiguous()
            vals = vals.contiguous()
            d = _lib.SqllmNuq(bits=bits, N=r1 - r0, K=K, values=vals.data_ptr(),
                              weights=None if wts is None else wts.data_ptr(),
                              centroids=lut[r0:r1].data_ptr(), cost=cost[r0:r1].data_ptr())
            _lib.check(lib.sqllm_nuq_fit(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream), "sqllm_nuq_fit")
            del vals, wts, order  # (the caching allocator keeps them stream-ordered)
    return lut, cost, w


def assign_indices(weight: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    """uint8 [N, K]: the first j minimising |w - lut[n, j]| in fp32 (strict < over ascending j)."""
    w = weight.to(torch.float32)
    best = (w - lut[:, :1]).abs()
    idx = torch.zeros(w.shape, dtype=torch.uint8, device=w.device)
    for j in range(1, lut.shape[1]):
        d = (w - lut[:, j:j + 1]).abs()
        upd = d < best
        best = torch.where(upd, d, best)
        idx = torch.where(upd, j, idx)
    return idx


def quantize_linear(weight: torch.Tensor, gradient: torch.Tensor | None, bits: int, sensitivity: float = 0.0,
                    threshold: float | None = None, topX: int = 0, bias: torch.Tensor | None = None) -> dict:
    """One linear's weight [N, K] (and Fisher diagonal of the same shape) -> the operand dict of pack.pack_layer, which
    quant.QuantLinearLUT.from_operands, squeezellm_amd.decode and checkpoint.to_state_dict take as-is.  With
    sensitivity > 0 or a threshold the outliers go into the CSR (dense-and-sparse), topX of its densest rows into
    full_rows; the dense part is fitted with the outliers zeroed, as nuq.py does."""
    dev = weight.device
    g = None if gradient is None else gradient.to(dev)
    sparse = bool(sensitivity) or threshold is not None
    mask = outlier_mask(weight, g, sensitivity, threshold) if sparse else None
    dense = weight.to(torch.float32)
    if mask is not None:
        dense = dense * ~mask
    lut, _, dense = _fit_codebooks(dense, g, bits)  # (rejects non-finite weights)
    b32 = None if bias is None else bias.to(device=dev, dtype=torch.float32)
    if weight.shape[0] % 4:  # not a shape the kernels take (N % 4 == 0): the torch packer still writes its buffers
        return pack.pack_layer(assign_indices(dense, lut), lut, bits, weight.to(torch.float32) * mask if sparse else None,
                               topX=topX if sparse else 0, bias=b32)
    del dense
    # fit, then encode on the GPU: neither the uint8 index matrix nor the dense outlier matrix is built
    return pack.encode_layer(weight, lut, bits, mask, topX=topX if sparse else 0, bias=b32, check_finite=False)


def reconstruction_error(weight: torch.Tensor, gradient: torch.Tensor | None, layer: dict) -> dict:
    """How far a packed layer is from the weight [N, K] it was made from: the FINAL dense-and-sparse layer is decoded on
    the GPU (decode.dequantize_layer, fp32: codebook entry + CSR + top-X columns) and compared in fp64 there.
    Returns {"sse": sum (W - W_hat)^2, "weighted_sse": sum g (W - W_hat)^2 with the Fisher diagonal `gradient` as
    weights (None: ones), "max_abs": max |W - W_hat|} as Python floats."""
    from . import decode

    w_hat = decode.dequantize_layer(layer, dtype=torch.float32)
    dev = w_hat.device
    if tuple(weight.shape) != tuple(w_hat.shape):
        raise ValueError(f"weight is {tuple(weight.shape)}, the layer decodes to {tuple(w_hat.shape)}")
    diff = weight.to(device=dev, dtype=torch.float64) - w_hat.to(torch.float64)
    sq = diff * diff
    wsse = sq.sum() if gradient is None else (sq * gradient.to(device=dev, dtype=torch.float64)).sum()
    return {"sse": float(sq.sum()), "weighted_sse": float(wsse), "max_abs": float(diff.abs().max())}


def _short_name(name: str) -> str:
    return _SHORT.get(name.rsplit(".", 1)[-1], name.rsplit(".", 1)[-1])


def _layer_index(name: str) -> int | None:
    m = re.search(r"layers\.(\d+)\.", name)
    return int(m.group(1)) if m else None


def default_names(model_sd) -> list[str]:
    """The linears nuq.py quantises: every 2-D `<name>.weight` whose module is one of q/k/v/o/gate/up/down (LLaMA) or
    q/k/v/out_proj/fc1/fc2 (OPT) inside a decoder layer."""
    out = []
    for key, t in model_sd.items():
        if key.endswith(".weight") and getattr(t, "dim", lambda: 0)() == 2:
            name = key[: -len(".weight")]
            if name.rsplit(".", 1)[-1] in _SHORT and _layer_index(name) is not None:
                out.append(name)
    return out


def quantize_state_dict(model_sd: dict, grad_sd: dict, bits: int, names=None, sensitivity: float = 0.0,
                        outlier_config: dict | None = None, topX: int = 0, device=None, report: bool = False) -> dict:
    """A model's state dict + its Fisher diagonal (same keys, or the keys without `.weight`) -> a flat checkpoint in the
    reference's format (checkpoint.to_state_dict).  Every linear of `names` (default: default_names) is quantised;
    everything else is copied through.  `outlier_config` is the JSON generate_outlier_config.py writes:
    {"outlier_threshold": ..., "outlier_config": [{short module name: threshold} per decoder layer]}.
    report=True prints every layer's reconstruction_error (one line per layer, stderr)."""
    device = torch.device(device or "cuda")
    names = list(names) if names is not None else default_names(model_sd)
    per_layer = None if outlier_config is None else outlier_config["outlier_config"]
    layers = {}
    for name in names:
        weight = model_sd[f"{name}.weight"]
        grad = grad_sd.get(f"{name}.weight", grad_sd.get(name))
        if grad is None:
            raise KeyError(f"{name}: no gradient")
        thres = None
        if per_layer is not None:
            li = _layer_index(name)
            if li is None or li >= len(per_layer) or _short_name(name) not in per_layer[li]:
                raise KeyError(f"{name}: not in the outlier config")
            thres = float(per_layer[li][_short_name(name)])
        lay = quantize_linear(weight.to(device), grad.to(device), bits, sensitivity=sensitivity, threshold=thres,
                              topX=topX, bias=model_sd.get(f"{name}.bias"))
        layers[name] = lay
        if report:
            err = reconstruction_error(weight.to(device), grad.to(device), lay)
            print(f"{name}: sse {err['sse']:.6e}  weighted_sse {err['weighted_sse']:.6e}  max_abs {err['max_abs']:.6e}", file=sys.stderr)
    done = {f"{n}.weight" for n in names} | {f"{n}.bias" for n in names}
    extra = {k: v for k, v in model_sd.items() if k not in done}
    return checkpoint.to_state_dict(layers, extra)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m squeezellm_amd.nuq", description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", required=True, help="torch.save'd state dict of the fp16 model")
    ap.add_argument("--gradient", required=True, help="torch.save'd state dict of its Fisher diagonal (squared gradients)")
    ap.add_argument("--bits", type=int, choices=(3, 4), required=True)
    ap.add_argument("--out", required=True, help="checkpoint to write (sq-*.pt format)")
    ap.add_argument("--sensitivity", type=float, default=0.0, help="percent of weights kept as sensitivity outliers")
    ap.add_argument("--outlier-config", default=None, help="JSON from generate_outlier_config.py")
    ap.add_argument("--topx", type=int, default=0, help="densest outlier rows held dense (full_rows)")
    ap.add_argument("--report", action="store_true", help="print every layer's reconstruction error (plain and Fisher-weighted)")
    a = ap.parse_args(argv)
    cfg = None
    if a.outlier_config:
        with open(a.outlier_config) as f:
            cfg = json.load(f)
    model_sd = torch.load(a.model, map_location="cpu")
    grad_sd = torch.load(a.gradient, map_location="cpu")
    sd = quantize_state_dict(model_sd, grad_sd, a.bits, sensitivity=a.sensitivity, outlier_config=cfg, topX=a.topx, report=a.report)
    torch.save(sd, a.out)
    print(f"wrote {a.out}: {len(checkpoint.quantized_names(sd))} quantised linears, {a.bits}-bit", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
