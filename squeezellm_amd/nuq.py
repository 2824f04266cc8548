"""Making a SqueezeLLM checkpoint on the GPU: outlier extraction, optimal Fisher-weighted lookup tables, packing.

The reference's route is quantization/nuq.py (one sklearn KMeans per output channel on the CPU: Lloyd from a k-means++
start, a local optimum) followed by quantization/pack.py.  Here the codebooks are the EXACT optimum of the same
objective, sum over a row of g * (w - c)^2 with g the Fisher diagonal, computed per row by the HIP kernel behind
sqllm_nuq_fit (csrc/sqllm_nuq.hip); which weights are outliers is decided on the GPU too (csrc/sqllm_select.hip: the
quartiles of a whole matrix and the num-th largest gradient are exact order statistics found by sqllm_select, the mask is
written by sqllm_outlier_mask -- the reference's quantization/generate_outlier_config.py is not needed); torch does the
plumbing around them (sorting the rows for the fit), sqllm_encode (csrc/sqllm_encode.hip, through pack.encode_layer)
turns weight + codebooks + mask into the packed operands, and squeezellm_amd.checkpoint writes the checkpoint.

    python -m squeezellm_amd.nuq --model sd.pt --gradient g.pt --bits 4 --out sq.pt \\
        [--sensitivity 0.05] [--range 1.8 | --outlier-config cfg.json] [--write-outlier-config cfg.json] [--topx 0]
    python -m squeezellm_amd.nuq --model sd.pt --range 1.8 --write-outlier-config cfg.json      # the config alone
"""
from __future__ import annotations

import argparse
import ctypes
import json
import math
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
    a candidate whose weight is 0 leaves no outlier behind) -- what pack.encode_layer takes as `mask`.  CUDA tensors of
    shapes sqllm_outlier_mask takes (2-D, K % 32 == 0, fp16 / fp32) go through that kernel, with the sensitivity cut from
    sensitivity_threshold; everything else through torch (_outlier_masks, the specification).  The same mask either way."""
    if _mask_kernel_takes(weight, gradient if sensitivity else None):
        if sensitivity and gradient is None:
            raise ValueError("sensitivity-based outliers need the gradient")
        g_thres = sensitivity_threshold(gradient, sensitivity) if sensitivity else None
        # (the comparison of an fp32 tensor with a Python float is made in fp32: the float is rounded first)
        w_thres = None if threshold is None else torch.tensor(float(threshold), dtype=torch.float32, device=weight.device)
        return _mask_kernel(weight, gradient if g_thres is not None else None, g_thres, w_thres, want_mask=True)[0]
    w = weight.to(torch.float32)
    t, t2 = _outlier_masks(w, gradient, sensitivity, threshold)
    if t is None and t2 is None:
        return torch.zeros(w.shape, dtype=torch.bool, device=w.device)
    if t is None or t2 is None:
        return t if t2 is None else t2
    return torch.logical_or(t, t2)


def _kernel_dtype(t: torch.Tensor) -> int | None:
    return {torch.float16: _lib.DTYPE_F16, torch.float32: _lib.DTYPE_F32}.get(t.dtype)


def _as_kernel_dtype(w: torch.Tensor) -> torch.Tensor:
    """w itself if it is fp16 / fp32, else widened to fp32 (bf16 and the like: exactly)."""
    return w if _kernel_dtype(w) is not None else w.to(torch.float32)


def _mask_kernel_takes(weight: torch.Tensor, gradient: torch.Tensor | None) -> bool:
    for t in (weight, gradient):
        if t is None:
            continue
        if not t.is_cuda or t.dim() != 2 or _kernel_dtype(t) is None or t.shape != weight.shape or t.device != weight.device:
            return False
    return weight.shape[0] >= 1 and weight.shape[1] >= 32 and weight.shape[1] % 32 == 0


def _rows_in_place(t: torch.Tensor) -> torch.Tensor:
    """t itself where the kernels can read its rows in place (unit stride along K, a row stride that is a multiple of a
    16-byte vector, a 16-byte aligned start), else a contiguous copy."""
    m = 16 // t.element_size()
    if t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.stride(0) % m == 0 and t.data_ptr() % 16 == 0:
        return t
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _mask_kernel(weight, gradient, g_thres, w_thres, want_mask: bool, want_count: bool = False):
    """sqllm_outlier_mask on 2-D CUDA tensors: (bool mask [N, K] or None, int64 count [1] on the device or None)."""
    N, K = weight.shape
    w = _rows_in_place(weight)
    g = None if gradient is None else _rows_in_place(gradient)
    mask = torch.empty((N, K), dtype=torch.bool, device=w.device) if want_mask else None
    count = torch.empty(1, dtype=torch.int64, device=w.device) if want_count else None
    d = _lib.SqllmOutlier(weight_dtype=_kernel_dtype(w), grad_dtype=0 if g is None else _kernel_dtype(g), K=K, N=N,
                          weight=w.data_ptr(), ld_w=w.stride(0), gradient=None if g is None else g.data_ptr(),
                          ld_g=0 if g is None else g.stride(0), g_threshold=None if g is None else g_thres.data_ptr(),
                          w_threshold=None if w_thres is None else w_thres.data_ptr(),
                          mask=None if mask is None else mask.data_ptr(), count=None if count is None else count.data_ptr())
    with torch.cuda.device(w.device):
        stream = torch.cuda.current_stream(w.device).cuda_stream
        _lib.check(_lib.load().sqllm_outlier_mask(ctypes.byref(d), stream), "sqllm_outlier_mask")
    return mask, count


def order_statistics(t: torch.Tensor, ranks):
    """Exact order statistics of ALL elements of a contiguous CUDA fp16 / fp32 tensor (seen as [numel / last_dim,
    last_dim]): (values fp32 [len(ranks)], less int64 [len(ranks)]) on the device, values[i] the element at 0-based
    position ranks[i] of the ascending order (as a value: -0.0 is +0.0) and less[i] the number of elements strictly
    below it.  sqllm_select (a radix select: no sort), eight ranks per call.  There is no CPU path."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("order_statistics takes a CUDA tensor (there is no CPU path)")
    dt = _kernel_dtype(t)
    if dt is None or t.dim() < 1 or t.numel() == 0 or not t.is_contiguous():
        raise ValueError("order_statistics takes a contiguous, non-empty fp16 or fp32 tensor")
    cols = t.shape[-1]
    rows = t.numel() // cols
    if cols % (16 // t.element_size()):
        raise ValueError(f"order_statistics: the last dimension ({cols}) must be a multiple of {16 // t.element_size()}")
    ranks = [int(r) for r in ranks]
    if any(r < 0 or r >= t.numel() for r in ranks):
        raise ValueError("order_statistics: a rank outside [0, numel)")
    if t.data_ptr() % 16:
        t = t.clone()
    out = torch.empty(len(ranks), dtype=torch.float32, device=t.device)
    less = torch.empty(len(ranks), dtype=torch.int64, device=t.device)
    lib = _lib.load()
    with torch.cuda.device(t.device):
        stream = torch.cuda.current_stream(t.device).cuda_stream
        ws = None
        for i0 in range(0, len(ranks), _lib.SELECT_MAX_RANKS):
            part = ranks[i0:i0 + _lib.SELECT_MAX_RANKS]
            d = _lib.SqllmSelect(dtype=dt, n_ranks=len(part), values=t.data_ptr(), rows=rows, cols=cols, ld=cols,
                                 out=out[i0:].data_ptr(), less=less[i0:].data_ptr())
            for j, r in enumerate(part):
                d.ranks[j] = r
            need = _lib.select_workspace_bytes(dt, len(part), rows, cols)
            if ws is None or ws.numel() < need:
                ws = torch.empty(need, dtype=torch.uint8, device=t.device)
            _lib.check(lib.sqllm_select(ctypes.byref(d), ws.data_ptr(), ws.numel(), stream), "sqllm_select")
    return out, less


def quantile_ranks(n: int, q: float):
    """numpy's default ("linear") quantile of n sorted values as two order statistics: (lo, hi, g) with
    pos = q (n - 1), lo = floor(pos), hi = min(lo + 1, n - 1), g = pos - lo; the quantile is x_lo + (x_hi - x_lo) g."""
    if n < 1 or not 0.0 <= q <= 1.0:
        raise ValueError("quantile_ranks: n >= 1 and 0 <= q <= 1")
    pos = q * (n - 1)
    lo = min(int(math.floor(pos)), n - 1)
    return lo, min(lo + 1, n - 1), pos - lo


def quantiles(t: torch.Tensor, qs) -> list[float]:
    """np.quantile(t, q) (method "linear") for every q of qs, over all elements of a CUDA tensor of any size: the two
    exact order statistics either side of each position from order_statistics, interpolated in fp64 on the host."""
    pos = [quantile_ranks(t.numel(), float(q)) for q in qs]
    vals, _ = order_statistics(t, [r for lo, hi, _ in pos for r in (lo, hi)])
    v = vals.to(torch.float64).cpu().tolist()
    return [v[2 * i] + (v[2 * i + 1] - v[2 * i]) * g for i, (_, _, g) in enumerate(pos)]


def outlier_threshold(weight: torch.Tensor, range_: float) -> float:
    """The reference's threshold of one linear (quantization/generate_outlier_config.py:47-53): with the quartiles q1, q3
    of all its weights, T = max(|q1 - r (q3 - q1)|, |q3 + r (q3 - q1)|), in fp64.  Weights with |w| >= T are outliers."""
    _check_finite("weight", weight)
    q1, q3 = quantiles(weight.contiguous(), (0.25, 0.75))
    return max(abs(q1 - range_ * (q3 - q1)), abs(q3 + range_ * (q3 - q1)))


def sensitivity_threshold(gradient: torch.Tensor, sensitivity: float):
    """The cut of the sensitivity step as a 0-dim fp32 device tensor: the num-th largest gradient, num = int(n *
    sensitivity / 100) -- the order statistic at rank n - num, bit for bit what gradient.reshape(-1).topk(num).values[-1]
    gives, found without the partial sort.  None for num == 0 (no sensitivity outliers, as _outlier_masks has it).
    A non-finite gradient raises ValueError (the select leaves NaN input unspecified)."""
    n = gradient.numel()
    num = int(n * sensitivity / 100)
    if num <= 0:
        return None
    _check_finite("gradient", gradient)
    return order_statistics(gradient.contiguous(), [n - num])[0][0]


def outlier_config(model_sd: dict, range_: float, names=None, device=None) -> dict:
    """The JSON generate_outlier_config.py writes, from a state dict, on the GPU: {"outlier_threshold": round(pct, 2),
    "outlier_config": [{short module name: T} per decoder layer]} with T = outlier_threshold(weight, range_) as a Python
    float, for every linear of `names` (default: default_names; LLaMA and OPT module names).  pct is the share of all
    those weights that the removal takes, |w| >= T (sqllm_outlier_mask, count only); the reference's printout counts
    |w| > T instead: the two differ only where a weight equals T exactly."""
    device = torch.device(device or "cuda")
    names = list(names) if names is not None else default_names(model_sd)
    layers: dict[int, dict] = {}
    total = 0
    count = torch.zeros(1, dtype=torch.int64, device=device)
    for name in names:
        li = _layer_index(name)
        if li is None:
            raise KeyError(f"{name}: not inside a decoder layer")
        w = _as_kernel_dtype(model_sd[f"{name}.weight"].to(device))
        T = outlier_threshold(w, range_)
        layers.setdefault(li, {})[_short_name(name)] = T
        total += w.numel()
        if _mask_kernel_takes(w, None):
            count += _mask_kernel(w, None, None, torch.tensor(T, dtype=torch.float32, device=device), want_mask=False, want_count=True)[1]
        else:
            count += outlier_mask(w, threshold=T).sum()
    pct = int(count.item()) / total * 100 if total else 0.0
    return {"outlier_threshold": round(pct, 2), "outlier_config": [layers.get(i, {}) for i in range(max(layers, default=-1) + 1)]}


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
                        outlier_config: dict | None = None, topX: int = 0, device=None, report: bool = False,
                        outlier_range: float | None = None) -> dict:
    """A model's state dict + its Fisher diagonal (same keys, or the keys without `.weight`) -> a flat checkpoint in the
    reference's format (checkpoint.to_state_dict).  Every linear of `names` (default: default_names) is quantised;
    everything else is copied through.  `outlier_config` is the JSON generate_outlier_config.py writes:
    {"outlier_threshold": ..., "outlier_config": [{short module name: threshold} per decoder layer]}; `outlier_range`
    instead computes every linear's threshold on the fly (outlier_threshold: the same numbers outlier_config writes);
    giving both raises ValueError.
    report=True prints every layer's reconstruction_error (one line per layer, stderr)."""
    if outlier_range is not None and outlier_config is not None:
        raise ValueError("outlier_range and outlier_config are mutually exclusive")
    device = torch.device(device or "cuda")
    names = list(names) if names is not None else default_names(model_sd)
    per_layer = None if outlier_config is None else outlier_config["outlier_config"]
    layers = {}
    for name in names:
        grad = grad_sd.get(f"{name}.weight", grad_sd.get(name))
        if grad is None:
            raise KeyError(f"{name}: no gradient")
        weight, grad = model_sd[f"{name}.weight"].to(device), grad.to(device)  # one upload each, shared by every step below
        thres = None
        if per_layer is not None:
            li = _layer_index(name)
            if li is None or li >= len(per_layer) or _short_name(name) not in per_layer[li]:
                raise KeyError(f"{name}: not in the outlier config")
            thres = float(per_layer[li][_short_name(name)])
        elif outlier_range is not None:
            thres = outlier_threshold(_as_kernel_dtype(weight), outlier_range)
        lay = quantize_linear(weight, grad, bits, sensitivity=sensitivity, threshold=thres,
                              topX=topX, bias=model_sd.get(f"{name}.bias"))
        layers[name] = lay
        if report:
            err = reconstruction_error(weight, grad, lay)
            print(f"{name}: sse {err['sse']:.6e}  weighted_sse {err['weighted_sse']:.6e}  max_abs {err['max_abs']:.6e}", file=sys.stderr)
    done = {f"{n}.weight" for n in names} | {f"{n}.bias" for n in names}
    extra = {k: v for k, v in model_sd.items() if k not in done}
    return checkpoint.to_state_dict(layers, extra)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m squeezellm_amd.nuq", description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", required=True, help="torch.save'd state dict of the fp16 model")
    ap.add_argument("--gradient", default=None, help="torch.save'd state dict of its Fisher diagonal (squared gradients)")
    ap.add_argument("--bits", type=int, choices=(3, 4), default=None)
    ap.add_argument("--out", default=None, help="checkpoint to write (sq-*.pt format)")
    ap.add_argument("--sensitivity", type=float, default=0.0, help="percent of weights kept as sensitivity outliers")
    ap.add_argument("--outlier-config", default=None, help="JSON of per-linear thresholds (generate_outlier_config.py's format)")
    ap.add_argument("--range", type=float, default=None, dest="range_",
                    help="threshold outliers by interquartile range, e.g. 1.8: every linear's threshold is computed on the fly")
    ap.add_argument("--write-outlier-config", default=None, help="with --range: write the thresholds as that JSON")
    ap.add_argument("--topx", type=int, default=0, help="densest outlier rows held dense (full_rows)")
    ap.add_argument("--report", action="store_true", help="print every layer's reconstruction error (plain and Fisher-weighted)")
    a = ap.parse_args(argv)
    if a.range_ is not None and a.outlier_config:
        ap.error("--range and --outlier-config are mutually exclusive")
    if a.write_outlier_config and a.range_ is None:
        ap.error("--write-outlier-config needs --range")
    config_only = bool(a.write_outlier_config) and a.gradient is None and a.bits is None and a.out is None
    if not config_only and (a.gradient is None or a.bits is None or a.out is None):
        ap.error("--gradient, --bits and --out are required (only --range with --write-outlier-config does without them)")
    cfg = None
    if a.outlier_config:
        with open(a.outlier_config) as f:
            cfg = json.load(f)
    model_sd = torch.load(a.model, map_location="cpu")
    if a.write_outlier_config:
        cfg = outlier_config(model_sd, a.range_)
        with open(a.write_outlier_config, "w") as f:
            json.dump(cfg, f, indent=4)
        print(f"wrote {a.write_outlier_config}: {cfg['outlier_threshold']} % outliers at range {a.range_}", file=sys.stderr)
        if config_only:
            return 0
    grad_sd = torch.load(a.gradient, map_location="cpu")
    sd = quantize_state_dict(model_sd, grad_sd, a.bits, sensitivity=a.sensitivity, outlier_config=cfg, topX=a.topx, report=a.report,
                             outlier_range=a.range_ if cfg is None else None)
    torch.save(sd, a.out)
    print(f"wrote {a.out}: {len(checkpoint.quantized_names(sd))} quantised linears, {a.bits}-bit", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
