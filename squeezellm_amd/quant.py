"""QuantLinearLUT for MI355X -- host-side mirror of the reference layer
(/root/reference/squeezellm/quant.py:28-383): same constructor signature, same buffer names /
shapes / dtypes (so reference checkpoints load with `load_state_dict`), same choice of operator
per configuration and the same pre/post-processing around it.  The reference's own quant.py also
runs unchanged on top of the top-level `quant_cuda` shim; this module exists so
that the path can be exercised where the reference tree is absent, and to host the MI355X-only
conveniences (`from_operands`, `operands`).

Packing (`pack2`, quant.py:97-208) is offline tooling and out of scope here; see oracle/ for the
format restatement used by the tests.
"""
from __future__ import annotations

import ctypes
import math
import operator

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, quant_cuda


class QuantLinearLUT(nn.Module):
    """Drop-in for the reference class of the same name (quant.py:28-95 buffers, :211-383 forward)."""

    def __init__(self, bits, infeatures, outfeatures, bias, include_sparse=False, numvals=0, topX=0,
                 balanced=False, num_nonzero_per_thread=10):
        super().__init__()
        if bits not in (3, 4):
            raise NotImplementedError("Only 3 and 4 bits is supported.")  # quant.py:42-43
        self.bits, self.infeatures, self.outfeatures = bits, infeatures, outfeatures
        self.include_sparse, self.numvals, self.topX, self.balanced = include_sparse, numvals, topX, balanced
        i32, f32 = torch.int32, torch.float32
        self.register_buffer("qweight", torch.zeros((infeatures // 32 * bits, outfeatures), dtype=i32))
        self.include_bias = bool(bias)
        if self.include_bias:
            self.register_buffer("bias", torch.zeros(outfeatures, dtype=f32))
        else:
            self.bias = None
        self.register_buffer("lookup_table", torch.zeros((outfeatures, 2**bits), dtype=f32))
        if numvals > 0:  # quant.py:66-71
            self.register_buffer("rows", torch.zeros(outfeatures + 1, dtype=i32))
            self.register_buffer("cols", torch.zeros(numvals, dtype=i32))
            self.register_buffer("vals", torch.zeros(numvals, dtype=f32))
        if topX > 0:  # quant.py:74-80
            self.register_buffer("full_rows", torch.zeros((infeatures, topX), dtype=f32))
            self.register_buffer("full_row_indices", torch.zeros(topX, dtype=i32))
        if include_sparse and balanced and numvals > 0:  # quant.py:84-95
            nt = int((numvals + num_nonzero_per_thread - 1) / num_nonzero_per_thread)
            self.num_threads = 128 * math.ceil(nt / 128)
            self.register_buffer("startrows", torch.zeros(self.num_threads, dtype=i32))

    # -- which operator a configuration maps to: hybrid > balanced > spmv > dense (quant.py:224-265;
    #    the batched branch has no balanced arm, :322-349)
    def op_kind(self, batched: bool) -> str:
        if self.include_sparse and self.topX > 0:
            return "spmv_hybrid"
        if self.include_sparse and self.balanced and not batched:
            return "spmv_balanced"
        if self.include_sparse:
            return "spmv"
        return "dense"

    def _call(self, x32: torch.Tensor, y: torch.Tensor, batched: bool) -> None:
        kind = self.op_kind(batched)
        sfx = "_batched" if batched else ""
        b = self.bits
        if kind == "dense":
            getattr(quant_cuda, f"vecquant{b}matmul_nuq_perchannel{sfx}")(x32, self.qweight, y, self.lookup_table)
        elif kind == "spmv":
            getattr(quant_cuda, f"vecquant{b}matmul_spmv_nuq_perchannel{sfx}")(
                self.rows, self.cols, self.vals, x32, y, self.outfeatures, self.qweight, self.lookup_table)
        elif kind == "spmv_hybrid":
            getattr(quant_cuda, f"vecquant{b}matmul_spmv_hybrid_nuq_perchannel{sfx}")(
                self.rows, self.cols, self.vals, x32, self.full_rows, self.full_row_indices, y,
                self.outfeatures, self.qweight, self.lookup_table)
        else:
            getattr(quant_cuda, f"vecquant{b}matmul_spmv_balanced_nuq_perchannel")(
                self.rows, self.cols, self.startrows, self.vals, x32, y, self.qweight, self.lookup_table,
                self.outfeatures, self.num_threads, self.numvals)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        dtype = x.dtype
        if x.shape[-1] == x.numel():  # single token: the matvec ops (quant.py:212-312)
            y = self.bias.clone() if self.bias is not None else torch.zeros(
                self.outfeatures, device=x.device, dtype=torch.float32)
            self._call(x.float().contiguous(), y, batched=False)
            return y.to(dtype).reshape(*x.shape[:-1], self.outfeatures)
        # several rows: the *_batched ops; bias is added AFTER the cast back (quant.py:313-383)
        x2 = x.reshape(-1, x.shape[-1])
        out = torch.zeros((x2.shape[0], self.outfeatures), device=x.device, dtype=torch.float32)
        self._call(x2.float().contiguous(), out, batched=True)
        out = out.to(dtype).reshape(*x.shape[:-1], self.outfeatures)
        # `out + self.bias` exactly as the reference writes it (quant.py:382): with the fp32 bias buffer
        # the constructor registers, an fp16 result is promoted to fp32 (checked against the unmodified
        # reference module in tests/test_gpu_reference_forward.py)
        return out + self.bias if self.bias is not None else out

    # -- MI355X-side conveniences -------------------------------------------------------------
    @classmethod
    def from_operands(cls, layer: dict, balanced: bool = False) -> "QuantLinearLUT":
        """Wrap already-packed operands (e.g. squeezellm_amd.synth.make_layer) without copying."""
        nnz = 0 if layer.get("vals") is None else layer["vals"].numel()
        topX = 0 if layer.get("full_rows") is None else layer["full_rows"].shape[1]
        # a layer whose outliers ALL moved into full_rows (pack_layer with every outlier in <= topX
        # rows) has an empty CSR but still needs the hybrid op: the sparse path is on whenever either
        # term exists
        m = cls(layer["bits"], layer["K"], layer["N"], layer.get("bias") is not None,
                include_sparse=nnz > 0 or topX > 0, numvals=nnz, topX=topX, balanced=balanced)
        m.qweight, m.lookup_table = layer["qweight"], layer["lookup_table"]
        if layer.get("bias") is not None:
            m.bias = layer["bias"]
        if nnz:
            m.rows, m.cols, m.vals = layer["rows"], layer["cols"], layer["vals"]
            if balanced:
                m.startrows = torch.zeros(m.num_threads, dtype=torch.int32, device=layer["vals"].device)
        elif topX:  # empty CSR operands for the hybrid op (the constructor registers none for numvals == 0)
            dev = layer["qweight"].device
            m.rows = layer["rows"] if layer.get("rows") is not None else torch.zeros(layer["N"] + 1, dtype=torch.int32, device=dev)
            m.cols = torch.zeros(0, dtype=torch.int32, device=dev)
            m.vals = torch.zeros(0, dtype=torch.float32, device=dev)
        if topX:
            m.full_rows, m.full_row_indices = layer["full_rows"], layer["full_row_indices"]
        return m

    def _operands(self) -> dict:
        """The operand dict of this module (no copies) with exactly the weight terms its forward applies: the sparse
        terms follow `include_sparse`, `numvals` and `topX` as `op_kind` does -- a module built with
        include_sparse=False yields the dense term alone even if it carries sparse buffers, and the top-X columns
        count only where the hybrid op would run."""
        lay = dict(bits=self.bits, K=self.infeatures, N=self.outfeatures, qweight=self.qweight, lookup_table=self.lookup_table,
                   bias=self.bias)
        if self.include_sparse:
            if self.numvals > 0 and getattr(self, "vals", None) is not None:
                lay.update(rows=self.rows, cols=self.cols, vals=self.vals)
            if self.topX > 0:
                lay.update(full_rows=self.full_rows, full_row_indices=self.full_row_indices)
        return lay

    def dequantize(self, dtype=torch.float16, out=None) -> torch.Tensor:
        """The dense weight [outfeatures, infeatures] this module multiplies by (all weight terms its forward applies: the sparse ones follow `include_sparse`, `numvals` and `topX` as `op_kind` does, summed
        in fp32, rounded once to `dtype`): one kernel on the current stream (decode.dequantize_layer)."""
        from . import decode

        return decode.dequantize_layer(self._operands(), dtype=dtype, out=out)

    def to_linear(self, dtype=torch.float16) -> nn.Linear:
        """An ordinary nn.Linear on the module's device: weight = dequantize(dtype), bias copied (cast to `dtype`)."""
        w = self.dequantize(dtype)
        lin = nn.Linear(self.infeatures, self.outfeatures, bias=self.bias is not None, device="meta")
        lin.weight = nn.Parameter(w, requires_grad=False)
        if self.bias is not None:
            lin.bias = nn.Parameter(self.bias.detach().to(device=w.device, dtype=dtype, copy=True), requires_grad=False)
        return lin


_is_capturing = torch.cuda.is_current_stream_capturing
_FRONT_DTYPES = (torch.float16, torch.bfloat16)  # the activation dtypes the front kernels take; anything else is a torch route
# (front, norm prologue, KV cache, fp8 cache, activation dtype) -> the entry point of include/sqllm_hip.h.  "linear_ep" is the
# linear with an epilogue (QuantLinearLUTFused.act, forward's residual / out); one descriptor per front serves both dtypes.
_FRONT_ENTRY = {
    (front, "norm" in variant, "cache" in variant, "fp8" in variant, dtype): f"sqllm_{front}{variant}_{sfx}"
    for front, variants in (("linear", ("",)), ("linear_ep", ("",)), ("gated", ("", "_norm")),
                            ("qkv_rope", ("", "_norm", "_cache", "_norm_cache", "_cache_fp8", "_norm_cache_fp8")))
    for variant in variants for dtype, sfx in zip(_FRONT_DTYPES, ("f16", "bf16"))}
_EP_ACT = {None: _lib.ACT_IDENTITY, "relu": _lib.ACT_RELU, "silu": _lib.ACT_SILU, "gelu": _lib.ACT_GELU, "gelu_tanh": _lib.ACT_GELU_TANH}


def _torch_epilogue(y: torch.Tensor, act, residual, dtype) -> torch.Tensor:
    """act(y) + residual in fp32 with the formulas of the kernel (include/sqllm_hip.h, sqllm_linear_ep), rounded once to `dtype`."""
    v = y.float()
    if act == "relu":
        v = torch.where(v > 0, v, torch.where(v != v, v, torch.zeros_like(v)))
    elif act == "silu":
        v = v / (1 + torch.exp(-v))
    elif act == "gelu":
        v = 0.5 * v * (1 + torch.erf(v * 0.70710678))
    elif act == "gelu_tanh":
        v = 0.5 * v * (1 + torch.tanh(0.79788456 * (v + 0.044715 * v * v * v)))
    if residual is not None:
        v = v + residual.float()
    return v.to(dtype)


_ws_need = {}  # (_lib.option_epoch, a *_workspace_bytes function of _lib, its arguments) -> bytes


def _workspace_of(mod: nn.Module, size, shape: tuple, device, stream=None) -> torch.Tensor:
    """The workspace rules of QuantLinearLUTFused._workspace (see there) on a module's cache dict `_ws`, for `size(*shape)` bytes:
    `size` is one of _lib's *_workspace_bytes, a call into the library, so each answer is kept.  `stream`: the raw current one."""
    key = (_lib.option_epoch, size, shape)
    need = _ws_need.get(key)
    if need is None:
        need = _ws_need[key] = size(*shape)
    cache, graph_max = mod.__dict__.setdefault("_ws", {}), mod.GRAPH_WS_MAX_BYTES
    if _is_capturing():
        ws = cache.get((device, "graph"))
        if ws is not None and ws.numel() >= need:
            return ws
        return torch.zeros(need, dtype=torch.uint8, device=device)  # (not remembered: it belongs to this graph's pool)
    if stream is None:
        stream = quant_cuda._raw_stream(device.index if device.index is not None else torch.cuda.current_device())
    key = (device, stream)
    ws = cache.get(key)
    if ws is None or ws.numel() < need:
        ws = torch.zeros(need, dtype=torch.uint8, device=device)  # zero-filled once
        cache[key] = ws
    if need <= graph_max:
        gws = cache.get((device, "graph"))
        if gws is None or gws.numel() < need:
            if gws is not None:
                cache.setdefault("retired", []).append(gws)
            cache[(device, "graph")] = torch.zeros(need, dtype=torch.uint8, device=device)
    return ws


# ---- what the front modules share on the host ("Adding a front"): intake, torch sums, descriptors, side structs ----

def _rows_of(x: torch.Tensor, K: int, contiguous: bool = True):
    """-> (x2: x as [rows, K], rows, batch: the descriptors' row count, 0 for one row).  x2 is made contiguous unless
    `contiguous` is False: a front whose remaining operand checks come before that copy makes it behind them."""
    if x.shape[-1] != K:
        raise ValueError(f"last dimension of x must be {K}, got {tuple(x.shape)}")
    x2 = x if x.dim() == 2 else x.reshape(-1, K)
    if contiguous and not x2.is_contiguous():
        x2 = x2.contiguous()
    rows = x2.shape[0]
    return x2, rows, 0 if rows == 1 else rows


def _fp32_sums(members, xin: torch.Tensor) -> list:
    """The dense route of a call with an epilogue, a norm or a rotation, fp32 from end to end so that the kernel's ONE rounding is
    the only one here too: per member its fp32 matrix (a temporary, 4 * K * N bytes) under torch's fp32 GEMM, plus the bias.
    (_forward_dense, the plain linear's and the plain pair's, keeps 16 bits: there the sum is rounded to 16 bits either way.)"""
    sums = []
    for m in members:
        s = F.linear(xin, m.dequantize(torch.float32))
        sums.append(s if m.bias is None else s + m.bias)
    return sums


def _composite_descriptor(cache: dict, dev: int, stream: int, members, build):
    """The descriptor of (device, stream) a front keeps in `cache` over its members' own sqllm_linear entries
    (QuantLinearLUTFused._descriptor): `build(entries)`, called only when one of those was rebuilt, returns the front's struct.
    -> entry = (struct, byref, the members' entries: they keep the folded CSRs alive).  Cached for every front as (those entries,
    entry, entry): the span-ladder suites read a cached descriptor at [1] (epilogue linear, q/k/v) and at [2] (the pair)."""
    member = QuantLinearLUTFused._descriptor
    entries = [member(m, dev, stream) for m in members]
    hit = cache.get((dev, stream))
    if hit is not None and all(map(operator.is_, hit[0], entries)):  # (a member's entry is the same object until it is rebuilt)
        return hit[1]
    s = build(entries)
    entry = (s, ctypes.byref(s), entries)
    cache[(dev, stream)] = (entries, entry, entry)
    return entry


def _side_struct(cache: dict, key, struct):
    """(the `struct` a front keeps for (device, stream) beside its descriptor -- filled anew by every call --, byref)"""
    hit = cache.get(key)
    if hit is None:
        s = struct()
        hit = cache[key] = (s, ctypes.byref(s))
    return hit


def _norm_ref(cache: dict, key, norm_weight: torch.Tensor, norm_eps: float):
    """The sqllm_rmsnorm of (device, stream), filled for this call; the ctypes reference to it."""
    nm, ref = _side_struct(cache, key, _lib.SqllmRmsNorm)
    nm.weight, nm.eps = norm_weight.data_ptr(), norm_eps
    return ref


def _kv_ref(cache: dict, key, k_cache: torch.Tensor, v_cache: torch.Tensor, slots: torch.Tensor, head_dim: int, scales=None):
    """The sqllm_kv_cache (with `scales`: the sqllm_kv_cache_fp8, in a dict of its own) of (device, stream), filled for this call."""
    c, ref = _side_struct(cache, key, _lib.SqllmKvCache if scales is None else _lib.SqllmKvCacheFp8)
    c.k_cache, c.v_cache, c.slots = k_cache.data_ptr(), v_cache.data_ptr(), slots.data_ptr()
    c.n_slots, c.slot_stride = k_cache.shape[0], k_cache.stride(0)
    c.head_stride = k_cache.stride(1) if k_cache.shape[1] > 1 else head_dim  # (one head: its stride is anything, and never used)
    if scales is not None:
        c.k_scale, c.v_scale = scales
    return ref


def _int32_vector(t: torch.Tensor) -> torch.Tensor:
    """`t` as a contiguous int32 vector; what already is one is returned as it is, so that a captured graph follows it."""
    if t.dim() != 1:
        t = t.reshape(-1)
    if t.dtype != torch.int32:
        t = t.to(torch.int32)  # (a kernel)
    return t if t.is_contiguous() else t.contiguous()


class QuantLinearLUTFused(QuantLinearLUT):
    """Opt-in forward for fp16 and bf16 activations: ONE kernel per call (sqllm_linear_f16 / sqllm_linear_bf16) instead of the
    reference's four (`zeros`/`bias.clone()`, `x.float()`, the op, `y.to(fp16)`; quant.py:214-223,
    :311-312 and :314-321, :380-383).  Same buffers and state dict as QuantLinearLUT -- switch an
    existing model over with `fuse_quant_lut(model)`.  Result = fp16(fp32 accumulation + bias);
    the reference's batched branch rounds to fp16 before adding the bias (and then promotes to
    fp32), so the two differ by at most one fp16 rounding of the output.  bf16 input gives
    bf16(fp32 accumulation + bias) the same way, from the same module, workspace and descriptor cache -- fp16 and bf16
    calls may alternate -- with ONE difference: a partial sum (one K slice of one output) beyond +-131072 in magnitude
    makes that output +-inf instead of a finite number (include/sqllm_hip.h, sqllm_linear_bf16, with the one corner
    where this is not guaranteed; the fp32 path returns the finite value there).  Other dtypes take the parent's path.

    Prompt-width inputs: the fused kernel decodes the packed weights once per 8 rows.  With `dense_min_rows` set, a call
    of at least that many rows instead writes the layer's dense matrix in the activations' 16-bit type once (`dequantize`:
    one kernel) and multiplies with torch's GEMM of that type (the bias is added in fp32, one rounding).  That matrix is a temporary of the call -- a torch allocation on the current
    stream, capture-safe, never cached on the module -- so the peak extra memory is ONE layer's matrix
    (2 * infeatures * outfeatures bytes: 142 MB for a 13B gate/up layer).  Recommended value: 128 -- on the 13B shapes
    the dense route measured 2.8 - 6.4x faster at 128 rows and 17 - 34x at 2048 (the figures per shape stand beside the
    attribute, the table in DESIGN.md 4.5); the break-even lies lower and is not measured.  The default stays None.

    Epilogue: with the class or instance attribute `act` set ("relu", "silu", "gelu", "gelu_tanh") and / or a `residual`
    given to forward, the call is still ONE kernel (sqllm_linear_ep_f16 / _bf16): out = OT(act(linear(x)) + residual),
    evaluated in fp32 and rounded once (include/sqllm_hip.h, sqllm_linear_ep: the formulas, non-finite values, and the
    range rule -- a partial sum beyond +-131072 makes the sum +-inf for fp16 too, never a clamped number).  `out` may be a
    tensor to write into; `out is residual` is the in-place form `h += linear(x)`.  The parent's path for other dtypes applies
    the same formulas in torch, in fp32 with one rounding.  So does the dense route (`dense_min_rows`), which for such a call
    stays in fp32 from end to end -- the layer's matrix in fp32 (a temporary of 4 * infeatures * outfeatures bytes, twice the
    plain dense route's) and torch's fp32 GEMM -- so that its result is within one rounding of the kernel's; its speed against
    the kernel is not measured.  `last_route` is "fused_ep" for the kernel.
    Speed against the same module followed by torch relu / add, graph-replayed on an MI355X (tools/epilogue_bench.py, table in
    DESIGN.md 4.4, raw output profiles/epilogue_bench.txt; 7B / 13B o_proj and down_proj + add, OPT-6.7B fc1 + relu): 1.1 - 2.7 us
    less per linear at 1 and 4 rows (4 - 27 %); at 16 rows 0 - 7 % less, with three bf16 dense-only points of 40 not faster
    (+0.9 % at most, inside the spread)."""

    # rows from which forward takes the dense route; None (default): never -- every call runs the fused kernel, as before
    # the route existed.
    # Recommended where prompts are run through this class: 128.  Measured on an MI355X (tools/dequant_bench.py, table in
    # DESIGN.md 4.5, raw output profiles/dequant_bench.txt), 13B shapes, w3 and w4, with and without sparse terms, the
    # dense route is faster at every row count the tool runs:
    #     gate/up (5120 x 13824):  128 rows 5.6 - 6.4x,  512 rows 14 - 17x,  2048 rows 21 - 29x
    #     o_proj  (5120 x 5120):   128 rows 2.8 - 4.3x,  512 rows 7.8 - 14x,  2048 rows 18 - 34x
    # so the break-even lies below 128 rows on both shapes and has not been measured; 128 is the lowest row count with a
    # measurement behind it, not the break-even.  The price is the temporary matrix (see the class docstring).
    dense_min_rows = None

    # the activation forward applies to the linear's fp32 result before the residual and the one rounding: None (default:
    # nothing, today's forward), "relu", "silu", "gelu" (erf form) or "gelu_tanh"
    act = None

    @property
    def last_route(self):
        """"fused", "fused_ep" (the kernel with the epilogue) or "dense": the way the most recent fp16 / bf16 GPU forward of this module went (None before the first)."""
        return self.__dict__.get("_last_route")

    def _forward_dense(self, x: torch.Tensor, x2: torch.Tensor) -> torch.Tensor:
        w = self.dequantize(x2.dtype)  # a temporary of this call (fp16 or bf16, as the activations)
        y = F.linear(x2, w)
        if self.bias is not None:
            y = (y.float() + self.bias).to(x2.dtype)
        return y.reshape(*x.shape[:-1], self.outfeatures)

    GRAPH_WS_MAX_BYTES = 4 << 20  # eager calls keep a second, graph-only workspace ready up to this size (decode batches)

    def _workspace(self, batch: int, device, stream=None) -> torch.Tensor:
        """ONE zero-filled workspace per (device, stream), sized for the largest batch seen so far: a
        launch uses the first 8 * batch * N bytes and leaves them zero-filled, so smaller batches
        reuse the same buffer (a cache keyed by batch size would grow without bound under variable
        prompt lengths).  Two launches of one module that may overlap -- i.e. on different streams --
        must not share the accumulator words, hence the stream in the key.

        Captured calls: a graph bakes the workspace's address in, and the capture stream is never the stream of the
        warm-up calls, so a buffer keyed on it would be allocated AND zero-filled inside the capture -- a fill kernel in
        front of every linear of the graph, replayed every time (that was 25 % of a replayed 7B pass: 484 against 603
        tokens/s for the same kernels as a C-ABI sequence, BENCH_r05 `drop_in`).  Every eager call therefore also keeps
        a graph-only workspace of its size ready (key (device, "graph"); up to GRAPH_WS_MAX_BYTES: decode batches), a
        captured call takes that one -- the graph then holds the linear's kernel and nothing else -- and superseded
        buffers are retired, not freed (older graphs may still point at them).  All graphs captured from this module
        share it: replaying two of them CONCURRENTLY on different streams is not supported (set GRAPH_WS_MAX_BYTES = 0
        on the module for private, in-graph workspaces).  Without a prepared buffer (no eager call of this size before
        the capture) the workspace is a zero-filled temporary of the captured region."""
        return _workspace_of(self, _lib.linear_workspace_bytes, (self.outfeatures, batch), device, stream)

    def _check_csr_once(self) -> None:
        """The fused kernel detects completion by COUNTING the contributions `rows` announces: an
        inconsistent CSR (rows not non-decreasing, rows[N] != nnz -- e.g. buffers not loaded yet)
        would leave columns unfinished and the shared workspace dirty for every later call.  Checked
        once per module and CSR buffer (one device round trip), so that it fails loudly instead."""
        key = (self.rows.data_ptr(), self.rows._version, self.vals.data_ptr(), self.vals.numel())
        if self.__dict__.get("_csr_ok") == key:
            return
        if torch.cuda.is_current_stream_capturing():
            return  # the check reads back from the device, which would invalidate the capture: deferred to the next eager call
        r = self.rows
        ok = r.numel() == self.outfeatures + 1 and bool((r[1:] >= r[:-1]).all()) and int(r[0]) == 0 and int(r[-1]) == self.vals.numel()
        if not ok:
            raise ValueError("QuantLinearLUTFused: inconsistent CSR operands (rows must be non-decreasing with rows[0] == 0 and "
                             "rows[N] == vals.numel()); the fused kernel counts contributions from `rows`")
        self.__dict__["_csr_ok"] = key

    fold_topx = True  # fold the top-X dense rows into the CSR the fused kernel is given (set False to pass them separately)

    def _csr_with_topx(self):
        """(rows, cols, vals) with the top-X rows folded in (decode.fold_topx_into_csr), rebuilt whenever one of the
        buffers it was built from is replaced OR written in place (load_state_dict copies into the same storage: the
        key carries the tensors' version counters); not built while the stream is capturing -- that call then passes
        the top-X rows separately."""
        from . import decode

        has_csr = self.numvals > 0
        src = [self.full_rows, self.full_row_indices] + ([self.rows, self.cols, self.vals] if has_csr else [])
        key = tuple((t.data_ptr(), t._version) for t in src) + (self.numvals,)
        hit = self.__dict__.get("_folded")
        if hit is not None and hit[0] == key:
            return hit[1]
        if torch.cuda.is_current_stream_capturing():
            return None
        lay = dict(N=self.outfeatures, full_rows=self.full_rows, full_row_indices=self.full_row_indices)
        if has_csr:
            lay.update(rows=self.rows, cols=self.cols, vals=self.vals)
        out = decode.fold_topx_into_csr(lay)
        self.__dict__["_folded"] = (key, out)
        return out

    def _descriptor(self, dev: int, stream: int):
        """The pre-marshalled sqllm_linear of this module for (device, stream): every persistent field filled in once --
        weights, codebook, the (folded) sparse operands, bias -- and re-used call after call; vec / mul, the batch and the
        workspace pointer are set per call (ONE entry per device and stream whatever row counts arrive: an entry per
        batch would pin a superseded workspace each and grow without bound under variable prompt lengths).  Rebuilt when
        a buffer is replaced, moved or written in place (identity, storage and version counter of every buffer it was
        built from) or when a routing attribute changes (fold_topx, include_sparse, topX, numvals).
        (QuantGatedLUTFused calls this on plain QuantLinearLUT members too: what it needs beyond the parent's attributes is
        reached through this class, not through `self`.)"""
        # (straight from the module's buffer dict: nn.Module.__getattr__ costs ~0.5 us per buffer, ten times a dict lookup)
        bufs = self.__dict__["_buffers"]
        fold_topx = getattr(self, "fold_topx", QuantLinearLUTFused.fold_topx)
        key = (tuple((id(t), t.data_ptr(), t._version) for t in bufs.values() if t is not None),
               fold_topx, self.include_sparse, self.topX, self.numvals)
        cache = self.__dict__.setdefault("_desc", {})
        hit = cache.get((dev, stream))
        if hit is not None and hit[0] == key:
            return hit[1]
        capturing = torch.cuda.is_current_stream_capturing()
        K, N = self.infeatures, self.outfeatures
        lin = _lib.SqllmLinear()
        o = lin.op
        o.bits, o.K, o.N = self.bits, K, N
        o.qweight, o.lookup_table = self.qweight.data_ptr(), self.lookup_table.data_ptr()
        if self.include_sparse and self.numvals > 0:
            QuantLinearLUTFused._check_csr_once(self)
        folded = QuantLinearLUTFused._csr_with_topx(self) if self.include_sparse and self.topX > 0 and fold_topx else None
        keep = [folded]
        if folded is not None:  # one CSR term that contains the top-X rows (decode.fold_topx_into_csr)
            if folded[2].numel():
                o.rows, o.cols, o.vals, o.nnz = folded[0].data_ptr(), folded[1].data_ptr(), folded[2].data_ptr(), folded[2].numel()
        else:
            if self.include_sparse and self.numvals > 0:
                o.rows, o.cols, o.vals, o.nnz = self.rows.data_ptr(), self.cols.data_ptr(), self.vals.data_ptr(), self.vals.numel()
            if self.include_sparse and self.topX > 0:  # independent of the CSR term (which may be empty)
                o.full_rows, o.full_row_indices, o.topX = self.full_rows.data_ptr(), self.full_row_indices.data_ptr(), self.topX
        lin.bias = None if self.bias is None else self.bias.data_ptr()
        entry = (key, (lin, ctypes.byref(lin), keep))
        # (while a stream is capturing, the folded CSR and the CSR check are deferred: do not pin that state)
        if not (capturing and self.include_sparse):
            cache[(dev, stream)] = entry
        return entry[1]

    @staticmethod
    def _build_epilogue(entries):
        e = _lib.SqllmLinearEp()
        e.lin = entries[0][0]  # (a copy)
        return e

    def _epilogue_descriptor(self, dev: int, stream: int):
        """The sqllm_linear_ep of (device, stream): the module's own pre-marshalled sqllm_linear (see _descriptor) copied
        into it, rebuilt when that one is; residual, act, vec / mul, the batch and the workspace are set per call."""
        return _composite_descriptor(self.__dict__.setdefault("_ep_desc", {}), dev, stream, (self,), self._build_epilogue)

    def _check_epilogue(self, x: torch.Tensor, act, residual, out):
        """The checks of a call with an epilogue, in their order -> _rows_of's (x2, rows, batch), not yet copied, and the shape."""
        if act not in _EP_ACT:
            raise ValueError(f"act must be one of None, 'relu', 'silu', 'gelu', 'gelu_tanh', got {act!r}")
        intake = _rows_of(x, self.infeatures, False)
        shape = (*x.shape[:-1], self.outfeatures)
        for name, t in (("residual", residual), ("out", out)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.device != x.device or t.dtype != x.dtype or tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {x.dtype} tensor of shape {shape} on {x.device}")
        if out is not None and out is not residual and residual is not None and out.data_ptr() != residual.data_ptr():
            lo, hi = out.data_ptr(), out.data_ptr() + out.numel() * out.element_size()
            if residual.data_ptr() < hi and lo < residual.data_ptr() + residual.numel() * residual.element_size():
                raise ValueError("out must be residual itself or must not overlap it")
        return (*intake, shape)

    def forward(self, x: torch.Tensor, residual=None, out=None) -> torch.Tensor:
        act = self.act
        ep = act is not None or residual is not None or out is not None  # (a call with an epilogue: sqllm_linear_ep)
        dtype = x.dtype
        kernel = dtype in _FRONT_DTYPES and x.is_cuda
        if ep:
            x2, rows, batch, shape = self._check_epilogue(x, act, residual, out)
            if not kernel:
                y = _torch_epilogue(QuantLinearLUT.forward(self, x), act, residual, dtype)
                return y if out is None else out.copy_(y)
            if not x2.is_contiguous():
                x2 = x2.contiguous()
        elif not kernel:
            return super().forward(x)
        else:
            x2, rows, batch = _rows_of(x, self.infeatures)
        if self.dense_min_rows is not None and rows >= self.dense_min_rows:
            self.__dict__["_last_route"] = "dense"
            if not ep:
                return self._forward_dense(x, x2)
            y = _torch_epilogue(_fp32_sums((self,), x2.float())[0].reshape(shape), act, residual, dtype)
            return y if out is None else out.copy_(y)
        dev = x.get_device()
        stream = quant_cuda._raw_stream(dev)
        if ep:
            self.__dict__["_last_route"] = "fused_ep"
            if out is None:
                out = torch.empty(shape, dtype=dtype, device=x.device)
            e, ref, _keep = self._epilogue_descriptor(dev, stream)
            lin = e.lin
            e.residual = None if residual is None else residual.data_ptr()
            e.act = _EP_ACT[act]
        else:
            self.__dict__["_last_route"] = "fused"
            out = torch.empty((rows, self.outfeatures), dtype=dtype, device=x.device)
            lin, ref, _keep = self._descriptor(dev, stream)
        o = lin.op
        o.batch, o.vec, o.mul = batch, x2.data_ptr(), out.data_ptr()
        # (qweight straight from the buffer dict, as in _descriptor; `ws` lives until the launch is queued: a captured call's temporary)
        ws = self._workspace(batch, self._buffers["qweight"].device, stream)
        lin.workspace = ws.data_ptr()
        quant_cuda._launch(quant_cuda._fn(_FRONT_ENTRY["linear_ep" if ep else "linear", False, False, False, dtype]), dev, (ref,))
        return out if ep else out.reshape(*x.shape[:-1], self.outfeatures)


def fuse_quant_lut(module: nn.Module) -> int:
    """Switch every QuantLinearLUT under `module` to the fused fp16 / bf16 forward (in place, buffers and
    state dict untouched).  Returns the number of layers switched."""
    n = 0
    for m in module.modules():
        if type(m) is QuantLinearLUT:
            m.__class__ = QuantLinearLUTFused
            n += 1
    return n


def _check_norm_weight(x: torch.Tensor, norm_weight: torch.Tensor, K: int, norm_eps: float) -> torch.Tensor:
    """The norm weight of a norm front: [K], of x's dtype, on x's device (anything else: ValueError); returned contiguous."""
    if not isinstance(norm_weight, torch.Tensor) or norm_weight.dtype != x.dtype or norm_weight.device != x.device:
        raise ValueError(f"norm_weight must be a {x.dtype} tensor on {x.device}, got "
                         f"{getattr(norm_weight, 'dtype', type(norm_weight).__name__)} on {getattr(norm_weight, 'device', None)}")
    if norm_weight.dim() != 1 or norm_weight.numel() != K:
        raise ValueError(f"norm_weight must have {K} elements, got {tuple(norm_weight.shape)}")
    if not (norm_eps >= 0.0) or norm_eps == float("inf"):
        raise ValueError(f"norm_eps must be finite and >= 0, got {norm_eps}")
    return norm_weight if norm_weight.is_contiguous() else norm_weight.contiguous()


def _torch_rmsnorm(x2: torch.Tensor, norm_weight: torch.Tensor, norm_eps: float) -> torch.Tensor:
    """xn of the norm fronts (include/sqllm_hip.h, sqllm_rmsnorm) in torch: fp32, NOT rounded to x's type."""
    xf = x2.float()
    r = 1.0 / torch.sqrt(xf.pow(2).mean(dim=-1, keepdim=True) + norm_eps)
    return xf * norm_weight.float() * r


class QuantGatedLUTFused(nn.Module):
    """`silu(gate(x)) * up(x)` for fp16 and bf16 GPU activations as ONE kernel (sqllm_gated_f16 / sqllm_gated_bf16) instead of
    two fused linears and two torch kernels over two [rows, N] temporaries: both sums are formed as in QuantLinearLUTFused,
    the activation and the product are evaluated in fp32 and the result is rounded once to the activations' type
    (include/sqllm_hip.h, sqllm_gated: semantics, non-finite values, and the range rule -- a partial sum beyond +-131072 in
    magnitude makes that sum +-inf for fp16 as well as bf16, never a clamped finite number).

    `gate` and `up` are two QuantLinearLUT / QuantLinearLUTFused modules of equal shape and bit width, held BY REFERENCE:
    this module owns no buffers, no parameters and no state-dict keys, and does not appear among nobody's children because
    of them; their folded top-X CSR and one-time CSR check are the members' own (shared with their own fused forward).  It keeps one
    descriptor per (device, stream) and one workspace by the rules of QuantLinearLUTFused._workspace.  Other dtypes and CPU
    tensors return F.silu(gate(x)) * up(x); with `gate.dense_min_rows` set, a call of at least that many rows sends both
    members down their dense route and applies the activation in torch (in fp32, rounded once).  `last_route`: "gated" / "dense" / "fallback".

    Speed, graph-replayed on an MI355X (tools/gated_bench.py, table in DESIGN.md 4.4, raw output profiles/gated_linear.txt; 7B
    and 13B gate / up pairs, w3 / w4, s0 / s45 + top-10, fp16 / bf16): against two fused modules + torch silu / mul, 6 - 23 us
    less per pair on all 48 points (-41 .. -3.5 %).  Against one grouped launch + torch: 3.0 - 6.2 us less at 1 row, 0.9 - 3.7 us
    less at 4 rows; at 8 rows NOT faster on 11 of 16 points (every s45 + top-10 point, +2.0 .. +3.7 %; three s0 points inside
    the spread).

    forward(x, norm_weight=None, norm_eps=1e-6).  With a `norm_weight` ([K], x's dtype and device; anything else is a
    ValueError) x is the UN-normalised hidden state and the RMSNorm in front of the MLP is a prologue of the same kernel
    (sqllm_gated_norm_f16 / _bf16; include/sqllm_hip.h, sqllm_rmsnorm: xn = float(x) * float(weight) * r in fp32, never
    rounded to 16 bits, which is NOT bit-identical to a torch norm module in front -- that one rounds xn twice).  The
    fallback and the dense route compute the same formulas in torch, in fp32 with one rounding.  `last_route` is then
    "gated_norm".  Without a weight nothing changes: same entry point, same bits.  Speed, graph-replayed (tools/norm_front_bench.py,
    table in DESIGN.md 4.4, raw output profiles/norm_front_bench.txt; 7B and 13B gate / up): at 1 row the prologue costs 1.5 - 4.5 us
    where torch.nn.functional.rms_norm in front costs 4.2 - 6.2 us and the norm as the checkpoints' modules write it 17 - 20 us --
    faster than either on all 16 points; at 4 rows NOT faster than rms_norm on 8 of 16 points (every s45 + top-10 point, +3.6 us at
    most); at 16 rows NOT faster on any of 16 (+3.8 .. +29.2 us: every workgroup sums the squares of all its tile's rows) -- keep
    rms_norm in front there."""

    GRAPH_WS_MAX_BYTES = QuantLinearLUTFused.GRAPH_WS_MAX_BYTES

    def __init__(self, gate: QuantLinearLUT, up: QuantLinearLUT):
        super().__init__()
        for name, m in (("gate", gate), ("up", up)):
            if not isinstance(m, QuantLinearLUT):
                raise TypeError(f"{name} must be a QuantLinearLUT or QuantLinearLUTFused, got {type(m).__name__}")
        if (gate.infeatures, gate.outfeatures) != (up.infeatures, up.outfeatures):
            raise ValueError(f"gate and up must have the same shape: {gate.infeatures} x {gate.outfeatures} against "
                             f"{up.infeatures} x {up.outfeatures}")
        if gate.bits != up.bits:
            raise ValueError(f"gate and up must have the same bit width: {gate.bits} against {up.bits}")
        # by reference: nn.Module.__setattr__ would register them as children (and their buffers under this module's keys)
        self.__dict__["gate"], self.__dict__["up"] = gate, up

    @property
    def last_route(self):
        """"gated", "gated_norm", "dense" or "fallback": the way the most recent forward went (None before the first)."""
        return self.__dict__.get("_last_route")

    def _descriptor(self, dev: int, stream: int):
        """The sqllm_gated of (device, stream): the members' own pre-marshalled descriptors (QuantLinearLUTFused._descriptor:
        rebuilt when a buffer or a routing attribute of the member changes) copied side by side, rebuilt when either is."""
        return _composite_descriptor(self.__dict__.setdefault("_desc", {}), dev, stream, (self.gate, self.up), self._build)

    @staticmethod
    def _build(entries):
        lg, lu = entries[0][0], entries[1][0]
        g = _lib.SqllmGated()
        g.gate, g.up = lg.op, lu.op  # (copies)
        g.gate.mul = g.up.mul = None
        g.bias_gate, g.bias_up = lg.bias, lu.bias
        g.act = _lib.ACT_SILU
        return g

    def forward(self, x: torch.Tensor, norm_weight=None, norm_eps: float = 1e-6) -> torch.Tensor:
        gate, up = self.gate, self.up
        K, N = gate.infeatures, gate.outfeatures
        norm = norm_weight is not None
        if norm:
            x2, rows, batch = _rows_of(x, K, False)
            norm_weight = _check_norm_weight(x, norm_weight, K, norm_eps)
        dtype = x.dtype
        if dtype not in _FRONT_DTYPES or not x.is_cuda:
            self.__dict__["_last_route"] = "fallback"
            if norm:  # (fp32 from end to end, one rounding)
                xn = _torch_rmsnorm(x2, norm_weight, norm_eps)
                y = F.silu(QuantLinearLUT.forward(gate, xn).float()) * QuantLinearLUT.forward(up, xn).float()
                return y.to(dtype).reshape(*x.shape[:-1], N)
            return F.silu(gate(x)) * up(x)
        if not norm:
            x2, rows, batch = _rows_of(x, K)
        elif not x2.is_contiguous():
            x2 = x2.contiguous()
        dense_min_rows = getattr(gate, "dense_min_rows", None)
        if dense_min_rows is not None and rows >= dense_min_rows:
            self.__dict__["_last_route"] = "dense"
            if norm:
                sums = _fp32_sums((gate, up), _torch_rmsnorm(x2, norm_weight, norm_eps))
                return (F.silu(sums[0]) * sums[1]).to(dtype).reshape(*x.shape[:-1], N)
            dense = QuantLinearLUTFused._forward_dense
            # (the two 16-bit sums widened: activation and product in fp32, one rounding -- as the kernel evaluates them)
            return (F.silu(dense(gate, x, x2).float()) * dense(up, x, x2).float()).to(dtype)
        self.__dict__["_last_route"] = "gated_norm" if norm else "gated"
        dev = x.get_device()
        out = torch.empty((rows, N), dtype=dtype, device=x.device)
        stream = quant_cuda._raw_stream(dev)
        g, ref, _keep = self._descriptor(dev, stream)
        g.gate.batch = g.up.batch = batch
        g.gate.vec = g.up.vec = x2.data_ptr()
        ws = _workspace_of(self, _lib.gated_workspace_bytes, (N, batch), gate._buffers["qweight"].device, stream)
        g.out, g.workspace = out.data_ptr(), ws.data_ptr()
        args = (ref, _norm_ref(self.__dict__.setdefault("_norm", {}), (dev, stream), norm_weight, norm_eps)) if norm else (ref,)
        quant_cuda._launch(quant_cuda._fn(_FRONT_ENTRY["gated", norm, False, False, dtype]), dev, args)
        return out.reshape(*x.shape[:-1], N)


def fuse_gated_mlps(module: nn.Module, gate: str = "gate_proj", up: str = "up_proj", down: str = "down_proj") -> int:
    """Give every submodule of `module` that has the attributes `gate`, `up` and `down` -- gate and up two quantised layers
    of equal shape and bit width -- and whose `act_fn` is an nn.SiLU the forward `down(gated(x))`, with `gated` a
    QuantGatedLUTFused over its gate and up (in place; parameters, buffers and state dict untouched).  Anything else is left
    alone: a submodule without `act_fn`, or with another activation, keeps its forward.  Where `down` is a
    QuantLinearLUTFused the submodule also gets `forward_residual(x, residual)` = `residual + down(gated(x))` with the add
    done by down's kernel (QuantLinearLUTFused.forward: residual).  Returns the number converted."""
    n = 0
    for m in module.modules():
        g, u, d = getattr(m, gate, None), getattr(m, up, None), getattr(m, down, None)
        if d is None or not isinstance(g, QuantLinearLUT) or not isinstance(u, QuantLinearLUT):
            continue
        if not isinstance(getattr(m, "act_fn", None), nn.SiLU):
            continue
        if (g.infeatures, g.outfeatures, g.bits) != (u.infeatures, u.outfeatures, u.bits):
            continue
        gated = QuantGatedLUTFused(g, u)
        m.__dict__["gated"] = gated  # (not a child: the module tree and the state dict stay as they are)
        m.forward = (lambda gated, d: lambda x: d(gated(x)))(gated, d)
        if isinstance(d, QuantLinearLUTFused):  # `residual + down(gated(x))` with the add inside down's kernel
            m.__dict__["forward_residual"] = (lambda gated, d: lambda x, residual: d(gated(x), residual=residual))(gated, d)
        n += 1
    return n


_ROPE_LAYOUT = {"half": _lib.ROPE_HALF, "interleaved": _lib.ROPE_INTERLEAVED}


def rope_tables(head_dim: int, n_pos: int, theta: float = 10000.0, device=None):
    """fp32 (cos, sin) of shape [n_pos, head_dim / 2] for QuantQKVRopeFused: angle[p, j] = p * theta ** (-2 j / head_dim),
    computed in fp64 and rounded once.  (The kernel computes no angles: tables built by any other base or scaling rule
    serve as well.)"""
    if head_dim < 2 or head_dim % 2 or n_pos < 1:
        raise ValueError(f"head_dim must be even and >= 2 and n_pos >= 1, got {head_dim}, {n_pos}")
    j = torch.arange(head_dim // 2, dtype=torch.float64)
    inv_freq = torch.tensor(float(theta), dtype=torch.float64) ** (-2.0 * j / head_dim)
    ang = torch.arange(n_pos, dtype=torch.float64)[:, None] * inv_freq[None, :]
    return ang.cos().float().to(device), ang.sin().float().to(device)


def _torch_rope(s: torch.Tensor, positions: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, head_dim: int, layout: str, dtype) -> torch.Tensor:
    """The rotation of the kernel (include/sqllm_hip.h, sqllm_qkv_rope) on sums s [rows, N] in torch: fp32, rounded once to
    `dtype`; a position outside the tables makes its row NaN."""
    rows, N = s.shape
    half = head_dim // 2
    p = positions.long()
    ok = (p >= 0) & (p < cos.shape[0])
    pc = torch.where(ok, p, torch.zeros_like(p))
    nan = torch.full((), float("nan"), dtype=torch.float32, device=s.device)
    c = torch.where(ok[:, None], cos.float()[pc], nan)[:, None, :]  # [rows, 1, half]
    sn = torch.where(ok[:, None], sin.float()[pc], nan)[:, None, :]
    v = s.float().reshape(rows, N // head_dim, head_dim)
    if layout == "half":
        lo, hi = v[..., :half], v[..., half:]
        out = torch.cat((lo * c - hi * sn, hi * c + lo * sn), dim=-1)
    else:
        lo, hi = v[..., 0::2], v[..., 1::2]
        out = torch.stack((lo * c - hi * sn, hi * c + lo * sn), dim=-1)
    return out.reshape(rows, N).to(dtype)


FP8_KV_DTYPES = (torch.float8_e4m3fn, torch.uint8)  # what an fp8 KV cache may be held as: OCP e4m3fn elements, or their bytes
FP8_KV_MAX = 448.0  # the largest finite e4m3fn value


def fp8_kv_scale(absmax):
    """The scale of an fp8 KV cache whose largest magnitude is to be `absmax` (a float or a tensor; calibration is the caller's)."""
    return absmax / FP8_KV_MAX


def _check_fp8_scales(fp8: bool, k_scale, v_scale):
    """The scales of forward(): both with an fp8 cache -- finite, positive, with finite fp32 reciprocals --, none without."""
    if not fp8:
        if k_scale is not None or v_scale is not None:
            raise ValueError("k_scale and v_scale belong to a float8_e4m3fn (or uint8) KV cache: this call has none")
        return None, None
    if k_scale is None or v_scale is None:
        raise ValueError("an fp8 KV cache needs both k_scale and v_scale")
    out = []
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        f = torch.tensor(float(t), dtype=torch.float32)
        if not bool(torch.isfinite(f)) or float(f) <= 0.0 or not bool(torch.isfinite(1.0 / f)):
            raise ValueError(f"{name} must be finite and positive with a finite fp32 reciprocal, got {t}")
        out.append(float(f))
    return out[0], out[1]


def _fp8_bytes(x32: torch.Tensor, scale: float) -> torch.Tensor:
    """The bytes of include/sqllm_hip.h's encoding of fp32 values: e4m3_rne(clamp(x * (1 / scale), +-448)), NaN staying NaN."""
    inv = (1.0 / torch.tensor(scale, dtype=torch.float32)).to(x32.device)
    return (x32.float() * inv).clamp(-FP8_KV_MAX, FP8_KV_MAX).to(torch.float8_e4m3fn).view(torch.uint8)


def kv_cache_view(cache: torch.Tensor, layout: str = "nhd") -> torch.Tensor:
    """The 3-D view [n_slots, H_kv, head_dim] of a KV cache that QuantQKVRopeFused.forward takes as `k_cache` / `v_cache`
    (no copy; strides 0 and 1 of the view become slot_stride and head_stride of include/sqllm_hip.h, sqllm_kv_cache).
      "nhd":  slot-major [n_slots, H, D], or paged [blocks, block, H, D] with slot = block_index * block + offset;
      "bhsd": head-major static [B, H, S, D] with slot = b * H * S + p (static_cache_slots): an OVERLAPPING as_strided view
              of H rows S * D apart for each of (B - 1) * H * S + S slots D apart."""
    if cache.stride(-1) != 1:
        raise ValueError("the last dimension of a KV cache must be contiguous")
    if layout == "nhd":
        if cache.dim() == 3:
            return cache
        if cache.dim() == 4 and cache.stride(0) == cache.shape[1] * cache.stride(1):
            return cache.as_strided((cache.shape[0] * cache.shape[1], cache.shape[2], cache.shape[3]), (cache.stride(1), cache.stride(2), 1),
                                    cache.storage_offset())
        raise ValueError(f"an 'nhd' cache is [n_slots, H, D] or a paged [blocks, block, H, D] whose blocks lie block * stride(1) apart, got "
                         f"{tuple(cache.shape)} with strides {cache.stride()}")
    if layout == "bhsd":
        if cache.dim() != 4 or not cache.is_contiguous():
            raise ValueError(f"a 'bhsd' cache is a contiguous [B, H, S, D], got {tuple(cache.shape)} with strides {cache.stride()}")
        B, H, S, D = cache.shape
        return cache.as_strided(((B - 1) * H * S + S, H, D), (D, S * D, 1), cache.storage_offset())
    raise ValueError(f"layout must be 'nhd' or 'bhsd', got {layout!r}")


def static_cache_slots(positions: torch.Tensor, n_kv_heads: int, max_seq: int) -> torch.Tensor:
    """int32 slots of a head-major static cache [B, H, S, D] seen through kv_cache_view(cache, "bhsd"): row b at position p
    goes to slot b * H * S + p.  (A position outside [0, S) would land in a neighbouring head's or row's slots: it gets -1,
    an out-of-range slot, which writes nothing.)"""
    p = positions.reshape(-1).long()
    slot = torch.arange(p.numel(), device=p.device) * (int(n_kv_heads) * int(max_seq)) + p
    return torch.where((p >= 0) & (p < max_seq), slot, torch.full_like(slot, -1)).to(torch.int32)


def _torch_cache_write(cache: torch.Tensor, slots: torch.Tensor, rows_: torch.Tensor) -> None:
    """cache[slots[b]] = rows_[b] for the slots inside [0, n_slots), in torch (the dense and fallback routes): by element
    offsets into a flat view of the cache's extent, so that an overlapping as_strided view (kv_cache_view "bhsd") works too."""
    n_slots, H, D = cache.shape
    s = slots.reshape(-1).long()
    ok = (s >= 0) & (s < n_slots)
    ss, hs = cache.stride(0), cache.stride(1)
    flat = cache.as_strided(((n_slots - 1) * ss + (H - 1) * hs + D,), (1,), cache.storage_offset())
    at = (s[ok][:, None, None] * ss + torch.arange(H, device=s.device)[None, :, None] * hs + torch.arange(D, device=s.device)[None, None, :])
    flat.index_put_((at.reshape(-1),), rows_.reshape(-1, H, D)[ok].reshape(-1))


def _torch_cache_write_fp8(cache: torch.Tensor, slots: torch.Tensor, rows32: torch.Tensor, scale: float) -> None:
    """_torch_cache_write for an fp8 cache: the fp32 values `rows32`, encoded once, as bytes (torch has no indexing for float8)."""
    _torch_cache_write(cache.view(torch.uint8), slots, _fp8_bytes(rows32, scale))


class QuantQKVRopeFused(nn.Module):
    """q_proj, k_proj, v_proj and the rotary position embedding of q and k for fp16 and bf16 GPU activations as ONE kernel
    (sqllm_qkv_rope_f16 / _bf16) instead of one grouped launch and the string of torch element-wise kernels behind it (the
    gather of cos and sin, rotate_half, two multiplies and an add, for q and again for k): the three sums are formed as in
    QuantLinearLUTFused, q and k are rotated in fp32 and everything is rounded once to the activations' type
    (include/sqllm_hip.h, sqllm_qkv_rope: semantics, layouts, non-finite values, and the range rule -- a partial sum beyond
    +-131072 in magnitude makes that sum +-inf for fp16 as well as bf16).

    `q`, `k`, `v` are three QuantLinearLUT / QuantLinearLUTFused modules of equal infeatures and bit width (k and v may be
    narrower than q), held BY REFERENCE: this module owns no buffers, no parameters and no state-dict keys.  `head_dim` is even
    and divides q's and k's outfeatures; `layout` is "half" (the rotate_half form: partner head_dim / 2 away) or "interleaved"
    (partner next door).  It keeps one descriptor per (device, stream) and one workspace by the rules of
    QuantLinearLUTFused._workspace.

    forward(x, positions, cos, sin) -> (q, k, v), each [..., N_m].  `cos`, `sin`: fp32 [n_pos, head_dim / 2] on x's device
    (rope_tables, or the caller's own).  `positions`: one per row of x, an int32 tensor on x's device, used WITHOUT a copy -- a
    captured graph follows a position updated in place; int64 is accepted and converted, which costs a kernel (and a captured
    graph then follows the int64 tensor through that kernel).  A position outside [0, n_pos) makes that row of q and k NaN.
    Other dtypes and CPU tensors, and calls of at least `q.dense_min_rows` rows (the members' dense route), compute the same
    formulas in torch, in fp32 with one rounding.  `last_route`: "qkv_rope" / "dense" / "fallback".

    Speed, graph-replayed on an MI355X (tools/qkv_rope_bench.py, table in DESIGN.md 4.4, raw output profiles/qkv_rope_bench.txt;
    K = 4096, head_dim 128, 3 x 4096 and 4096 + 2 x 1024, w3 / w4, s0 / s45 + top-10, fp16 / bf16, 1 / 4 / 16 rows): 28 - 40 us
    less per layer than one grouped launch + the rotary step in torch (-79 .. -34 %), 37 - 75 us less than three fused modules +
    the same step; faster on all 48 points.

    forward(x, positions, cos, sin, norm_weight=None, norm_eps=1e-6).  With a `norm_weight` ([K], x's dtype and device;
    anything else is a ValueError) x is the UN-normalised hidden state and the RMSNorm in front of the attention is a
    prologue of the same kernel (sqllm_qkv_rope_norm_f16 / _bf16; include/sqllm_hip.h, sqllm_rmsnorm: xn in fp32, never
    rounded to 16 bits -- NOT bit-identical to a torch norm module in front).  The fallback and the dense route compute the
    same formulas in torch, in fp32 with one rounding; `last_route` is then "qkv_rope_norm".  Without a weight nothing
    changes: same entry point, same bits.  Speed, graph-replayed (tools/norm_front_bench.py, table in DESIGN.md 4.4, raw output
    profiles/norm_front_bench.txt; 7B and 13B q / k / v): at 1 row the prologue costs 0.7 - 3.0 us where
    torch.nn.functional.rms_norm in front costs 4.3 - 5.9 us and the norm as the checkpoints' modules write it 18 - 21 us -- faster
    than either on all 16 points; at 4 rows NOT faster than rms_norm on 2 of 16 points (+0.4 us at most); at 16 rows NOT faster on
    any of 16 (+2.4 .. +22.0 us: every workgroup sums the squares of all its tile's rows) -- keep rms_norm in front there.

    forward(..., k_cache=None, v_cache=None, slots=None, return_kv=True).  With a KV cache the same kernel stores k and v
    into it as their columns finish (sqllm_qkv_rope_cache_* / sqllm_qkv_rope_norm_cache_*; include/sqllm_hip.h, sqllm_kv_cache):
    row b's k and v go to k_cache[slots[b]] and v_cache[slots[b]], bit for bit what the returned k and v hold.  `k_cache`,
    `v_cache`: 3-D views [n_slots, H_kv, head_dim] (kv_cache_view) of x's dtype and device, of equal shape and strides,
    stride(-1) == 1, H_kv * head_dim == N_k == N_v; overlapping as_strided views are allowed.  `slots`: one per row, int32 on
    x's device, used WITHOUT a copy (int64 is converted, which costs a kernel, as for positions); a slot outside
    [0, n_slots) -- the usual -1 padding -- writes nothing; two rows with one slot leave one of the two rows' values.  All three
    or none: anything else is a ValueError.  `return_kv=False` (only with a cache): k and v go to the cache alone and the call
    returns (q, None, None).  The dense and fallback routes make the same writes in torch; `last_route` is unchanged.  What it
    saves, graph-replayed (tools/kv_cache_bench.py, table in DESIGN.md 4.4, raw output profiles/kv_cache_bench.txt; the shapes of
    qkv_rope_bench.py, a slot-major cache): two index_copy_ behind the parent cost 5.6 - 7.2 us per layer at any row count, the
    scattered stores 0.1 - 0.4 us at 1 row and 1.4 - 4.4 us at 16 -- 5.4 - 6.1 us less per layer at 1 row, 2.7 - 5.3 us less at 16,
    faster than the copies on all 48 points.

    module(..., k_scale=None, v_scale=None) -- keyword arguments of the module call, `self.qkv_rope(x, ..., k_scale=, v_scale=)`,
    not of `forward`, whose parameter list stays what it was.  Caches of torch.float8_e4m3fn (or uint8: the same bytes) select the fp8 entries
    (sqllm_qkv_rope_cache_fp8_* / sqllm_qkv_rope_norm_cache_fp8_*; include/sqllm_hip.h, sqllm_kv_cache_fp8): each element is
    e4m3_rne(clamp(x / scale, +-448)) of the fp32 value x BEFORE its rounding to 16 bits, one scale per cache (fp8_kv_scale; finite
    and positive floats, calibrated by the caller).  Both scales are required then; scales with a 16-bit cache, or an fp8 cache
    without them, are a ValueError.  The returned k and v are the 16-bit ones, as ever.  The dense and fallback routes make the
    same writes by the same formula in torch."""

    GRAPH_WS_MAX_BYTES = QuantLinearLUTFused.GRAPH_WS_MAX_BYTES

    def __init__(self, q: QuantLinearLUT, k: QuantLinearLUT, v: QuantLinearLUT, head_dim: int, layout: str = "half"):
        super().__init__()
        for name, m in (("q", q), ("k", k), ("v", v)):
            if not isinstance(m, QuantLinearLUT):
                raise TypeError(f"{name} must be a QuantLinearLUT or QuantLinearLUTFused, got {type(m).__name__}")
            if (m.infeatures, m.bits) != (q.infeatures, q.bits):
                raise ValueError(f"q, k and v must share infeatures and bit width: {name} has {m.infeatures} / w{m.bits} against "
                                 f"{q.infeatures} / w{q.bits}")
        if layout not in _ROPE_LAYOUT:
            raise ValueError(f"layout must be 'half' or 'interleaved', got {layout!r}")
        head_dim = int(head_dim)
        if head_dim < 2 or head_dim % 2 or q.outfeatures % head_dim or k.outfeatures % head_dim:
            raise ValueError(f"head_dim must be even, >= 2 and divide the widths of q and k ({q.outfeatures}, {k.outfeatures}), got {head_dim}")
        # by reference: nn.Module.__setattr__ would register them as children (and their buffers under this module's keys)
        self.__dict__["q"], self.__dict__["k"], self.__dict__["v"] = q, k, v
        self.head_dim, self.layout = head_dim, layout

    @property
    def last_route(self):
        """"qkv_rope", "qkv_rope_norm", "dense" or "fallback": the way the most recent forward went (None before the first)."""
        return self.__dict__.get("_last_route")

    def __call__(self, *args, k_scale=None, v_scale=None, **kwargs):
        """forward(*args, **kwargs) with the two scales of an fp8 KV cache.  They are keyword arguments of the module CALL:
        forward's own parameter list is pinned (tests/test_qkv_cache_cpu.py) and stays what it was."""
        if k_scale is None and v_scale is None:
            return super().__call__(*args, **kwargs)
        self.__dict__["_fp8_scales"] = (k_scale, v_scale)
        try:
            return super().__call__(*args, **kwargs)
        finally:
            del self.__dict__["_fp8_scales"]

    def _descriptor(self, dev: int, stream: int):
        """The sqllm_qkv_rope of (device, stream): the members' own pre-marshalled descriptors (QuantLinearLUTFused._descriptor)
        copied side by side, rebuilt when any of them is."""
        return _composite_descriptor(self.__dict__.setdefault("_desc", {}), dev, stream, (self.q, self.k, self.v), self._build)

    @staticmethod
    def _build(entries):
        lq, lk, lv = entries[0][0], entries[1][0], entries[2][0]
        r = _lib.SqllmQkvRope()
        r.q, r.k, r.v = lq.op, lk.op, lv.op  # (copies)
        r.q.mul = r.k.mul = r.v.mul = None
        r.bias_q, r.bias_k, r.bias_v = lq.bias, lk.bias, lv.bias
        return r

    def _check_cache(self, x: torch.Tensor, rows: int, k_cache, v_cache, slots, return_kv: bool) -> bool:
        """The cache arguments of forward: all three or none, and the views as the class docstring wants them."""
        given = [t is not None for t in (k_cache, v_cache, slots)]
        if not any(given):
            if not return_kv:
                raise ValueError("return_kv=False needs a KV cache: k and v would go nowhere")
            return False
        if not all(given):
            raise ValueError("k_cache, v_cache and slots go together: give all three or none")
        D, N = self.head_dim, self.k.outfeatures
        if self.v.outfeatures != N:
            raise ValueError(f"a KV cache needs k and v of one width, got {N} and {self.v.outfeatures}")
        for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
            if not isinstance(t, torch.Tensor) or (t.dtype != x.dtype and t.dtype not in FP8_KV_DTYPES) or t.device != x.device:
                raise ValueError(f"{name} must be a {x.dtype} (or float8_e4m3fn / uint8) tensor on {x.device}, got "
                                 f"{getattr(t, 'dtype', type(t).__name__)} on {getattr(t, 'device', None)}")
            if t.dim() != 3 or t.shape[0] < 1 or t.shape[1] * t.shape[2] != N or t.shape[2] != D or t.stride(2) != 1:
                raise ValueError(f"{name} must be a view [n_slots, {N // D}, {D}] with a contiguous last dimension, got {tuple(t.shape)} "
                                 f"with strides {t.stride()}")
        if k_cache.dtype != v_cache.dtype:
            raise ValueError(f"k_cache and v_cache must have one dtype, got {k_cache.dtype} and {v_cache.dtype}")
        if k_cache.shape != v_cache.shape or k_cache.stride() != v_cache.stride():
            raise ValueError(f"k_cache and v_cache must have equal shape and strides, got {tuple(k_cache.shape)} / {k_cache.stride()} and "
                             f"{tuple(v_cache.shape)} / {v_cache.stride()}")
        if k_cache.stride(0) < D or (k_cache.stride(1) < D and k_cache.shape[1] > 1):
            raise ValueError(f"the strides of a cache view must be at least head_dim = {D}, got {k_cache.stride()}")
        if not isinstance(slots, torch.Tensor) or slots.dtype not in (torch.int32, torch.int64) or slots.numel() != rows or slots.device != x.device:
            raise ValueError(f"slots must be {rows} int32 (or int64) values on {x.device}")
        return True

    def forward(self, x: torch.Tensor, positions: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, norm_weight=None,
                norm_eps: float = 1e-6, k_cache=None, v_cache=None, slots=None, return_kv: bool = True):
        k_scale, v_scale = self.__dict__.get("_fp8_scales", (None, None))  # (the module call's keyword arguments: __call__)
        q, k, v = self.q, self.k, self.v
        K, D, half = q.infeatures, self.head_dim, self.head_dim // 2
        x2, rows, batch = _rows_of(x, K, False)  # (the copy: behind the operand checks)
        norm = norm_weight is not None
        if norm:
            norm_weight = _check_norm_weight(x, norm_weight, K, norm_eps)
        cached = self._check_cache(x, rows, k_cache, v_cache, slots, return_kv)
        dtype = x.dtype
        fp8 = cached and k_cache.dtype in FP8_KV_DTYPES and k_cache.dtype != dtype
        k_scale, v_scale = _check_fp8_scales(fp8, k_scale, v_scale)
        for name, t in (("cos", cos), ("sin", sin)):
            if t.dim() != 2 or t.shape[1] != half or t.shape[0] < 1 or t.shape != cos.shape or t.device != x.device:
                raise ValueError(f"{name} must be [n_pos, {half}] on {x.device}, got {tuple(t.shape)} on {t.device}")
        if positions.dtype not in (torch.int32, torch.int64) or positions.numel() != rows or positions.device != x.device:
            raise ValueError(f"positions must be {rows} int32 (or int64) values on {x.device}")
        lead = x.shape[:-1]
        dense_min_rows = getattr(q, "dense_min_rows", None)
        kernel = dtype in _FRONT_DTYPES and x.is_cuda
        if kernel and not x2.is_contiguous():
            x2 = x2.contiguous()
        if not kernel or (dense_min_rows is not None and rows >= dense_min_rows):
            pos = positions.reshape(-1)
            if kernel:  # (fp32 from end to end, as the epilogue's dense route)
                self.__dict__["_last_route"] = "dense"
                sums = _fp32_sums((q, k, v), x2.float() if not norm else _torch_rmsnorm(x2, norm_weight, norm_eps))
            else:
                self.__dict__["_last_route"] = "fallback"
                xin = x2 if not norm else _torch_rmsnorm(x2, norm_weight, norm_eps)  # (fp32 sums from fp32 xn)
                sums = [QuantLinearLUT.forward(m, xin) for m in (q, k, v)]
            oq = _torch_rope(sums[0], pos, cos, sin, D, self.layout, dtype)
            ok32 = _torch_rope(sums[1], pos, cos, sin, D, self.layout, torch.float32)  # (the value before its one rounding)
            ok = ok32.to(dtype)
            ov = sums[2].to(dtype)
            if cached:
                if fp8:  # (the same fp32 values, rounded once, straight to fp8)
                    _torch_cache_write_fp8(k_cache, slots, ok32, k_scale)
                    _torch_cache_write_fp8(v_cache, slots, sums[2].float(), v_scale)
                else:
                    _torch_cache_write(k_cache, slots, ok)
                    _torch_cache_write(v_cache, slots, ov)
                if not return_kv:
                    return oq.reshape(*lead, -1), None, None
            return oq.reshape(*lead, -1), ok.reshape(*lead, -1), ov.reshape(*lead, -1)
        if cos.dtype != torch.float32 or sin.dtype != torch.float32 or not cos.is_contiguous() or not sin.is_contiguous():
            raise ValueError("cos and sin must be contiguous fp32 tensors")
        pos = _int32_vector(positions)
        self.__dict__["_last_route"] = "qkv_rope_norm" if norm else "qkv_rope"
        dev = x.get_device()
        outs = [torch.empty((rows, m.outfeatures), dtype=dtype, device=x.device) if return_kv or m is q else None for m in (q, k, v)]
        stream = quant_cuda._raw_stream(dev)
        r, ref, _keep = self._descriptor(dev, stream)
        r.q.batch = r.k.batch = r.v.batch = batch
        r.q.vec = r.k.vec = r.v.vec = x2.data_ptr()
        r.out_q, r.out_k, r.out_v = [o.data_ptr() if o is not None else None for o in outs]
        r.cos, r.sin, r.positions = cos.data_ptr(), sin.data_ptr(), pos.data_ptr()
        r.n_pos, r.head_dim, r.layout = cos.shape[0], D, _ROPE_LAYOUT[self.layout]
        ws = _workspace_of(self, _lib.qkv_rope_workspace_bytes, (q.outfeatures, k.outfeatures, v.outfeatures, batch),
                           q._buffers["qweight"].device, stream)
        r.workspace = ws.data_ptr()
        args = (ref,)
        if norm:
            args += (_norm_ref(self.__dict__.setdefault("_norm", {}), (dev, stream), norm_weight, norm_eps),)
        if cached:
            sl = _int32_vector(slots)
            kv = self.__dict__.setdefault("_kv8" if fp8 else "_kv", {})
            args += (_kv_ref(kv, (dev, stream), k_cache, v_cache, sl, D, (k_scale, v_scale) if fp8 else None),)
        quant_cuda._launch(quant_cuda._fn(_FRONT_ENTRY["qkv_rope", norm, cached, fp8, dtype]), dev, args)
        return tuple(o.reshape(*lead, -1) if o is not None else None for o in outs)


def fuse_qkv_rope(module: nn.Module, q: str = "q_proj", k: str = "k_proj", v: str = "v_proj", head_dim=None) -> int:
    """Give every submodule of `module` that has the attributes `q`, `k` and `v` -- three quantised layers of equal
    infeatures and bit width -- an attribute `qkv_rope`, a QuantQKVRopeFused over them (not a child: the module tree, the
    state dict and every `forward` stay as they are; an attention forward calls `self.qkv_rope(x, positions, cos, sin)`
    where it called the three projections and the rotary step).  `head_dim`: the submodule's own `head_dim`
    attribute where None.  Submodules without one, or whose widths it does not divide, are left alone.  Returns the count."""
    n = 0
    for m in module.modules():
        mq, mk, mv = getattr(m, q, None), getattr(m, k, None), getattr(m, v, None)
        if not all(isinstance(t, QuantLinearLUT) for t in (mq, mk, mv)):
            continue
        if any((t.infeatures, t.bits) != (mq.infeatures, mq.bits) for t in (mk, mv)):
            continue
        d = head_dim if head_dim is not None else getattr(m, "head_dim", None)
        if not isinstance(d, int) or d < 2 or d % 2 or mq.outfeatures % d or mk.outfeatures % d:
            continue
        m.__dict__["qkv_rope"] = QuantQKVRopeFused(mq, mk, mv, d)
        n += 1
    return n


# The four kinds of DecodeAttention._launch, kind = 2 * (several new tokens per sequence) + (fp8 cache): the descriptor and the
# entry of each dtype
_ATTN_KINDS = (
    (_lib.SqllmAttnDecode, {torch.float16: "sqllm_attn_decode_f16", torch.bfloat16: "sqllm_attn_decode_bf16"}),
    (_lib.SqllmAttnDecodeFp8, {torch.float16: "sqllm_attn_decode_fp8_f16", torch.bfloat16: "sqllm_attn_decode_fp8_bf16"}),
    (_lib.SqllmAttnAppend, {torch.float16: "sqllm_attn_append_f16", torch.bfloat16: "sqllm_attn_append_bf16"}),
    (_lib.SqllmAttnAppendFp8, {torch.float16: "sqllm_attn_append_fp8_f16", torch.bfloat16: "sqllm_attn_append_fp8_bf16"}),
)
# ... and with a sliding window (DecodeAttention(..., window=)): the one-query descriptors, kind = (fp8 cache)
_ATTN_WINDOW_ENTRIES = (
    {torch.float16: "sqllm_attn_decode_window_f16", torch.bfloat16: "sqllm_attn_decode_window_bf16"},
    {torch.float16: "sqllm_attn_decode_window_fp8_f16", torch.bfloat16: "sqllm_attn_decode_window_fp8_bf16"},
)
_ATTN_DTYPES = (torch.float16, torch.bfloat16)


ATTN_PARTITION = _lib.ATTN_PARTITION  # keys per partition of the decode attention's kernel (SQLLM_ATTN_PARTITION)
ATTN_APPEND_MAX_Q_LEN = 16  # new tokens per sequence the append kernels serve


def append_as_decode_rows(block_table: torch.Tensor, seq_lens: torch.Tensor, q_len: int, q_lens, block_size: int):
    """The one-query call that sqllm_attn_append (include/sqllm_hip.h) is defined by: (table [batch * q_len, max_blocks],
    lengths [batch * q_len]) for DecodeAttention without q_len -- row b * q_len + t carries sequence b's table row and
    L(b, t) = seq_lens[b] - (n_b - 1 - t), n_b = q_lens[b] (q_len where q_lens is None, 0 where negative).  Padding rows
    (t >= n_b) and L <= 0 become length 0, the +0 row; L beyond max_blocks * block_size and the rows of a sequence with
    n_b > q_len become max_blocks * block_size + 1, the NaN row.  Dtypes and device are the operands'.  The torch fallback
    of DecodeAttention(..., q_len=) runs on it, and it is the emulation the append kernels are measured and tested against:
    correct, but K and V are read q_len times."""
    T, B = int(q_len), block_table.shape[0]
    dev = seq_lens.device
    seq = seq_lens.reshape(-1).long()
    n = torch.full_like(seq, T) if q_lens is None else q_lens.reshape(-1).long()
    over = (n > T)[:, None]
    n = n.clamp(min=0)
    t = torch.arange(T, device=dev)[None, :]
    cap = block_table.shape[1] * int(block_size)
    nan_len = min(cap + 1, (1 << 31) - 1)
    lens = (seq[:, None] - (n[:, None] - 1 - t)).clamp(min=0, max=nan_len)
    lens = torch.where(t < n[:, None], lens, torch.zeros_like(lens))
    lens = torch.where(over, torch.full_like(lens, nan_len), lens)
    table = block_table[:, None, :].expand(B, T, block_table.shape[1]).reshape(B * T, block_table.shape[1])
    return table, lens.reshape(-1).to(seq_lens.dtype)


def static_cache_blocks(batch: int, n_kv_heads: int, device=None) -> torch.Tensor:
    """The int32 block table [batch, 1] of a head-major static cache [B, H, S, D] seen through kv_cache_view(cache, "bhsd"),
    for DecodeAttention with block_size = S: block_table[b, 0] = b * H, so that key p of row b lies in slot b * H * S + p --
    the slot static_cache_slots gave the front for it."""
    return (torch.arange(int(batch), dtype=torch.int32, device=device) * int(n_kv_heads)).reshape(-1, 1)


def ring_block_table(batch: int, window: int, block_size: int, max_len: int, device=None) -> torch.Tensor:
    """The int32 block table [batch, ceil(max_len / block_size)] of a ROLLING buffer for DecodeAttention(..., window=window):
    logical block j of row b is physical block b * R + j % R, with R = ceil(window / block_size) + 1, so a sequence of any
    length up to max_len lives in R blocks (batch * R blocks in all; the front writes position p of row b into slot
    table[b, p // block_size] * block_size + p % block_size, as with any table).  Why R suffices: writing position p overwrites
    position p - R * block_size, and R * block_size >= window + block_size, so with L = p + 1 keys that position is below
    lo = L - window -- it has left the window, at this step and at every later one; the blocks below lo / block_size are never
    read (include/sqllm_hip.h, sliding-window decode attention).  Without a window the table is wrong: old keys are gone."""
    batch, window, block_size, max_len = int(batch), int(window), int(block_size), int(max_len)
    if batch < 1 or window < 1 or block_size < 1 or max_len < 1:
        raise ValueError(f"batch, window, block_size and max_len must be positive, got {batch}, {window}, {block_size}, {max_len}")
    R = (window + block_size - 1) // block_size + 1
    j = torch.arange((max_len + block_size - 1) // block_size, dtype=torch.int32, device=device)
    b = torch.arange(batch, dtype=torch.int32, device=device)
    return (b[:, None] * R + (j % R)[None, :]).contiguous()


def _torch_attn_decode(q, k_cache, v_cache, block_table, seq_lens, block_size, n_heads, n_kv_heads, head_dim, scale, dtype,
                       k_scale=None, v_scale=None, window=None):
    """The formulas of sqllm_attn_decode (include/sqllm_hip.h) in torch: fp32, rounded once to `dtype`; the +0 row, the NaN
    rows; unaddressed slots never enter a result.  q: [rows, n_heads * head_dim].  With `k_scale` and `v_scale` the caches
    hold e4m3fn bytes (sqllm_attn_decode_fp8): scale * k_scale is the score's scale, rounded once to fp32, and v_scale
    multiplies the sum over the keys.  With `window` a row of length L attends the keys [max(0, L - window), L) only: table
    entries and slots below them are never looked at."""
    rows, D, G = q.shape[0], head_dim, n_heads // n_kv_heads
    n_slots, H = k_cache.shape[0], k_cache.shape[1]
    ss, hs = k_cache.stride(0), (k_cache.stride(1) if H > 1 else D)
    dev = q.device
    lens = seq_lens.reshape(-1).long()
    cap = block_table.shape[1] * int(block_size)
    over = lens > cap
    use = torch.where(over, torch.zeros_like(lens), lens.clamp(min=0))
    S = max(int(use.max().item()), 1)
    p = torch.arange(S, device=dev)
    valid = p[None, :] < use[:, None]  # [rows, S]
    if window is not None:
        valid = valid & (p[None, :] >= (use - int(window))[:, None])
    entry = block_table.long()[:, (p // block_size).clamp(max=block_table.shape[1] - 1)]  # [rows, S]
    slot = entry * int(block_size) + (p % block_size)[None, :]
    bad = (valid & ((slot < 0) | (slot >= n_slots))).any(dim=1)
    valid = valid & ~bad[:, None]
    slot = torch.where(valid, slot, torch.zeros_like(slot))
    at = slot[:, :, None, None] * ss + torch.arange(H, device=dev)[None, None, :, None] * hs + torch.arange(D, device=dev)[None, None, None, :]
    zero = torch.zeros((), dtype=torch.float32, device=dev)

    fp8 = k_scale is not None

    def gather(cache):
        if fp8:  # (through the bytes: torch has no indexing for float8)
            cache = cache.view(torch.uint8)
        flat = cache.as_strided(((n_slots - 1) * ss + (H - 1) * hs + D,), (1,), cache.storage_offset())
        got = flat[at.reshape(-1)]
        got = got.view(torch.float8_e4m3fn).float() if fp8 else got.float()
        return torch.where(valid[:, :, None, None], got.reshape(at.shape), zero)  # [rows, S, H, D]

    k, v = gather(k_cache), gather(v_cache)
    qf = q.float().reshape(rows, n_kv_heads, G, D)
    if fp8:
        scale = float(torch.tensor(float(scale), dtype=torch.float32) * torch.tensor(float(k_scale), dtype=torch.float32))
    s = torch.einsum("bhgd,bshd->bhgs", qf, k) * float(scale)
    s = torch.where(valid[:, None, None, :], s, torch.full((), float("-inf"), dtype=torch.float32, device=dev))
    m = s.max(dim=-1, keepdim=True).values
    m = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), m)  # (a row without keys: w = 0 everywhere)
    w = torch.where(valid[:, None, None, :], torch.exp(s - m), zero)
    o = torch.einsum("bhgs,bshd->bhgd", w, v)
    if fp8:
        o = o * torch.tensor(float(v_scale), dtype=torch.float32, device=dev)
    o = o / w.sum(dim=-1, keepdim=True)
    o = o.reshape(rows, n_heads * D)
    o = torch.where((lens <= 0)[:, None], zero, o)
    o = torch.where((over | bad)[:, None], torch.full((), float("nan"), dtype=torch.float32, device=dev), o)
    return o.to(dtype)


class DecodeAttention(nn.Module):
    """Decode attention -- ONE new query per sequence -- over the KV cache QuantQKVRopeFused writes, as HIP kernels
    (sqllm_attn_decode_f16 / _bf16; include/sqllm_hip.h, sqllm_attn_decode: the formulas, the fixed partitions of
    ATTN_PARTITION keys and their order, the +0 and NaN rows, non-finite values): the step between the front's q and o_proj.
    It reads K and V once for all the query heads of a kv group, only the keys below each row's length, and follows lengths
    and block tables in device memory -- no mask tensor, no expanded heads.

    DecodeAttention(n_heads, n_kv_heads, head_dim, scale=None, block_size=None, window=None); scale: 1 / sqrt(head_dim) where
    None.  No parameters, no buffers, no state-dict keys.

    forward(q, k_cache, v_cache, block_table, seq_lens, out=None, block_size=None) -> [..., n_heads * head_dim].
    `q`: [..., n_heads * head_dim] with a contiguous last dimension, one row per sequence (the front's q).  `k_cache`,
    `v_cache`: the 3-D views [n_slots, n_kv_heads, head_dim] of kv_cache_view, as QuantQKVRopeFused takes them (q's dtype and
    device, equal shape and strides, stride(-1) == 1; overlapping as_strided views are allowed).  `block_table`: int32
    [rows, max_blocks] on q's device; key p of row b lies in slot block_table[b, p // block_size] * block_size + p % block_size
    (a paged cache's own table; static_cache_blocks for a "bhsd" cache, with block_size = S).  `seq_lens`: int32 [rows], the
    number of keys each row attends to -- position + 1 when the front wrote the new token in the same step.  Both are used
    WITHOUT a copy, so a captured graph follows them updated in place; int64 is converted, which costs a kernel each (as for
    positions).  `block_size`: per call, or the constructor's.  `out`: a [rows, n_heads * head_dim] tensor of q's dtype with a
    contiguous last dimension to be overwritten, or None for a new one.

    A row with seq_lens <= 0 is +0; a row whose length exceeds max_blocks * block_size, or whose table leads outside the cache,
    is NaN (nothing outside the cache is read).  Slots the table and the lengths do not address never influence a result.

    fp16 / bf16 GPU tensors with head_dim 64 or 128, n_heads / n_kv_heads of 1 to 8 and at most 64 rows take the kernels
    (`last_route` "attn_decode"): two launches, one when max_blocks * block_size <= ATTN_PARTITION; one workspace per
    (device, stream) by the rules of QuantLinearLUTFused._workspace.  CPU tensors, other dtypes and other shapes compute the
    same formulas in torch, in fp32 with one rounding (`last_route` "fallback").

    Speed, graph-replayed on an MI355X against torch SDPA over the static cache with a length mask (tools/attn_decode_bench.py,
    table in DESIGN.md 4.4, raw output profiles/attn_decode_bench.txt; 32/32 and 32/8 heads of 128, 1 / 4 / 16 rows, 128 / 1024 /
    4096 keys in a cache of 4096, static and paged, fp16 / bf16): 9.7 - 207 us per call against 160 - 1761 us, faster on all 72
    points; ABOVE the `3 us + bytes / 4.8 TB/s` per-launch fit on all but 32/32 at 4096 keys with 4 and 16 rows (5.3 TB/s there),
    by up to 3.7x at 16 rows of 128 keys.

    forward(..., k_scale=None, v_scale=None).  Caches of torch.float8_e4m3fn (or uint8: the same bytes), as QuantQKVRopeFused
    writes them with the same two scales, take the kernels for byte caches (sqllm_attn_decode_fp8_f16 / _bf16; include/sqllm_hip.h,
    sqllm_attn_decode_fp8): float(k) = k_scale * f32(byte), float(v) = v_scale * f32(byte) in the formulas above, half the bytes
    read.  Both scales are required then; scales with a 16-bit cache, or an fp8 cache without them, are a ValueError.  The torch
    fallback dequantises.  Speed against the 16-bit kernel: tools/attn_decode_bench.py --cache fp8, DESIGN.md 4.4.

    forward(..., q_len=None, q_lens=None).  SEVERAL new tokens per sequence -- the verification step of speculative decoding, a
    chunk of a prompt -- behind a front that wrote all of them (include/sqllm_hip.h, sqllm_attn_append): `q` is
    [batch * q_len, W] or [batch, q_len, W], row b * q_len + t new token t of sequence b; `block_table` [batch, max_blocks] and
    `seq_lens` [batch] are per SEQUENCE, seq_lens counting the new tokens too; `q_lens`: int32 [batch] on the device (used
    without a copy; int64 is converted) or None, the real tokens n_b of each sequence -- rows t >= n_b are padding and +0,
    n_b > q_len makes the sequence's rows NaN.  Token t attends the keys below seq_lens[b] - (n_b - 1 - t), and its row holds
    exactly the bits the one-query call gives a row of that length: append_as_decode_rows is that call's table and lengths.
    The defaults keep today's call.  q_len 1 to 16 and batch * q_len <= 64 on the served shapes take kernels; which ones is
    routed by measurement and changes no bit (`append_route`: "auto", or "kernel" / "emulate" to force): the append kernels
    (`last_route` "attn_append": two kernel nodes, K and V read once per sequence) everywhere but over an fp8 cache at 64 rows,
    which takes the expansion on the one-query kernels (`last_route` "attn_decode": append_as_decode_rows in every call, a
    dozen small kernels and 24 - 34 us in a replayed graph, then the one-query kernels).  Kernel against kernel, with the
    expansion prepared outside the timed region, the one-query kernels are the faster ones on 313 of 384 measured points (the
    repeated rows hit the caches; the append kernels win by up to 3.0x with 32/32 heads, a 16-bit cache and 4096 keys); end to
    end, as a caller of this module pays, the append route is faster on 361 of 384, by 0.90x - 3.2x (tools/attn_append_bench.py,
    DESIGN.md 4.4, profiles/attn_append_bench.txt).  Everything else is the torch fallback on the expansion.

    DecodeAttention(..., window=W): a SLIDING WINDOW (Mistral's `sliding_window`; an int of at least 1, anything else is a
    ValueError; None is the module above, bit for bit and launch for launch).  A row of length L attends the keys
    [max(0, L - W), L) -- the query's own key included, W keys in all -- through kernels of their own
    (sqllm_attn_decode_window_f16 / _bf16 / _fp8_f16 / _fp8_bf16; include/sqllm_hip.h, sliding-window decode attention;
    `last_route` "attn_window"): the launch, the workspace and the bytes read are sized by the window, not by the table.  Rows
    with L <= W hold exactly the bits of the module without a window.  Table entries and slots behind the window are never
    looked at: the caller may free or reuse those blocks, and ring_block_table is the table of a rolling buffer.  The torch
    fallback applies the same window.  With `q_len=` a windowed module ALWAYS takes the expansion (append_as_decode_rows) on
    the windowed one-query kernels -- row (b, t) attends [max(0, L(b,t) - W), L(b,t)) -- and `append_route` is ignored: the
    append kernels have no window."""

    GRAPH_WS_MAX_BYTES = QuantLinearLUTFused.GRAPH_WS_MAX_BYTES
    append_route = "auto"  # forward(..., q_len=): "auto" routes by measurement, "kernel" / "emulate" force one way (same bits)

    def __init__(self, n_heads: int, n_kv_heads: int, head_dim: int, scale=None, block_size=None, window=None):
        super().__init__()
        n_heads, n_kv_heads, head_dim = int(n_heads), int(n_kv_heads), int(head_dim)
        if n_heads < 1 or n_kv_heads < 1 or head_dim < 1 or n_heads % n_kv_heads:
            raise ValueError(f"n_heads must be a positive multiple of n_kv_heads and head_dim positive, got {n_heads}, {n_kv_heads}, {head_dim}")
        scale = head_dim ** -0.5 if scale is None else float(scale)
        if scale != scale or scale in (float("inf"), float("-inf")):
            raise ValueError(f"scale must be finite, got {scale}")
        if block_size is not None and int(block_size) < 1:
            raise ValueError(f"block_size must be positive, got {block_size}")
        self.n_heads, self.n_kv_heads, self.head_dim, self.scale = n_heads, n_kv_heads, head_dim, scale
        self.block_size = None if block_size is None else int(block_size)
        if window is not None and (isinstance(window, bool) or not isinstance(window, int) or not 1 <= window <= (1 << 31) - 1):
            raise ValueError(f"window must be None or an int in [1, 2^31), got {window!r}")
        self.window = window

    @property
    def last_route(self):
        """"attn_decode", "attn_append", "attn_window" or "fallback": the way the most recent forward went (None before the first)."""
        return self.__dict__.get("_last_route")

    def _check_cache(self, q: torch.Tensor, k_cache, v_cache) -> None:
        """The cache views as QuantQKVRopeFused._check_cache wants them."""
        D, H = self.head_dim, self.n_kv_heads
        for name, t in (("k_cache", k_cache), ("v_cache", v_cache)):
            if not isinstance(t, torch.Tensor) or (t.dtype != q.dtype and t.dtype not in FP8_KV_DTYPES) or t.device != q.device:
                raise ValueError(f"{name} must be a {q.dtype} (or float8_e4m3fn / uint8) tensor on {q.device}, got "
                                 f"{getattr(t, 'dtype', type(t).__name__)} on {getattr(t, 'device', None)}")
            if t.dim() != 3 or t.shape[0] < 1 or t.shape[1] != H or t.shape[2] != D or t.stride(2) != 1:
                raise ValueError(f"{name} must be a view [n_slots, {H}, {D}] with a contiguous last dimension, got {tuple(t.shape)} "
                                 f"with strides {t.stride()}")
        if k_cache.dtype != v_cache.dtype:
            raise ValueError(f"k_cache and v_cache must have one dtype, got {k_cache.dtype} and {v_cache.dtype}")
        if k_cache.shape != v_cache.shape or k_cache.stride() != v_cache.stride():
            raise ValueError(f"k_cache and v_cache must have equal shape and strides, got {tuple(k_cache.shape)} / {k_cache.stride()} and "
                             f"{tuple(v_cache.shape)} / {v_cache.stride()}")
        if k_cache.stride(0) < D or (k_cache.stride(1) < D and H > 1):
            raise ValueError(f"the strides of a cache view must be at least head_dim = {D}, got {k_cache.stride()}")

    def _check_operands(self, q, k_cache, v_cache, block_table, seq_lens, out, block_size, k_scale, v_scale, T, q_lens):
        """Every operand check of forward, for one query per sequence (T None) and for T new tokens per sequence.
        -> (q2 [rows, W] with rows at least W apart, rows, block size, fp8 cache?, k_scale, v_scale).  The number of sequences is
        block_table.shape[0] from here on: rows for one query per sequence, rows / T otherwise."""
        D, H = self.head_dim, self.n_kv_heads
        W = self.n_heads * D
        if q.shape[-1] != W or q.stride(-1) != 1:
            raise ValueError(f"q must be [..., {W}] with a contiguous last dimension, got {tuple(q.shape)} with strides {q.stride()}")
        if T is not None and (q.dim() not in (2, 3) or (q.dim() == 3 and q.shape[1] != T)):
            raise ValueError(f"q must be [batch * {T}, {W}] or [batch, {T}, {W}], got {tuple(q.shape)}")
        bs = self.block_size if block_size is None else int(block_size)
        if bs is None or bs < 1:
            raise ValueError("block_size must be given, at construction or per call, and be positive")
        self._check_cache(q, k_cache, v_cache)
        fp8 = k_cache.dtype in FP8_KV_DTYPES and k_cache.dtype != q.dtype
        k_scale, v_scale = _check_fp8_scales(fp8, k_scale, v_scale)
        if fp8 and not math.isfinite(float(torch.tensor(self.scale, dtype=torch.float32) * torch.tensor(k_scale, dtype=torch.float32))):
            raise ValueError(f"scale * k_scale must be finite in fp32, got {self.scale} * {k_scale}")
        q2 = q if q.dim() == 2 else q.reshape(-1, W)
        rows = q2.shape[0]
        if T is None:
            if rows < 1:
                raise ValueError("q has no rows")
            batch, per_table, per_value = rows, "", ""
        else:
            if rows < 1 or rows % T:
                raise ValueError(f"q must have a positive multiple of q_len = {T} rows, got {rows}")
            batch, per_table, per_value = rows // T, ": one row per sequence", ": one per sequence"
        if (not isinstance(block_table, torch.Tensor) or block_table.dtype not in (torch.int32, torch.int64) or block_table.dim() != 2
                or block_table.shape[0] != batch or block_table.shape[1] < 1 or block_table.device != q.device):
            raise ValueError(f"block_table must be int32 (or int64) [{batch}, max_blocks] on {q.device}{per_table}")
        if (not isinstance(seq_lens, torch.Tensor) or seq_lens.dtype not in (torch.int32, torch.int64) or seq_lens.numel() != batch
                or seq_lens.device != q.device):
            raise ValueError(f"seq_lens must be {batch} int32 (or int64) values on {q.device}{per_value}")
        if q_lens is not None and (not isinstance(q_lens, torch.Tensor) or q_lens.dtype not in (torch.int32, torch.int64)
                                   or q_lens.numel() != batch or q_lens.device != q.device):
            raise ValueError(f"q_lens must be {batch} int32 (or int64) values on {q.device}{per_value}")
        if out is not None:
            if (not isinstance(out, torch.Tensor) or out.dtype != q.dtype or out.device != q.device or out.shape != (rows, W)
                    or out.stride(1) != 1 or (rows > 1 and out.stride(0) < W)):
                raise ValueError(f"out must be a {q.dtype} [{rows}, {W}] tensor on {q.device} with a contiguous last dimension")
        if rows > 1 and q2.stride(0) < W:
            q2 = q2.contiguous()
        return q2, rows, bs, fp8, k_scale, v_scale

    @staticmethod
    def _int32_operands(block_table, seq_lens, q_lens):
        """The table and the lengths as the kernels read them: int32 (a conversion is a kernel), table rows at least a row apart,
        vectors contiguous; what already is, is used WITHOUT a copy."""
        bt = block_table if block_table.dtype == torch.int32 else block_table.to(torch.int32)
        if bt.stride(1) != 1 or (bt.shape[0] > 1 and bt.stride(0) < bt.shape[1]):
            bt = bt.contiguous()
        return bt, _int32_vector(seq_lens), (None if q_lens is None else _int32_vector(q_lens))

    def _launch(self, kind: int, q2, k_cache, v_cache, bt, sl, ql, T, out, bs, k_scale, v_scale) -> torch.Tensor:
        """Kind `kind` of _ATTN_KINDS on the current stream: the workspace, the kind's descriptor of this (device, stream), the
        entry.  bt has one row per sequence.  -> out, or a new [rows, W]."""
        D, H, HQ = self.head_dim, self.n_kv_heads, self.n_heads
        rows, W = q2.shape
        batch, max_blocks = bt.shape
        dev = q2.get_device()
        o = out if out is not None else torch.empty((rows, W), dtype=q2.dtype, device=q2.device)
        stream = quant_cuda._raw_stream(dev)
        window = self.window
        if window is None:
            ws = _workspace_of(self, _lib.attn_decode_workspace_bytes, (rows, HQ, D, max_blocks, bs), q2.device)
        else:  # (kind 0 or 1: the one-query descriptors)
            ws = _workspace_of(self, _lib.attn_window_workspace_bytes, (rows, HQ, D, max_blocks, bs, window), q2.device)
        struct, entries = _ATTN_KINDS[kind]
        if window is not None:
            entries = _ATTN_WINDOW_ENTRIES[kind]
        descs = self.__dict__.setdefault("_desc", {})
        hit = descs.get((kind, dev, stream))
        if hit is None:
            a = struct()
            hit = descs[(kind, dev, stream)] = (a, ctypes.byref(a))
        a, ref = hit
        a.q, a.out, a.k_cache, a.v_cache = q2.data_ptr(), o.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr()
        a.block_table, a.seq_lens = bt.data_ptr(), sl.data_ptr()
        a.batch, a.n_q_heads, a.n_kv_heads, a.head_dim = batch, HQ, H, D
        a.n_slots, a.block_size, a.max_blocks = k_cache.shape[0], bs, max_blocks
        a.table_stride = bt.stride(0) if batch > 1 else max_blocks
        a.slot_stride = k_cache.stride(0)
        a.head_stride = k_cache.stride(1) if H > 1 else D  # (one head: its stride is anything, and never used)
        a.q_stride = q2.stride(0) if rows > 1 else W
        a.out_stride = o.stride(0) if rows > 1 else W
        a.scale, a.workspace = self.scale, ws.data_ptr()
        if kind & 1:
            a.k_scale, a.v_scale = k_scale, v_scale
        if kind & 2:
            a.q_lens, a.q_len = (None if ql is None else ql.data_ptr()), T
        quant_cuda._launch(quant_cuda._fn(entries[q2.dtype]), dev, (ref,) if window is None else (ref, window))
        return o

    def forward(self, q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, block_table: torch.Tensor, seq_lens: torch.Tensor,
                out=None, block_size=None, k_scale=None, v_scale=None, q_len=None, q_lens=None) -> torch.Tensor:
        D, H, HQ = self.head_dim, self.n_kv_heads, self.n_heads
        W = HQ * D
        T = None  # one query per sequence; forward(..., q_len=T, q_lens=None): T new tokens per sequence (sqllm_attn_append_*)
        if q_len is not None or q_lens is not None:
            if q_len is None:
                raise ValueError("q_lens needs q_len, the rows per sequence")
            T = int(q_len)
            if T < 1:
                raise ValueError(f"q_len must be positive, got {q_len}")
        q2, rows, bs, fp8, k_scale, v_scale = self._check_operands(q, k_cache, v_cache, block_table, seq_lens, out, block_size,
                                                                   k_scale, v_scale, T, q_lens)
        kernel = (q.dtype in _ATTN_DTYPES and q.is_cuda and D in (64, 128) and HQ // H <= 8 and rows <= 64
                  and (T is None or T <= ATTN_APPEND_MAX_Q_LEN))
        if not kernel:
            self.__dict__["_last_route"] = "fallback"
            table, lens = (block_table, seq_lens) if T is None else append_as_decode_rows(block_table, seq_lens, T, q_lens, bs)
            o = _torch_attn_decode(q2, k_cache, v_cache, table, lens, bs, HQ, H, D, self.scale, q.dtype, k_scale, v_scale, self.window)
            if out is not None:
                out.copy_(o)
                return out
            return o.reshape(*q.shape[:-1], W)
        if T is not None:
            if self.append_route not in ("auto", "kernel", "emulate"):
                raise ValueError(f"append_route must be 'auto', 'kernel' or 'emulate', got {self.append_route!r}")
            # routed by measurement, END TO END (tools/attn_append_bench.py `route_emul` against `append`): the expansion
            # below is a dozen small kernels in every call, 24 - 34 us in a replayed graph, which the one-query kernels win back only
            # over an fp8 cache at 64 rows (by up to 10 %); everywhere else the append kernels are faster.  The same bits either way.
            # (a window: the append kernels have none -- always the expansion, on the windowed one-query kernels)
            if self.window is not None or self.append_route == "emulate" or (self.append_route == "auto" and fp8 and rows >= 64):
                table, lens = append_as_decode_rows(block_table, seq_lens, T, q_lens, bs)
                o = self.forward(q2, k_cache, v_cache, table, lens, out=out, block_size=bs, k_scale=k_scale if fp8 else None,
                                 v_scale=v_scale if fp8 else None)  # (`last_route` "attn_decode", "attn_window" with a window)
                return o if out is not None else o.reshape(*q.shape[:-1], W)
        bt, sl, ql = self._int32_operands(block_table, seq_lens, q_lens)
        self.__dict__["_last_route"] = "attn_append" if T is not None else "attn_decode" if self.window is None else "attn_window"
        o = self._launch(2 * (T is not None) + fp8, q2, k_cache, v_cache, bt, sl, ql, T, out, bs, k_scale, v_scale)
        return o if out is not None else o.reshape(*q.shape[:-1], W)


def fuse_decode_attention(module: nn.Module, n_heads=None, n_kv_heads=None, window=None) -> int:
    """Give every submodule of `module` that carries a `qkv_rope` (fuse_qkv_rope) an attribute `attend_decode`, a
    DecodeAttention for its heads: head_dim the front's, n_heads and n_kv_heads the widths of the front's q and k over it
    (or the arguments).  Not a child, through `__dict__`: the module tree, the state dict and every `forward` stay as they
    are; an attention forward calls `self.attend_decode(q, k_cache, v_cache, block_table, seq_lens)` between `self.qkv_rope`
    and `o_proj`.  `window`: the model's sliding window (Mistral: model.config.sliding_window), passed to every
    DecodeAttention; None: no window.  Returns the count."""
    n = 0
    for m in module.modules():
        front = m.__dict__.get("qkv_rope")
        if not isinstance(front, QuantQKVRopeFused):
            continue
        d = front.head_dim
        hq = int(n_heads) if n_heads is not None else front.q.outfeatures // d
        hk = int(n_kv_heads) if n_kv_heads is not None else front.k.outfeatures // d
        if hq < 1 or hk < 1 or hq % hk:
            continue
        m.__dict__["attend_decode"] = DecodeAttention(hq, hk, d, window=window)
        n += 1
    return n


def _norm_of(m):
    """(weight, eps) of an RMSNorm-like module: a `weight` and a `variance_epsilon` (or `eps`); None for anything else."""
    w = getattr(m, "weight", None)
    eps = getattr(m, "variance_epsilon", None)
    if eps is None:
        eps = getattr(m, "eps", None)
    if not isinstance(w, torch.Tensor) or w.dim() != 1 or eps is None or getattr(m, "bias", None) is not None:
        return None
    return w, float(eps)


def fuse_norm_fronts(module: nn.Module, input_norm: str = "input_layernorm", post_norm: str = "post_attention_layernorm",
                     down_name: str = "down_proj") -> int:
    """Hand the two RMSNorms of every decoder layer of `module` to the kernels behind them.  On every submodule that has
      * an attribute `input_norm` -- a norm with a 1-D `weight`, no bias and a `variance_epsilon` (or `eps`) -- next to a
        child that carries `qkv_rope` (fuse_qkv_rope), that child gets `front_norm` = (weight, eps);
      * an attribute `post_norm` of the same kind next to a child that carries `gated` (fuse_gated_mlps), that child gets
        `front_norm` = (weight, eps), `forward_normed(x)` = down(gated(x, weight, eps)) -- down: its attribute `down_name` -- x the UN-normalised hidden
        state -- and, where it has `forward_residual`, `forward_normed_residual(x, residual)`.
    The weight is attached BY REFERENCE, through `__dict__`: module tree, state dict and every existing `forward` are
    untouched; the decoder layer's own forward chooses to call the normed forms (INTEGRATION.md shows it).  LayerNorm
    (a bias, a mean) is not RMSNorm and is left alone.  Returns the number of fronts attached."""
    n = 0
    for layer in module.modules():
        for norm_name, mark in ((input_norm, "qkv_rope"), (post_norm, "gated")):
            nm = _norm_of(getattr(layer, norm_name, None)) if hasattr(layer, norm_name) else None
            if nm is None:
                continue
            for child in layer.children():
                fused = child.__dict__.get(mark)
                if fused is None:
                    continue
                K = fused.q.infeatures if mark == "qkv_rope" else fused.gate.infeatures
                if nm[0].numel() != K:
                    continue
                child.__dict__["front_norm"] = nm
                if mark == "gated":
                    down = getattr(child, down_name, None)  # (the layer fuse_gated_mlps put behind the gated front)
                    if down is None:
                        del child.__dict__["front_norm"]
                        continue
                    child.__dict__["forward_normed"] = (lambda g, d, nm: lambda x: d(g(x, nm[0], nm[1])))(fused, down, nm)
                    if "forward_residual" in child.__dict__:
                        child.__dict__["forward_normed_residual"] = (
                            lambda g, d, nm: lambda x, residual: d(g(x, nm[0], nm[1]), residual=residual))(fused, down, nm)
                n += 1
    return n


def make_quant_lut(module, names, bits, name="", include_sparse=False, numvals=None, topX=0, balanced=False,
                   num_nonzero_per_thread=10):
    """Swap the nn.Linear children listed in `names` for QuantLinearLUT, recursively
    (reference: quant.py:386-435)."""
    if isinstance(module, QuantLinearLUT):
        return
    for child_name, child in list(module.named_children()):
        full = f"{name}.{child_name}" if name else child_name
        if full in names:
            setattr(module, child_name, QuantLinearLUT(
                bits, child.in_features, child.out_features, child.bias is not None,
                include_sparse=include_sparse, numvals=(numvals[full] if numvals is not None else 0),
                topX=topX, balanced=balanced, num_nonzero_per_thread=num_nonzero_per_thread))
        else:
            make_quant_lut(child, names, bits, full, include_sparse=include_sparse, numvals=numvals, topX=topX,
                           balanced=balanced, num_nonzero_per_thread=num_nonzero_per_thread)
