/* sqllm_hip.h -- C ABI of libsqllm_hip.so: MI355X (gfx950) implementation of SqueezeLLM's
 * dense-and-sparse LUT-quantised matvec operator family.
 *
 * This header is the drop-in boundary.  It replaces the reference's pybind11 extension
 * `quant_cuda` (/root/reference/squeezellm/quant_cuda.cpp:112-270, launchers in
 * squeezellm/quant_cuda_kernel.cu:132-738): every `sqllm_vecquant*` entry point below has the
 * name, argument order and meaning of the reference function it replaces, with each
 * torch::Tensor argument replaced by a device pointer and the sizes the reference reads from it
 * via `.size()` passed explicitly after the tensor arguments, plus the HIP stream to launch on.
 *
 * Contract common to all entry points (reference behaviour: SURVEY.md section 8(b)):
 *   - all pointers are DEVICE pointers on the current HIP device; tensors are contiguous,
 *     row-major; `vec`, `mul`, `lookup_table`, `vals`, `full_rows` are fp32; `mat*` (qweight),
 *     `rows`, `cols`, `full_row_indices` are int32;
 *   - `mul` is ACCUMULATED INTO, never overwritten (the caller pre-loads bias or zeros:
 *     squeezellm/quant.py:214-219, :316-318);
 *   - qweight is int32 [height, width] = [K/32*bits, N]; lookup_table is [N, 2^bits];
 *   - the callee retains nothing and never synchronises; it enqueues its kernels on `stream` (NULL = the
 *     legacy default stream, which is what the reference used; the Python binding passes torch's current
 *     stream so calls are graph-capturable): exactly ONE kernel and no allocation for batch 1 and the batch
 *     tiles (up to mfma_min_batch - 1 rows, and every dense-only op up to 16 rows); the `_ws` entry points
 *     (sqllm_launch_ws ...) with a workspace of sqllm_workspace_bytes allocate nothing at ANY batch -- what a
 *     batch needs beside its operands comes out of the caller's workspace, as the reference's launchers
 *     allocate nothing (quant_cuda_kernel.cu:580-657) -- and with a NULL workspace nothing up to 16 rows;
 *     the workspace-less names (sqllm_launch, sqllm_launch_group(s), the reference operator names) take
 *     stream-ordered scratch instead wherever a workspace would have been used (see sqllm_launch);
 *   - return value: 0 on success, a negative SQLLM_E_* code for rejected arguments (the reference
 *     validated nothing and read out of bounds instead), or a positive hipError_t from the launch.
 *
 * Shape requirements: K % 32 == 0 and N % 4 == 0 (the reference needed K % 128 == 0 and
 * N % 128 == 0: quant_cuda_kernel.cu:754,776,841-852).  qweight must be 16-byte aligned.
 *
 * Non-finite operands.  The reference's kernels are fp32 FMA chains into `mul`: every term of an output
 * -- its `mul` element, each dense product lookup_table[n][idx] * vec[k], each CSR and each top-X product
 * -- is formed once, so an output is NaN if a term is NaN or terms of both infinities meet, otherwise the
 * infinity one of its terms has, otherwise finite; 0 x inf occurs only where the operands hold it.  Every
 * route follows this for NaN / +-inf in vec, vals, full_rows and mul, at every K and N the shape rule
 * admits (tests/test_gpu_nonfinite_routes.py): no kernel forms a product of its own out of a clamped
 * re-read.  ONE narrower case: a +-inf entry of lookup_table, on the routes whose dense term is an fp32
 * chain or the fp32 matrix instruction -- batch 1 on the fused kernel, the batch tiles, option
 * mfma_split = 0, and the fused linears below.  There the column of that entry is non-finite in every row,
 * and it is NaN or that infinity (the reference: that infinity, for a vec of one sign); nothing else is
 * touched.  (A slot behind the end of a workgroup's K slice re-reads the slice's last unit against a vec of
 * zeros: 0 x inf where that unit uses the entry.)  A NaN entry gives NaN on every route.
 */
#ifndef SQLLM_HIP_H
#define SQLLM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SQLLM_ABI_VERSION 1

/* error codes (negative; positive return values are hipError_t) */
#define SQLLM_OK 0
#define SQLLM_E_BITS (-1)      /* bits not in {3, 4} (quant.py:42-43) */
#define SQLLM_E_SHAPE (-2)     /* K % 32 != 0, N % 4 != 0, height != K/32*bits, non-positive dims */
#define SQLLM_E_NULL (-3)      /* a required pointer is NULL */
#define SQLLM_E_ALIGN (-4)     /* qweight not 16-byte aligned */
#define SQLLM_E_SPARSE (-5)    /* inconsistent sparse operands (nnz < 0, num_rows != N, topX < 0; with "validate_csr": bad rows[]) */
#define SQLLM_E_BATCH (-6)     /* batch < 1 or vec_height != K for a batched op */
#define SQLLM_E_OPTION (-7)    /* unknown option name / bad value */
#define SQLLM_E_GROUP (-8)     /* group of 0 or > 4 ops, or members differ in vec / K / bits / batch */

typedef void* sqllm_stream_t; /* a hipStream_t */

/* ---------------------------------------------------------------------------------------------
 * Generic descriptor form.  All twelve named entry points are thin adapters over sqllm_launch.
 * ------------------------------------------------------------------------------------------- */
typedef struct sqllm_op {
  int32_t bits;  /* 3 or 4 */
  int32_t batch; /* 0: matvec op, vec [K], mul [N].  >= 1: *_batched op, vec [batch, K], mul [batch, N] */
  int32_t K;     /* infeatures  */
  int32_t N;     /* outfeatures */
  const float* vec;
  const int32_t* qweight;     /* [K/32*bits, N] */
  float* mul;                 /* accumulated into */
  const float* lookup_table;  /* [N, 2^bits] */
  /* CSR outliers; rows == NULL -> no sparse term */
  const int32_t* rows; /* [N + 1] */
  const int32_t* cols; /* [nnz]   */
  const float* vals;   /* [nnz]   */
  int32_t nnz;
  /* "top-X" dense rows; full_rows == NULL -> no such term */
  int32_t topX;
  const float* full_rows;           /* [K, topX] */
  const int32_t* full_row_indices;  /* [topX]    */
} sqllm_op;

/* Enqueue  mul += W_lut . vec (+ CSR . vec) (+ full_rows^T . vec scattered)  on `stream`: one fused
 * kernel up to 16 rows -- from mfma_min_batch rows on, an op WITH sparse terms gets a small kernel in
 * front of it that writes vec transposed (and split into bf16 planes) into stream-ordered scratch
 * (hipMallocAsync / hipFreeAsync on `stream`; never inside a stream capture: the sparse terms gather
 * from vec itself there).  A wider batch is up to four kernels -- a transpose of vec into such scratch
 * (only with a CSR term), the sparse terms, (wide form only: "mfma_wide_min_batch") the split of vec
 * into bf16 planes, again in such scratch, and the dense term on the matrix cores; inside a stream
 * capture that scratch becomes memory nodes of the graph unless option "scratch_in_capture" is 0.
 * No host synchronisation in any case.  On first use of the scratch per device the release threshold of
 * the device's default memory pool is raised (option "scratch_pool_threshold").
 * Callers that own a workspace use sqllm_launch_ws instead: nothing is allocated then. */
int sqllm_launch(const sqllm_op* op, sqllm_stream_t stream);

/* The same with a CALLER-OWNED workspace -- the form that keeps the reference's contract at every batch
 * (its launchers allocate nothing: quant_cuda_kernel.cu:580-657): `workspace` is `workspace_bytes` of
 * device memory, 16-byte aligned, contents irrelevant before and after; sqllm_workspace_bytes(ops, n)
 * says how much the op (n = 1) or the group can use (0: none -- batch 1, batch tiles).  It serves one
 * launch at a time: launches on one stream may share it, concurrent streams may not.  What lives in it:
 *   mfma_min_batch..16 rows (fused small launch: 4-bit from 7 rows, 3-bit from 9; only with sparse terms)  vec transposed, xT[k][rows rounded up to 8 / 16]: the
 *            CSR walk of the dense workgroups and the top-X slabs then read one cache line per k for all batch rows
 *            instead of one per row; behind it vec as three bf16 planes in fragment order ((K / 32 + 1) x 3 KB): the
 *            dense term loads its operands already split (one small kernel in front of the launch writes both);
 *   17+ rows  what sqllm_launch takes from stream-ordered scratch: vec transposed, its bf16 planes, the
 *            wide form's slabs.
 * A NULL or too small workspace is not an error: 2..16 rows then gather from vec itself (ONE kernel, no
 * allocation, the default memory pool untouched), 17+ rows fall back to the stream-ordered scratch of
 * sqllm_launch.  A stream capture of a `_ws` launch with a sufficient workspace contains kernel nodes only. */
int64_t sqllm_workspace_bytes(const sqllm_op* ops, int32_t n_ops);
int sqllm_launch_ws(const sqllm_op* op, void* workspace, int64_t workspace_bytes, sqllm_stream_t stream);

/* Enqueue `n_ops` ops back to back on `stream` from one host call (a decode pass over a stack of
 * QuantLinearLUT layers costs one FFI crossing instead of n_ops).  Stops at the first error and
 * returns it; *n_done (may be NULL) receives the number of ops enqueued. */
int sqllm_launch_sequence(const sqllm_op* ops, int32_t n_ops, sqllm_stream_t stream, int32_t* n_done);

/* Same-input fusion: ONE kernel for 1..4 ops that read the same `vec` (same K, bits and batch) --
 * in a decoder layer q_proj/k_proj/v_proj, and gate_proj/up_proj (squeezellm/model_parse.py:53-61).
 * Every op keeps its own qweight / lookup_table / mul / sparse operands; the launch's workgroups
 * are simply divided between them.  Halves the launch count of a LLaMA decode pass, which matters
 * because each launch carries ~2-3 us of fixed cost against 1-4 us of streaming. */
int sqllm_launch_group(const sqllm_op* ops, int32_t n_ops, sqllm_stream_t stream);
int sqllm_launch_group_ws(const sqllm_op* ops, int32_t n_ops, void* workspace, int64_t workspace_bytes, sqllm_stream_t stream);

/* A whole pass as consecutive groups: group g covers the next group_sizes[g] entries of `ops`.
 * *n_done (may be NULL) receives the number of groups enqueued. */
int sqllm_launch_groups(const sqllm_op* ops, const int32_t* group_sizes, int32_t n_groups,
                        sqllm_stream_t stream, int32_t* n_done);
/* ... with one workspace for all of them (they run one after the other on `stream`): the largest
 * sqllm_workspace_bytes of any group serves the pass */
int sqllm_launch_groups_ws(const sqllm_op* ops, const int32_t* group_sizes, int32_t n_groups, void* workspace,
                           int64_t workspace_bytes, sqllm_stream_t stream, int32_t* n_done);

/* Measurement aid (used by bench.py's roofline leg, never on the serving path): enqueue the ops like
 * sqllm_launch_sequence, but attach a start/stop event pair to EVERY kernel dispatch
 * (hipExtLaunchKernelGGL), so that each kernel's own device-side duration -- the quantity
 * rocprofv3 --kernel-trace reports -- is available without a profiler.  Runs `reps` passes,
 * synchronises `stream` after each, and writes the per-op average in microseconds to
 * avg_us[0..n_ops).  Blocks the host; not graph-capturable. */
int sqllm_profile_sequence(const sqllm_op* ops, int32_t n_ops, sqllm_stream_t stream, int32_t reps,
                           float* avg_us);
/* the same for grouped launches: avg_us[0..n_groups) */
int sqllm_profile_groups(const sqllm_op* ops, const int32_t* group_sizes, int32_t n_groups,
                         sqllm_stream_t stream, int32_t reps, float* avg_us);
int sqllm_profile_groups_ws(const sqllm_op* ops, const int32_t* group_sizes, int32_t n_groups, void* workspace,
                            int64_t workspace_bytes, sqllm_stream_t stream, int32_t reps, float* avg_us);

/* ---------------------------------------------------------------------------------------------
 * Fused linear: the whole matvec branch of QuantLinearLUT.forward in one kernel.
 *
 * The reference wraps every operator call in three more launches -- `y = bias.clone()` or
 * `torch.zeros`, `x.float()`, `y.to(fp16)` (squeezellm/quant.py:214-223, :311-312; batched:
 * :314-321, :380-383).  sqllm_linear_f16 takes the activations as fp16 and writes fp16:
 *
 *     out[b, n] = fp16( bias[n] + sum_k W[n, k] * float(x[b, k]) )      (all three weight terms)
 *
 * `op` is read as for sqllm_launch except that  op.vec  is  const _Float16* [batch, K]  and
 * op.mul  is  _Float16* [batch, N], OVERWRITTEN (not accumulated into).  Accumulation is fp32.
 * `workspace`: sqllm_linear_workspace_bytes(&op) bytes of device memory, 16-byte aligned, that the
 * caller zero-fills ONCE; every launch leaves it zero-filled again.  A workspace serves one
 * launch at a time (launches on one stream may share it; concurrent streams may not).
 * Like every entry point: one kernel, nothing allocated, nothing retained, no synchronisation.
 * Accumulation runs in 2^-28 fixed point inside the workspace (so that one returning atomic both
 * deposits a partial sum and counts it): every partial sum is clamped to +-131072 (2 x the
 * largest finite fp16), i.e. results are exact to well below one fp16 ulp wherever the fp16 result
 * is finite.  Non-finite partial sums are carried by three sticky flag bits of the accumulator word:
 * a column that received a NaN comes out NaN, one that received +inf / -inf comes out +inf / -inf
 * (NaN if infinities of both signs met) -- the same pattern the operator path's fp32 atomics produce.  The CSR operands must be consistent (rows[N] == nnz, rows non-decreasing):
 * completion is detected by counting the contributions `rows` announces.  Shapes whose columns
 * could receive more than 63 partial sums (K slices + K / 1024 + 2 CSR chunks) are rejected with
 * SQLLM_E_SHAPE.
 * ------------------------------------------------------------------------------------------- */
typedef struct sqllm_linear {
  sqllm_op op;
  const float* bias; /* fp32 [N] or NULL */
  void* workspace;
} sqllm_linear;

int64_t sqllm_linear_workspace_bytes(const sqllm_op* op);
int sqllm_linear_f16(const sqllm_linear* lin, sqllm_stream_t stream);
/* a pass of fused linears as consecutive same-input groups (cf. sqllm_launch_groups); the members
 * of a group share op.vec, K, bits and batch and each has its own workspace */
int sqllm_linear_f16_groups(const sqllm_linear* lins, const int32_t* group_sizes, int32_t n_groups,
                            sqllm_stream_t stream, int32_t* n_done);

/* The same linear with bf16 at its two ends -- the 16-bit type most checkpoints are held in:
 *
 *     out[b, n] = bf16_rne( bias[n] + sum_k W[n, k] * float(x[b, k]) )      (all three weight terms)
 *
 * The same sqllm_linear struct:  op.vec  is bf16 [batch, K] (widened EXACTLY: a 16-bit shift),  op.mul  is bf16
 * [batch, N], OVERWRITTEN;  bias  stays fp32.  Everything else is sqllm_linear_f16's, word for word: one kernel, nothing
 * allocated, validation, grouping rules, the 63-contribution limit and every error code; the workspace and
 * sqllm_linear_workspace_bytes are unchanged, and because a workspace is all-zero between launches ONE workspace may
 * serve fp16 and bf16 launches alternately on one stream.  Inside a contribution (a dense K slice with the top-X rows of
 * its tile, a CSR chunk's part of a row) accumulation is fp32 in the SAME ORDER as the fp16 kernel; between contributions
 * it is the 2^-28 fixed-point word; the finished sum plus the bias is rounded ONCE, to nearest-even, to bf16.  NaN and
 * +-inf in the operands travel through the three sticky flag bits as above.
 *
 * One thing differs, and it differs loudly.  The word holds contributions only up to +-131072 (2^17).  The fp16 kernel
 * clamps there, because such a result is not finite in fp16 anyway; in bf16 it IS finite, and a clamp would return a wrong
 * finite number.  sqllm_linear_bf16 therefore treats a FINITE contribution with |v| > 131072 as the infinity of its sign:
 * the matching sticky flag is set and nothing is added.  So
 *   - a result built from in-range contributions is exact to the fixed-point rounding (2^-28 per contribution), up to
 *     63 x 131072 in magnitude;
 *   - a result with a contribution beyond the range is +inf or -inf, or NaN if contributions of both signs were beyond
 *     it -- never a finite wrong value, with ONE exception: a CSR chunk of 1024 consecutive non-zeros that spans more
 *     than 2048 rows (an extremely sparse region of the matrix) adds its values to the word UNCOUNTED, one per non-zero,
 *     and while such a word is transiently negative a sticky flag can be lost (the same corner in which the fp16 kernel
 *     can report a NaN as a finite number).  There, a single outlier product vals[i] * x[cols[i]] beyond +-131072 may be
 *     dropped and the result come out finite and wrong.  Dense contributions and ordinary CSR chunks are not affected.
 * The reference's fp32 path (and the fp32 operator names here) would return the finite value there: a caller whose
 * activations can drive one K slice of one output past 131072 in magnitude must use those.  (How K is cut into
 * contributions is the planner's choice -- sqllm_plan_query: k_slices -- so between 131072 and 63 x 131072 whether a
 * large result comes out finite depends on the shape; below 131072 in sum_k |W[n, k] x[b, k]| it always does.) */
int sqllm_linear_bf16(const sqllm_linear* lin, sqllm_stream_t stream);
int sqllm_linear_bf16_groups(const sqllm_linear* lins, const int32_t* group_sizes, int32_t n_groups,
                             sqllm_stream_t stream, int32_t* n_done);

/* ---------------------------------------------------------------------------------------------
 * Gated fused linear: the front half of a LLaMA MLP -- gate_proj, up_proj, SiLU and the product -- in one kernel.
 *
 * For two packed layers `gate` and `up` with the same K, N, bits and batch, over the same 16-bit activations x:
 *
 *     g = bias_gate[n] + sum_k Wg[n,k] * float(x[b,k])      (all three weight terms, fp32 as in sqllm_linear_*)
 *     u = bias_up[n]   + sum_k Wu[n,k] * float(x[b,k])
 *     out[b,n] = OT( (g / (1 + exp(-g))) * u )              evaluated in fp32, rounded ONCE to OT (fp16 or bf16, = type of x)
 *
 *   - Accumulation inside and between contributions is exactly sqllm_linear_f16 / _bf16's: fixed-point words, counted
 *     returning atomics, sticky flags, the same order of additions.  The 63-contribution limit applies per member.
 *   - Non-finite g or u follow the fp32 formula above, which is what torch.nn.functional.silu(g) * u gives in fp32:
 *     silu(+inf) = +inf, silu(-inf) = NaN, silu(NaN) = NaN, silu of a large negative finite value is -0.
 *   - The range rule is the bf16 rule for BOTH output types.  The fp16 linear clamps a contribution beyond +-131072
 *     because such an fp16 result is not finite anyway.  Here that argument fails: g = 200000, u = 0.05 has a finite fp16
 *     product, and a clamp would return a wrong finite number.  Both gated kernels therefore use the no-clamp form of
 *     sqllm_linear_bf16: a finite contribution with |v| > 131072 sets the infinity flag of its sign and adds nothing.  The
 *     corner carved out above stays as it is, 256 rows earlier: a CSR chunk spanning more than 1792 rows adds its values uncounted, a flag
 *     can be lost there, and the result can be finite and wrong.
 *   - The result is a function of the operands alone: integer sums commute, and the final step is computed from the same
 *     two fp32 values whichever member finishes first.  Run to run it is bit-identical.  (Inside a contribution the order
 *     of additions is fixed as well: where the linears let a CSR chunk's waves add their parts of a long row in arrival
 *     order, these kernels add them in wave order.  ONE exception: top-X rows passed as full_rows -- not folded into the
 *     CSR, as the Python module folds them -- are summed per K slice by eight waves in arrival order, as in the linears;
 *     such a column's last fp32 bit, and with it an output on a rounding boundary of OT, can differ between runs.)
 *
 * The two members may differ in their sparse terms (a dense-only gate with an up that has CSR and top-X rows).
 * `workspace`: sqllm_gated_workspace_bytes(&gate) bytes, 16-byte aligned -- the two members' accumulator planes and a plane
 * of 64-bit pair words [batch, N] in which the two finished values of an output meet -- zero-filled ONCE by the caller and
 * left zero-filled by every launch; it serves one launch at a time.  Like every entry point: one kernel, nothing
 * allocated, nothing retained, no synchronisation, capturable as one kernel node.  Rejected before the device is touched:
 * act other than SQLLM_ACT_SILU (SQLLM_E_OPTION); a non-NULL mul in either member, members that differ in vec / K / N /
 * bits / batch (SQLLM_E_GROUP); a NULL descriptor, out or workspace (SQLLM_E_NULL); a workspace that is not 16-byte aligned
 * (SQLLM_E_ALIGN); and everything sqllm_linear_* rejects, with its codes.
 * ------------------------------------------------------------------------------------------- */
#define SQLLM_ACT_SILU 0
typedef struct sqllm_gated {
  sqllm_op gate, up;      /* as for sqllm_linear_*: vec = 16-bit [batch, K], shared; mul must be NULL */
  const float* bias_gate; /* fp32 [N] or NULL */
  const float* bias_up;
  void* out;              /* fp16 / bf16 [batch, N], OVERWRITTEN */
  void* workspace;        /* sqllm_gated_workspace_bytes(), zero-filled ONCE, left zero-filled */
  int32_t act;            /* SQLLM_ACT_SILU; anything else: SQLLM_E_OPTION */
} sqllm_gated;
int64_t sqllm_gated_workspace_bytes(const sqllm_op* gate); /* two accumulator planes + the pair plane */
int sqllm_gated_f16(const sqllm_gated* g, sqllm_stream_t stream);
int sqllm_gated_bf16(const sqllm_gated* g, sqllm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Fused linear with an epilogue: activation and residual add in the linear's own kernel.
 *
 * What a model wraps around a linear -- `relu(fc1(x))`, `residual + o_proj(x)`, `residual + down_proj(h)` -- as part of
 * the finishing step of each output element, instead of one or two element-wise kernels behind it:
 *
 *     out[b,n] = OT( act(bias[n] + sum_k W[n,k] * float(x[b,k])) + float(residual[b,n]) )
 *
 * `lin` is read exactly as sqllm_linear_f16 / _bf16 read it (OT = the type of x = the type of out and of residual); the
 * workspace is sqllm_linear_workspace_bytes(&lin.op) bytes, is left zero-filled, and may be shared with plain
 * sqllm_linear_* launches on the same stream.  Accumulation inside and between contributions is sqllm_linear_*'s.  The
 * thread that completes a column holds its fp32 value; it applies `act`, adds the residual element and rounds ONCE, to
 * nearest-even.  The activations are evaluated in fp32 as written here, and the values at +-inf and NaN are what these
 * formulas give in IEEE fp32 (they are the specification; not every framework's GELU agrees at +inf):
 *
 *     act                  | formula                                                 | +inf | -inf | NaN
 *     ---------------------+---------------------------------------------------------+------+------+-----
 *     SQLLM_ACT_IDENTITY   | v                                                       | +inf | -inf | NaN
 *     SQLLM_ACT_RELU       | v > 0 ? v : (v != v ? v : 0)                            | +inf |  0   | NaN
 *     SQLLM_ACT_SILU       | v / (1 + expf(-v))                                      | +inf | NaN  | NaN
 *     SQLLM_ACT_GELU       | 0.5 v (1 + erff(v * 0.70710678))                        | +inf | NaN  | NaN
 *     SQLLM_ACT_GELU_TANH  | 0.5 v (1 + tanhf(0.79788456 (v + 0.044715 v^3)))        | +inf | NaN  | NaN
 *
 *   - The residual is added AFTER the activation by plain fp32 addition: +inf + (-inf) = NaN, a NaN residual gives NaN.
 *   - The range rule is the bf16 rule for BOTH output types, as in the gated kernels: a finite contribution with
 *     |v| > 131072 sets the infinity flag of its sign and adds nothing.  The fp16 linear clamps there because such an fp16
 *     result is not finite anyway; here a contribution of 200000 can meet a residual of -180000, and a clamp would return
 *     a wrong finite number.  So SQLLM_ACT_IDENTITY without a residual equals sqllm_linear_bf16 bit for bit, and equals
 *     sqllm_linear_f16 wherever every contribution is within +-131072.
 *   - The corner carved out for sqllm_linear_bf16 is inherited unchanged: a CSR chunk spanning more than 2048 rows adds its
 *     values uncounted, a flag can be lost there, and the result can be finite and wrong.
 *   - `residual` may be the output buffer itself (residual == lin.op.mul, the in-place form: each element is read and
 *     written by the same single thread) and may equal lin.op.vec when K == N (both are only read).  Any other overlap of
 *     the [batch, N] residual range with the output range is rejected.
 *
 * Like every entry point: one kernel, nothing allocated, nothing retained, no synchronisation, capturable as one kernel
 * node.  Rejected before the device is touched: an act outside the five codes (SQLLM_E_OPTION); a residual that partly
 * overlaps the output (SQLLM_E_SHAPE); a NULL descriptor (SQLLM_E_NULL); and everything sqllm_linear_* rejects, with its
 * codes.  (sqllm_gated_* keeps rejecting every act but SQLLM_ACT_SILU.)  There is no group form.
 * ------------------------------------------------------------------------------------------- */
#define SQLLM_ACT_IDENTITY 1
#define SQLLM_ACT_RELU 2
#define SQLLM_ACT_GELU 3
#define SQLLM_ACT_GELU_TANH 4
typedef struct sqllm_linear_ep {
  sqllm_linear lin;     /* exactly as for sqllm_linear_f16 / _bf16; workspace rules unchanged */
  const void* residual; /* 16-bit [batch, N] of the output's type, or NULL; may equal lin.op.mul */
  int32_t act;          /* SQLLM_ACT_*; note that 0 is SiLU */
} sqllm_linear_ep;
int sqllm_linear_ep_f16(const sqllm_linear_ep* e, sqllm_stream_t stream);
int sqllm_linear_ep_bf16(const sqllm_linear_ep* e, sqllm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Attention front: q_proj, k_proj, v_proj and the rotary position embedding of q and k in one kernel.
 *
 * For three packed layers q, k, v over the same 16-bit activations x (OT = the type of x and of all three outputs) that
 * share K, bits and batch -- N may differ per member: grouped-query models have narrower k and v --
 *
 *     s_m[b,n]   = bias_m[n] + sum_k W_m[n,k] * float(x[b,k])        m in {q, k, v}; all three weight terms, as sqllm_linear_*
 *     out_v[b,n] = OT( s_v[b,n] )
 *     for m in {q, k}, head h, j in [0, D/2), p = positions[b]:
 *         (lo, hi) = the pair's two columns of s_m[b, :]
 *         out_m[b, col_lo] = OT( lo * cos[p,j] - hi * sin[p,j] )
 *         out_m[b, col_hi] = OT( hi * cos[p,j] + lo * sin[p,j] )
 *
 *   - Everything is evaluated in fp32 and rounded ONCE, to nearest-even.  (The two products and the sum of an output may
 *     or may not be contracted into a fused multiply-add; either way it is the same instruction sequence for both columns
 *     of a pair in every run.)
 *   - D = head_dim is even and divides N_q and N_k.  `cos` and `sin` are fp32 [n_pos, D/2] in device memory, supplied by
 *     the caller: the kernel computes no angles, so any base or scaling rule works.  `positions` is int32 [batch] in
 *     DEVICE memory: a captured graph follows a position the host updates in place.
 *   - layout SQLLM_ROPE_HALF (0): col_lo = h*D + j, col_hi = h*D + j + D/2 -- the `rotate_half` form of the checkpoints the
 *     reference loads.  SQLLM_ROPE_INTERLEAVED (1): col_lo = h*D + 2j, col_hi = h*D + 2j + 1.
 *   - Accumulation inside and between contributions is exactly sqllm_linear_*'s.  The range rule is the bf16 rule for BOTH
 *     output types, as in the gated and epilogue kernels: a value beyond +-131072 can rotate to a finite fp16 result, and
 *     a clamp would return a wrong finite number.  The CSR-span corner is inherited with the gated kernels' limit: a chunk
 *     spanning more than 1792 rows adds its values uncounted, a flag can be lost there, and the result can be finite and wrong.
 *   - Non-finite values: what the formulas give in IEEE fp32 is the specification (inf * 0 = NaN: an infinite sum makes
 *     both outputs of its pair NaN wherever the other factor is 0).  A positions[b] outside [0, n_pos) makes every q and k
 *     output of row b NaN and reads nothing from the tables; v and the other rows are unaffected.
 *   - Bit-exact equalities that follow: out_v equals sqllm_linear_bf16 (bf16) or sqllm_linear_ep_f16 with
 *     SQLLM_ACT_IDENTITY and no residual (fp16), bit for bit; with cos = 1, sin = 0 and finite operands so do out_q and out_k.
 *   - The result is a function of the operands alone: integer sums commute, and the rotation is computed from the same
 *     two fp32 values whichever column finishes first.  Run to run it is bit-identical.  (Inside a contribution the order
 *     of additions is fixed as well, as in the gated kernels.  ONE exception, theirs: top-X rows passed as full_rows -- not
 *     folded into the CSR, as the Python module folds them -- are summed per K slice by eight waves in arrival order;
 *     such a column's last fp32 bit, and with it an output on a rounding boundary of OT, can differ between runs.)
 *
 * `workspace`: sqllm_qkv_rope_workspace_bytes() bytes, 16-byte aligned -- the three members' accumulator planes
 * (sqllm_linear_workspace_bytes each, in the order q, k, v), then one plane of 64-bit pair words [batch, N/2] for q and one
 * for k, in which the two finished values of a pair meet -- zero-filled ONCE by the caller and left zero-filled by every
 * launch; it serves one launch at a time.  Like every entry point: one kernel, nothing allocated, nothing retained, no
 * synchronisation, capturable as one kernel node.  Rejected before the device is touched:
 *   members that differ in vec / K / bits / batch, or a non-NULL mul                        SQLLM_E_GROUP
 *   head_dim odd, < 2, or not a divisor of N_q or N_k; n_pos < 1                            SQLLM_E_SHAPE
 *   N_q * head_dim or N_k * head_dim above 2^32; batch * N_q or batch * N_k at or above 2^31;
 *   more than 2^20 rows (the kernel's division-free index arithmetic)                        SQLLM_E_SHAPE
 *   a NULL descriptor, out, table, positions or workspace                                   SQLLM_E_NULL
 *   a workspace that is not 16-byte aligned                                                 SQLLM_E_ALIGN
 *   a layout other than 0 or 1                                                              SQLLM_E_OPTION
 *   outputs that overlap each other or the workspace                                        SQLLM_E_SHAPE
 *   and everything sqllm_linear_* rejects, with its codes.
 * ------------------------------------------------------------------------------------------- */
#define SQLLM_ROPE_HALF 0
#define SQLLM_ROPE_INTERLEAVED 1
typedef struct sqllm_qkv_rope {
  sqllm_op q, k, v;        /* as for sqllm_linear_*: vec = 16-bit [batch, K], shared; mul must be NULL */
  const float* bias_q;     /* fp32 [N_m] or NULL */
  const float* bias_k;
  const float* bias_v;
  void* out_q;             /* fp16 / bf16 [batch, N_m], OVERWRITTEN */
  void* out_k;
  void* out_v;
  const float* cos;        /* fp32 [n_pos, head_dim / 2], device memory */
  const float* sin;
  const int32_t* positions; /* int32 [batch], device memory */
  int32_t n_pos;
  int32_t head_dim;
  int32_t layout;          /* SQLLM_ROPE_HALF or SQLLM_ROPE_INTERLEAVED; anything else: SQLLM_E_OPTION */
  void* workspace;         /* sqllm_qkv_rope_workspace_bytes(), zero-filled ONCE, left zero-filled */
} sqllm_qkv_rope;
int64_t sqllm_qkv_rope_workspace_bytes(const sqllm_op* q, const sqllm_op* k, const sqllm_op* v); /* three accumulator planes + two pair planes */
int sqllm_qkv_rope_f16(const sqllm_qkv_rope* r, sqllm_stream_t stream);
int sqllm_qkv_rope_bf16(const sqllm_qkv_rope* r, sqllm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Norm fronts: the RMSNorm in front of gate/up and in front of q/k/v, as a prologue of those two kernels.
 *
 * For 16-bit activations x [batch, K] (fp16 or bf16, OT = its type) -- the UN-normalised hidden state --, a norm weight
 * g [K] of the same 16-bit type and eps:
 *
 *     ms[b]   = (1/K) * sum_k float(x[b,k])^2
 *     r[b]    = 1.0f / sqrtf(ms[b] + eps)                  fp32, correctly rounded divide and square root
 *     xn[b,k] = float(x[b,k]) * float(g[k]) * r[b]         fp32 (the two products in this order), NEVER rounded to 16 bits
 *
 * and the kernel is exactly sqllm_gated_* / sqllm_qkv_rope_* with float(x[b,k]) replaced by xn[b,k] in all three weight
 * terms: dense, CSR and top-X (folded into the CSR or passed as full_rows).
 *
 *   - The sums that enter the fixed-point words are sums over xn.  The range rule (+-131072, the bf16 rule), the flags,
 *     the 63-contribution limit, the ordered CSR adds, the finishers and every documented corner of the parent entry are
 *     unchanged: what overflows, and what the bias meets, is the normalised sum.
 *   - ms[b] is summed in fp32 in ONE fixed order, the same in every workgroup of every launch, so every column of a row
 *     sees the same r[b] bits: thread t of 512 adds the squares (exact in fp32) of elements [8t, 8t + 8) of every round of
 *     4096 elements, in ascending k, into one accumulator; the 64 lanes of a wave meet in a butterfly (lane distances 32,
 *     16, 8, 4, 2, 1); the eight wave sums are added in wave order; the total is divided by float(K).  The result is a
 *     function of the operands alone and bit-identical run to run, with the parent entry's one exception (full_rows).
 *   - Non-finite values follow the fp32 formulas in IEEE arithmetic.  A NaN in row b makes every output of row b NaN.  A
 *     sum of squares that overflows fp32 (an infinite x[b,k] included) gives r[b] = 0; xn is then 0 where x is finite and
 *     NaN where x is infinite.  WHERE a finite row overflows depends on the order above: a row whose exact sum of squares
 *     is within a few units in the last place of FLT_MAX may overflow in another order and not in this one.
 *   - This is not bit-identical to the norm as the checkpoints' modules write it in torch (upcast, pow, mean, + eps,
 *     rsqrt, mul, DOWNCAST, mul weight), which rounds x * r to 16 bits and the product with the weight to 16 bits again
 *     before the linear reads it, and whose rsqrt need not be correctly rounded: the fused form keeps xn in fp32 and is
 *     the closer of the two to the exact value, by up to two 16-bit roundings per element of xn.
 *   - vec need not be aligned beyond its elements, as for sqllm_linear_*.
 *
 * Workspace sizes and rules are the parent entry's, and one workspace may serve norm and plain launches alternately.  Each
 * call is one kernel: nothing allocated, capturable as one kernel node.  Rejected before the device is touched: first
 * a NULL norm descriptor or weight (SQLLM_E_NULL), then eps negative or not finite (SQLLM_E_OPTION); after those, everything
 * the parent entry rejects, with its own codes, and a weight whose [K] range overlaps an output or the workspace
 * (SQLLM_E_SHAPE).
 * ------------------------------------------------------------------------------------------- */
typedef struct sqllm_rmsnorm {
  const void* weight; /* 16-bit [K], the type of x, device memory */
  float eps;          /* >= 0 and finite */
} sqllm_rmsnorm;
int sqllm_gated_norm_f16(const sqllm_gated* g, const sqllm_rmsnorm* norm, sqllm_stream_t stream);
int sqllm_gated_norm_bf16(const sqllm_gated* g, const sqllm_rmsnorm* norm, sqllm_stream_t stream);
int sqllm_qkv_rope_norm_f16(const sqllm_qkv_rope* r, const sqllm_rmsnorm* norm, sqllm_stream_t stream);
int sqllm_qkv_rope_norm_bf16(const sqllm_qkv_rope* r, const sqllm_rmsnorm* norm, sqllm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Attention front writing k and v straight into the KV cache: sqllm_qkv_rope_* / sqllm_qkv_rope_norm_* whose finishers
 * store the elements of k and v into a cache as well as, or instead of, into out_k / out_v.  One kernel takes the place of
 * the front and the two copies into the cache that follow it.
 *
 *   - Same values.  Everything sqllm_qkv_rope_* / sqllm_qkv_rope_norm_* specify holds word for word: the sums, the
 *     rotation, the one rounding, the range rule, the flags, every documented corner, the workspace size and rules, and
 *     one kernel that allocates nothing and is capturable as one kernel node.
 *   - Where k and v go.  With s = slots[b], 0 <= s < n_slots, and column n = h * head_dim + d of member k (resp. v): the
 *     element that out_k[b, n] receives is stored with the SAME BITS at k_cache[s * slot_stride + h * head_stride + d]
 *     (resp. v_cache).  Offsets are 64-bit.  The cache gets exactly what the output would get, the NaN row of an
 *     out-of-range position included.  `slots` is int32 [batch] in DEVICE memory: a captured graph follows slots the host
 *     updates in place.
 *   - Optional outputs.  out_k and out_v may each be NULL in these four entries: only the cache then receives that
 *     member.  Non-NULL, both are written.  out_q stays required; q is never cached.
 *   - Out-of-range slots.  With slots[b] outside [0, n_slots) -- the usual -1 padding -- nothing of row b is written to
 *     either cache; row b's out_* are unaffected.  Nothing outside the addressed elements is ever written.
 *   - Duplicate slots.  Two rows with the same slot leave, element by element, one of the two rows' values: the caller's
 *     error, not detected.
 *   - N_k == N_v, and head_dim divides N_v (H = N_v / head_dim kv heads).
 *   - The two standard layouts.  Slot-major [n_slots, H, D]: slot_stride = H*D, head_stride = D; a paged
 *     [blocks, block, H, D] is the same thing.  Head-major static [B, H, S, D]: slot = b*H*S + p, slot_stride = D,
 *     head_stride = S*D, n_slots = (B-1)*H*S + S.  Overlapping addressing such as the second is the caller's business: the
 *     kernel only evaluates the formula.
 *
 * Rejected before the device is touched: first the parent entry's own rejections (its list above, the norm's in front
 * where there is one), in its order and with its codes, except that a NULL out_k / out_v is admitted; then
 *   a NULL cache descriptor, k_cache, v_cache or slots                                      SQLLM_E_NULL
 *   n_slots < 1, or a stride < head_dim                                                     SQLLM_E_SHAPE
 *   N_k != N_v, or N_v not a multiple of head_dim                                           SQLLM_E_SHAPE
 *   a stride at or above 2^32 that is ever multiplied (slot_stride with n_slots > 1, head_stride with H > 1: the kernel
 *   forms its 64-bit offsets out of 32 x 32 -> 64-bit products), or an extent at or above 2^62 elements
 *                                                                                           SQLLM_E_SHAPE
 *   a cache extent that overlaps the other cache, the workspace, any non-NULL output, vec or the norm weight
 *                                                                                           SQLLM_E_SHAPE
 *   and, behind those, everything sqllm_linear_* rejects, with its codes.
 * The extent is [base, base + (n_slots-1)*slot_stride + (H-1)*head_stride + head_dim) elements.
 * ------------------------------------------------------------------------------------------- */
typedef struct sqllm_kv_cache {
  void* k_cache;          /* 16-bit elements of x's type, device memory */
  void* v_cache;
  const int32_t* slots;   /* int32 [batch], DEVICE memory: a captured graph follows slots updated in place */
  int32_t n_slots;        /* >= 1 */
  int64_t slot_stride;    /* elements between consecutive slots,            >= head_dim */
  int64_t head_stride;    /* elements between consecutive kv heads of a slot, >= head_dim */
} sqllm_kv_cache;
int sqllm_qkv_rope_cache_f16(const sqllm_qkv_rope* r, const sqllm_kv_cache* c, sqllm_stream_t stream);
int sqllm_qkv_rope_cache_bf16(const sqllm_qkv_rope* r, const sqllm_kv_cache* c, sqllm_stream_t stream);
int sqllm_qkv_rope_norm_cache_f16(const sqllm_qkv_rope* r, const sqllm_rmsnorm* norm, const sqllm_kv_cache* c, sqllm_stream_t stream);
int sqllm_qkv_rope_norm_cache_bf16(const sqllm_qkv_rope* r, const sqllm_rmsnorm* norm, const sqllm_kv_cache* c, sqllm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Decode attention over the KV cache the attention front writes: ONE new query per sequence, attending to the keys the
 * cache holds for that sequence.  The consumer of sqllm_kv_cache's layout; the step between the front's out_q and o_proj.
 *
 *   - Addressing.  Key p of row b lives in slot  block_table[b, p / block_size] * block_size + p % block_size  (64-bit), and
 *     element (slot, kv head h, d) at slot*slot_stride + h*head_stride + d of k_cache / v_cache, as in sqllm_kv_cache.  One
 *     form covers both layouts of the front: a paged [blocks, block, H, D] takes the usual table; the head-major static
 *     [B, H, S, D] (slot_stride = D, head_stride = S*D) takes block_size = S, max_blocks = 1, block_table[b, 0] = b * H,
 *     which is slot = b*H*S + p.  block_size is any positive int32, not only a power of two.  block_table and seq_lens are
 *     DEVICE memory: a captured graph follows lengths and tables updated in place.  seq_lens[b] = position + 1 when the
 *     front wrote the new token in the same step: the new key attends to itself.
 *   - Values.  Query head h uses kv head h / (n_q_heads / n_kv_heads).  For the keys p = 0 .. seq_lens[b]-1:
 *         s[p]      = scale * sum_d float(q[d]) * float(k[p,d])          fp32
 *         m         = max_p s[p],   w[p] = expf(s[p] - m)                fp32, max-subtracted
 *         out[d]    = (sum_p w[p] * float(v[p,d])) / (sum_p w[p])        fp32, rounded ONCE to the output type
 *   - Order.  The sequence is cut into partitions of SQLLM_ATTN_PARTITION = 256 keys (keys [256 i, 256 i + 256)); every
 *     partition is reduced in an order that depends on head_dim, n_q_heads / n_kv_heads and the keys' indices alone, and the
 *     partitions' (max, sum, acc) are combined in ascending partition order.  Row b's output bits are a function of row b's
 *     own operands and the descriptor's shape fields only: not of the other rows, not of the batch size, not of timing;
 *     bit-identical run to run.  Launch geometry depends on host fields (max_blocks * block_size) and never on device data.
 *   - Slots not addressed by (block_table, seq_lens) are never read in a way that can influence a result: whatever bits
 *     they hold, NaN included, the output bits are the same.  Nothing outside the cache extent is ever read.
 *   - Nothing but out[b, 0 .. n_q_heads*head_dim) of every row and the workspace is written.
 *   - seq_lens[b] <= 0: the row of out is +0.
 *   - Row b of out is NaN for all heads when seq_lens[b] > max_blocks * block_size, or when a table entry used by row b
 *     addresses any slot outside [0, n_slots) -- the front's rule for an out-of-range position.
 *   - A NaN among the attended elements of q or k makes that head's outputs NaN.  A NaN in attended v[p, d] makes column d
 *     of the heads of that kv group NaN.  Infinities follow IEEE arithmetic on the formulas above (an infinite score gives
 *     inf - inf) and are not pinned further.
 *   - Workspace: sqllm_attn_decode_workspace_bytes() bytes, 4-byte aligned, CONTENTS IRRELEVANT: every word that is read
 *     was written by the same call.  (max, sum, acc[head_dim]) in fp32 per (row, query head, partition).
 *   - Each call allocates nothing and is capturable: TWO kernel nodes (partials, then combine), ONE when
 *     max_blocks * block_size <= SQLLM_ATTN_PARTITION.
 *
 * Served: head_dim 64 or 128; n_q_heads a multiple of n_kv_heads with a ratio of 1 to 8; batch 1 to 64; anything else is
 * SQLLM_E_SHAPE.  Rejected before the device is touched, in this order:
 *   a NULL descriptor, q, out, k_cache, v_cache, block_table, seq_lens or workspace          SQLLM_E_NULL
 *   a count < 1 (batch, heads, head_dim, n_slots, block_size, max_blocks, table_stride); slot_stride or head_stride
 *   < head_dim; q_stride or out_stride < n_q_heads*head_dim; max_blocks > table_stride; a shape that is not served; a
 *   stride at or above 2^32 that is ever multiplied, or an extent at or above 2^62 elements, as for sqllm_kv_cache
 *                                                                                           SQLLM_E_SHAPE
 *   a scale that is not finite                                                              SQLLM_E_OPTION
 *   out or the workspace overlapping q, a cache, block_table, seq_lens or each other         SQLLM_E_SHAPE
 *   q, out, k_cache or v_cache not aligned to 2 bytes, the workspace not to 4                SQLLM_E_ALIGN
 * ------------------------------------------------------------------------------------------- */
#define SQLLM_ATTN_PARTITION 256
typedef struct sqllm_attn_decode {
  const void* q;            /* 16-bit [batch, n_q_heads * head_dim], row stride q_stride elements: the front's out_q */
  void* out;                /* 16-bit [batch, n_q_heads * head_dim], row stride out_stride; OVERWRITTEN; what o_proj reads */
  const void* k_cache;      /* as sqllm_kv_cache: element (slot, kv head h, d) at slot*slot_stride + h*head_stride + d */
  const void* v_cache;
  const int32_t* block_table; /* int32 [batch, table_stride], DEVICE memory */
  const int32_t* seq_lens;    /* int32 [batch], DEVICE memory: keys 0 .. seq_lens[b]-1 of row b are attended */
  int32_t batch, n_q_heads, n_kv_heads, head_dim;
  int32_t n_slots, block_size, max_blocks, table_stride;   /* max_blocks <= table_stride */
  int64_t slot_stride, head_stride, q_stride, out_stride;
  float scale;              /* the caller's, usually 1/sqrt(head_dim); finite */
  void* workspace;          /* sqllm_attn_decode_workspace_bytes(); contents irrelevant */
} sqllm_attn_decode;
int64_t sqllm_attn_decode_workspace_bytes(int32_t batch, int32_t n_q_heads, int32_t head_dim, int32_t max_blocks, int32_t block_size);
int sqllm_attn_decode_f16(const sqllm_attn_decode* a, sqllm_stream_t stream);
int sqllm_attn_decode_bf16(const sqllm_attn_decode* a, sqllm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * FP8 KV cache: the attention front writes 1-byte OCP e4m3fn elements (NOT the fnuz format), decode attention reads them.
 * One fp32 scale per cache, k_scale and v_scale, chosen by the caller (calibration is the caller's; absmax / 448 is the usual
 * choice).  Half the bytes of the 16-bit cache for the step of a decode layer that is bound by them.
 *
 *   - Encoding (sqllm_qkv_rope_cache_fp8_* / sqllm_qkv_rope_norm_cache_fp8_*).  With inv = 1.0f / scale, computed once on the host
 *     in fp32:
 *         byte = e4m3_rne(min(max(x * inv, -448), 448))
 *     where x is the fp32 value that out_k[b, n] / out_v[b, n] would round to 16 bits: the rotated value for k, the plain sum
 *     for v.  The fp32 value is rounded ONCE, straight to fp8; it does not go through the 16-bit output.  Rounding is to
 *     nearest, ties to even; e4m3's subnormals are produced, not flushed; +-inf saturates to +-448; NaN stays NaN (exponent
 *     and mantissa bits all ones, either sign).  The clamp is explicit in the kernel.
 *   - Decoding (sqllm_attn_decode_fp8_*).  float(k) = k_scale * f32(byte) and float(v) = v_scale * f32(byte) stand in the
 *     formulas of sqllm_attn_decode.  scale * k_scale is folded into the score's scale, rounded once on the host; v_scale
 *     multiplies each partition's sum over its keys once per output element, in fp32, before the one rounding to the output
 *     type.  A NaN byte among the attended elements behaves as a NaN element does there.
 *   - Everything else holds word for word, for the front as for the attention: the paged and the head-major static layout
 *     through the two strides, which now count BYTES; int32 slots, tables and lengths in device memory; out-of-range slots
 *     write nothing; optional out_k / out_v, written as by the 16-bit entries when given; the +0 row and the NaN rows;
 *     unaddressed slots never influence a result; fixed partitions of SQLLM_ATTN_PARTITION keys combined in ascending order;
 *     the workspace of sqllm_attn_decode_workspace_bytes(); no allocation; one kernel node for the front, two for the
 *     attention, one when max_blocks * block_size <= SQLLM_ATTN_PARTITION.  Cache elements are aligned to one byte only: any
 *     base address and any strides >= head_dim, head_stride = head_dim + 3 included.
 *   - Determinism.  Every sum's order depends on head_dim, n_q_heads / n_kv_heads and the key's index alone: bit-identical
 *     run to run and row by row.  The order is not the 16-bit kernel's.
 *
 * Rejected before the device is touched: everything the 16-bit sibling rejects, with its codes and in its order (the cache
 * extents in bytes, and no alignment rule for k_cache / v_cache); then
 *   a k_scale or v_scale that is not finite, not positive, or whose fp32 reciprocal is not finite     SQLLM_E_OPTION
 *   in the attention entries, a scale * k_scale that is not finite                                    SQLLM_E_OPTION
 * Not covered: per-head or per-token scales, e5m2, int8 or 4-bit caches, computing the scales, prefill attention beyond the
 * up to 16 query rows per sequence of sqllm_attn_append_fp8 (below): prompt-length prefill stays out.
 * ------------------------------------------------------------------------------------------- */
typedef struct sqllm_kv_cache_fp8 {
  void* k_cache;          /* 1-byte e4m3fn elements, device memory */
  void* v_cache;
  const int32_t* slots;   /* int32 [batch], DEVICE memory: a captured graph follows slots updated in place */
  int32_t n_slots;        /* >= 1 */
  int64_t slot_stride;    /* bytes between consecutive slots,            >= head_dim */
  int64_t head_stride;    /* bytes between consecutive kv heads of a slot, >= head_dim */
  float k_scale, v_scale; /* finite, positive, with finite fp32 reciprocals */
} sqllm_kv_cache_fp8;
int sqllm_qkv_rope_cache_fp8_f16(const sqllm_qkv_rope* r, const sqllm_kv_cache_fp8* c, sqllm_stream_t stream);
int sqllm_qkv_rope_cache_fp8_bf16(const sqllm_qkv_rope* r, const sqllm_kv_cache_fp8* c, sqllm_stream_t stream);
int sqllm_qkv_rope_norm_cache_fp8_f16(const sqllm_qkv_rope* r, const sqllm_rmsnorm* norm, const sqllm_kv_cache_fp8* c, sqllm_stream_t stream);
int sqllm_qkv_rope_norm_cache_fp8_bf16(const sqllm_qkv_rope* r, const sqllm_rmsnorm* norm, const sqllm_kv_cache_fp8* c, sqllm_stream_t stream);
typedef struct sqllm_attn_decode_fp8 {
  const void* q;            /* 16-bit [batch, n_q_heads * head_dim], row stride q_stride elements */
  void* out;                /* 16-bit [batch, n_q_heads * head_dim], row stride out_stride; OVERWRITTEN */
  const void* k_cache;      /* as sqllm_kv_cache_fp8: byte (slot, kv head h, d) at slot*slot_stride + h*head_stride + d */
  const void* v_cache;
  const int32_t* block_table; /* int32 [batch, table_stride], DEVICE memory */
  const int32_t* seq_lens;    /* int32 [batch], DEVICE memory */
  int32_t batch, n_q_heads, n_kv_heads, head_dim;
  int32_t n_slots, block_size, max_blocks, table_stride;   /* max_blocks <= table_stride */
  int64_t slot_stride, head_stride, q_stride, out_stride;  /* the first two in bytes, the last two in 16-bit elements */
  float scale;              /* the caller's, usually 1/sqrt(head_dim); finite */
  void* workspace;          /* sqllm_attn_decode_workspace_bytes(); contents irrelevant */
  float k_scale, v_scale;   /* the cache's, as the front was given them */
} sqllm_attn_decode_fp8;
/* the suffix names the type of q and out */
int sqllm_attn_decode_fp8_f16(const sqllm_attn_decode_fp8* a, sqllm_stream_t stream);
int sqllm_attn_decode_fp8_bf16(const sqllm_attn_decode_fp8* a, sqllm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Decode attention for SEVERAL new tokens per sequence in one read of K and V: the verification step of speculative decoding
 * (2 to 8 drafted tokens) or a chunk of a prompt (16 tokens per step), behind a front that wrote all of the step's tokens.
 * sqllm_attn_append is the fields of sqllm_attn_decode, in the same order, followed by q_lens and q_len;
 * sqllm_attn_append_fp8 is the fields of sqllm_attn_decode_fp8 followed by the same two.
 *
 *   - Rows.  batch counts SEQUENCES, q_len = T is a host field.  Row r = b*T + t of q and out is new token t of sequence b;
 *     strides as before.  block_table is [batch, table_stride]: ONE table row per sequence.  seq_lens[b] is the number of
 *     keys of sequence b INCLUDING all its new tokens, which the front wrote in the same step.
 *   - q_lens: int32 [batch] in DEVICE memory, or NULL.  n_b = q_lens ? q_lens[b] : T is the number of real new tokens of
 *     sequence b; a captured graph follows it updated in place.
 *   - Token t < n_b attends the keys p < L(b,t) = seq_lens[b] - (n_b - 1 - t): causal, bottom-right aligned.
 *   - Values, by reduction to the one-query entry.  Row (b, t) with t < n_b holds EXACTLY THE BITS that sqllm_attn_decode_*
 *     (sqllm_attn_decode_fp8_* for the byte caches) writes for a row with table row b and length L(b,t), all other
 *     descriptor fields equal: the +0 row (L <= 0); the NaN rows (L > max_blocks * block_size, or a table entry outside
 *     [0, n_slots) used by a key below L -- a bad entry at key p makes NaN only the tokens with L > p); NaN propagation and
 *     infinities.  Verifying T tokens at once yields what T decode steps would; isolation, determinism and row independence
 *     carry over.  A key at or beyond L(b,t) that a later token attends never influences row (b, t), whatever bits it holds.
 *   - Rows t >= n_b are padding and are +0.  n_b < 0 is treated as 0.  n_b > T makes all T rows of the sequence NaN.
 *   - As the sibling: unaddressed slots never influence a result; nothing outside the cache extent is read; nothing but the
 *     batch*T rows of out and the workspace is written; the workspace is sqllm_attn_decode_workspace_bytes(batch*q_len, ...),
 *     CONTENTS IRRELEVANT; a call allocates nothing and is capturable: TWO kernel nodes, ONE when
 *     max_blocks * block_size <= SQLLM_ATTN_PARTITION; launch geometry comes from host fields only.
 *
 * Served: head_dim 64 or 128; a head ratio of 1 to 8; q_len 1 to 16; batch*q_len <= 64.  Rejections are the sibling's, with
 * its codes and in its order: q_len < 1 counts among the counts; q_len > 16 or batch*q_len > 64 among the shapes that are not
 * served; q_lens, when given, among the tensors out and the workspace must not overlap; the fp8 scale checks come last.
 * Not covered: more than 16 rows per sequence -- prompt-length prefill stays the integrator's.
 * ------------------------------------------------------------------------------------------- */
typedef struct sqllm_attn_append {
  const void* q;            /* 16-bit [batch * q_len, n_q_heads * head_dim], row stride q_stride elements */
  void* out;                /* 16-bit [batch * q_len, n_q_heads * head_dim], row stride out_stride; OVERWRITTEN */
  const void* k_cache;      /* as sqllm_kv_cache */
  const void* v_cache;
  const int32_t* block_table; /* int32 [batch, table_stride], DEVICE memory: one row per sequence */
  const int32_t* seq_lens;    /* int32 [batch], DEVICE memory: the keys of sequence b, its new tokens included */
  int32_t batch, n_q_heads, n_kv_heads, head_dim;   /* batch: sequences */
  int32_t n_slots, block_size, max_blocks, table_stride;   /* max_blocks <= table_stride */
  int64_t slot_stride, head_stride, q_stride, out_stride;
  float scale;              /* the caller's, usually 1/sqrt(head_dim); finite */
  void* workspace;          /* sqllm_attn_decode_workspace_bytes(batch * q_len, ...); contents irrelevant */
  const int32_t* q_lens;    /* int32 [batch], DEVICE memory, or NULL: q_len real tokens in every sequence */
  int32_t q_len;            /* rows per sequence, 1 to 16 */
} sqllm_attn_append;
int sqllm_attn_append_f16(const sqllm_attn_append* a, sqllm_stream_t stream);
int sqllm_attn_append_bf16(const sqllm_attn_append* a, sqllm_stream_t stream);
typedef struct sqllm_attn_append_fp8 {
  const void* q;            /* 16-bit [batch * q_len, n_q_heads * head_dim], row stride q_stride elements */
  void* out;                /* 16-bit [batch * q_len, n_q_heads * head_dim], row stride out_stride; OVERWRITTEN */
  const void* k_cache;      /* as sqllm_kv_cache_fp8 */
  const void* v_cache;
  const int32_t* block_table; /* int32 [batch, table_stride], DEVICE memory: one row per sequence */
  const int32_t* seq_lens;    /* int32 [batch], DEVICE memory: the keys of sequence b, its new tokens included */
  int32_t batch, n_q_heads, n_kv_heads, head_dim;   /* batch: sequences */
  int32_t n_slots, block_size, max_blocks, table_stride;   /* max_blocks <= table_stride */
  int64_t slot_stride, head_stride, q_stride, out_stride;  /* the first two in bytes, the last two in 16-bit elements */
  float scale;              /* the caller's, usually 1/sqrt(head_dim); finite */
  void* workspace;          /* sqllm_attn_decode_workspace_bytes(batch * q_len, ...); contents irrelevant */
  float k_scale, v_scale;   /* the cache's, as the front was given them */
  const int32_t* q_lens;    /* int32 [batch], DEVICE memory, or NULL */
  int32_t q_len;            /* rows per sequence, 1 to 16 */
} sqllm_attn_append_fp8;
/* the suffix names the type of q and out */
int sqllm_attn_append_fp8_f16(const sqllm_attn_append_fp8* a, sqllm_stream_t stream);
int sqllm_attn_append_fp8_bf16(const sqllm_attn_append_fp8* a, sqllm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Sliding-window decode attention: ONE new query per sequence, attending the LAST `window` keys the cache holds for that
 * sequence (Mistral's sliding_window).  The descriptors are sqllm_attn_decode and sqllm_attn_decode_fp8, unchanged; `window`
 * is a HOST field of the call.
 *
 *   - Keys.  A row of length L = seq_lens[b] with 1 <= L <= max_blocks * block_size attends the keys p in [lo, L),
 *     lo = max(0, L - window): the query's own key included, `window` keys in all -- Hugging Face's Mistral mask
 *     kv_idx > q_idx - sliding_window.  Addressing is sqllm_attn_decode's.
 *   - Values.  The formulas of sqllm_attn_decode (for the byte caches: of sqllm_attn_decode_fp8) over those keys only.
 *   - Order.  The partitions stay the ABSOLUTE key ranges [256 i, 256 i + 256); only the partitions lo / 256 ..
 *     ceil(L / 256) - 1 take part, combined in ascending order; inside a partition the order depends on head_dim,
 *     n_q_heads / n_kv_heads and the key's index alone, as without a window; keys below lo are left out of the first partition
 *     the way keys at or above L are left out of the last.  Hence, bit for bit:
 *       (a) a row with L <= window holds EXACTLY THE BITS sqllm_attn_decode_* (sqllm_attn_decode_fp8_*) gives it;
 *       (b) where lo is a multiple of both 256 and block_size, the row holds exactly the bits the entry without a window gives
 *           a row of length L - lo over the table row advanced by lo / block_size entries.
 *   - What is read.  Only the table entries of blocks that hold an attended key: blocks lo / block_size ..
 *     (L - 1) / block_size.  Entries below them may hold anything (-1, a recycled block, an id far outside the cache) and never
 *     make a row NaN; slots of keys below lo never influence a result, whatever bits they hold.  A caller may free or reuse the
 *     blocks behind the window; a table whose logical blocks repeat over a ring of ceil(window / block_size) + 1 physical
 *     blocks is a rolling buffer, with no further support.
 *   - L <= 0: the row of out is +0.  L > max_blocks * block_size: NaN.  A USED table entry outside [0, n_slots): NaN, and
 *     nothing of the caches is read.  NaN and infinities propagate as in sqllm_attn_decode, over the attended keys only.
 *     Capture, determinism run to run and row by row, and launch geometry from host fields only stay as they are.
 *   - Geometry.  A window touches at most  win_parts = min(n_parts, (window - 1 + 255) / 256 + 1)  partitions (64-bit: window
 *     may be INT32_MAX), n_parts = ceil(max_blocks * block_size / 256).  The partial launch has win_parts workgroups per
 *     (kv head, row); workgroup x of row b serves the absolute partition lo_b / 256 + x, lo_b from seq_lens on the device.  The
 *     workspace holds (max, sum, acc[head_dim]) in fp32 per (row, query head, RELATIVE partition):
 *     sqllm_attn_window_workspace_bytes() = batch * n_q_heads * win_parts * (head_dim + 2) * 4 bytes, never more than
 *     sqllm_attn_decode_workspace_bytes(); 4-byte aligned, CONTENTS IRRELEVANT.  TWO kernel nodes, ONE when win_parts == 1.
 *
 * Served shapes and rejections are sqllm_attn_decode's (sqllm_attn_decode_fp8's), with their codes and in their order;
 * window < 1 counts among the counts (SQLLM_E_SHAPE), before the device is touched; the workspace that must not overlap is
 * the windowed one.  A library without the window kernels answers hipErrorNotSupported, never with the kernels above.
 * Not covered: a window for several new tokens per sequence (sqllm_attn_append_*; expand the rows as that block defines them
 * and call these entries), attention sinks, soft-capping, ALiBi, a wrap-around table mode.
 * ------------------------------------------------------------------------------------------- */
int64_t sqllm_attn_window_workspace_bytes(int32_t batch, int32_t n_q_heads, int32_t head_dim, int32_t max_blocks, int32_t block_size,
                                          int32_t window);
int sqllm_attn_decode_window_f16(const sqllm_attn_decode* a, int32_t window, sqllm_stream_t stream);
int sqllm_attn_decode_window_bf16(const sqllm_attn_decode* a, int32_t window, sqllm_stream_t stream);
/* the suffix names the type of q and out */
int sqllm_attn_decode_window_fp8_f16(const sqllm_attn_decode_fp8* a, int32_t window, sqllm_stream_t stream);
int sqllm_attn_decode_window_fp8_bf16(const sqllm_attn_decode_fp8* a, int32_t window, sqllm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The reference operator names.
 * height/width = mat.size(0)/mat.size(1) of the qweight tensor (quant_cuda_kernel.cu:138-139).
 * ------------------------------------------------------------------------------------------- */

/* replaces vecquant3matmul_nuq_perchannel / vecquant4matmul_nuq_perchannel
 * (quant_cuda.cpp:112-125 -> quant_cuda_kernel.cu:132-154 / :157-179) */
int sqllm_vecquant3matmul_nuq_perchannel(const float* vec, const int32_t* mat, float* mul,
                                         const float* lookup_table, int height, int width,
                                         sqllm_stream_t stream);
int sqllm_vecquant4matmul_nuq_perchannel(const float* vec, const int32_t* mat, float* mul,
                                         const float* lookup_table, int height, int width,
                                         sqllm_stream_t stream);

/* replaces vecquant{3,4}matmul_nuq_perchannel_batched (quant_cuda.cpp:126-139 ->
 * quant_cuda_kernel.cu:182-207 / :210-235); batch = vec.size(0), vec_height = vec.size(1) */
int sqllm_vecquant3matmul_nuq_perchannel_batched(const float* vec, const int32_t* mat, float* mul,
                                                 const float* lookup_table, int height, int width,
                                                 int batch, int vec_height, sqllm_stream_t stream);
int sqllm_vecquant4matmul_nuq_perchannel_batched(const float* vec, const int32_t* mat, float* mul,
                                                 const float* lookup_table, int height, int width,
                                                 int batch, int vec_height, sqllm_stream_t stream);

/* replaces vecquant{3,4}matmul_spmv_nuq_perchannel (quant_cuda.cpp:141-166 ->
 * quant_cuda_kernel.cu:238-281 / :284-327).  `mat` is the CSR value array (the reference's name),
 * `mat3`/`mat4` the packed qweight; nnz = cols.size(0). */
int sqllm_vecquant3matmul_spmv_nuq_perchannel(const int32_t* rows, const int32_t* cols,
                                              const float* mat, const float* vec, float* mul,
                                              int num_rows, const int32_t* mat3,
                                              const float* lookup_table, int height, int width,
                                              int nnz, sqllm_stream_t stream);
int sqllm_vecquant4matmul_spmv_nuq_perchannel(const int32_t* rows, const int32_t* cols,
                                              const float* mat, const float* vec, float* mul,
                                              int num_rows, const int32_t* mat4,
                                              const float* lookup_table, int height, int width,
                                              int nnz, sqllm_stream_t stream);

/* replaces vecquant{3,4}matmul_spmv_nuq_perchannel_batched (quant_cuda.cpp:168-193 ->
 * quant_cuda_kernel.cu:331-382 / :385-435) */
int sqllm_vecquant3matmul_spmv_nuq_perchannel_batched(const int32_t* rows, const int32_t* cols,
                                                      const float* mat, const float* vec,
                                                      float* mul, int num_rows,
                                                      const int32_t* mat3,
                                                      const float* lookup_table, int height,
                                                      int width, int nnz, int batch,
                                                      int vec_height, sqllm_stream_t stream);
int sqllm_vecquant4matmul_spmv_nuq_perchannel_batched(const int32_t* rows, const int32_t* cols,
                                                      const float* mat, const float* vec,
                                                      float* mul, int num_rows,
                                                      const int32_t* mat4,
                                                      const float* lookup_table, int height,
                                                      int width, int nnz, int batch,
                                                      int vec_height, sqllm_stream_t stream);

/* replaces vecquant{3,4}matmul_spmv_hybrid_nuq_perchannel (quant_cuda.cpp:195-224 ->
 * quant_cuda_kernel.cu:439-506 / :510-577); full_rows is [full_height = K, topX] */
int sqllm_vecquant3matmul_spmv_hybrid_nuq_perchannel(
    const int32_t* rows, const int32_t* cols, const float* mat, const float* vec,
    const float* full_rows, const int32_t* full_row_indices, float* mul, int num_rows,
    const int32_t* mat3, const float* lookup_table, int height, int width, int nnz, int topX,
    sqllm_stream_t stream);
int sqllm_vecquant4matmul_spmv_hybrid_nuq_perchannel(
    const int32_t* rows, const int32_t* cols, const float* mat, const float* vec,
    const float* full_rows, const int32_t* full_row_indices, float* mul, int num_rows,
    const int32_t* mat4, const float* lookup_table, int height, int width, int nnz, int topX,
    sqllm_stream_t stream);

/* replaces vecquant{3,4}matmul_spmv_hybrid_nuq_perchannel_batched (quant_cuda.cpp:226-255 ->
 * quant_cuda_kernel.cu:580-657 / :661-738) */
int sqllm_vecquant3matmul_spmv_hybrid_nuq_perchannel_batched(
    const int32_t* rows, const int32_t* cols, const float* mat, const float* vec,
    const float* full_rows, const int32_t* full_row_indices, float* mul, int num_rows,
    const int32_t* mat3, const float* lookup_table, int height, int width, int nnz, int topX,
    int batch, int vec_height, sqllm_stream_t stream);
int sqllm_vecquant4matmul_spmv_hybrid_nuq_perchannel_batched(
    const int32_t* rows, const int32_t* cols, const float* mat, const float* vec,
    const float* full_rows, const int32_t* full_row_indices, float* mul, int num_rows,
    const int32_t* mat4, const float* lookup_table, int height, int width, int nnz, int topX,
    int batch, int vec_height, sqllm_stream_t stream);

/* The two names squeezellm/quant.py:237-250 / :281-294 call for `balanced=True` layers but the
 * reference never defined or exported (quant_cuda.cpp:257-270).  Argument order is quant.py's.
 * `startrows`/`num_threads` describe the reference's intended thread partition; this
 * implementation balances by nnz on its own and ignores them (they may be NULL/0).
 * Semantics = the spmv op: mul += W_lut . vec + CSR . vec. */
int sqllm_vecquant3matmul_spmv_balanced_nuq_perchannel(
    const int32_t* rows, const int32_t* cols, const int32_t* startrows, const float* mat,
    const float* vec, float* mul, const int32_t* mat3, const float* lookup_table, int num_rows,
    int num_threads, int numvals, int height, int width, sqllm_stream_t stream);
int sqllm_vecquant4matmul_spmv_balanced_nuq_perchannel(
    const int32_t* rows, const int32_t* cols, const int32_t* startrows, const float* mat,
    const float* vec, float* mul, const int32_t* mat4, const float* lookup_table, int num_rows,
    int num_threads, int numvals, int height, int width, sqllm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Library services
 * ------------------------------------------------------------------------------------------- */
int sqllm_abi_version(void);
const char* sqllm_error_string(int code); /* static string for SQLLM_E_* and hipError_t values */

/* Launch-geometry knobs (for measurement sweeps; defaults are chosen per shape).  Options are kept
 * PER DEVICE: a set / get applies to the calling thread's current HIP device.
 *   "target_wgs"      dense workgroups to aim for (default 0 = 1 x CU count for layers <= 12 MB,
 *                     3 x CU count above)
 *   "groups_per_wave" force the K units each wave walks (default 0 = derived from target_wgs)
 *   "sparse_last"     1 = CSR / top-X workgroups after the dense ones in the grid (default 0: first)
 *   "cu_count"        override the CU count used for planning (GPU-less tests)
 *   "mfma_min_batch", "cols_min_batch", "cols_max_batch"
 *                     routing of the *_batched operators by batch size: cols_min_batch .. cols_max_batch
 *                     rows run on the column-lane kernel (lane = output column, vec in SGPRs),
 *                     mfma_min_batch rows and more on the matrix cores, everything else on the
 *                     batch tiles of the batch-1 kernel (tiles of exactly 1..8 rows).  Defaults (value 0 =
 *                     measured default, which depends on the bit width; get_option returns the stored 0): 4-bit 2..4 / 7
 *                     (9 for an op of <= 16 MB of packed weights alone in its launch), 3-bit 2..8 / 9.
 *                     At ONE row (batch 1, or the matvec names) the defaults route by launch shape instead (round 6, sqllm_capi.hip: cols_pays_batch1 --
 *                     dense-only launches of >= 16 MB that are a three-op group, a tall single op, a 3-bit two-op group or -- round 7 -- a 4-bit two-op group
 *                     whose one-row plan is whole ranges per column tile with >= 95 % of their unit slots live (7B gate/up: two ranges of 256 units per tile,
 *                     -10.6 % against the fused kernel build against build; 13B: one of 640, -13 %; 65B: one of 1024, -10.5 % -- these two measured once each, on the previous build with the cut asked for through "target_wgs"), and the 7B-class sparse groups,
 *                     take the column-lane kernel; launches with sparse roles otherwise keep the fused kernel: 7B s45 gate/up 15.3 against 19.2 us); an explicit cols_min_batch = 1 sends every one-row launch there, a huge cols_min_batch none.
 *                     With the two cols_* options at their defaults the column-lane kernel is further reserved
 *                     for what it measured faster on: 4-bit, groups of three or more ops (up to 4 rows) and single ops of
 *                     >= 20 MB packed weights (up to 6 rows); 3-bit, >= 16 MB at up to 4 rows or N >= 8192; setting either option
 *                     takes the range at its word.
 *   "cols_groups"     1 (default): a GROUP of ops over one vec (sqllm_launch_group) may take the column-lane kernel
 *                     too, as one launch, judged by the sum of its columns; 0: groups stay on the batch tiles
 *   "cols_slot_cut"   0 (default): a ONE-ROW launch of the column-lane kernel whose equal ranges would cross column-tile boundaries is cut into whole
 *                     ranges per tile instead -- the cut that executes the fewest unit slots of the kernel's loop (it works in quanta of 64 units per
 *                     workgroup at 4 bits, 32 at 3 bits) among those whose workgroups are resident at once; a plan that is tile-aligned already stays.
 *                     1: every one-row plan is re-cut that way wherever that executes no more slots (measured slower on the 7B down_proj).
 *                     "target_wgs" / "groups_per_wave" override both: with either set the plan is that of the shared range cut, and the dense-only 4-bit
 *                     two-op group, whose one-row route depends on this cut, goes back to the fused kernel unless "cols_min_batch" = 1 forces the
 *                     column-lane kernel (geometry sweeps on that pair set it).
 *   "sparse_transpose" 1 (default): the sparse terms of a batched op (mfma_min_batch rows and more) read a transposed copy of
 *                     vec (lane = batch row, coalesced) out of the caller's workspace (sqllm_launch_ws) or, for the
 *                     workspace-less names, out of stream-ordered scratch; 0: they gather from vec itself, as they do
 *                     anyway when neither can be had
 *                     The scratch is stream-ordered (hipMallocAsync / hipFreeAsync on the caller's
 *                     stream, K x ceil64(batch) floats per op or group); on first use per device the
 *                     library raises the release threshold of the device's DEFAULT memory pool to
 *                     1 GiB (never lowers it) so that the block survives synchronisations.
 *   "scratch_pool_threshold" 1 (default): on first use of that scratch per device the library raises the release threshold of
 *                     the device's DEFAULT memory pool to 1 GiB (process-wide state, never lowered); 0: it leaves the pool alone
 *                     (every synchronisation may then hand the scratch back to the OS)
 *   "scratch_in_capture" 1 (default): that scratch is also taken while the stream is capturing --
 *                     a captured wide-batch op with a CSR term then carries a memory-allocation
 *                     and a memory-free node in the graph; 0 keeps captures allocation-free (the
 *                     CSR term gathers from vec instead)
 *   "mfma_split"      1 (default): the dense term of a wide batch (mfma_min_batch rows and more) runs on the bf16 matrix
 *                     instructions with every fp32 operand split EXACTLY into three bf16 values and six of the nine partial
 *                     products kept (fp32-class results, 2.7 x the matrix rate of the fp32 instruction); 0: the fp32 matrix
 *                     instruction (bit-for-bit an fp32 FMA chain per output)
 *   "mfma_fuse_small" 1 (default, with mfma_split): from mfma_min_batch up to 16 rows an op -- or a whole GROUP of ops over one vec
 *                     (sqllm_launch_group) -- is ONE launch of the split matrix-core kernel: every dense workgroup walks the CSR
 *                     non-zeros of its own 64 output channels (no chunk workgroups), the top-X slabs ride in the same grid; with a
 *                     workspace (or, eagerly, scratch) a small kernel in front transposes vec for those two (K < 2^26);
 *                     0: one launch per op plus a launch for its sparse terms (as from 17 rows on)
 *   "mfma_fuse_sparse" 1 (default, with mfma_split): from 17 rows up to the wide form an op's CSR / top-X workgroups run in the grid of
 *                     its dense launch -- always up to 64 rows (33-64 rows: as two 32-row passes if they outnumber the CUs),
 *                     beyond that while they are fewer than the CUs; 0: a launch of their own first
 *   "mfma_wide_min_batch"  0 (default): with mfma_split, the WIDE form of that kernel -- workgroups of eight 64-column tiles, one per
 *                     wave, all on the same k's: the vec values of a step are fetched once per workgroup instead of once per tile --
 *                     takes over from 64 rows up once batch * K * N >= 5.7e9 (3-bit: 4e9; three times that while the stream is
 *                     capturing; without scratch: once its units of 64 rows x 8 tiles fill 80 % of the CUs).  13B shapes: 128
 *                     rows 104 -> 85 us, 2048 rows 1.66 -> 0.96 ms.  n > 0: from n rows on, whatever the shape; a huge value:
 *                     never.  Geometry through sqllm_plan_query: grid_y = 1, dense_blocks = workgroups (whole rounds of units
 *                     over all of K + the last round's units in k_slices K slices of groups_per_wave units, whose sums a
 *                     second launch adds to mul).
 *   "split_planes_min_batch"  0 (default: 64): rows from which the wide form takes vec split ONCE into bf16 planes in stream-ordered
 *                     scratch (6 bytes per vec value, rows padded to 64, plus 16 KB per K slice and tile; a split kernel in front of the op; fp16-born vec -- what
 *                     QuantLinearLUT.forward passes -- then costs five partial products instead of six); below, or without
 *                     scratch (scratch_in_capture = 0 while capturing, allocation failure), every wave splits its values in
 *                     registers and K slices add atomically; a huge value: never.
 *   "small_wgs_per_cu" 0 (default: 2): dense workgroups per CU the planner of the fused small launch (mfma_min_batch .. 16 rows)
 *                     aims at -- one round of workgroups, as many as the kernel's registers admit at once
 *   "small_reserve_topx" 0 (default): with a transposed vec at hand the dense ranges of that launch are always planned for the
 *                     slots the (8-24) top-X workgroups leave; 1 does the same without one (one workgroup per top-X slab:
 *                     measured slower, profiles/r05_small_split_reserve.txt)
 *   "small_planes"    1 (default): with a transposed vec at hand the fused small launch also takes vec split into bf16 planes
 *                     (written by the same kernel in front); 0: its dense term splits vec in registers
 *   "validate_csr"    debugging aid, default 0.  1 = before every launch that carries a CSR term,
 *                     check ON THE DEVICE that rows[] is non-decreasing with rows[0] == 0 and
 *                     rows[N] == nnz, and return SQLLM_E_SPARSE otherwise.  Blocks the host (one
 *                     tiny kernel, a 4-byte read-back, a stream synchronise; 4 bytes of stream-ordered
 *                     scratch on the current device per check); skipped while the stream is capturing.
 *                     Meant for the fused linear, which counts on `rows` to detect completion.
 * Returns SQLLM_E_OPTION for an unknown name and for a value outside the option's range: switches take 0 / 1 only,
 * "small_wgs_per_cu" 0..8, "cu_count" up to 65536, "target_wgs" / "groups_per_wave" up to 2^24, the *_min_batch /
 * *_max_batch thresholds any non-negative int.  No value of any option changes a result beyond fp32 round-off. */
int sqllm_set_option(const char* name, int value);
int sqllm_get_option(const char* name, int* value);

/* Geometry the library would use for this op launched ALONE (sqllm_launch / the operator names).  Ops
 * that share a launch (sqllm_launch_group) are planned with other workgroup counts (the launch's
 * workgroup target is divided between them), on the kernel the GROUP routes to: the batch tiles, the
 * column-lane kernel (judged by the sum of the group's columns, option "cols_groups") or, from
 * mfma_min_batch up to 16 rows, the split matrix-core kernel. */
typedef struct sqllm_plan {
  int32_t col_tiles, k_slices, groups_per_wave, dense_blocks, csr_blocks, topx_blocks, grid_x, grid_y;
} sqllm_plan;
int sqllm_plan_query(const sqllm_op* op, sqllm_plan* plan);

/* ---------------------------------------------------------------------------------------------
 * Offline quantisation: the lookup tables of a checkpoint (the reference computes them with one
 * sklearn KMeans per output channel on the CPU, quantization/nuq.py:50-58).
 * ------------------------------------------------------------------------------------------- */
typedef struct sqllm_nuq {
  int32_t bits, N, K;    /* bits in {3, 4}; 2^bits <= K <= 65535; N >= 1 */
  const float* values;   /* [N, K], each row ascending */
  const float* weights;  /* [N, K], >= 0, same order; NULL = all ones */
  float* centroids;      /* [N, 2^bits] out, ascending */
  double* cost;          /* [N] out, may be NULL */
} sqllm_nuq;

/* Bytes of caller workspace sqllm_nuq_fit needs for these shapes (the pointers are not looked at; no GPU
 * needed), or a negative SQLLM_E_* code for bad shapes.  Grows with min(N, 1024) x K. */
int64_t sqllm_nuq_workspace_bytes(const sqllm_nuq* d);

/* Exact weighted 1-D k-means of every row: the 2^bits centroids of the partition of the row into 2^bits
 * contiguous ranges that minimises sum w (x - c)^2, each centroid the weighted mean of its range (fp64
 * dynamic programming over prefix sums, divide and conquer per level: O(2^bits K log K) per row).  cost[r]
 * (if given) is the minimum, summed in fp64 around the fp64 centroids.  A row whose weights sum to 0 is
 * fitted with unit weights; a range of zero total weight gets the unweighted mean of its values; a row of
 * fewer than 2^bits distinct values repeats its largest value.  Enqueues one kernel on `stream`, allocates
 * nothing; `workspace` holds workspace_bytes >= sqllm_nuq_workspace_bytes(d) of device memory, contents
 * irrelevant before and after, one call at a time.  SQLLM_E_BITS / SQLLM_E_SHAPE / SQLLM_E_NULL (a NULL
 * descriptor, values, centroids or workspace) before the device is touched; a short workspace is SQLLM_E_SHAPE. */
int sqllm_nuq_fit(const sqllm_nuq* d, void* workspace, int64_t workspace_bytes, sqllm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Dense export: the matrix the three weight terms of an op stand for,
 *
 *     W[n, k] = lookup_table[n, idx(k, n)] + sum CSR(n, k) + sum_c [full_row_indices[c] == n] full_rows[k, c]
 *
 * written as out[n * ld + k] for every n < N, k < K: [N, K] with K contiguous, the layout of nn.Linear.weight.
 * Every element is summed in fp32 (duplicate CSR entries and duplicate top-X indices accumulate, as in the op)
 * and rounded ONCE: not at all for SQLLM_DTYPE_F32, to nearest-even _Float16 for SQLLM_DTYPE_F16, to nearest-even bf16
 * for SQLLM_DTYPE_BF16 (overflow gives +-inf; NaN / inf in the operands propagate).  A position with at most one sparse contribution is bit-exact:
 * the table entry, or one fp32 add.  Elements k in [K, ld) of a row are NOT written; nothing else is.
 * Enqueues ONE kernel on `stream`; allocates nothing, retains nothing, never synchronises (option "validate_csr"
 * aside, which blocks as it does for every launch): a stream capture of the call holds one kernel node.
 * SQLLM_E_NULL for a NULL descriptor, out, qweight or lookup_table; SQLLM_E_BITS; SQLLM_E_SHAPE for bad K / N,
 * ld < K, an ld that is no multiple of 8 (fp16, bf16) / 4 (fp32) or an unknown out_dtype; SQLLM_E_ALIGN for a qweight
 * or out that is not 16-byte aligned; SQLLM_E_SPARSE as for sqllm_launch -- all before the device is touched.
 * ------------------------------------------------------------------------------------------- */
#define SQLLM_DTYPE_F32 0
#define SQLLM_DTYPE_F16 1
#define SQLLM_DTYPE_BF16 3 /* sqllm_dequant's out_dtype only (2 stays unassigned); the offline entry points below take F32 / F16 */
typedef struct sqllm_dequant_desc {
  sqllm_op op;       /* bits, K, N, qweight, lookup_table, CSR and top-X operands as for sqllm_launch;
                        vec, mul and batch are ignored */
  void* out;         /* [N, ld] of out_dtype, 16-byte aligned */
  int64_t ld;        /* elements per output row, >= K; for fp16 and bf16 a multiple of 8, for fp32 of 4 */
  int32_t out_dtype; /* SQLLM_DTYPE_F32 / _F16 / _BF16 */
} sqllm_dequant_desc;
int sqllm_dequant(const sqllm_dequant_desc* d, sqllm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Encode: the inverse of sqllm_dequant -- from a weight matrix and its per-channel codebooks to the operands of an op,
 *
 *     idx(k, n) = the first j minimising |fl32(w[n, k] - lookup_table[n, j])|      (strict < over ascending j)
 *     z_n       = the entry of lookup_table[n, :] with the smallest |c|            (ties: the lowest index)
 *
 * weight is [N, ld] with K contiguous (nn.Linear.weight), fp32 or fp16 (widened exactly); `mask` (optional) is [N, K],
 * one byte per weight, non-zero = outlier candidate.  A position is an OUTLIER iff mask != 0, w != 0 and
 * fl32(w - z_n) != 0.  Every masked position (outlier or not) gets the index of z_n in qweight; every other position
 * idx(k, n).  These are the rules of the reference's packer (quant.py:117-131), so a layer encoded here equals one it packed.
 *
 * sqllm_encode writes all of qweight [K/32*bits, N] and, with a mask, all of rows [N + 1]: the exclusive scan of the
 * per-channel outlier counts (rows[0] == 0, rows[N] == nnz < 2^31), overwritten, never accumulated into.  It enqueues
 * one kernel without a mask and three nodes with one (a zero-fill of rows, the encode kernel, the scan); the counts are
 * integers, so the result does not depend on any order.
 * sqllm_encode_csr takes the same descriptor with the rows sqllm_encode wrote, and `nnz` >= rows[N], the capacity of
 * cols / vals (the caller reads rows[N] back to size them).  It writes cols[e] = k and vals[e] = fl32(w - z_n) for every
 * outlier, channel by channel and in ascending k within a channel, each at a position computed from rows and its rank
 * -- no atomics: the result is deterministic, byte for byte.  Nothing is written at or beyond cols / vals [nnz].  One kernel.
 * Both allocate nothing, retain nothing and never synchronise: a stream capture holds kernel and memset nodes only.
 * SQLLM_E_NULL for a NULL descriptor, weight, lookup_table or qweight, for NULL rows with a mask, and in
 * sqllm_encode_csr for a NULL mask, rows, cols or vals; SQLLM_E_BITS; SQLLM_E_SHAPE for bad K / N, ld < K, an ld that is
 * no multiple of 8 (fp16) / 4 (fp32) or an unknown weight_dtype; SQLLM_E_ALIGN for a weight or qweight that is not
 * 16-byte aligned or a mask that is not 8-byte aligned; SQLLM_E_SPARSE for nnz < 0 -- all before the device is touched.
 * ------------------------------------------------------------------------------------------- */
typedef struct sqllm_encode_desc {
  int32_t bits, K, N;        /* bits in {3, 4}; K % 32 == 0; N % 4 == 0 */
  int32_t weight_dtype;      /* SQLLM_DTYPE_* */
  const void* weight;        /* [N, ld] of weight_dtype, 16-byte aligned */
  int64_t ld;                /* elements per weight row, >= K; for fp16 a multiple of 8, for fp32 of 4 */
  const float* lookup_table; /* [N, 2^bits] */
  const uint8_t* mask;       /* [N, K] or NULL: no outliers, rows is not touched */
  int32_t* qweight;          /* out: [K/32*bits, N], 16-byte aligned */
  int32_t* rows;             /* [N + 1]: written by sqllm_encode, read by sqllm_encode_csr */
} sqllm_encode_desc;
int sqllm_encode(const sqllm_encode_desc* d, sqllm_stream_t stream);
int sqllm_encode_csr(const sqllm_encode_desc* d, int32_t* cols, float* vals, int32_t nnz, sqllm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Outlier selection: exact order statistics of a whole matrix, and the mask sqllm_encode takes.
 *
 * The reference decides a linear's outliers from the quartiles of all its weights (np.quantile on the CPU,
 * quantization/generate_outlier_config.py:47-53) and from the num-th largest gradient (topk, squeezellm/outliers.py:15-18).
 * Both are order statistics of one matrix of 16 M .. 180 M elements.  sqllm_select finds up to 8 of them in one call:
 *
 *     out[i]  = np.sort(values[:, :cols], axis=None)[ranks[i]]     compared as a VALUE: -0.0 and +0.0 are one value,
 *                                                                  returned as +0.0; +-inf order as usual
 *     less[i] = (values[:, :cols] < out[i]).sum()
 *
 * by a most-significant-digit radix select on the order-preserving unsigned key of every element (-0 -> +0, then all bits
 * of a negative value flipped, the sign bit of a non-negative one set; fp16 is widened exactly, so its keys are taken on
 * the 16 bits of the half): three passes over the matrix for fp32 (digits of 11 + 11 + 10 bits), two for fp16 (11 + 5),
 * each a histogram kernel (16-byte non-temporal loads, one LDS histogram per live prefix -- ranks that share a prefix
 * share one --, 64-bit integer atomics for the non-empty bins) and a one-workgroup kernel that picks every rank's bin.
 * Only integers are counted: the result is a function of the input alone, two runs are byte-identical.  NaN inputs give an
 * unspecified result (never a fault or a hang; nuq checks finiteness before it calls).  Elements [cols, ld) of a row are never read.
 * The call enqueues one memset node and 2 x passes kernels on `stream`; it allocates nothing, retains nothing and never
 * synchronises.  `workspace`: workspace_bytes >= sqllm_select_workspace_bytes(d) of device memory, 16-byte aligned,
 * contents irrelevant before and after (the library zero-fills what it needs), one call at a time.
 * SQLLM_E_NULL for a NULL descriptor, values, out or workspace; SQLLM_E_SHAPE for an unknown dtype, n_ranks outside 1..8,
 * a rank outside [0, rows * cols), rows or cols < 1, cols or ld that is no multiple of 4 (fp32) / 8 (fp16), ld < cols,
 * rows * cols >= 2^40 or a short workspace; SQLLM_E_ALIGN for values or workspace not 16-byte aligned (out: 4, less: 8)
 * -- all before the device is touched.
 * ------------------------------------------------------------------------------------------- */
#define SQLLM_SELECT_MAX_RANKS 8
typedef struct sqllm_select_desc {
  int32_t dtype;               /* SQLLM_DTYPE_F32 / _F16 (widened exactly) */
  int32_t n_ranks;             /* 1..8 */
  const void* values;          /* [rows, ld], 16-byte aligned; elements [cols, ld) of a row are never read */
  int64_t rows, cols, ld;      /* cols % 4 == 0 (fp32) / % 8 == 0 (fp16); ld >= cols, same multiple; rows*cols < 2^40 */
  int64_t ranks[SQLLM_SELECT_MAX_RANKS]; /* 0-based positions in ascending order, each in [0, rows*cols); any order, repeats allowed */
  float* out;                  /* device [n_ranks]: the value at each rank */
  int64_t* less;               /* device [n_ranks] or NULL: how many elements are strictly below out[i] */
} sqllm_select_desc;
/* bytes of workspace sqllm_select needs for this descriptor (the pointers are not looked at; no GPU needed; grows with
 * n_ranks), or a negative SQLLM_E_* code for bad shapes */
int64_t sqllm_select_workspace_bytes(const sqllm_select_desc* d);
int sqllm_select(const sqllm_select_desc* d, void* workspace, int64_t workspace_bytes, sqllm_stream_t stream);

/* The outlier mask of one linear (nuq.outlier_mask; squeezellm/outliers.py:18,53-55), both operands widened to fp32:
 *
 *     mask[n, k] = (g[n, k] > *g_threshold) || (w[n, k] >= *w_threshold) || (w[n, k] <= -*w_threshold)
 *
 * a NULL gradient / w_threshold contributes false.  The thresholds are DEVICE pointers: a sqllm_select on the same stream
 * feeds the mask without a host round trip.  mask is written as bytes 0 / 1 for all of [N, K] and nothing else; *count is
 * OVERWRITTEN with the number of ones.  One kernel (one integer atomic per workgroup) plus a memset node for count;
 * allocates nothing, retains nothing, never synchronises.
 * SQLLM_E_NULL for a NULL descriptor or weight, a gradient without g_threshold or the reverse, mask and count both NULL;
 * SQLLM_E_SHAPE for K % 32 != 0, K < 1, N < 1, N * K >= 2^40 (the select's bound; the kernel's 32-bit partial counts are
 * argued below it), an unknown dtype, ld < K or an ld that is no multiple of 8 (fp16) / 4 (fp32);
 * SQLLM_E_ALIGN for a weight or gradient not 16-byte aligned, a mask or count not 8-byte aligned, a threshold not 4-byte
 * aligned -- all before the device is touched. */
typedef struct sqllm_outlier_desc {
  int32_t weight_dtype, grad_dtype;   /* SQLLM_DTYPE_* */
  int32_t K, N;                       /* K % 32 == 0, N >= 1, N * K < 2^40 */
  const void* weight;  int64_t ld_w;  /* [N, ld_w], 16-byte aligned, ld rules of sqllm_encode */
  const void* gradient; int64_t ld_g; /* same rules, or NULL: no sensitivity step */
  const float* g_threshold;           /* DEVICE [1]; required iff gradient != NULL */
  const float* w_threshold;           /* DEVICE [1], or NULL: no threshold step */
  uint8_t* mask;                      /* out [N, K], 0 / 1, 8-byte aligned; NULL: count only */
  int64_t* count;                     /* DEVICE [1] or NULL: number of 1s, OVERWRITTEN */
} sqllm_outlier_desc;
int sqllm_outlier_mask(const sqllm_outlier_desc* d, sqllm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SQLLM_HIP_H */
