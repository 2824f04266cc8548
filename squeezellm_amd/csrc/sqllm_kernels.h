// Internal interface between the C-ABI layer (sqllm_capi.hip) and the kernels (sqllm_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Measurement switches.  Every one of them selects a kernel variant that is slower or deliberately
// WRONG (an ablation); they exist only in measurement builds (python -m squeezellm_amd.build
// --ablation -> libsqllm_hip_ablation.so, never the product library).  A product build that sets
// one of them does not compile.
#ifndef SQLLM_ABLATION_BUILD
#if defined(SQLLM_PAIR3) || defined(SQLLM_PAIR3_NOCONFLICT) || defined(SQLLM_MFMA_VAR) || defined(SQLLM_MFMA_FAKE) || \
    defined(SQLLM_HALF_STAGES) || defined(SQLLM_WAVES) || defined(SQLLM_STREAM_RING) || defined(SQLLM_STREAM_WGCU) || \
    defined(SQLLM_STREAM_PRO) || defined(SQLLM_TOPX_ROWS) || defined(SQLLM_CSR_CHUNK)
#error "kernel variant switches need -DSQLLM_ABLATION_BUILD (python -m squeezellm_amd.build --ablation)"
#endif
#endif
#ifndef SQLLM_WAVES
#define SQLLM_WAVES 8  // waves per workgroup (measurement builds: 4)
#endif
#ifndef SQLLM_CSR_CHUNK
#define SQLLM_CSR_CHUNK 1024  // non-zeros per CSR workgroup (measurement builds: 2048)
#endif
#ifndef SQLLM_TOPX_ROWS
#define SQLLM_TOPX_ROWS 256  // k's per top-X slab (measured 128 / 256 / 512: profiles/r03_csr_chunk_topx_slab.txt)
#endif

namespace sqllm {

constexpr int kWaves = SQLLM_WAVES;          // waves per workgroup (512 threads)
constexpr int kTileN = 64;         // output columns per dense tile = 16 lanes x 4 (one dwordx4 each)
constexpr int kCsrChunk = SQLLM_CSR_CHUNK;  // non-zeros per CSR workgroup (a multiple of 1024: a lane holds a run of 2+)
constexpr int kCsrSpanMax = 2048;  // CSR rows a chunk may span and still accumulate in LDS
constexpr int kCsrEdge = 256;      // ... minus this many in the gated pair's kernels (csr_role, ORD: the table of the rows that waves share)
constexpr int kCsrXtSpan = 191;    // ... and still keep a 64-row tile of sums in LDS (wide batches, transposed vec; half of it: a 128-row tile)
constexpr int kSparsePassRows = 128;  // batch rows per workgroup of the wide-batch sparse launch
constexpr int kTopxRows = SQLLM_TOPX_ROWS;  // k's per top-X slab (a multiple of 32)
constexpr int kTopxLds = 1024;     // topX up to which slab sums are kept in LDS
constexpr int kMaxBatchTile = 8;   // batch rows handled per weight pass
constexpr int kMaxSlices = 120;    // K slices per column tile
constexpr int kMaxContrib = 63;    // fused linear: contributions one column may receive (6-bit count under the three non-finite flags)

// The decode quantum of the column-lane kernel (sqllm_kernels.hip: dense_role_cols), in ONE place for the kernel and for the planner's one-row
// cut (sqllm_capi.hip: cut_ranges_one_row): a wave loads cols_chunk_units(bits) units per batch ("chunk") and keeps kColsChunksInFlight chunks in
// flight; its loop runs whole rounds of them ("chunk pairs"), so a wave executes unit SLOTS in multiples of cols_wave_quantum(bits) and a
// workgroup in multiples of cols_quantum(bits) = 64 units at 4 bits, 32 at 3 bits.  A slot without a unit costs what a live one does.
constexpr int kColsChunksInFlight = 2;
constexpr int cols_chunk_units(int bits) { return bits == 4 ? 4 : 2; }
constexpr int cols_wave_quantum(int bits) { return kColsChunksInFlight * cols_chunk_units(bits); }
constexpr int cols_quantum(int bits) { return cols_wave_quantum(bits) * kWaves; }

// LDS floats of one kernel instantiation: max over roles of
//   dense: codebooks 4 column sub-tables * lut_entries * 32 slots (2 copies of 16 lanes) PLUS the
//          cross-wave slabs waves * BT * 64, the epilogue ticket and the fused linear's top-X
//          sums BT * 64 (the slabs must not overlap the codebooks: the combine is barrier-free)
//   csr  : kCsrSpanMax ints + kCsrSpanMax floats
//   topx : kTopxLds
constexpr int cmax(int a, int b) { return a > b ? a : b; }
constexpr int lds_floats(int lut_entries, int waves, int bt, bool pair3 = false) {
  // pair3: the 3-bit batch-1 kernels stage 64-entry PAIR tables, 4 x 64 x 128 B per tile
  return cmax((pair3 ? 4 * 64 * 32 : 4 * lut_entries * 32) + waves * bt * kTileN + 4 + bt * kTileN,
              cmax(2 * kCsrSpanMax, kTopxLds));
}

// Launch geometry, computed on the host (sqllm_capi.hip: make_plan) and passed by value.
struct KernelGeom {
  int K, N, batch;
  int col_tiles;        // ceil(N / 64)
  int units_total;      // K / 8 (w4: qweight rows) or K / 32 (w3: three-row units)
  int units_per_wg;     // K-slice length of a workgroup, in units (a multiple of waves * 4)
  int k_slices;         // ceil(units_total / units_per_wg)
  int dense_blocks;     // col_tiles * k_slices
  int dense_block0;     // first dense blockIdx.x (csr + topx blocks rounded up to a multiple of 8)
  int csr_blocks;       // ceil(nnz / kCsrChunk) -- of 2 * kCsrChunk with csr_wide --, 0 without a sparse term or with fold_csr
  int topx_blocks;      // ceil(K / kTopxRows), 0 without a top-X term
  int nnz, topX;
  int sparse_last;      // 1: CSR / top-X workgroups come after the dense ones in the grid
  int fold_csr;         // 1: the CSR term is walked by the dense workgroups themselves (fused small launch: csr_tile_fold_staged; csr_blocks = 0)
  int csr_wide;         // 1: the CSR workgroups take 2 * kCsrChunk non-zeros each (csr_blocks counts those)
  int dense_prio;       // issue priority inside a batch-1 launch with sparse roles (sqllm_capi.hip: set_role_priority): 1 = the dense workgroups' waves at s_setprio 1, 2 = the CSR / top-X workgroups' waves, 0 = all equal
};

constexpr int kMaxSegments = 4;   // ops one launch can cover (they share vec, K, bits, batch)

// One op of a launch: its operands and its geometry.
struct Segment {
  const uint32_t* q;
  float* y;
  const float* lut;
  const int* rows;
  const int* cols;
  const float* vals;
  const float* full_rows;
  const int* full_idx;
  // fused-linear launches only (sqllm_linear_f16 / _bf16): `y` is then the plane of 64-bit accumulator
  // words [batch, N] in the caller's workspace (all zero between launches) and the finished
  // columns leave as fp16 / bf16
  const float* bias;    // fp32 [N] or null
  void* out16;          // fp16 or bf16 [batch, N]
  KernelGeom gm;
};

// Kernel argument block: up to kMaxSegments ops over the same input vector.  Workgroup ids
// [block0[s], block0[s+1]) belong to segment s (each range is a multiple of 8 long, so a dense
// tile's id modulo 8 -- its XCD -- does not depend on the segments before it).
struct GroupArgs {
  int n_seg;
  int block0[kMaxSegments + 1];
  Segment seg[kMaxSegments];
};

struct LaunchArgs {
  const void* x;        // fp32 (operator launches) or fp16 / bf16 (fused-linear launches)
  bool linear = false;  // fused-linear launch: fp16 in / fp16 out, bias, self-cleaning workspace
  bool bf16 = false;    // ... with bf16 at both ends instead (sqllm_linear_bf16.hip: launch_linear_bf16)
  GroupArgs ga;
  hipEvent_t ev_start = nullptr;  // optional: recorded at this kernel's begin / end (profiling aid)
  hipEvent_t ev_stop = nullptr;
  int ablate = 0;  // measurement builds only (SQLLM_ABLATION_BUILD)
  int lds_pad = 0;  // measurement builds only: bytes of unused dynamic LDS per workgroup (caps the workgroups per CU)
  const float* xT = nullptr;  // wide-batch launches: transposed copy of x ([K, Bp]) for the CSR role, or null
  int Bp = 0;
  // wide-batch launches on the split matrix-core kernel: vec already split into bf16 planes (split_vec), or null
  const void* planes = nullptr;
  const uint32_t* plane_flags = nullptr;  // kSplitFlagWgs words: any non-zero lo part?
  bool wide = false;  // the geometry is make_plan_wide's: workgroups of eight column tiles (sqllm_mfma_wide.hip: sqllm_fused_wide)
  int wide_full_units = 0;  // ... and this many of them over all of K; the rest in gm.k_slices slices
  float* wide_slabs = nullptr;  // scratch for the slices' sums (wide_slab_bytes), or null: they add atomically
  int row_blocks = 0;  // tile form: blocks of 16 rows per pass (1, 2 or 4); 0 = mfma_row_blocks(batch)
};

// batch rows handled per weight pass for a given batch size (template instantiations 1/2/4/8)
inline int batch_tile(int batch) { return batch <= 1 ? 1 : batch == 2 ? 2 : batch <= 4 ? 4 : 8; }
// ... of the fused batch-tile kernel behind the OPERATOR names (sqllm_fused_matvec<BITS, BT>, not the fused linear): a tile
// of exactly 3, 5, 6 or 7 rows too -- a 5-row batch on the 8-row tile pays the broadcasts and FMAs of 8 (round 6) -- and of the column-lane kernel
inline int batch_tile_op(int batch) { return (batch == 3 || batch == 5 || batch == 6 || batch == 7) ? batch : batch_tile(batch); }

// blocks of 16 batch rows one pass of the wide-batch (matrix-core) kernel covers: 1, 2 or 4
inline int mfma_row_blocks(int batch) { return batch <= 16 ? 1 : batch <= 32 ? 2 : 4; }

hipError_t launch_fused(int bits, const LaunchArgs& a, hipStream_t stream);
hipError_t launch_linear_bf16(int bits, const LaunchArgs& a, hipStream_t stream);  // the fused linear, bf16 in / bf16 out (a.linear && a.bf16): launch_fused hands such launches on
extern bool (*g_fused_variant)(int bits, const LaunchArgs& a, hipStream_t stream, hipError_t* err);  // measurement library hook (null in the product)
// The fronts: fused-linear launches whose columns are finished by a kernel of their own.  Each kind is one kernel file, which
// registers its launcher in g_launch_front when it is linked in (the table is defined all null in sqllm_capi.hip: the host layer
// links without the kernels, and a missing kernel is an error -- hipErrorNotSupported --, never a fallback).
//   gated (sqllm_gated_f16 / _bf16): exactly two segments, gate and up, on the kernel of sqllm_linear_gated.hip; FrontCall::pair is
//     the plane of pair words [batch, N].
//   ep (sqllm_linear_ep_f16 / _bf16): exactly one segment on the kernel of sqllm_linear_ep.hip; `residual`: 16-bit [batch, N] of the
//     output's type or null, `act`: SQLLM_ACT_*.
//   qkv (sqllm_qkv_rope_f16 / _bf16): exactly three segments, q, k and v, on the kernel of sqllm_linear_qkv.hip, which rotates q
//     and k by the rotary position embedding as their columns finish.
struct QkvRope {
  void* pair_q;          // plane of pair words [batch, N_q / 2], all zero between launches
  void* pair_k;          // ... [batch, N_k / 2]
  const float* cos;      // fp32 [n_pos, head_dim / 2], device memory
  const float* sin;
  const int* positions;  // int32 [batch], device memory
  int n_pos, head_dim;
  bool interleaved;      // SQLLM_ROPE_INTERLEAVED (partner next door) instead of SQLLM_ROPE_HALF (partner head_dim / 2 away)
};
//   gated_norm, qkv_norm (sqllm_gated_norm_* / sqllm_qkv_rope_norm_*): the two launches above with RMSNorm as a prologue, on the
//     kernels of sqllm_linear_gated_norm.hip / sqllm_linear_qkv_norm.hip -- every element of vec is read as
//     float(x) * float(weight[k]) * r[row].
struct VecNorm {
  const void* weight;  // 16-bit [K] of vec's type, device memory
  float eps;
};
//   qkv_cache, qkv_norm_cache (sqllm_qkv_rope_cache_* / sqllm_qkv_rope_norm_cache_*): the two q/k/v launches above on the kernels of
//     sqllm_linear_qkv_cache.hip / sqllm_linear_qkv_norm_cache.hip, whose finishers store the elements of k and v at
//     cache + slots[b] * slot_stride + head * head_stride + d as well as, or instead of, in the outputs.
struct KvCache {
  void* k_cache;         // 16-bit elements of the outputs' type, device memory
  void* v_cache;
  const int* slots;      // int32 [batch], device memory
  int n_slots;
  int64_t slot_stride, head_stride;  // in elements
  bool write_out_k, write_out_v;     // false: the caller gave no such output, and the segment's out16 is a stand-in to be ignored
  //   qkv_cache_fp8, qkv_norm_cache_fp8 (sqllm_qkv_rope_cache_fp8_* / sqllm_qkv_rope_norm_cache_fp8_*): the caches hold 1-byte e4m3fn
  //     elements, the strides count bytes, and the launch goes to the kernels of sqllm_linear_qkv_cache_fp8.hip /
  //     sqllm_linear_qkv_norm_cache_fp8.hip
  bool fp8;
  bool scales_ok;                    // both scales finite and positive with finite reciprocals (rejected behind the linear's validation)
  float inv_k_scale, inv_v_scale;    // 1 / k_scale, 1 / v_scale, fp32
};
enum FrontKind {
  kFrontGated, kFrontGatedNorm, kFrontEp, kFrontQkv, kFrontQkvNorm, kFrontQkvCache, kFrontQkvNormCache, kFrontQkvCacheFp8,
  kFrontQkvNormCacheFp8, kFrontKinds
};
// what a front's launch takes beyond the fused linear's LaunchArgs; a kind reads its own fields and rejects a call without them
struct FrontCall {
  void* pair = nullptr;            // the gated kinds
  const void* residual = nullptr;  // ep
  int act = 0;                     // ep
  const QkvRope* qkv = nullptr;    // the qkv kinds
  const VecNorm* vn = nullptr;     // the norm kinds
  const KvCache* kc = nullptr;     // the cache kinds
};
// the kind a call names: the pair plane makes it gated, the rotation qkv, neither ep; the norm and the cache choose the variant
inline FrontKind front_kind(const FrontCall& f) {
  if (f.pair) return f.vn ? kFrontGatedNorm : kFrontGated;
  if (!f.qkv) return kFrontEp;
  if (f.kc && f.kc->fp8) return f.vn ? kFrontQkvNormCacheFp8 : kFrontQkvCacheFp8;
  if (f.kc) return f.vn ? kFrontQkvNormCache : kFrontQkvCache;
  return f.vn ? kFrontQkvNorm : kFrontQkv;
}
typedef hipError_t (*FrontLauncher)(int bits, const LaunchArgs& a, const FrontCall& f, hipStream_t stream);
extern FrontLauncher g_launch_front[kFrontKinds];
// Decode attention over that cache (sqllm_attn_decode_* / sqllm_attn_append_*, 16-bit and e4m3fn caches): the partials of every
// (row, kv head, partition of kAttnPartition keys), then -- with more than one partition -- the combine.  Four kinds, each one
// kernel file that registers its launcher in g_launch_attn when it is linked in (a table as g_launch_front above: defined all
// null in sqllm_capi.hip, a null slot is hipErrorNotSupported); the launchers are one ladder, launch_attn<TAG> of sqllm_attn.h.
constexpr int kAttnPartition = 256;  // keys per partition (SQLLM_ATTN_PARTITION of include/sqllm_hip.h)
// one call, as the host layer validated it: HOST fields only, never device data
struct AttnCall {
  const void* q;
  void* out;
  const void* k_cache;
  const void* v_cache;
  const int* block_table;  // int32 [batch, table_stride], device memory
  const int* seq_lens;     // int32 [batch], device memory
  void* workspace;         // n_parts x (head_dim + 2) floats per (row, query head); contents irrelevant
  int batch, n_q_heads, n_kv_heads, head_dim, n_slots, block_size, table_stride;
  int capacity;            // min(max_blocks * block_size, INT32_MAX) keys
  int n_parts;             // ceil(capacity / kAttnPartition)
  int64_t slot_stride, head_stride, q_stride, out_stride;  // in elements (the first two in bytes with fp8)
  float scale;
  bool bf16;
  bool fp8;                // the caches hold 1-byte e4m3fn elements: scale then holds scale * k_scale, rounded once, and
  float v_scale;           // ... v_scale the cache's (1 otherwise)
  // several new tokens per sequence (sqllm_attn_append_*): `batch` counts SEQUENCES; q, out and the workspace have batch * q_len rows
  const int* q_lens;       // int32 [batch], device memory, or null: q_len real tokens everywhere
  int q_len;               // rows per sequence, 1 to 16; 0: the one-query entries
  // a sliding window (sqllm_attn_decode_window_*): the keys [max(0, L - window), L) of a row of length L; n_parts then holds
  // win_parts, the partitions a window can touch, and the workspace is laid out by it
  int window;              // at least 1; 0: the entries without a window
};
enum AttnKind { kAttnDecode, kAttnDecodeFp8, kAttnAppend, kAttnAppendFp8, kAttnKinds };
inline AttnKind attn_kind(const AttnCall& c) {
  if (c.q_len) return c.fp8 ? kAttnAppendFp8 : kAttnAppend;
  return c.fp8 ? kAttnDecodeFp8 : kAttnDecode;
}
typedef hipError_t (*AttnLauncher)(const AttnCall& c, hipStream_t stream);
extern AttnLauncher g_launch_attn[kAttnKinds];
// The kernels' argument (sqllm_attn_decode.hip: the partials and the combine; sqllm_attn_decode_fp8.hip: the partials over bytes).
// Its layout is part of the generated code: field order and types stay.
struct AttnArgs {
  const void* q;
  void* out;
  const void* k_cache;
  const void* v_cache;
  const int* block_table;
  const int* seq_lens;
  float* ws_acc;  // [batch, n_q_heads, n_parts, head_dim]
  float* ws_ml;   // [batch, n_q_heads, n_parts, 2]
  long long q_stride, out_stride;
  unsigned slot_stride, head_stride;  // (below 2^32 wherever they are multiplied: checked by the host)
  int n_q_heads, group, n_slots, block_size, table_stride;
  int capacity;  // min(max_blocks * block_size, INT32_MAX)
  int n_parts;
  float scale;
};
// The append kernels' argument: AttnArgs' fields (the kernel bodies are copies of their one-query siblings) and the tokens.
struct AttnAppendArgs {
  const void* q;
  void* out;
  const void* k_cache;
  const void* v_cache;
  const int* block_table;  // [batch, table_stride]: one table row per sequence
  const int* seq_lens;     // [batch]: keys of the sequence, its new tokens included
  const int* q_lens;       // [batch] or null
  float* ws_acc;  // [batch * q_len, n_q_heads, n_parts, head_dim]
  float* ws_ml;   // [batch * q_len, n_q_heads, n_parts, 2]
  long long q_stride, out_stride;
  unsigned slot_stride, head_stride;  // (below 2^32 wherever they are multiplied: checked by the host)
  int n_q_heads, group, n_slots, block_size, table_stride;
  int capacity;  // min(max_blocks * block_size, INT32_MAX)
  int n_parts;
  int batch;     // sequences
  int q_len;
  float scale;
};
// The window kernels' argument (sqllm_attn_window.hip, sqllm_attn_window_fp8.hip): AttnArgs' fields and the window.  n_parts is
// win_parts here: the workgroups per (kv head, row) and the partials per (row, query head), indexed RELATIVE to the row's first
// attended partition.
struct AttnWindowArgs {
  const void* q;
  void* out;
  const void* k_cache;
  const void* v_cache;
  const int* block_table;
  const int* seq_lens;
  float* ws_acc;  // [batch, n_q_heads, n_parts, head_dim]
  float* ws_ml;   // [batch, n_q_heads, n_parts, 2]
  long long q_stride, out_stride;
  unsigned slot_stride, head_stride;  // (below 2^32 wherever they are multiplied: checked by the host)
  int n_q_heads, group, n_slots, block_size, table_stride;
  int capacity;  // min(max_blocks * block_size, INT32_MAX)
  int n_parts;   // win_parts
  int window;
  float scale;
};
inline void attn_token_args(AttnArgs&, const AttnCall&) {}
inline void attn_token_args(AttnWindowArgs& k, const AttnCall& c) { k.window = c.window; }
inline void attn_token_args(AttnAppendArgs& k, const AttnCall& c) {
  k.q_lens = c.q_lens;
  k.batch = c.batch;
  k.q_len = c.q_len;
}
template <typename ARGS>
inline ARGS make_attn_args(const AttnCall& c) {
  ARGS k;
  k.q = c.q;
  k.out = c.out;
  k.k_cache = c.k_cache;
  k.v_cache = c.v_cache;
  k.block_table = c.block_table;
  k.seq_lens = c.seq_lens;
  k.ws_acc = static_cast<float*>(c.workspace);
  k.ws_ml = k.ws_acc + (long long)c.batch * (c.q_len ? c.q_len : 1) * c.n_q_heads * c.n_parts * c.head_dim;
  k.q_stride = c.q_stride;
  k.out_stride = c.out_stride;
  k.slot_stride = (unsigned)c.slot_stride;
  k.head_stride = (unsigned)c.head_stride;
  k.n_q_heads = c.n_q_heads;
  k.group = c.n_q_heads / c.n_kv_heads;
  k.n_slots = c.n_slots;
  k.block_size = c.block_size;
  k.table_stride = c.table_stride;
  k.capacity = c.capacity;
  k.n_parts = c.n_parts;
  k.scale = c.scale;
  attn_token_args(k, c);
  return k;
}
// The combines (they do not see the cache): one workgroup of head_dim threads per (query head, row) over the partials in the
// workspace -- sqllm_attn_decode.hip's, and sqllm_attn_append.hip's with every row's own length.  Hooks those files set, so that
// the byte caches' partials are followed by the same kernels.
extern hipError_t (*g_launch_attn_combine)(const AttnArgs& k, int head_dim, bool bf16, int batch, hipStream_t stream);
extern hipError_t (*g_launch_attn_append_combine)(const AttnAppendArgs& k, int head_dim, bool bf16, hipStream_t stream);
// The window entries (sqllm_attn_decode_window_*): a table of their own beside g_launch_attn, [0] the 16-bit caches
// (sqllm_attn_window.hip), [1] the byte caches (sqllm_attn_window_fp8.hip), and the window combine both reach through its hook.
// Null until the file is linked in: hipErrorNotSupported, never the kernels without a window.
extern AttnLauncher g_launch_attn_window[2];
extern hipError_t (*g_launch_attn_window_combine)(const AttnWindowArgs& k, int head_dim, bool bf16, int batch, hipStream_t stream);
hipError_t launch_batched_mfma(int bits, const LaunchArgs& a, hipStream_t stream);        // fp32 matrix instructions
hipError_t launch_batched_mfma_split(int bits, const LaunchArgs& a, hipStream_t stream);  // bf16 matrix instructions on exactly split operands (sqllm_mfma_split.hip)
hipError_t launch_batched_mfma_split_all(int bits, const LaunchArgs& a, hipStream_t stream);  // ... tile form, the op's sparse terms in the same grid
hipError_t launch_batched_mfma_wide(int bits, const LaunchArgs& a, hipStream_t stream);   // ... in the wide form (sqllm_mfma_wide.hip)
hipError_t launch_batched_cols(int bits, const LaunchArgs& a, hipStream_t stream);
constexpr int kSplitFlagWgs = 256;  // workgroups (and flag words) of split_vec
// planes of split_vec, in 16-byte chunks: 3 planes x 64 lanes per (16 rows, 32 k's); rows padded to a multiple of 64, every
// block of 16 rows K / 32 + 1 k blocks long, the last one all zero
inline uint64_t split_planes_chunks(int batch, int K) { return (uint64_t)((batch + 63) / 64 * 4) * (uint64_t)(K / 32 + 1) * 192u; }
// scratch for the sums of the wide form's K slices: 64 x 64 floats per slice and column tile
inline uint64_t wide_slab_bytes(int dense_blocks, int full_units, int k_slices) {
  return k_slices > 1 ? (uint64_t)(dense_blocks - full_units) * 8u * 64u * 64u * 4u : 0;
}
hipError_t split_vec(const float* x, void* planes, uint32_t* flags, int batch, int K, hipStream_t stream, hipEvent_t ev_start);
constexpr int kSmallSplitRows = 16;  // rows up to which a group of ops runs as ONE launch on the split matrix-core kernel (all three terms)
hipError_t launch_small_split(int bits, const LaunchArgs& a, hipStream_t stream);
hipError_t transpose_vec(const float* x, float* xT, int batch, int K, int Bp, hipStream_t stream, hipEvent_t ev_start);
// rows of the small transposed vec (2..16 batch rows rounded up to a power of two), as its logarithm
constexpr int small_rows_log2(int batch) { return batch <= 2 ? 1 : batch <= 4 ? 2 : batch <= 8 ? 3 : 4; }
// 2..16 rows: xT[k][rp], rp = the batch rounded up to a power of two (K * rp floats)
hipError_t transpose_small(const float* x, float* xT, int batch, int K, hipStream_t stream, hipEvent_t ev_start);
// ... + vec as three bf16 planes in fragment order, row block 0 (K / 32 + 1 k blocks of 3 KB; planes 16-byte aligned behind xT)
hipError_t prepare_small(const float* x, float* xT, void* planes, int batch, int K, hipStream_t stream, hipEvent_t ev_start);
inline int64_t small_planes_bytes(int K) { return (int64_t)(K / 32 + 1) * 3072; }
inline int64_t transpose_small_bytes(int batch, int K) { return ((int64_t)K << small_rows_log2(batch)) * 4; }
hipError_t launch_batched_sparse(const LaunchArgs& a, hipStream_t stream);
hipError_t check_csr(const int* rows, int N, int nnz, hipStream_t stream, int* bad);

}  // namespace sqllm
