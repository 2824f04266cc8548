// sqllm_capi.hip -- the extern "C" surface declared in include/sqllm_hip.h: argument validation,
// launch planning, and the reference operator names as thin adapters over sqllm_launch().
// How a group of ops is launched is decided in ONE place -- route_of (which kernel family) and plan_group (its geometry);
// the launch, sqllm_plan_query and sqllm_workspace_bytes all ask there.  tests/native/launch_recorder.cpp links this file
// against recording launchers: a change to the planner can be diffed launch by launch on a machine without a GPU.
// Replaces the reference's pybind11 layer squeezellm/quant_cuda.cpp:112-270 and the grid math of
// its launchers squeezellm/quant_cuda_kernel.cu:132-738 (no torch types cross this boundary).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <atomic>

#include "sqllm_hip.h"
#include "sqllm_host.h"
#include "sqllm_kernels.h"

namespace sqllm {
FrontLauncher g_launch_front[kFrontKinds] = {};  // each slot set by its kernel file (sqllm_linear_gated.hip ... sqllm_linear_qkv_norm_cache_fp8.hip)
AttnLauncher g_launch_attn[kAttnKinds] = {};  // each slot set by its kernel file (sqllm_attn_decode.hip ... sqllm_attn_append_fp8.hip)
hipError_t (*g_launch_attn_combine)(const AttnArgs& k, int head_dim, bool bf16, int batch, hipStream_t stream) = nullptr;  // set by sqllm_attn_decode.hip
hipError_t (*g_launch_attn_append_combine)(const AttnAppendArgs& k, int head_dim, bool bf16, hipStream_t stream) = nullptr;  // set by sqllm_attn_append.hip
AttnLauncher g_launch_attn_window[2] = {};  // [0] set by sqllm_attn_window.hip, [1] by sqllm_attn_window_fp8.hip
hipError_t (*g_launch_attn_window_combine)(const AttnWindowArgs& k, int head_dim, bool bf16, int batch, hipStream_t stream) = nullptr;  // set by sqllm_attn_window.hip
}

namespace sqllm_host {

ExperimentalHooks g_experimental;
static Knobs g_knobs[kMaxDevices];

int device_slot() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();  // no usable device: not an error of the call being served
    dev = 0;
  }
  if (dev < 0 || dev >= kMaxDevices) dev = 0;
  return dev;
}

Knobs& knobs() { return g_knobs[device_slot()]; }
static int opt(std::atomic<int> Knobs::*field) { return (knobs().*field).load(std::memory_order_relaxed); }

// The wide-batch paths take stream-ordered scratch (hipMallocAsync) per group of ops.  The default pool's
// release threshold is 0: every synchronisation hands the block back to the OS and the next call pays
// a real allocation + map.  Raise it once per device (never lower it) so that the pool keeps what one
// group needs (2048 rows x K = 22016: transposed vec 180 MB + bf16 planes 271 MB + slabs <= 32 MB).
static void keep_scratch_in_pool() {
  static std::atomic<unsigned> done{0};
  if (!opt(&Knobs::scratch_pool_threshold)) return;  // opted out: the pool is left as the application set it
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) { (void)hipGetLastError(); return; }
  const unsigned bit = 1u << dev;
  if (done.load(std::memory_order_relaxed) & bit) return;
  hipMemPool_t pool = nullptr;
  if (hipDeviceGetDefaultMemPool(&pool, dev) != hipSuccess || !pool) { (void)hipGetLastError(); return; }  // (retried on the next call)
  uint64_t cur = 0;
  const uint64_t want = 1024ull << 20;
  if (hipMemPoolGetAttribute(pool, hipMemPoolAttrReleaseThreshold, &cur) != hipSuccess) { (void)hipGetLastError(); cur = 0; }
  if (cur < want) {
    uint64_t v = want;
    if (hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &v) != hipSuccess) { (void)hipGetLastError(); return; }  // (retried)
  }
  done.fetch_or(bit, std::memory_order_relaxed);  // only once it has succeeded
}

int cu_count() {
  int c = opt(&Knobs::cu_count);
  if (c > 0) return c;
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
      prop.multiProcessorCount > 0)
    c = prop.multiProcessorCount;
  else
    c = 256;  // MI355X
  knobs().cu_count.store(c, std::memory_order_relaxed);
  return c;
}

// the sparse operands of an op: shared by every entry point that takes them (sqllm_launch ..., sqllm_dequant)
int validate_sparse(const sqllm_op* op) {
  if (op->rows) {
    if (op->nnz < 0) return SQLLM_E_SPARSE;
    if (op->nnz > 0 && (!op->cols || !op->vals)) return SQLLM_E_NULL;
  }
  if (op->full_rows) {
    if (op->topX < 0) return SQLLM_E_SPARSE;
    if (op->topX > 0 && !op->full_row_indices) return SQLLM_E_NULL;
  }
  return SQLLM_OK;
}

int validate(const sqllm_op* op) {
  if (!op) return SQLLM_E_NULL;
  if (op->bits != 3 && op->bits != 4) return SQLLM_E_BITS;
  if (op->K <= 0 || op->N <= 0 || (op->K % 32) != 0 || (op->N % 4) != 0) return SQLLM_E_SHAPE;
  // the kernels address qweight with 32-bit byte offsets
  if ((uint64_t)op->K / 32u * (uint64_t)op->bits * (uint64_t)op->N * 4u >= (1ull << 32)) return SQLLM_E_SHAPE;
  if (op->batch < 0) return SQLLM_E_BATCH;
  if (!op->vec || !op->qweight || !op->mul || !op->lookup_table) return SQLLM_E_NULL;
  if ((reinterpret_cast<uintptr_t>(op->qweight) & 15u) != 0 ||
      (reinterpret_cast<uintptr_t>(op->lookup_table) & 15u) != 0)
    return SQLLM_E_ALIGN;
  return validate_sparse(op);
}

// option "validate_csr": a value check of rows[] on the device (blocks the host; debugging aid)
int validate_csr_values(const sqllm_op* op, sqllm_stream_t stream) {
  if (!opt(&Knobs::validate_csr) || !op->rows || op->nnz <= 0) return SQLLM_OK;
  int bad = 0;
  hipError_t e = sqllm::check_csr(op->rows, op->N, op->nnz, static_cast<hipStream_t>(stream), &bad);
  if (e != hipSuccess) return static_cast<int>(e);
  return bad ? SQLLM_E_SPARSE : SQLLM_OK;
}

constexpr int round8(int v) { return (v + 7) / 8 * 8; }

// Workgroups of the fused batch-tile kernel (sqllm_fused_matvec<BITS, BT>) that one CU holds at once, by bit width and batch tile
// (batch_tile_op): four at one row and on the 4-bit 2-row tile, three where the tile compiles to <= 80 VGPRs (4-bit: up to 6 rows; 3-bit:
// up to 3), two beyond (sqllm_fused.h: fused_min_waves).  THE residency table of the host layer: make_plan's one-round cut,
// widen_csr_chunks and set_role_priority all read it.
int resident_per_cu(int bits, int bt) {
  return (bt == 1 || (bt == 2 && bits == 4)) ? 4 : (bits == 4 ? (bt <= 6 ? 3 : 2) : (bt <= 3 ? 3 : 2));
}

// where an op's dense workgroups start, behind its CSR / top-X workgroups: at a multiple of 8 so that (dense id % 8) is the XCD of
// the workgroup -- or right behind them with sparse_last (grid = dense + sparse)
static void place_dense(sqllm::KernelGeom* gm) {
  const int sparse = gm->csr_blocks + gm->topx_blocks;
  gm->dense_block0 = (gm->sparse_last & 1) ? sparse : round8(sparse);
}

// workgroups of one op in a launch of several: padded to a multiple of 8 (dense ids keep their XCD alignment)
static int padded_blocks(const sqllm::KernelGeom& gm) { return round8(gm.dense_block0 + gm.dense_blocks); }

// Launch geometry.  The dense part is cut into 64-column tiles x K slices so that about `target`
// workgroups exist (1-3 per CU, 8 waves each, of the 4 that fit: the 7B shapes hold only
// ~32-90 KiB of weights per CU, so the grid must be wide rather than deep).  A slice is a whole
// number of workgroup steps (waves x 4 units) so only the last slice has a ragged end.
void make_plan(const sqllm_op* op, sqllm::KernelGeom* gm, int ops_in_launch, int max_slices, int waves) {
  const int kK = (op->bits == 4) ? 8 : 32;
  memset(gm, 0, sizeof(*gm));
  gm->K = op->K;
  gm->N = op->N;
  gm->batch = op->batch <= 0 ? 1 : op->batch;
  gm->col_tiles = (op->N + sqllm::kTileN - 1) / sqllm::kTileN;
  gm->units_total = op->K / kK;
  const int step = waves * 4;  // units one workgroup step covers
  int upw = opt(&Knobs::groups_per_wave) * waves;
  if (upw <= 0) {
    int target = opt(&Knobs::target_wgs);
    if (target <= 0) {
      // measured on MI355X (tools/sweep.py, bench.py): an op under ~12 MB of packed weights runs
      // best with one 8-wave workgroup per CU when it shares its launch with others (q/k/v) and
      // with two when it is alone (o_proj); larger ones with ~3 per CU (gate/up) or 4 when alone
      // (down_proj) -- the chip holds four per CU.  In between (the 13B q/k/v at 4 bits, 13 MB each, sharing a
      // launch): two per CU and op -- three made 2400 workgroups of the group, 6 % slower
      // (profiles/r03_target_wgs_groups_batch1.txt)
      const double mb = (double)op->K * op->N * op->bits / 8.0 / 1e6;
      const bool alone = ops_in_launch <= 1;
      // ... and the DENSE-ONLY 3-bit 7B gate/up pair, 16.9 MB each: two per CU and op = 688 workgroups of two K slices per tile, one
      // resident round, 10.7 us against 11.0 for three per CU (1376 workgroups); at 4 bits the same cut loses, and with sparse roles in the
      // grid it is 1 % slower (profiles/r06_group_geometry.txt, r06_w3_gateup_geometry_ab.txt)
      const bool dense_only = !(op->rows && op->nnz > 0) && !(op->full_rows && op->topX > 0);
      const double two_per_cu_mb = (op->bits == 3 && dense_only) ? 18.0 : 16.0;
      target = (mb <= 12.0 ? (alone ? 2 : 1) : (!alone && mb <= two_per_cu_mb) ? 2 : (alone ? 4 : 3)) * cu_count();
      if (waves > sqllm::kWaves) target = target * sqllm::kWaves / waves;  // (16-wave workgroups: half as many, twice the rows each)
    }
    int slices = (target + gm->col_tiles / 2) / gm->col_tiles;
    if (slices < 1) slices = 1;
    if (slices > max_slices) slices = max_slices;
    upw = (gm->units_total + slices - 1) / slices;
    // ONE resident round for an op alone in its launch on a batch tile that holds two or three workgroups per CU (round 6).  The targets above
    // presume the batch-1 kernel's four: on a narrower residency the same plan is a full round plus a few stragglers, which start when the first
    // workgroups END -- 13B o_proj (4-bit, 3-6 rows, three per CU): 800 (+136 sparse) against 768 slots, 9.4 / 10.0 -> 7.6 / 9.15 us at 3 / 4 rows with
    // 560; 7B o_proj (4-bit, 7-8 rows, two per CU): 512 + 90 against 512, 11.6 / 13.3 -> 10.75 / 12.1 with 384; 13B o_proj at 3 bits (4-8 rows): 400 +
    // 136 against 512, -6...-11 % with 240 (profiles/r06_oproj_one_round.txt).  So: if dense + sparse workgroups exceed the slots by up to 35 %,
    // take the K slices that fit beside the sparse workgroups.  Not at four per CU (batch 1: 7B down_proj 960 + 242 against 1024 is 3 % FASTER than
    // 768 + 242), not for launches that are several rounds anyway, not for groups (flat: r06_launch_geometry_cols.txt, last block).
    const int bt = sqllm::batch_tile_op(gm->batch);
    const int per_cu = resident_per_cu(op->bits, bt);
    // ... and, at four per CU, for a 3-BIT op alone in its batch-1 launch: a launch that fits gets the dense-wave priority (set_role_priority, rule 1) -- 65B
    // o_proj, 1024 + 359 against 1024: 11.8 -> 11.2 us with 512 (10.85 with 384; profiles/r06_launch_geometry_b1.txt)
    const bool w3_batch1 = per_cu == 4 && op->bits == 3 && gm->batch == 1;
    if (ops_in_launch <= 1 && (per_cu <= 3 || w3_batch1) && opt(&Knobs::target_wgs) <= 0) {
      const int slots = per_cu * cu_count();
      const int sparse = ((op->rows && op->nnz > 0) ? (op->nnz + sqllm::kCsrChunk - 1) / sqllm::kCsrChunk : 0) +
                         ((op->full_rows && op->topX > 0) ? (op->K + sqllm::kTopxRows - 1) / sqllm::kTopxRows : 0);
      auto dense_of = [&](int sl) {
        int u = (gm->units_total + sl - 1) / sl;
        u = (u + step - 1) / step * step;
        return gm->col_tiles * ((gm->units_total + u - 1) / u);
      };
      const int total = dense_of(slices) + sparse;
      if (total > slots && 100ll * total <= (w3_batch1 ? 140ll : 135ll) * slots) {
        while (slices > 1 && dense_of(slices) + sparse > slots) --slices;
        upw = (gm->units_total + slices - 1) / slices;
      }
    }
  }
  upw = (upw + step - 1) / step * step;
  // 4-bit batch-1 waves work in chunks of four steps (128 units per workgroup, sqllm_fused.h: NBUF): a K slice of ONE chunk plus ONE step -- 160 units, the
  // 13B gate/up and down_proj under the size classes above -- pays a second round of loads for a quarter of a chunk.  One chunk per slice instead
  // (more slices): 13B s45 gate/up 22.2-22.8 -> 21.2-21.9 us, down_proj 12.85-13.5 -> 12.2-12.35 (profiles/r06_launch_geometry_b1.txt).
  if (op->bits == 4 && gm->batch == 1 && waves == sqllm::kWaves && opt(&Knobs::groups_per_wave) <= 0 &&
      opt(&Knobs::target_wgs) <= 0 && upw == 5 * step && (gm->units_total + 4 * step - 1) / (4 * step) <= max_slices)
    upw = 4 * step;
  gm->units_per_wg = upw;
  gm->k_slices = (gm->units_total + upw - 1) / upw;
  gm->dense_blocks = gm->col_tiles * gm->k_slices;
  gm->nnz = (op->rows && op->nnz > 0) ? op->nnz : 0;
  gm->csr_blocks = (gm->nnz + sqllm::kCsrChunk - 1) / sqllm::kCsrChunk;
  gm->topX = (op->full_rows && op->topX > 0) ? op->topX : 0;
  // top-X rows: a role of their own, one workgroup per kTopxRows k's (the fused linear folds them
  // into the dense tiles instead and drops these workgroups from its plan)
  gm->topx_blocks = gm->topX ? (op->K + sqllm::kTopxRows - 1) / sqllm::kTopxRows : 0;
  gm->sparse_last = opt(&Knobs::sparse_last);
  place_dense(gm);
  if (g_experimental.csr_ablation_bits) gm->sparse_last |= g_experimental.csr_ablation_bits() << 1;  // (measurement library)
}

// Whose waves win the issue arbitration in a BATCH-1 operator launch with sparse roles (round 6; `gm` = the geometry of the launch's
// ops as make_plan left it, `total` = its workgroups).  The CSR / top-X workgroups are chains of memory round trips in front of the grid; the dense
// workgroups are issue-bound.  Same-box A/Bs of variant builds, three alternating repetitions each, on two to three boxes per rule
// (profiles/r06_dense_priority_ab.txt, r06_sparse_order_ab.txt, r06_final_ab.txt, r06_sparse_priority_ab.txt, r06_role_priority_ab.txt):
//  1 (dense waves at s_setprio 1): 3-bit launches whose workgroups are all resident at once (four 8-wave workgroups per CU) -- the sparse
//    workgroups finish before the dense tail anyway, and every issue slot they win is taken from the decode: 7B w3 s45 +2.1 / +2.5 / +3.5 %
//    tokens/s (o_proj 5.1 -> 4.7-4.9 us, down_proj 8.1 -> 7.4-8.0).  In a multi-round launch the same setting starves the sparse workgroups
//    that hold the slots the next dense workgroups wait for (gate/up +5 %), and at 4 bits it measured +-0 / -2 %.
//  2 (sparse waves at s_setprio 1: out of the way sooner): 4-bit launches (7B w4 s45 +0.9 / +2.3 %: o_proj -4...-6 %, q/k/v -2 %; 13B +0.3 %),
//    and 3-bit multi-round launches whose sparse workgroups alone are half a round or more (65B: q/k/v and gate/up -7 %, the pass +3.0 /
//    +3.3 %); NOT the smaller 3-bit multi-round launches (7B gate/up +1.3 % on both boxes).
// Built on the way and dropped: the sparse workgroups LAST in the grid per launch (-3...-9 % per launch on one box, +3...+12 % on another;
// as a global switch it costs o_proj +12 %, which is why option sparse_last measured as "no change" in rounds 3 and 5).
void set_role_priority(sqllm::KernelGeom* gm, int n, int bits, int batch, int total, bool widened) {
  if (batch > 1 || (gm[0].sparse_last & 1)) return;
  int sparse = 0;
  for (int i = 0; i < n; ++i) sparse += (gm[i].csr_wide ? 2 : 1) * gm[i].csr_blocks + gm[i].topx_blocks;  // (counted in chunks of kCsrChunk)
  if (!sparse) return;
  const bool fits = !widened && total <= resident_per_cu(bits, 1) * cu_count();  // (batch-1 launches only: four per CU, as the table has it)
  int prio = 0;
  if (bits == 3) prio = fits ? 1 : (sparse >= 2 * cu_count() ? 2 : 0);
  else prio = 2;
  for (int i = 0; i < n; ++i) gm[i].dense_prio = prio;
}

// CSR chunks of 2 * kCsrChunk non-zeros in operator launches of the fused kernel that exceed the resident slots AND carry many sparse workgroups (>= 1.25 x
// CUs at kCsrChunk each): half as many workgroups in front of the grid, each with twice the non-zeros in the same chain of round trips.  A build with
// 2048 everywhere (profiles/r06_sparse_granularity_ab.txt) showed both sides: gate/up -2.7...-6.4 % (7B 430 / 13B 702 sparse workgroups), 13B
// down_proj -5.7 % (365), 13B q/k/v -3 % (408), against o_proj +13...+29 % (its fewer, longer sparse workgroups become the launch's tail), 7B q/k/v
// +1-1.5 % (270) and the 7B 3-bit down_proj +13 % (fits: dense priority).  `total` = the launch's workgroups; returns true if it widened (the caller lays the ops out again).
// The batch tiles of up to 5 rows take part (three workgroups per CU there, four in the 4-bit 2-row tile): 13B s45 layer at 2 / 4 / 5 rows -1.7 / -1.1 / -1.1 % (r06_wide_chunks_tiles.txt).
bool widen_csr_chunks(sqllm::KernelGeom* gm, int n, int bits, int batch, int total) {
  // Workgroups per CU of the tile that serves `batch` rows -- but never fewer than three.  This DIFFERS from resident_per_cu for the
  // 3-bit 4- and 5-row tiles (88 VGPRs: two per CU there, three here): the rule was measured with three, and moving its threshold is a
  // routing change that wants a same-box A/B of its own.
  const int table = resident_per_cu(bits, sqllm::batch_tile_op(batch <= 0 ? 1 : batch));
  const int resident = table > 3 ? table : 3;
  if (batch > 5 || total <= resident * cu_count() || (gm[0].sparse_last & 1)) return false;
  int sparse = 0;
  for (int i = 0; i < n; ++i) sparse += gm[i].csr_blocks + gm[i].topx_blocks;
  if (4 * sparse < 5 * cu_count()) return false;
  for (int i = 0; i < n; ++i)
    if (gm[i].csr_blocks > 0) {
      gm[i].csr_wide = 1;
      gm[i].csr_blocks = (gm[i].nnz + 2 * sqllm::kCsrChunk - 1) / (2 * sqllm::kCsrChunk);
      place_dense(&gm[i]);
    }
  return true;
}

void fill_segment(const sqllm_op* op, sqllm::Segment* sg) {
  sg->q = reinterpret_cast<const uint32_t*>(op->qweight);
  sg->y = op->mul;
  sg->lut = op->lookup_table;
  sg->rows = op->rows;
  sg->cols = op->cols;
  sg->vals = op->vals;
  // (full_rows without columns is no term at all: the kernels key the top-X work on the pointer)
  sg->full_rows = op->topX > 0 ? op->full_rows : nullptr;
  sg->full_idx = op->topX > 0 ? op->full_row_indices : nullptr;
  sg->bias = nullptr;
  sg->out16 = nullptr;
}

// The range cut shared by the matrix-core kernel (tile form, fused small launch) and the column-lane kernel: the dense work of a
// pass is the FLATTENED (column tile, unit) space cut into equal contiguous ranges, one per workgroup -- `target` workgroups for the
// launch (option target_wgs overrides it), shared by its ops and its `grid_y` passes.  A range is a whole number of `step` units.
static void cut_ranges(sqllm::KernelGeom* gm, int bits, int ops_in_launch, int step, int target, int grid_y) {
  const long long total_units = (long long)gm->col_tiles * gm->units_total;
  long long upw = (long long)opt(&Knobs::groups_per_wave) * step;
  bool aligned = false;
  if (upw <= 0) {
    if (opt(&Knobs::target_wgs) > 0) target = opt(&Knobs::target_wgs);
    target = (target + ops_in_launch - 1) / ops_in_launch;  // the ops of a group share the launch's workgroups
    long long ranges = (target + grid_y - 1) / grid_y;
    if (ranges < 1) ranges = 1;
    upw = (total_units + ranges - 1) / ranges;
    // A range that crosses a column-tile boundary is worked off as two pieces, each with its own table build.
    // Where a whole number of ranges per tile comes within 10 % of the wanted count, cut the tiles that way
    // instead (K = 5120: 640 units per tile against ranges of 200 -- two of three ranges crossed; the 5120-wide
    // ops were the one family the column-lane kernel lost on, profiles/r03_tile_vs_cols_by_shape.txt).
    const long long upws = (upw + step - 1) / step * step;
    const long long need = (gm->units_total + upws - 1) / upws;  // ranges of that length a tile needs
    for (long long per_tile = need; per_tile >= 1 && per_tile >= need - 1 && !aligned; --per_tile) {
      long long even = (gm->units_total + per_tile - 1) / per_tile;
      even = (even + step - 1) / step * step;
      const long long n_even = (long long)gm->col_tiles * ((gm->units_total + even - 1) / even);
      if (n_even <= ranges && 10 * n_even >= 9 * ranges) { upw = even; aligned = true; }
    }
    // Measured exception (profiles/r06_launch_geometry_cols.txt): a 4-bit group of three ops WITH sparse terms whose aligned cut is three
    // UNEVEN ranges per tile (K = 5120: 216 / 216 / 208 units) is 5-7 % faster on two even ones -- 13B q/k/v at 3 / 4 rows 19.5 / 22.0 ->
    // 18.6 / 20.5 us (four per tile: 18.8 / 20.8; the 408 sparse workgroups hold half the slots first).  Not so dense-only, at 3 bits, or where
    // the cut is even already (7B, 65B: fewer ranges cost 5-17 % there).
    if (aligned && ops_in_launch >= 3 && bits == 4 && gm->nnz > 0 && (gm->units_total + upw - 1) / upw == 3 &&
        gm->units_total % upw != 0 && gm->units_total % (2 * sqllm::kWaves) == 0)
      upw = gm->units_total / 2;
  }
  upw = (upw + step - 1) / step * step;
  if (upw > 0x3fffffff) upw = 0x3fffffff / step * step;
  gm->units_per_wg = (int)upw;
  gm->k_slices = (int)((gm->units_total + upw - 1) / upw);  // pieces per column tile (reported by plan_query)
  // (how the kernels tell the two cuts apart, and why either reading covers every unit once: sqllm_ranges.h, units_stride_of)
  gm->dense_blocks = aligned ? gm->col_tiles * gm->k_slices : (int)((total_units + upw - 1) / upw);
  gm->sparse_last = 0;
  place_dense(gm);
}

// Geometry of the wide-batch (matrix-core) kernel: one pass covers 16 * mb batch rows (blockIdx.y
// walks the passes).  The dense work of a pass is cut into equal ranges (cut_ranges), as many as the
// chip holds at once (2 per CU; 1 for the 64-row kernels, by their registers) divided by the number
// of passes: one round of workgroups, none of them short (N / 64 is rarely a multiple of the CU
// count: cutting K slices per column tile left the last round 27 % full on the 13B gate/up shape).
// A range is a whole number of workgroup steps (waves x 4 units); one that crosses a tile boundary costs a second piece.
// `reserve`: workgroups of the launch that are not dense ranges (the fused small launch's top-X slabs) -- they hold
// slots of the one round too.
void make_plan_mfma(const sqllm_op* op, sqllm::KernelGeom* gm, int ops_in_launch = 1, int row_blocks = 0, int wgs_per_cu = 0, int reserve = 0) {
  make_plan(op, gm, 1);
  const int mb = row_blocks > 0 ? row_blocks : sqllm::mfma_row_blocks(gm->batch);
  int target = (wgs_per_cu > 0 ? wgs_per_cu : mb == 4 ? 1 : 2) * cu_count();
  if (reserve > 0 && target - reserve >= target / 2) target -= reserve;
  cut_ranges(gm, op->bits, ops_in_launch, sqllm::kWaves * 4, target, (gm->batch + 16 * mb - 1) / (16 * mb));
}

// Geometry of the WIDE matrix-core kernel (sqllm_mfma_wide.hip: sqllm_fused_wide).  A UNIT is a block of 64 rows x a
// group of 8 column tiles (one per wave).  Units are worked off one workgroup per CU at a time; as many whole rounds as
// there are run every unit over ALL of K (no atomics, one table build); the units of the last, partial round are cut
// into as many K slices as fill the idle CUs (their workgroups add atomically).  dense_blocks = workgroups of the 1-D
// grid = full_units + (units - full_units) * k_slices; units_per_wg = units of K per slice.
constexpr int kWideTiles = 8;
int make_plan_wide(const sqllm_op* op, sqllm::KernelGeom* gm) {  // returns full_units
  make_plan(op, gm, 1);
  const int row_blocks = (gm->batch + 63) / 64;
  const int col_groups = (gm->col_tiles + kWideTiles - 1) / kWideTiles;
  const long long units = (long long)col_groups * row_blocks;
  const int cus = cu_count();
  const long long full = units / cus * cus;
  const long long rem = units - full;
  int max_s = gm->units_total / (op->bits == 4 ? 32 : 8);  // a slice is at least 8 steps of 32 k's x 64 rows x 64 columns
  if (max_s > sqllm::kMaxSlices) max_s = sqllm::kMaxSlices;
  if (max_s < 1) max_s = 1;
  int s = rem > 0 ? (int)(cus / rem) : 1;
  if (s > max_s) s = max_s;
  if (s < 1) s = 1;
  const int want = opt(&Knobs::groups_per_wave) * 4;  // (option: units of K per slice, in groups of 4)
  int upw = want > 0 ? want : ((gm->units_total + s - 1) / s + 3) / 4 * 4;
  if (upw > gm->units_total) upw = (gm->units_total + 3) / 4 * 4;
  gm->units_per_wg = upw;
  gm->k_slices = (gm->units_total + upw - 1) / upw;
  const long long blocks = full + rem * gm->k_slices;
  gm->dense_blocks = blocks > 0x7fffffff ? 0x7fffffff : (int)blocks;
  gm->sparse_last = 0;
  place_dense(gm);
  return (int)full;
}

// When the wide form pays (13B shapes, 64-2048 rows, profiles/r04_wide_slabs.txt).  With vec as planes and the K slices'
// sums as slabs it beats the tile kernel (~175 dense-equivalent TFLOP/s at any size) once the op is ~65 us of that: 4-bit
// batch * K * N >= 5.7e9 (5120x13824: 128 rows 104 -> 85 us, 256 rows 206 -> 145, 2048 rows 1.66 -> 0.96 ms; 5120x5120: 256
// rows 75 -> 71, below that it loses), 3-bit >= 4e9 (its tile kernel is slower: 64 rows 71 -> 62).  Inside a stream capture
// the scratch costs an allocation and a free node (~25 us per group): three times that.  WITHOUT scratch (vec split in
// registers, slices add atomically) only once its units fill 80 % of the CUs (5120x13824: from 512 rows).  An explicit
// mfma_wide_min_batch is taken at its word.
bool takes_wide_path(const sqllm_op* op, bool with_scratch, bool capturing) {
  if (!opt(&Knobs::mfma_split)) return false;
  const int from = opt(&Knobs::mfma_wide_min_batch);
  if (from > 0) return op->batch >= from;
  if (op->batch < 64) return false;
  if (with_scratch) {
    const double work = (double)op->batch * op->K * op->N;
    return work >= (op->bits == 4 ? 5.7e9 : 4e9) * (capturing ? 3.0 : 1.0);
  }
  const long long col_groups = ((op->N + sqllm::kTileN - 1) / sqllm::kTileN + kWideTiles - 1) / kWideTiles;
  const long long units = col_groups * ((op->batch + 63) / 64);
  return 5 * units >= 4 * (long long)cu_count();
}

// The CSR term walked by the dense workgroups themselves (csr_tile_fold, sqllm_roles.h): no chunk workgroups in the grid.
void fold_csr_into_dense(sqllm::KernelGeom* gm) {
  gm->fold_csr = gm->nnz > 0 ? 1 : 0;
  gm->csr_blocks = 0;
  place_dense(gm);
}

// top-X workgroups of an op in the fused small launch: with the transposed vec at hand 8 (K <= 40 slabs) or 16 of them
// share the op's slabs (topx_role_xt: all batch rows at once) -- few enough to hold their slots beside ONE round of
// dense workgroups; without it one workgroup per slab, as everywhere else
int small_topx_blocks(const sqllm_op* op, bool with_xT, int ops_in_launch) {
  if (!(op->full_rows && op->topX > 0)) return 0;
  const int slabs = (op->K + sqllm::kTopxRows - 1) / sqllm::kTopxRows;
  if (!with_xT || op->topX > 16) return slabs;
  // (an op alone in its launch is short-lived -- 13B o_proj: 11 us -- and leaves slots free: more, shorter-lived workgroups)
  const int want = ops_in_launch == 1 ? (slabs <= 24 ? 24 : 16) : slabs <= 40 ? 8 : 16;
  return slabs < want ? slabs : want;
}

// dense workgroups per CU the fused small launch's planner aims at: as many as the kernel holds (two, by its registers:
// capped at 80 for a third one, the dense role measured 10 % slower -- profiles/r05_small_split_register_cap.txt)
int small_wgs_per_cu_of(const sqllm_op* op) {
  const int v = opt(&Knobs::small_wgs_per_cu);
  return v > 0 ? v : 2;
}

// rows from which an op -- or, n_ops > 1, the group it leads -- leaves the batch tiles / the column-lane kernel for the matrix cores
int mfma_min_batch_of(const sqllm_op* op, int n_ops = 1) {
  const int v = opt(&Knobs::mfma_min_batch);
  if (v > 0) return v;  // (an explicit value is taken at its word, whatever the shape)
  // 3-bit: 17 until round 4 -- from 9 rows the fused small-batch launch of the split matrix-core kernel beats the
  // column-lane kernel (13B s45 layer 191-226 vs 270-286 us at 9-16 rows).
  if (op->bits != 4) return 9;
  // 4-bit: 5 in rounds 4-5 (the fused small launch against the 8-ROW tile, which a 5-row batch paid in full).  Round 6: batch
  // tiles of exactly 5 and 6 rows, 78 / 80 VGPRs = three workgroups per CU like the 2- / 4-row ones -- same box, 13B s45 layer
  // at 5 / 6 rows 121 / 121 us (fused small launch) -> 104 / 115 (tiles); at 7 / 8 rows the 8-row tile (96 VGPRs, two per CU)
  // loses, 150 / 155 against 122 / 123 (profiles/r06_small_batch_tiles_5_6.txt).  Except for a SMALL op alone in its launch
  // (<= 16 MB of packed weights: the 13B o_proj), whose fused small launch is mostly head, tail and the kernel in front of
  // it: 8-row tile up to 8 rows (o_proj 16.5 against 22.4 us by events).
  const double mb = (double)op->K * op->N / 2e6;
  if (n_ops == 1 && mb <= 16.0) return 9;
  return 7;
}
int cols_max_batch_of(const sqllm_op* op) {
  const int v = opt(&Knobs::cols_max_batch);
  // 4-bit: up to 4 rows; single ops of >= 20 MB up to 6 (round 6, with the kernel's passes of exactly 5 / 6 rows: 13B down_proj 22.4 / 25.7 us against
  // 23.6 / 26.7 on the 5- / 6-row tiles, the layer -0.8 / -1.9 %; at 7 rows its 7-row pass beats the fused small launch by events, 29.6 against
  // 32.5 us, and loses by graph wall, the layer +1.1 %: profiles/r06_cols_single_ops_5_7.txt; groups are kept at 4 rows by cols_pays)
  return v > 0 ? v : (op->bits == 3 ? 16 : ((double)op->K * op->N / 2e6 >= 20.0 ? 6 : 4));
}

bool takes_mfma_path(const sqllm_op* op, int n_ops = 1) { return op->batch >= 1 && op->batch >= mfma_min_batch_of(op, n_ops); }

// does this op (or the group it leads) run as the fused small launch of the split matrix-core kernel (sqllm_fused_small_split)?
bool takes_small_split(const sqllm_op* op, int n_ops = 1) {
  if (op->K >= (1 << 26)) return false;  // (its folded CSR walk packs a local row beside the column)
  return takes_mfma_path(op, n_ops) && op->batch <= sqllm::kSmallSplitRows && opt(&Knobs::mfma_split) &&
         opt(&Knobs::mfma_fuse_small);
}

// Geometry of the small-batch column-lane kernel: passes of batch_tile_op(batch) <= 8 rows
// (blockIdx.y: 1-8 rows in one pass, 8 per pass beyond); the dense work of a pass is cut into equal
// ranges of the flattened (column tile, unit) space like make_plan_mfma's (cut_ranges; a range is a
// whole number of waves here), three workgroups per CU (the phases of a
// workgroup -- table build, decode, combine -- hide behind its neighbours').
void make_plan_cols(const sqllm_op* op, sqllm::KernelGeom* gm, int ops_in_launch = 1) {
  make_plan(op, gm, 1);
  const int bt = sqllm::batch_tile_op(gm->batch);
  cut_ranges(gm, op->bits, ops_in_launch, sqllm::kWaves, 3 * cu_count(), (gm->batch + bt - 1) / bt);
}

// ---- the ONE-ROW cut of the column-lane kernel (sqllm_fused_cols<BITS, 1, 8>) ----
// Unit slots a workgroup executes for a piece of n units: wave w takes units w, w + kWaves, ... (n_w of them) and runs
// ceil(ceil(n_w / D) / NB) chunk pairs of NB * D slots each, as the one-row loop of dense_role_cols counts them (the constants: sqllm_kernels.h).
static long long cols_piece_slots(int bits, long long n) {
  const int D = sqllm::cols_chunk_units(bits), NB = sqllm::kColsChunksInFlight, W = sqllm::kWaves;
  auto wave = [&](long long n_w) { return (long long)NB * D * (((n_w + D - 1) / D + NB - 1) / NB); };
  return (n % W) * wave(n / W + 1) + (W - n % W) * wave(n / W);
}
// ... for a column tile of U units cut into tile-aligned ranges of L units (the last one ragged)
static long long cols_tile_slots(int bits, int U, int L) {
  const int k = (U + L - 1) / L;
  return (k - 1) * cols_piece_slots(bits, L) + cols_piece_slots(bits, U - (long long)(k - 1) * L);
}
// ... and for a whole op as cut_ranges left it, in the reading the kernel gives the plan (sqllm_ranges.h: units_stride_of).  Contiguous reading: the
// ranges cross tile boundaries (*crossing; such a range is two pieces: two table builds, two epilogues, a barrier more) and the count is a LOWER bound in
// O(1) -- every range as one piece; the pieces of a crossing range only add slots.  (This runs in front of every eager launch: no walk over the ranges.)
static long long cols_plan_slots(int bits, const sqllm::KernelGeom& gm, bool* crossing) {
  const long long U = gm.units_total, L = gm.units_per_wg, total = gm.col_tiles * U;
  if (gm.dense_blocks == gm.col_tiles * gm.k_slices) return gm.col_tiles * cols_tile_slots(bits, (int)U, (int)L);
  *crossing = true;
  return total / L * cols_piece_slots(bits, L) + cols_piece_slots(bits, total % L);
}

// The best tile-aligned cut of a one-row launch whose ops have `tiles` column tiles in all and U units per tile, beside `sparse`
// workgroups: candidates are p = 1, 2, ... ranges per tile of ceil(U / p) units rounded up to whole waves; among those whose workgroups
// fit the four resident per CU the one with the fewest executed slots wins.  Ties go to the largest workgroup count up to the column-lane kernel's
// target of three per CU, and only without one to the smallest above it: nearest-to-target was measured on the 13B 4-bit gate/up pair, 864 workgroups
// (two ranges of 320 units per tile) 19.9 us against 18.6 for 432 (one of 640) -- while under the target more is better: 7B gate/up 688 (2 x 256) 12.7
// against 14.4 us for 344 (1 x 512), 7B q/k/v 768 (4 x 128) 8.3 against 9.0 for 384 (profiles/cols_batch1_cut_ab.txt).
// Returns the range length (0: nothing fits) and the slots per tile.
static int best_aligned_cut(int bits, int U, long long tiles, long long sparse, long long* slots_per_tile) {
  const int W = sqllm::kWaves;
  const long long room = 4ll * cu_count() - sparse, want = 3ll * cu_count();
  int best = 0, prev = 0;
  long long best_slots = 0;
  for (int p = 1; p <= U; ++p) {
    const int L = ((U + p - 1) / p + W - 1) / W * W;
    if (L == prev) continue;
    prev = L;
    const long long k = (U + L - 1) / L, wgs = tiles * k;
    if (wgs > room || tiles * k * L >= (1ll << 31)) break;  // (more ranges only make both larger; the kernel walks the padded space in 32 bits)
    const long long slots = cols_tile_slots(bits, U, L);
    // (candidates come with growing workgroup counts: the last one up to three per CU, else the first above)
    if (!best || slots < best_slots || (slots == best_slots && wgs <= want)) { best = L; best_slots = slots; }
    if (L == W) break;
  }
  *slots_per_tile = best_slots;
  return best;
}

// cut_ranges aims at a workgroup COUNT and takes whole ranges per tile only where that comes within 10 % of it.  At one row the kernel is bound by
// issue, and what a launch pays for a near miss was measured on the 7B 4-bit gate/up pair (two ranges per tile = 344 per op against 384
// wanted: 10 x 344 < 9 x 384): ranges of 232 units across tile boundaries -- most workgroups two pieces, 29 units per wave in 32 slots --
// 15.6 us against 12.7 for two whole-tile ranges of 256 (one range per tile: 14.4; profiles/cols_batch1_cut_ab.txt).  So: where the plan of
// cut_ranges has ranges that cross tile boundaries, a one-row launch takes the best tile-aligned cut instead, unless that executes more slots.
// A plan that is tile-aligned already STAYS, whatever its slots: the 7B down_proj (twelve ranges of 120 units per tile, 93.5 % of its slots
// live, 768 workgroups = three per CU) measured 3.5 % SLOWER on eleven of 128 (97.7 %, 704 workgroups: 8.25 against 7.97 us), and q/k/v on
// two of 256 instead of four of 128 (both 100 %) 8.5 % slower -- the even three per CU is worth more than the last dead slots.
// Option cols_slot_cut = 1 is the rule by slots alone, as it was first written down: the best tile-aligned cut wherever it executes no more slots than the
// plan of cut_ranges, aligned or not (the 7B down_proj then gets its eleven ranges).  Kept for re-measuring on other parts, off by default.
// Options target_wgs / groups_per_wave: cut_ranges has obeyed them, and that stands.  `gm`: the n ops of the launch as make_plan_cols left them.
static void cut_ranges_one_row(const sqllm_op* ops, sqllm::KernelGeom* gm, int n) {
  if (opt(&Knobs::groups_per_wave) > 0 || opt(&Knobs::target_wgs) > 0) return;
  const int bits = ops[0].bits, U = gm[0].units_total;
  long long tiles = 0, sparse = 0, today = 0;
  bool crossing = false;
  for (int i = 0; i < n; ++i) {
    tiles += gm[i].col_tiles;
    sparse += gm[i].dense_block0;
    today += cols_plan_slots(bits, gm[i], &crossing);
  }
  const bool by_slots = opt(&Knobs::cols_slot_cut) != 0;
  if (!crossing && !by_slots) return;
  long long slots = 0;
  const int L = best_aligned_cut(bits, U, tiles, sparse, &slots);
  // (for a crossing plan `today` is a lower bound -- cols_plan_slots -- so this comparison is biased towards KEEPING the crossing plan)
  if (!L || tiles * slots > today) return;
  for (int i = 0; i < n; ++i) {
    gm[i].units_per_wg = L;
    gm[i].k_slices = (U + L - 1) / L;
    gm[i].dense_blocks = gm[i].col_tiles * gm[i].k_slices;  // (the tile-aligned reading: sqllm_ranges.h, units_stride_of)
  }
}

int cols_min_batch_of() {
  const int v = opt(&Knobs::cols_min_batch);
  return v > 0 ? v : 2;
}

// Does the column-lane kernel pay?  Measured by shape and group size (profiles/r03_tile_vs_cols_by_shape.txt, hybrid
// ops, 2-16 rows), after the 2- / 4-row batch tiles went to three workgroups per CU and the column-lane kernel
// to tile-aligned ranges.  4-bit: groups of THREE ops (q/k/v: -6...-14 %) and single ops of >= 20 MB packed weights
// (down_proj: -7...-8 %); small single ops and two-op groups (gate/up, whose tile count does not cut evenly) are
// 5-19 % faster on the tiles.  3-bit: >= 16 MB packed at up to 4 rows, or many column tiles (N >= 8192); the small
// square ops stay on the tiles.  Applied only while the routing options are at their defaults: an explicit
// cols_min_batch / cols_max_batch is taken at its word.
bool cols_pays(const sqllm_op* op, int n_ops) {
  if (opt(&Knobs::cols_min_batch) > 0 || opt(&Knobs::cols_max_batch) > 0) return true;
  const double mb = (double)op->K * op->N * op->bits / 8e6;  // (of a group: the sum of its ops)
  // (round 6: the 4-bit 2-row tile went to four workgroups per CU -- a three-op group WITH sparse terms of >= 32 MB is then faster on the tiles at exactly
  // 2 rows: 13B q/k/v 17.1 -> 15.4 us, 65B 35 -> 32; 7B's 25 MB and every dense-only group stay here: profiles/r06_tile2_half.txt)
  if (op->bits == 4) return (n_ops >= 3 && op->batch <= 4 && !(op->batch == 2 && op->nnz > 0 && mb >= 32.0)) || (n_ops == 1 && mb >= 20.0);
  if (op->batch <= 4 && mb >= 16.0) return true;
  return op->N >= 8192;
}

// ... and at BATCH 1 (the matvec operators; a *_batched call with one row) -- round 6, second session.  The column-lane kernel's loop is 1.5 vector + 1 LDS
// instructions per weight at one row (vec in SGPRs: no broadcasts) against the fused kernel's 2.1 + 1; it had lost at batch 1 in round 3, before its ranges were cut
// tile by tile and before groups ran as one launch.  Re-measured per launch shape (tools/experiments/launch_geometry.py --batch 1 --options cols_min_batch=1
// against --batch 0; graph wall, column-lane against fused; profiles/r06_cols_batch1.txt):
//                 o_proj (alone)   down_proj (alone)   q/k/v (3 ops)   gate/up (2 ops)
//   7B  w4 s0        +12 %             -3.5 %             -11.5 %          +1.3 %
//   7B  w3 s0        +13 %             -2 %               -6.7 %           -11 %
//   13B w4 s0        +20 %             -11.5 %            -3.6 %           -2.5 %
//   13B w3 s0        +38 %             -0.2 %             -8.3 %           -8 %
//   65B w3 s0        +7.6 %            -6.7 %             -9.8 %           -1.3 %
//   7B  w4 s45       +4.5 %            +1 %               -1.7 %           +18 %
//   7B  w3 s45       +10.6 %           -2.7 %             -2.3 %           -9 %
//   13B w4 s45       +27 %             +6.5 %             +2 %             +17 %
//   13B w3 s45       +27 %             +9.7 %             +5.5 %           +6.1 %
//   65B w3 s45       +15 %             +0.7 %             -5 %             +13 %
// Round 7, with the kernel's one-row decode loop and the one-row cut (cut_ranges_one_row) -- same protocol, dense-only, graph wall in us, fused | column-lane
// on the plan of cut_ranges | column-lane on whole-tile ranges (profiles/cols_batch1_cut_ab.txt; the 7B pair in two runs, of which the first alone -- gain 1.64 us against a
// fused spread of 1.02 -- fell short of the adoption rule, and again build against build: 14.54 -> 13.00; the 13B / 65B rows are ONE process each on the parent build, the whole-tile cut asked for through target_wgs):
//   7B  w4 gate/up   14.4 / 15.5 | 15.6 (3 x 232 units across tiles)  | 12.7 / 13.0 (2 x 256: -11.5 / -16 % against fused)   1 x 512: 14.4
//   13B w4 gate/up   21.4        | 20.6 (2 x 360 across tiles)        | 18.6 (1 x 640: -13 %)                                   2 x 320: 19.9
//   65B w4 gate/up   43.9        | 41.0 (2 x 920 across tiles)        | 39.3 (1 x 1024: -10.5 %)
//   65B w3 gate/up   35.5        | 36.0 (2 x 232 across tiles)        | 33.5 (1 x 256: -5.7 %)
//   7B  w4 q/k/v      8.75       |  8.33 (4 x 128, aligned: -4.8 %)   | (2 x 256: 9.04)
//   7B  w4 down_proj  8.31       |  7.97 (12 x 120, aligned: -4.1 %)  | (11 x 128: 8.25; 16 x 88: 10.4)
//   7B  w4 s45 gate/up 15.3      | 19.6                               | 19.2 (1 x 512: the sparse workgroups leave no room for two)  -> stays fused
// So the 4-bit pair's tie / loss in the table above was its CUT (ranges across tile boundaries: two table builds, two epilogues, 29 units in 32 slots), not the kernel.
// Dense-only launches of >= 16 MB win on it -- three-op groups always, a single op if it is tall (K >= 2 N: the square 65B o_proj loses), two-op groups at 3 bits, and
// at 4 bits where the plan is whole-tile ranges with >= 95 % of their slots live (7B, 13B, 65B: all 100 %).
// With sparse roles in the grid (which have none of the fused path's role priorities and wide chunks here) only the 3-bit groups whose K cuts into even ranges
// (K a multiple of 2048) up to 40 MB do: 7B q/k/v and gate/up -- and the 4-bit 7B q/k/v group, by a little.
bool cols_pays_batch1(const sqllm_op* sum, int n_ops, bool sparse, const sqllm_op* ops) {  // (ops: the launch's ops themselves)
  const double mb = (double)sum->K * sum->N * sum->bits / 8e6;
  if (mb < 16.0) return false;
  if (!sparse) {
    if (n_ops >= 3 || (n_ops == 1 && sum->K >= 2ll * sum->N) || (n_ops == 2 && sum->bits == 3)) return true;
    if (n_ops != 2 || opt(&Knobs::groups_per_wave) > 0 || opt(&Knobs::target_wgs) > 0) return false;
    // the 4-bit pair: where its plan is whole-tile ranges with >= 95 % of their slots live (cut_ranges_one_row: 7B two ranges of 256 units per tile,
    // 13B one of 640, 65B one of 1024 -- all 100 %)
    // (route_of runs in front of validate_group: a pair that validation will refuse -- a shape validate() rejects, ops that do not share K and bits -- is
    // not planned here; it keeps the fused route and gets its error code there)
    for (int i = 0; i < 2; ++i)
      if (ops[i].bits != 4 || ops[i].K != ops[0].K || ops[i].K <= 0 || ops[i].N <= 0 || ops[i].K % 32 != 0 || ops[i].N % 4 != 0) return false;
    // (the launch is planned here and again in plan_group: two make_plan calls and at most a few candidates of best_aligned_cut, no walk over ranges)
    sqllm::KernelGeom gm[2];
    for (int i = 0; i < 2; ++i) make_plan_cols(&ops[i], &gm[i], 2);
    cut_ranges_one_row(ops, gm, 2);
    long long slots = 0, units = 0;
    bool crossing = false;
    for (int i = 0; i < 2; ++i) {
      slots += cols_plan_slots(4, gm[i], &crossing);
      units += (long long)gm[i].col_tiles * gm[i].units_total;
    }
    return !crossing && 100 * units >= 95 * slots;
  }
  // (4-bit: the three-op group only -- 7B q/k/v -1.7 / -3.5 % on two boxes; its gate/up loses 18 %)
  return sum->K % 2048 == 0 && mb <= 40.0 && n_ops >= (sum->bits == 3 ? 2 : 3);
}

static bool op_has_sparse(const sqllm_op* op) { return (op->rows && op->nnz > 0) || (op->full_rows && op->topX > 0); }

// the routing test shared by single ops and groups: `sum` = the op, or the group as the one op it is to the kernel (the sum of its columns)
static bool cols_route(const sqllm_op* sum, int n_ops, bool sparse, const sqllm_op* ops) {
  const int b = sum->batch <= 0 ? 1 : sum->batch;
  const bool explicit_range = opt(&Knobs::cols_min_batch) > 0 || opt(&Knobs::cols_max_batch) > 0;
  if (b == 1 && !explicit_range) return cols_pays_batch1(sum, n_ops, sparse, ops);
  return b >= cols_min_batch_of() && b <= cols_max_batch_of(sum) && cols_pays(sum, n_ops);
}

// a group of ops over one vec (q/k/v, gate/up) is judged as the one op it is to the kernel: the sum of its columns
bool group_takes_cols_path(const sqllm_op* ops, int n) {
  sqllm_op sum = ops[0];
  long long N = 0;
  bool sparse = false;
  for (int i = 0; i < n; ++i) {
    N += ops[i].N;
    sparse = sparse || op_has_sparse(&ops[i]);
  }
  sum.N = N > 0x7fffffff ? 0x7fffffff : (int)N;
  return !takes_mfma_path(&ops[0], n) && cols_route(&sum, n, sparse, ops);
}

bool takes_cols_path(const sqllm_op* op) { return !takes_mfma_path(op) && cols_route(op, 1, op_has_sparse(op), op); }

// ---- the launch planner --------------------------------------------------------------------------------------------------
// ONE place decides how a group of ops is launched: route_of picks the kernel family, plan_group the geometry.  The launch
// (launch_group_with_events), sqllm_plan_query and sqllm_workspace_bytes all ask here.

enum Route {
  kFusedTiles,   // ONE launch of the fused batch-tile kernel over the group (batch 1 and the small batches the other routes leave)
  kFusedLinear,  // ... as the fused 16-bit linear (sqllm_linear_f16 / sqllm_linear_bf16: one route, one plan, two kernels)
  kColsGroup,    // ONE launch of the column-lane kernel, its workgroups divided between the ops
  kFusedSmall,   // up to 16 rows on the split matrix-core kernel: ONE launch for the whole group, sparse roles included
  kPerOpMfma,    // one launch per op (the members of a group only share their input) of the matrix-core kernel (wide batches)
  kPerOpCols,    // a single op on the column-lane kernel (small batches)
};

// (small batches: a group whose summed columns pass the column-lane kernel's test takes that kernel as ONE launch --
// make_plan_cols divides the workgroup target by the number of ops; other groups stay on the batch tiles, which beat
// one column-lane launch per op -- 13B s45 decoder layer at 2 rows: 88 vs 101 us)
static Route route_of(const sqllm_op* ops, int n, bool is_linear) {
  if (is_linear) return kFusedLinear;
  if (n > 1 && opt(&Knobs::cols_groups) && group_takes_cols_path(ops, n)) return kColsGroup;
  if (takes_small_split(&ops[0], n)) return kFusedSmall;
  if (takes_mfma_path(&ops[0], n)) return kPerOpMfma;
  if (n == 1 && takes_cols_path(&ops[0])) return kPerOpCols;
  return kFusedTiles;
}

// Every op of a group is valid and the ops share vec, K, bits and batch.  The batch-tile kernels read batch <= 0 as one row
// (a matvec op and a one-row *_batched op may share a launch); the other kernels address vec with 32-bit row offsets.
static int validate_group(const sqllm_op* ops, int n, sqllm_stream_t stream, Route route) {
  const bool tiles = route == kFusedTiles || route == kFusedLinear;
  for (int i = 0; i < n; ++i) {
    const sqllm_op* op = &ops[i];
    int rc = validate(op);
    if (rc == SQLLM_OK) rc = validate_csr_values(op, stream);
    if (rc != SQLLM_OK) return rc;
    const bool same_batch = tiles ? (op->batch <= 0 ? 1 : op->batch) == (ops[0].batch <= 0 ? 1 : ops[0].batch) : op->batch == ops[0].batch;
    if (op->vec != ops[0].vec || op->K != ops[0].K || op->bits != ops[0].bits || !same_batch) return SQLLM_E_GROUP;
    if (!tiles && (uint64_t)op->batch * (uint64_t)op->K >= (1ull << 31)) return SQLLM_E_SHAPE;  // 32-bit row offsets into vec
  }
  return SQLLM_OK;
}

// what the plan depends on beside the ops and the options: the scratch the launch has obtained
struct ScratchFacts {
  bool xT = false;         // a transposed vec is at hand (fused small launch)
  bool planes = false;     // vec split into bf16 planes is at hand (matrix-core kernel, wide form)
  bool capturing = false;  // ... and the scratch had to be allocated inside a stream capture
};

struct LaunchPlan {
  int first = 0, n_seg = 0;  // its segments are ops[first .. first + n_seg)
  int block0[sqllm::kMaxSegments + 1] = {};
  // matrix-core launches of one op:
  bool wide = false;            // the wide form (make_plan_wide) ...
  int wide_full_units = 0;      // ... with this many units over all of K
  int row_blocks = 0;           // tile form: blocks of 16 rows per pass, 0 = mfma_row_blocks(batch)
  bool split = true;            // bf16 matrix instructions on exactly split operands (option mfma_split)
  bool sparse_in_grid = false;  // the op's CSR / top-X workgroups ride in the dense launch's grid ...
  bool sparse_launch = false;   // ... or are a launch of their own in front of it
};

struct GroupPlan {
  Route route = kFusedTiles;
  int rc = SQLLM_OK;  // SQLLM_E_SHAPE: a fused linear whose columns would receive more than kMaxContrib contributions
  int n_launches = 0;
  LaunchPlan launch[sqllm::kMaxSegments];
  sqllm::KernelGeom gm[sqllm::kMaxSegments];  // per op
};

// block0[]: workgroup ids [block0[s], block0[s + 1]) belong to segment s.  `pad`: every segment a multiple of 8 long (launches of several
// ops: dense ids keep their XCD alignment); the one-op launches of the matrix-core and column-lane kernels end with their last workgroup.
static int layout_blocks(const sqllm::KernelGeom* gm, int n, bool pad, int* block0) {
  int at = 0;
  for (int i = 0; i < n; ++i) {
    block0[i] = at;
    at += pad ? padded_blocks(gm[i]) : gm[i].dense_block0 + gm[i].dense_blocks;
  }
  for (int i = n; i <= sqllm::kMaxSegments; ++i) block0[i] = at;
  return at;
}

// one op on the matrix-core kernel: wide or tile form, and where its sparse terms run
static void plan_mfma_op(const sqllm_op* op, const ScratchFacts& f, LaunchPlan* lp, sqllm::KernelGeom* gm) {
  lp->split = opt(&Knobs::mfma_split) != 0;
  lp->wide = takes_wide_path(op, f.planes, f.capturing);
  if (lp->wide) lp->wide_full_units = make_plan_wide(op, gm);
  else make_plan_mfma(op, gm);
  // the sparse terms first, as a launch of their own (see sqllm_sparse_batched), then the dense term
  // (running the two on different streams was tried: they do not overlap -- the dense kernel holds
  // every CU's registers -- and the two event waits cost 14 us per op)
  const int sparse = gm->csr_blocks + gm->topx_blocks;
  // tile form: the sparse terms ride in the dense launch's grid (sqllm_fused_batched_split_all) -- always up to 32 rows
  // (two workgroups per CU: 13B shapes 59-69 -> 55-57 us, 5120x5120 35-46 -> 28-38); from 33 rows, where the kernel
  // takes a whole CU per workgroup, only while the sparse workgroups are fewer than the CUs (5120x5120 at 64 rows
  // 81 -> 54 us; with 331 of them, 5120x13824, 112 -> 117: profiles/r04_mid_rows_fused_sparse.txt)
  const bool may_fuse = sparse > 0 && !lp->wide && lp->split && opt(&Knobs::mfma_fuse_sparse);
  lp->sparse_in_grid = may_fuse && (op->batch <= 32 || sparse < cu_count());
  if (may_fuse && !lp->sparse_in_grid && op->batch <= 64) {
    // 33-64 rows with more sparse workgroups than CUs: two passes of 32 rows on the kernel that leaves room for two
    // workgroups per CU, sparse terms in its grid, instead of one 64-row pass + their own launch
    // (profiles/r04_mid_rows_fused_sparse.txt, "mb2")
    lp->row_blocks = 2;
    make_plan_mfma(op, gm, 1, 2);
    lp->sparse_in_grid = true;
  }
  lp->sparse_launch = sparse > 0 && !lp->sparse_in_grid;
}

// Everything the launch of a (validated) group needs, from the ops, the options, the CU count and the scratch facts alone: touches no
// stream, allocates nothing, launches nothing.
static void plan_group(const sqllm_op* ops, int n, Route route, const ScratchFacts& f, GroupPlan* p) {
  p->route = route;
  const bool per_op = route == kPerOpMfma || route == kPerOpCols;
  switch (route) {
    case kColsGroup:
    case kPerOpCols:
      for (int i = 0; i < n; ++i) make_plan_cols(&ops[i], &p->gm[i], n);
      // (one row: the launch as a whole is cut again where its ranges cross tile boundaries -- kPerOpCols: every op is a launch of its own)
      if (p->gm[0].batch == 1) {
        if (route == kColsGroup) cut_ranges_one_row(ops, p->gm, n);
        else for (int i = 0; i < n; ++i) cut_ranges_one_row(&ops[i], &p->gm[i], 1);
      }
      break;
    case kFusedSmall: {
      // The dense ranges are ONE round of workgroups, as many as the chip holds at once: the top-X slabs (8 per op, padded)
      // take their slots from the same count.  (Planned beside them, 20-50 dense workgroups of a 13B launch found no slot,
      // started when the first ones left and ran as a second round of their own: 34 instead of 22 us per down_proj launch at
      // 16 rows -- profiles/r05_small_split_timeline.txt.)
      int reserve = 0;
      if (f.xT || opt(&Knobs::small_reserve_topx))
        for (int i = 0; i < n; ++i) reserve += round8(small_topx_blocks(&ops[i], f.xT, n));
      for (int i = 0; i < n; ++i) {
        make_plan_mfma(&ops[i], &p->gm[i], n, 0, small_wgs_per_cu_of(&ops[i]), reserve);
        p->gm[i].topx_blocks = small_topx_blocks(&ops[i], f.xT, n);
        fold_csr_into_dense(&p->gm[i]);
      }
      break;
    }
    case kPerOpMfma:
      for (int i = 0; i < n; ++i) plan_mfma_op(&ops[i], f, &p->launch[i], &p->gm[i]);
      break;
    case kFusedLinear:
      for (int i = 0; i < n; ++i) {
        const sqllm_op* op = &ops[i];
        sqllm::KernelGeom* gm = &p->gm[i];
        // a column's K slices + the CSR chunks its row can be spread over must fit the 6-bit count
        const int csr_bound = (op->rows && op->nnz > 0) ? op->K / sqllm::kCsrChunk + 2 : 0;
        make_plan(op, gm, n, sqllm::kMaxContrib - csr_bound > 1 ? sqllm::kMaxContrib - csr_bound : 1);
        // the top-X rows are always handled inside the dense workgroups: no top-X role in the grid
        gm->topx_blocks = 0;
        place_dense(gm);
        // the 55-bit sum field holds at most kMaxContrib clamped contributions per column: the K
        // slices and one per CSR chunk a row can be spread over
        if (gm->k_slices + (gm->csr_blocks ? op->K / sqllm::kCsrChunk + 2 : 0) > sqllm::kMaxContrib) {
          p->rc = SQLLM_E_SHAPE;
          return;
        }
      }
      break;
    case kFusedTiles:
      for (int i = 0; i < n; ++i) make_plan(&ops[i], &p->gm[i], n);
      break;
  }
  p->n_launches = per_op ? n : 1;
  for (int l = 0; l < p->n_launches; ++l) {
    LaunchPlan* lp = &p->launch[l];
    lp->first = per_op ? l : 0;
    lp->n_seg = per_op ? 1 : n;
    const int total = layout_blocks(&p->gm[lp->first], lp->n_seg, !per_op, lp->block0);
    if (route != kFusedTiles) continue;
    const bool widened = widen_csr_chunks(p->gm, n, ops[0].bits, ops[0].batch, total);
    set_role_priority(p->gm, n, ops[0].bits, ops[0].batch, widened ? layout_blocks(p->gm, n, true, lp->block0) : total, widened);
  }
}

}  // namespace sqllm_host

using namespace sqllm_host;

extern "C" {

int sqllm_abi_version(void) { return SQLLM_ABI_VERSION; }

const char* sqllm_error_string(int code) {
  switch (code) {
    case SQLLM_OK: return "ok";
    case SQLLM_E_BITS: return "bits must be 3 or 4";
    case SQLLM_E_SHAPE: return "bad shape: need K % 32 == 0, N % 4 == 0, height == K/32*bits, positive dims";
    case SQLLM_E_NULL: return "a required pointer is NULL";
    case SQLLM_E_ALIGN: return "qweight / lookup_table must be 16-byte aligned";
    case SQLLM_E_SPARSE: return "inconsistent sparse operands";
    case SQLLM_E_BATCH: return "bad batch / vec_height";
    case SQLLM_E_OPTION: return "unknown option or bad value";
    case SQLLM_E_GROUP: return "ops of a group must share vec, K, bits and batch (1..4 ops per group)";
    default: break;
  }
  if (code > 0) return hipGetErrorString(static_cast<hipError_t>(code));
  return "unknown sqllm error";
}

// Every option value is range-checked: switches take 0 / 1 only, counts their documented range (include/sqllm_hip.h).
// (Until round 5 any non-negative value was stored as it came, and one of them -- sparse_transpose = 2 -- switched to a
// timing-only mode that left the kernels reading an unwritten workspace; that experiment now lives behind the measurement
// library's hook, ExperimentalHooks::skip_prepare_small.)
struct Option { const char* name; std::atomic<int> Knobs::*field; int max; };
static const Option kOptions[] = {
    {"target_wgs", &Knobs::target_wgs, 1 << 24},
    {"groups_per_wave", &Knobs::groups_per_wave, 1 << 24},
    {"cu_count", &Knobs::cu_count, 1 << 16},  // for GPU-less planning tests
    {"sparse_last", &Knobs::sparse_last, 1},
    {"cols_groups", &Knobs::cols_groups, 1},
    {"cols_slot_cut", &Knobs::cols_slot_cut, 1},
    {"mfma_min_batch", &Knobs::mfma_min_batch, 0x7fffffff},  // (a huge value: never)
    {"cols_min_batch", &Knobs::cols_min_batch, 0x7fffffff},
    {"cols_max_batch", &Knobs::cols_max_batch, 0x7fffffff},
    {"sparse_transpose", &Knobs::sparse_transpose, 1},
    {"scratch_in_capture", &Knobs::scratch_in_capture, 1},
    {"validate_csr", &Knobs::validate_csr, 1},
    {"mfma_split", &Knobs::mfma_split, 1},
    {"split_planes_min_batch", &Knobs::split_planes_min_batch, 0x7fffffff},
    {"mfma_wide_min_batch", &Knobs::mfma_wide_min_batch, 0x7fffffff},
    {"mfma_fuse_small", &Knobs::mfma_fuse_small, 1},
    {"mfma_fuse_sparse", &Knobs::mfma_fuse_sparse, 1},
    {"scratch_pool_threshold", &Knobs::scratch_pool_threshold, 1},
    {"small_wgs_per_cu", &Knobs::small_wgs_per_cu, 8},
    {"small_reserve_topx", &Knobs::small_reserve_topx, 1},
    {"small_planes", &Knobs::small_planes, 1},
};
static const Option* find_option(const char* name) {
  for (const Option& o : kOptions)
    if (!strcmp(name, o.name)) return &o;
  return nullptr;
}

int sqllm_set_option(const char* name, int value) {
  if (!name || value < 0) return SQLLM_E_OPTION;
  if (const Option* o = find_option(name)) {
    if (value > o->max) return SQLLM_E_OPTION;
    (knobs().*(o->field)).store(value);
    return SQLLM_OK;
  }
  if (g_experimental.set_option) return g_experimental.set_option(name, value);  // (measurement library)
  return SQLLM_E_OPTION;
}

int sqllm_get_option(const char* name, int* value) {
  if (!name || !value) return SQLLM_E_OPTION;
  if (const Option* o = find_option(name)) {
    *value = (knobs().*(o->field)).load();
    return SQLLM_OK;
  }
  if (g_experimental.get_option) return g_experimental.get_option(name, value);  // (measurement library)
  return SQLLM_E_OPTION;
}

// The plan of ONE op as launched alone through a `_ws` entry point with enough workspace, outside a stream capture: the scratch
// its route can use is at hand (vec transposed where option sparse_transpose allows it, vec as bf16 planes).
int sqllm_plan_query(const sqllm_op* op, sqllm_plan* plan) {
  if (!plan) return SQLLM_E_NULL;
  // planning needs shapes only; tolerate NULL data pointers here
  if (!op) return SQLLM_E_NULL;
  if (op->bits != 3 && op->bits != 4) return SQLLM_E_BITS;
  if (op->K <= 0 || op->N <= 0 || (op->K % 32) != 0 || (op->N % 4) != 0) return SQLLM_E_SHAPE;
  ScratchFacts facts;
  facts.xT = opt(&Knobs::sparse_transpose) != 0;
  facts.planes = true;
  GroupPlan p;
  plan_group(op, 1, route_of(op, 1, false), facts, &p);
  const sqllm::KernelGeom& gm = p.gm[0];
  const LaunchPlan& lp = p.launch[0];
  plan->col_tiles = gm.col_tiles;
  plan->k_slices = gm.k_slices;
  plan->groups_per_wave = gm.units_per_wg;
  plan->dense_blocks = gm.dense_blocks;
  plan->csr_blocks = gm.csr_blocks;
  plan->topx_blocks = gm.topx_blocks;
  const bool mfma = p.route == kPerOpMfma;
  plan->grid_x = mfma ? gm.dense_blocks : gm.dense_block0 + gm.dense_blocks;  // (wide batches: the dense workgroups; the sparse terms are counted in csr_blocks / topx_blocks)
  const int rows_per_pass = lp.wide ? gm.batch
                            : (mfma || p.route == kFusedSmall) ? 16 * (lp.row_blocks ? lp.row_blocks : sqllm::mfma_row_blocks(gm.batch))
                                                               : sqllm::batch_tile_op(gm.batch);
  plan->grid_y = (gm.batch + rows_per_pass - 1) / rows_per_pass;
  return SQLLM_OK;
}

static int64_t align16(int64_t v) { return (v + 15) / 16 * 16; }

// workspace of a fused linear: 64-bit accumulator words [batch, N]
int64_t sqllm_linear_workspace_bytes(const sqllm_op* op) {
  if (!op || op->N <= 0) return 0;
  return align16(8ll * (op->batch <= 0 ? 1 : op->batch) * op->N);
}

// Stream-ordered scratch of a wide-batch group (hipMallocAsync / hipFreeAsync on the caller's stream: no host
// synchronisation, the pool keeps the block for the next call; inside a stream capture the allocation and the free become
// memory nodes of the graph -- works under torch's graph capture on ROCm 7.2; option scratch_in_capture = 0 keeps
// captures allocation-free).  ONE block per group holds
//   xT     vec TRANSPOSED (xT[k][row]) for the CSR role: one coalesced read per non-zero serves every batch row instead
//          of `batch` gathers 4 K bytes apart (only with a CSR term; option sparse_transpose);
//   planes vec split once into bf16 planes in fragment order + the lo flags (sqllm_mfma_wide.hip: sqllm_split_vec) for
//          the wide form (from split_planes_min_batch rows, default 64);
//   slabs  the sums of the wide form's K slices (sqllm_wide_reduce adds them to mul).
// Without scratch: the CSR role gathers from vec, the wide form splits in registers and its slices add atomically.
constexpr int kSplitPlanesMinBatch = 64;
struct WideScratch {
  void* block = nullptr;  // stream-ordered allocation of our own (freed by the destructor), null when the caller's workspace serves
  float* xT = nullptr;
  int Bp = 0;
  void* planes = nullptr;
  uint32_t* flags = nullptr;
  float* slabs = nullptr;
  bool capturing = false;  // ... and the scratch would have to be allocated inside the capture (memory nodes)
  hipStream_t s = nullptr;
  // what a group wants, in bytes: [xT | planes | flags | slabs]
  struct Layout { uint64_t xt = 0, planes = 0, flags = 0, slabs = 0; int Bp = 0; uint64_t total() const { return xt + planes + flags + slabs; } };
  static Layout layout(const sqllm_op* ops, int n, bool capturing) {
    Layout L;
    if (!ops || n < 1 || ops[0].batch <= 0 || ops[0].K <= 0) return L;
    bool any_csr = false, any_wide = false;
    uint64_t slab_bytes = 0;
    for (int i = 0; i < n; ++i) {
      any_csr = any_csr || (ops[i].nnz > 0 && ops[i].rows && ops[i].cols && ops[i].vals);
      if (validate(&ops[i]) != SQLLM_OK || !takes_wide_path(&ops[i], true, capturing)) continue;  // (the launch loop reports errors)
      any_wide = true;
      sqllm::KernelGeom gm;  // room for the K slices' sums (the ops of a group run one after the other: the largest need serves all)
      const int full = make_plan_wide(&ops[i], &gm);
      const uint64_t b = sqllm::wide_slab_bytes(gm.dense_blocks, full, gm.k_slices);
      if (b > slab_bytes) slab_bytes = b;
    }
    const bool want_xT = any_csr && opt(&Knobs::sparse_transpose);
    int from = opt(&Knobs::split_planes_min_batch);
    if (from == 0) from = kSplitPlanesMinBatch;
    const uint64_t chunks = sqllm::split_planes_chunks(ops[0].batch, ops[0].K);
    const bool want_planes = any_wide && ops[0].batch >= from && chunks < (1ull << 31);  // (32-bit chunk numbers in the kernel)
    if (!want_xT && !want_planes) return L;
    L.Bp = (ops[0].batch + 63) / 64 * 64;
    L.xt = want_xT ? (uint64_t)ops[0].K * L.Bp * sizeof(float) : 0;
    L.planes = want_planes ? chunks * 16 : 0;
    L.flags = want_planes ? (sqllm::kSplitFlagWgs * sizeof(uint32_t) + 15) / 16 * 16 : 0;
    L.slabs = want_planes ? slab_bytes : 0;
    return L;
  }
  // ops[0] is validated; *e0 (the start event of a profiled group) goes to the first kernel enqueued here, if any.
  // ws / ws_bytes: the caller's workspace (sqllm_launch_*_ws), used instead of an allocation when it is large enough.
  int acquire(const sqllm_op* ops, int n, sqllm_stream_t stream, hipEvent_t* e0, void* ws, int64_t ws_bytes) {
    s = static_cast<hipStream_t>(stream);
    if (!ops[0].vec || ops[0].batch <= 0 || ops[0].K <= 0) return SQLLM_OK;
    bool in_capture = false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (!(hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone)) {
      (void)hipGetLastError();
      in_capture = true;
    }
    char* p = nullptr;
    Layout L = layout(ops, n, false);
    if (ws && (reinterpret_cast<uintptr_t>(ws) & 15u) == 0 && L.total() > 0 && (uint64_t)(ws_bytes > 0 ? ws_bytes : 0) >= L.total()) {
      p = static_cast<char*>(ws);  // nothing allocated, nothing to free: a capture stays free of memory nodes
    } else {
      capturing = in_capture;
      if (capturing && !opt(&Knobs::scratch_in_capture)) return SQLLM_OK;
      L = layout(ops, n, capturing);
      if (L.total() == 0) return SQLLM_OK;
      keep_scratch_in_pool();
      if (hipMallocAsync(&block, L.total(), s) != hipSuccess || !block) {
        (void)hipGetLastError();  // no scratch
        block = nullptr;
        return SQLLM_OK;
      }
      p = static_cast<char*>(block);
    }
    if (L.total() == 0) return SQLLM_OK;
    if (L.xt) {
      xT = reinterpret_cast<float*>(p);
      Bp = L.Bp;
      const hipError_t e = sqllm::transpose_vec(ops[0].vec, xT, ops[0].batch, ops[0].K, Bp, s, e0 ? *e0 : nullptr);
      if (e != hipSuccess) return static_cast<int>(e);  // (the destructor frees)
      if (e0) *e0 = nullptr;
    }
    if (L.planes) {
      planes = p + L.xt;
      flags = reinterpret_cast<uint32_t*>(p + L.xt + L.planes);
      if (L.slabs) slabs = reinterpret_cast<float*>(p + L.xt + L.planes + L.flags);
      const hipError_t e = sqllm::split_vec(ops[0].vec, planes, flags, ops[0].batch, ops[0].K, s, e0 ? *e0 : nullptr);
      if (e != hipSuccess) return static_cast<int>(e);
      if (e0) *e0 = nullptr;
    }
    return SQLLM_OK;
  }
  ~WideScratch() {
    if (block) (void)hipFreeAsync(block, s);
  }
};

// Scratch of a fused small launch (up to 16 rows): vec TRANSPOSED (xT[k][rows]: the folded CSR walk and the top-X slabs then read
// ONE line per k for all the batch rows) and behind it vec as bf16 planes for the dense term (option small_planes) --
// sqllm_prepare_small writes both.  Without it the sparse terms gather from vec itself.
struct SmallScratch {
  void* own = nullptr;  // stream-ordered allocation of our own (freed by the destructor)
  hipStream_t s = nullptr;
  float* xT = nullptr;
  void* planes = nullptr;
  struct Layout { int64_t xt = 0, planes = 0; int64_t total() const { return xt + planes; } };
  static Layout layout(const sqllm_op* ops, int n) {
    Layout L;
    bool any_sparse = false;
    for (int i = 0; i < n; ++i) any_sparse = any_sparse || (ops[i].nnz > 0 && ops[i].rows) || (ops[i].full_rows && ops[i].topX > 0);
    if (!any_sparse || ops[0].batch <= 0 || ops[0].K <= 0 || !opt(&Knobs::sparse_transpose)) return L;
    L.xt = sqllm::transpose_small_bytes(ops[0].batch, ops[0].K);
    L.planes = opt(&Knobs::small_planes) ? sqllm::small_planes_bytes(ops[0].K) : 0;
    return L;
  }
  // The caller's workspace where it is large enough.  Otherwise, for the workspace-less names only, stream-ordered scratch as for
  // the wider batches -- never inside a capture: its memory nodes cost more than the gathers (profiles/r04_small_batch_layer.txt);
  // never for a `_ws` entry point: those allocate nothing up to 16 rows and leave the default pool alone -- the walk gathers.
  void acquire(const sqllm_op* ops, int n, sqllm_stream_t stream, void* ws, int64_t ws_bytes, bool ws_entry) {
    const Layout L = layout(ops, n);
    if (!L.xt || !ops[0].vec || (reinterpret_cast<uintptr_t>(ops[0].vec) & 15u) != 0) return;  // (the transposition reads vec 16 bytes at a time)
    if (ws && (reinterpret_cast<uintptr_t>(ws) & 15u) == 0 && ws_bytes >= L.total()) {
      xT = static_cast<float*>(ws);
    } else if (!ws_entry) {
      s = static_cast<hipStream_t>(stream);
      hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
      if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) {
        keep_scratch_in_pool();
        if (hipMallocAsync(&own, (size_t)L.total(), s) == hipSuccess && own) xT = static_cast<float*>(own);
        else { (void)hipGetLastError(); own = nullptr; }
      } else {
        (void)hipGetLastError();
      }
    }
    if (xT && L.planes) planes = reinterpret_cast<char*>(xT) + L.xt;
  }
  ~SmallScratch() {
    if (own) (void)hipFreeAsync(own, s);
  }
};

// The operands of launch `lp` of a planned group.  `lin` (optional): the fused-linear descriptors the ops were taken from.
static void fill_args(sqllm::LaunchArgs* a, const sqllm_op* ops, const sqllm_linear* lin, const GroupPlan& plan, const LaunchPlan& lp,
                      bool bf16 = false) {
  a->x = ops[0].vec;
  a->linear = lin != nullptr;
  a->bf16 = lin != nullptr && bf16;
  a->wide = lp.wide;
  a->wide_full_units = lp.wide_full_units;
  a->row_blocks = lp.row_blocks;
  a->ga.n_seg = lp.n_seg;
  memcpy(a->ga.block0, lp.block0, sizeof(lp.block0));
  memset(a->ga.seg, 0, sizeof(a->ga.seg));
  for (int i = 0; i < lp.n_seg; ++i) {
    sqllm::Segment& sg = a->ga.seg[i];
    fill_segment(&ops[lp.first + i], &sg);
    sg.gm = plan.gm[lp.first + i];
    if (lin) {
      // accumulate into the workspace plane; op->mul is the fp16 / bf16 result
      sg.y = reinterpret_cast<float*>(lin[lp.first + i].workspace);
      sg.out16 = ops[lp.first + i].mul;
      sg.bias = lin[lp.first + i].bias;
    }
  }
}

// One group of 1..kMaxSegments ops that share vec, K, bits and batch: validate -> obtain scratch -> plan -> fill the operands ->
// call the launcher(s) the plan names.  `lin` (optional) points at the fused-linear descriptors: the ops are then lin[i].op.
// `ws` / `ws_bytes`: the caller's workspace (sqllm_launch_*_ws; sqllm_workspace_bytes says how much a group can use), or null.
// `ws_entry`: the call came through a `_ws` entry point -- up to 16 rows nothing is allocated then, workspace or not.
// `bf16` (fused linears only): vec and mul are bf16 -- same route, plan and workspace; the flag travels in LaunchArgs and
// launch_fused hands such a launch to launch_linear_bf16 (sqllm_linear_bf16.hip), so the host layer calls the launchers it always did.
// `front` (the gated pair, the epilogue linear, the attention front and their norm / cache variants): what the front's kernel takes
// beyond the fused linear's arguments (sqllm_kernels.h: FrontCall), checked by the caller; the launch then goes to the kernel of its kind.
static int launch_group_with_events(const sqllm_op* ops, int n, sqllm_stream_t stream, hipEvent_t e0,
                                    hipEvent_t e1, const sqllm_linear* lin = nullptr, void* ws = nullptr, int64_t ws_bytes = 0,
                                    bool ws_entry = false, bool bf16 = false, const sqllm::FrontCall* front = nullptr) {
  if (n < 1 || n > sqllm::kMaxSegments) return SQLLM_E_GROUP;
  if (!ops && !lin) return SQLLM_E_NULL;
  sqllm_op tmp[sqllm::kMaxSegments];
  if (lin) {
    for (int i = 0; i < n; ++i) {
      tmp[i] = lin[i].op;
      if (!lin[i].workspace) return SQLLM_E_NULL;
      if ((reinterpret_cast<uintptr_t>(lin[i].workspace) & 15u) != 0) return SQLLM_E_ALIGN;
    }
    ops = tmp;
  }
  const Route route = route_of(ops, n, lin != nullptr);
  if (route == kFusedTiles && g_experimental.route) {  // (measurement library: the measured-and-not-adopted batch-1 kernels)
    int rc = SQLLM_OK;
    if (g_experimental.route(ops, n, stream, e0, e1, &rc)) return rc;
  }
  int rc = validate_group(ops, n, stream, route);
  if (rc != SQLLM_OK) return rc;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  ScratchFacts facts;
  WideScratch wide;    // (matrix-core kernel: transposed vec for the CSR role, planes + slabs for the wide form)
  SmallScratch small;  // (fused small launch)
  if (route == kPerOpMfma) {
    rc = wide.acquire(ops, n, stream, &e0, ws, ws_bytes);
    if (rc != SQLLM_OK) return rc;
    facts.xT = wide.xT != nullptr;
    facts.planes = wide.planes != nullptr;
    facts.capturing = wide.capturing;
  } else if (route == kFusedSmall) {
    small.acquire(ops, n, stream, ws, ws_bytes, ws_entry);
    facts.xT = small.xT != nullptr;
  }
  GroupPlan plan;
  plan_group(ops, n, route, facts, &plan);
  if (plan.rc != SQLLM_OK) return plan.rc;
  if (front && front->kc && front->kc->fp8 && !front->kc->scales_ok) return SQLLM_E_OPTION;  // (the fp8 cache entries: behind everything their 16-bit siblings reject)
  if (small.xT && !(g_experimental.skip_prepare_small && g_experimental.skip_prepare_small())) {  // (measurement library only: what the kernel in front costs)
    const hipError_t e = small.planes ? sqllm::prepare_small(ops[0].vec, small.xT, small.planes, ops[0].batch, ops[0].K, s, e0)
                                      : sqllm::transpose_small(ops[0].vec, small.xT, ops[0].batch, ops[0].K, s, e0);
    if (e != hipSuccess) return static_cast<int>(e);
    e0 = nullptr;
  }
  for (int l = 0; l < plan.n_launches; ++l) {
    const LaunchPlan& lp = plan.launch[l];
    const sqllm_op* op = &ops[lp.first];
    sqllm::LaunchArgs a;
    fill_args(&a, ops, lin, plan, lp, bf16);
    a.ev_start = l == 0 ? e0 : nullptr;
    a.ev_stop = l == plan.n_launches - 1 ? e1 : nullptr;
    hipError_t e = hipSuccess;
    switch (route) {
      case kFusedTiles:
      case kFusedLinear:
        if (front) {  // (the kernel file of the front's kind; without it in the link there is no such kernel, and that is an error.  Not
                      // decorated: the measurement library's ablation bits, LDS pad and timeline buffer belong to the kernels it instantiates itself)
          const sqllm::FrontLauncher launch = sqllm::g_launch_front[sqllm::front_kind(*front)];
          e = launch ? launch(op->bits, a, *front, s) : hipErrorNotSupported;
          break;
        }
        if (g_experimental.decorate) g_experimental.decorate(&a);  // (measurement library: ablation bits, LDS pad, timeline buffer)
        e = sqllm::launch_fused(op->bits, a, s);  // (a.bf16, set above for the bf16 entry points: the launcher of sqllm_linear_bf16.hip)
        break;
      case kColsGroup:
      case kPerOpCols:
        if (g_experimental.decorate) g_experimental.decorate(&a);  // (measurement library: timeline buffer of the one-row instantiations, tools/timeline.py --cols)
        e = sqllm::launch_batched_cols(op->bits, a, s);
        break;
      case kFusedSmall:
        a.xT = small.xT;
        a.planes = small.planes;
        if (g_experimental.decorate) g_experimental.decorate(&a);  // (measurement library: timeline buffer)
        e = sqllm::launch_small_split(op->bits, a, s);
        break;
      case kPerOpMfma:
        a.xT = (op->nnz > 0 && op->rows && op->cols && op->vals) ? wide.xT : nullptr;
        a.Bp = wide.Bp;
        a.planes = wide.planes;
        a.plane_flags = wide.flags;
        a.wide_slabs = wide.slabs;
        if (lp.sparse_in_grid) {
          e = sqllm::launch_batched_mfma_split_all(op->bits, a, s);
          break;
        }
        if (lp.sparse_launch) {
          sqllm::LaunchArgs as = a;
          as.ev_stop = nullptr;
          if (g_experimental.decorate) g_experimental.decorate(&as);  // (measurement library: timeline probe, tools/timeline.py --batch)
          e = sqllm::launch_batched_sparse(as, s);
          if (e != hipSuccess) return static_cast<int>(e);
          a.ev_start = nullptr;
        }
        e = lp.split ? sqllm::launch_batched_mfma_split(op->bits, a, s) : sqllm::launch_batched_mfma(op->bits, a, s);
        break;
    }
    if (e != hipSuccess) return static_cast<int>(e);
  }
  return SQLLM_OK;
}

// A pass as consecutive same-input groups: `ops` or `lins`, group g of group_sizes[g] members; *n_done = groups enqueued.
static int launch_groups(const sqllm_op* ops, const sqllm_linear* lins, const int32_t* group_sizes, int32_t n_groups, sqllm_stream_t stream,
                         int32_t* n_done, void* ws = nullptr, int64_t ws_bytes = 0, bool ws_entry = false, bool bf16 = false) {
  if (n_done) *n_done = 0;
  if (n_groups < 0 || (n_groups > 0 && ((!ops && !lins) || !group_sizes))) return SQLLM_E_NULL;
  int32_t at = 0;
  for (int32_t g = 0; g < n_groups; ++g) {
    if (group_sizes[g] < 1) return SQLLM_E_GROUP;
    int rc = launch_group_with_events(ops ? ops + at : nullptr, group_sizes[g], stream, nullptr, nullptr, lins ? lins + at : nullptr, ws, ws_bytes, ws_entry, bf16);
    if (rc != SQLLM_OK) return rc;
    at += group_sizes[g];
    if (n_done) *n_done = g + 1;
  }
  return SQLLM_OK;
}

int sqllm_linear_f16(const sqllm_linear* lin, sqllm_stream_t stream) {
  if (!lin) return SQLLM_E_NULL;
  return launch_group_with_events(nullptr, 1, stream, nullptr, nullptr, lin);
}

int sqllm_linear_f16_groups(const sqllm_linear* lins, const int32_t* group_sizes, int32_t n_groups,
                            sqllm_stream_t stream, int32_t* n_done) {
  return launch_groups(nullptr, lins, group_sizes, n_groups, stream, n_done);
}

int sqllm_linear_bf16(const sqllm_linear* lin, sqllm_stream_t stream) {
  if (!lin) return SQLLM_E_NULL;
  return launch_group_with_events(nullptr, 1, stream, nullptr, nullptr, lin, nullptr, 0, false, true);
}

int sqllm_linear_bf16_groups(const sqllm_linear* lins, const int32_t* group_sizes, int32_t n_groups,
                             sqllm_stream_t stream, int32_t* n_done) {
  return launch_groups(nullptr, lins, group_sizes, n_groups, stream, n_done, nullptr, 0, false, true);
}

// workspace of a gated pair: the two members' accumulator planes, then the plane of pair words [batch, N]
int64_t sqllm_gated_workspace_bytes(const sqllm_op* gate) {
  if (!gate || gate->N <= 0) return 0;
  return 2 * sqllm_linear_workspace_bytes(gate) + align16(8ll * (gate->batch <= 0 ? 1 : gate->batch) * gate->N);
}

// gate and up as the two-op group of the fused linear (same route, plan and validation), finished by the gated kernel
// The norm fronts' own checks, ahead of the parent's: the descriptor and its weight, then eps.
static int check_rmsnorm(const sqllm_rmsnorm* nm) {
  if (!nm || !nm->weight) return SQLLM_E_NULL;
  if (!(nm->eps >= 0.f) || nm->eps > 3.402823466e38f) return SQLLM_E_OPTION;  // (negative, NaN, infinite)
  return SQLLM_OK;
}
// the norm weight [K] against a range the launch writes (an output, the workspace)
static bool norm_weight_overlaps(const sqllm_rmsnorm* nm, int K, const void* p, int64_t bytes) {
  const uintptr_t w0 = reinterpret_cast<uintptr_t>(nm->weight), w1 = w0 + 2u * (uintptr_t)K;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(p);
  return w0 < a0 + (uintptr_t)bytes && a0 < w1;
}

// `nm` (sqllm_gated_norm_*): vec is the un-normalised hidden state and the kernel is the norm front's
static int launch_gated(const sqllm_gated* g, sqllm_stream_t stream, bool bf16, const sqllm_rmsnorm* nm = nullptr) {
  if (!g) return SQLLM_E_NULL;
  if (g->act != SQLLM_ACT_SILU) return SQLLM_E_OPTION;
  const sqllm_op &a = g->gate, &b = g->up;
  if (a.mul || b.mul) return SQLLM_E_GROUP;
  if (a.vec != b.vec || a.K != b.K || a.N != b.N || a.bits != b.bits || a.batch != b.batch)
    return SQLLM_E_GROUP;
  if (!g->out || !g->workspace) return SQLLM_E_NULL;
  if ((reinterpret_cast<uintptr_t>(g->workspace) & 15u) != 0) return SQLLM_E_ALIGN;
  const int64_t plane = sqllm_linear_workspace_bytes(&a);
  sqllm_linear lin[2];
  lin[0].op = a;
  lin[1].op = b;
  lin[0].op.mul = lin[1].op.mul = static_cast<float*>(g->out);  // (what the linear's validation and fill_args read as the output)
  lin[0].bias = g->bias_gate;
  lin[1].bias = g->bias_up;
  lin[0].workspace = g->workspace;
  lin[1].workspace = static_cast<char*>(g->workspace) + plane;
  if (nm) {
    // (shapes the linear's own validation is about to reject are left to it)
    if (a.K > 0 && a.N > 0) {
      const int64_t rows = a.batch <= 0 ? 1 : a.batch;
      if (norm_weight_overlaps(nm, a.K, g->out, 2 * rows * a.N) || norm_weight_overlaps(nm, a.K, g->workspace, sqllm_gated_workspace_bytes(&a)))
        return SQLLM_E_SHAPE;
    }
  }
  const sqllm::VecNorm vn = {nm ? nm->weight : nullptr, nm ? nm->eps : 0.f};
  sqllm::FrontCall front;
  front.pair = static_cast<char*>(g->workspace) + 2 * plane;
  front.vn = nm ? &vn : nullptr;
  return launch_group_with_events(nullptr, 2, stream, nullptr, nullptr, lin, nullptr, 0, false, bf16, &front);
}

int sqllm_gated_f16(const sqllm_gated* g, sqllm_stream_t stream) { return launch_gated(g, stream, false); }
int sqllm_gated_bf16(const sqllm_gated* g, sqllm_stream_t stream) { return launch_gated(g, stream, true); }

int sqllm_gated_norm_f16(const sqllm_gated* g, const sqllm_rmsnorm* nm, sqllm_stream_t stream) {
  const int rc = check_rmsnorm(nm);
  return rc != SQLLM_OK ? rc : launch_gated(g, stream, false, nm);
}
int sqllm_gated_norm_bf16(const sqllm_gated* g, const sqllm_rmsnorm* nm, sqllm_stream_t stream) {
  const int rc = check_rmsnorm(nm);
  return rc != SQLLM_OK ? rc : launch_gated(g, stream, true, nm);
}

// one fused linear (same route, plan, validation and workspace), finished by the epilogue kernel
static int launch_linear_ep(const sqllm_linear_ep* e, sqllm_stream_t stream, bool bf16) {
  if (!e) return SQLLM_E_NULL;
  if (e->act < SQLLM_ACT_SILU || e->act > SQLLM_ACT_GELU_TANH) return SQLLM_E_OPTION;
  const sqllm_op& op = e->lin.op;
  // the residual may be the output itself (one thread reads and writes an element); any other overlap of the two [batch, N]
  // ranges is rejected.  (Shapes the linear's own validation is about to reject are left to it.)
  if (e->residual && op.mul && e->residual != op.mul && op.N > 0) {
    const uintptr_t r = reinterpret_cast<uintptr_t>(e->residual), o = reinterpret_cast<uintptr_t>(op.mul);
    const uintptr_t bytes = 2u * (uintptr_t)(op.batch <= 0 ? 1 : op.batch) * (uintptr_t)op.N;
    if (r < o + bytes && o < r + bytes) return SQLLM_E_SHAPE;
  }
  sqllm::FrontCall front;
  front.residual = e->residual;
  front.act = e->act;
  return launch_group_with_events(nullptr, 1, stream, nullptr, nullptr, &e->lin, nullptr, 0, false, bf16, &front);
}

int sqllm_linear_ep_f16(const sqllm_linear_ep* e, sqllm_stream_t stream) { return launch_linear_ep(e, stream, false); }
int sqllm_linear_ep_bf16(const sqllm_linear_ep* e, sqllm_stream_t stream) { return launch_linear_ep(e, stream, true); }

// workspace of the attention front: the three members' accumulator planes, then the pair planes [batch, N / 2] of q and of k
static int64_t qkv_pair_bytes(const sqllm_op* m) { return align16(8ll * (m->batch <= 0 ? 1 : m->batch) * (m->N / 2)); }
int64_t sqllm_qkv_rope_workspace_bytes(const sqllm_op* q, const sqllm_op* k, const sqllm_op* v) {
  if (!q || !k || !v || q->N <= 0 || k->N <= 0 || v->N <= 0) return 0;
  return sqllm_linear_workspace_bytes(q) + sqllm_linear_workspace_bytes(k) + sqllm_linear_workspace_bytes(v) + qkv_pair_bytes(q) +
         qkv_pair_bytes(k);
}

// two byte ranges that share a byte
static bool ranges_overlap(const void* p, int64_t p_bytes, const void* q, int64_t q_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(p), b0 = reinterpret_cast<uintptr_t>(q);
  return a0 < b0 + (uintptr_t)q_bytes && b0 < a0 + (uintptr_t)p_bytes;
}

// The cache entries' own checks (sqllm_qkv_rope_cache_* / sqllm_qkv_rope_norm_cache_*): the descriptor `c` against the call `r` it
// comes with, which has passed launch_qkv_rope's own checks -- behind those and in front of the linear's validation, to which
// widths it is about to reject are left (`widths_ok`).
// `elem`: bytes per cache element (2, or 1 in the fp8 entries, whose strides and extent then count bytes)
static int check_kv_cache(const sqllm_qkv_rope* r, const sqllm_kv_cache* c, const sqllm_rmsnorm* nm, bool widths_ok, int elem = 2) {
  if (!c || !c->k_cache || !c->v_cache || !c->slots) return SQLLM_E_NULL;
  const int64_t D = r->head_dim;
  if (c->n_slots < 1 || c->slot_stride < D || c->head_stride < D) return SQLLM_E_SHAPE;
  if (!widths_ok) return SQLLM_OK;
  if (r->k.N != r->v.N || r->v.N % D) return SQLLM_E_SHAPE;
  const int64_t H = r->v.N / D;
  // the kernel forms its 64-bit offsets out of 32 x 32 -> 64-bit products: a stride that is ever multiplied lies below 2^32
  if ((c->n_slots > 1 && c->slot_stride >= (1ll << 32)) || (H > 1 && c->head_stride >= (1ll << 32))) return SQLLM_E_SHAPE;
  // (in 128 bits: strides up to 2^63 are still to be rejected by the overlap rule, not to wrap)
  const unsigned __int128 extent = (unsigned __int128)(c->n_slots - 1) * (uint64_t)c->slot_stride + (unsigned __int128)(H - 1) * (uint64_t)c->head_stride + (uint64_t)D;
  if (extent >= ((unsigned __int128)1 << 62)) return SQLLM_E_SHAPE;
  const int64_t bytes = elem * (int64_t)extent;
  const int64_t rows = r->q.batch <= 0 ? 1 : r->q.batch;
  if (ranges_overlap(c->k_cache, bytes, c->v_cache, bytes)) return SQLLM_E_SHAPE;
  void* const cache[2] = {c->k_cache, c->v_cache};
  const void* const out[3] = {r->out_q, r->out_k, r->out_v};
  const int64_t out_bytes[3] = {2 * rows * r->q.N, 2 * rows * r->k.N, 2 * rows * r->v.N};
  for (int i = 0; i < 2; ++i) {
    if (ranges_overlap(cache[i], bytes, r->workspace, sqllm_qkv_rope_workspace_bytes(&r->q, &r->k, &r->v))) return SQLLM_E_SHAPE;
    for (int j = 0; j < 3; ++j)
      if (out[j] && ranges_overlap(cache[i], bytes, out[j], out_bytes[j])) return SQLLM_E_SHAPE;
    if (r->q.vec && r->q.K > 0 && ranges_overlap(cache[i], bytes, r->q.vec, 2 * rows * r->q.K)) return SQLLM_E_SHAPE;
    if (nm && r->q.K > 0 && norm_weight_overlaps(nm, r->q.K, cache[i], bytes)) return SQLLM_E_SHAPE;
  }
  return SQLLM_OK;
}

// q, k and v as the three-op group of the fused linear (same route, plan and validation), finished by the qkv kernel
// `nm` (sqllm_qkv_rope_norm_*): vec is the un-normalised hidden state and the kernel is the norm front's
// `cache_entry` (sqllm_qkv_rope_cache_* / sqllm_qkv_rope_norm_cache_*): k and v go to the KV cache `c`, and out_k / out_v may be NULL
// `fp8` (sqllm_qkv_rope_cache_fp8_* / sqllm_qkv_rope_norm_cache_fp8_*, with `cache_entry`): the cache is `c8`, of 1-byte e4m3fn elements
static bool fp8_scale_ok(float s) { return __builtin_isfinite(s) && s > 0.0f && __builtin_isfinite(1.0f / s); }
static int launch_qkv_rope(const sqllm_qkv_rope* r, sqllm_stream_t stream, bool bf16, const sqllm_rmsnorm* nm = nullptr, bool cache_entry = false,
                           const sqllm_kv_cache* c = nullptr, bool fp8 = false, const sqllm_kv_cache_fp8* c8 = nullptr) {
  if (!r) return SQLLM_E_NULL;
  const sqllm_op* m[3] = {&r->q, &r->k, &r->v};
  void* const out[3] = {r->out_q, r->out_k, r->out_v};
  for (int i = 0; i < 3; ++i) {
    if (m[i]->mul) return SQLLM_E_GROUP;
    if (m[i]->vec != m[0]->vec || m[i]->K != m[0]->K || m[i]->bits != m[0]->bits || m[i]->batch != m[0]->batch) return SQLLM_E_GROUP;
  }
  if (r->layout != SQLLM_ROPE_HALF && r->layout != SQLLM_ROPE_INTERLEAVED) return SQLLM_E_OPTION;
  if (!r->out_q || (!cache_entry && (!r->out_k || !r->out_v)) || !r->cos || !r->sin || !r->positions || !r->workspace) return SQLLM_E_NULL;
  if ((reinterpret_cast<uintptr_t>(r->workspace) & 15u) != 0) return SQLLM_E_ALIGN;
  const int D = r->head_dim;
  if (D < 2 || (D & 1) || r->n_pos < 1) return SQLLM_E_SHAPE;
  const int64_t rows = m[0]->batch <= 0 ? 1 : m[0]->batch;
  // (shapes the linear's own validation is about to reject are left to it)
  if (r->q.N > 0 && r->k.N > 0 && r->v.N > 0) {
    for (int i = 0; i < 2; ++i) {
      if (m[i]->N % D) return SQLLM_E_SHAPE;
      // the finisher's arithmetic: c / D as a 32-bit multiply-high, b * N in 32 bits, b out of it by an fp32 multiply
      if ((int64_t)m[i]->N * D > (1ll << 32) || rows * m[i]->N >= (1ll << 31) || rows > (1 << 20)) return SQLLM_E_SHAPE;
    }
    const int64_t ws_bytes = sqllm_qkv_rope_workspace_bytes(&r->q, &r->k, &r->v);
    const uintptr_t w0 = reinterpret_cast<uintptr_t>(r->workspace);
    for (int i = 0; i < 3; ++i) {
      if (!out[i]) continue;  // (a cache entry without this output)
      const uintptr_t a0 = reinterpret_cast<uintptr_t>(out[i]), a1 = a0 + 2u * (uintptr_t)rows * (uintptr_t)m[i]->N;
      if (a0 < w0 + (uintptr_t)ws_bytes && w0 < a1) return SQLLM_E_SHAPE;
      for (int j = 0; j < i; ++j) {
        if (!out[j]) continue;
        const uintptr_t b0 = reinterpret_cast<uintptr_t>(out[j]), b1 = b0 + 2u * (uintptr_t)rows * (uintptr_t)m[j]->N;
        if (a0 < b1 && b0 < a1) return SQLLM_E_SHAPE;
      }
      if (nm && m[0]->K > 0 && norm_weight_overlaps(nm, m[0]->K, out[i], 2 * rows * m[i]->N)) return SQLLM_E_SHAPE;
    }
    if (nm && m[0]->K > 0 && norm_weight_overlaps(nm, m[0]->K, r->workspace, ws_bytes)) return SQLLM_E_SHAPE;
  }
  sqllm::KvCache kc = {};
  sqllm_kv_cache c16;
  if (fp8 && c8) {  // (the fields the two descriptors share; the scales are judged behind the linear's validation)
    c16.k_cache = c8->k_cache;
    c16.v_cache = c8->v_cache;
    c16.slots = c8->slots;
    c16.n_slots = c8->n_slots;
    c16.slot_stride = c8->slot_stride;
    c16.head_stride = c8->head_stride;
    c = &c16;
    kc.fp8 = true;
    kc.scales_ok = fp8_scale_ok(c8->k_scale) && fp8_scale_ok(c8->v_scale);
    kc.inv_k_scale = 1.0f / c8->k_scale;
    kc.inv_v_scale = 1.0f / c8->v_scale;
  }
  if (cache_entry) {
    const int rc = check_kv_cache(r, c, nm, r->q.N > 0 && r->k.N > 0 && r->v.N > 0, fp8 ? 1 : 2);
    if (rc != SQLLM_OK) return rc;
    kc.k_cache = c->k_cache;
    kc.v_cache = c->v_cache;
    kc.slots = c->slots;
    kc.n_slots = c->n_slots;
    kc.slot_stride = c->slot_stride;
    kc.head_stride = c->head_stride;
    kc.write_out_k = r->out_k != nullptr;
    kc.write_out_v = r->out_v != nullptr;
  }
  sqllm_linear lin[3];
  char* ws = static_cast<char*>(r->workspace);
  const float* bias[3] = {r->bias_q, r->bias_k, r->bias_v};
  for (int i = 0; i < 3; ++i) {
    lin[i].op = *m[i];
    // (what the linear's validation and fill_args read as the output.  A cache entry without this output: the workspace
    // stands in for the validation, and the launcher takes it out again -- KvCache::write_out_*, sqllm_cache_finish.h)
    lin[i].op.mul = static_cast<float*>(out[i] ? out[i] : r->workspace);
    lin[i].bias = bias[i];
    lin[i].workspace = ws;
    ws += sqllm_linear_workspace_bytes(m[i]);
  }
  sqllm::QkvRope qr;
  qr.pair_q = ws;
  qr.pair_k = ws + qkv_pair_bytes(&r->q);
  qr.cos = r->cos;
  qr.sin = r->sin;
  qr.positions = r->positions;
  qr.n_pos = r->n_pos;
  qr.head_dim = D;
  qr.interleaved = r->layout == SQLLM_ROPE_INTERLEAVED;
  const sqllm::VecNorm vn = {nm ? nm->weight : nullptr, nm ? nm->eps : 0.f};
  sqllm::FrontCall front;
  front.qkv = &qr;
  front.vn = nm ? &vn : nullptr;
  front.kc = cache_entry ? &kc : nullptr;
  return launch_group_with_events(nullptr, 3, stream, nullptr, nullptr, lin, nullptr, 0, false, bf16, &front);
}

int sqllm_qkv_rope_f16(const sqllm_qkv_rope* r, sqllm_stream_t stream) { return launch_qkv_rope(r, stream, false); }
int sqllm_qkv_rope_bf16(const sqllm_qkv_rope* r, sqllm_stream_t stream) { return launch_qkv_rope(r, stream, true); }

int sqllm_qkv_rope_norm_f16(const sqllm_qkv_rope* r, const sqllm_rmsnorm* nm, sqllm_stream_t stream) {
  const int rc = check_rmsnorm(nm);
  return rc != SQLLM_OK ? rc : launch_qkv_rope(r, stream, false, nm);
}
int sqllm_qkv_rope_norm_bf16(const sqllm_qkv_rope* r, const sqllm_rmsnorm* nm, sqllm_stream_t stream) {
  const int rc = check_rmsnorm(nm);
  return rc != SQLLM_OK ? rc : launch_qkv_rope(r, stream, true, nm);
}

int sqllm_qkv_rope_cache_f16(const sqllm_qkv_rope* r, const sqllm_kv_cache* c, sqllm_stream_t stream) {
  return launch_qkv_rope(r, stream, false, nullptr, true, c);
}
int sqllm_qkv_rope_cache_bf16(const sqllm_qkv_rope* r, const sqllm_kv_cache* c, sqllm_stream_t stream) {
  return launch_qkv_rope(r, stream, true, nullptr, true, c);
}
int sqllm_qkv_rope_norm_cache_f16(const sqllm_qkv_rope* r, const sqllm_rmsnorm* nm, const sqllm_kv_cache* c, sqllm_stream_t stream) {
  const int rc = check_rmsnorm(nm);
  return rc != SQLLM_OK ? rc : launch_qkv_rope(r, stream, false, nm, true, c);
}
int sqllm_qkv_rope_norm_cache_bf16(const sqllm_qkv_rope* r, const sqllm_rmsnorm* nm, const sqllm_kv_cache* c, sqllm_stream_t stream) {
  const int rc = check_rmsnorm(nm);
  return rc != SQLLM_OK ? rc : launch_qkv_rope(r, stream, true, nm, true, c);
}

int sqllm_qkv_rope_cache_fp8_f16(const sqllm_qkv_rope* r, const sqllm_kv_cache_fp8* c, sqllm_stream_t stream) {
  return launch_qkv_rope(r, stream, false, nullptr, true, nullptr, true, c);
}
int sqllm_qkv_rope_cache_fp8_bf16(const sqllm_qkv_rope* r, const sqllm_kv_cache_fp8* c, sqllm_stream_t stream) {
  return launch_qkv_rope(r, stream, true, nullptr, true, nullptr, true, c);
}
int sqllm_qkv_rope_norm_cache_fp8_f16(const sqllm_qkv_rope* r, const sqllm_rmsnorm* nm, const sqllm_kv_cache_fp8* c, sqllm_stream_t stream) {
  const int rc = check_rmsnorm(nm);
  return rc != SQLLM_OK ? rc : launch_qkv_rope(r, stream, false, nm, true, nullptr, true, c);
}
int sqllm_qkv_rope_norm_cache_fp8_bf16(const sqllm_qkv_rope* r, const sqllm_rmsnorm* nm, const sqllm_kv_cache_fp8* c, sqllm_stream_t stream) {
  const int rc = check_rmsnorm(nm);
  return rc != SQLLM_OK ? rc : launch_qkv_rope(r, stream, true, nm, true, nullptr, true, c);
}

// Decode attention (sqllm_attn_decode_*): the partitions of the launch, from HOST fields alone.  capacity is what the table
// can address, clipped to what an int32 seq_lens can ask for.
static int64_t attn_capacity(int32_t max_blocks, int32_t block_size) {
  const int64_t cap = (int64_t)max_blocks * block_size;
  return cap < INT32_MAX ? cap : INT32_MAX;
}
static int64_t attn_parts(int32_t max_blocks, int32_t block_size) {
  return (attn_capacity(max_blocks, block_size) + SQLLM_ATTN_PARTITION - 1) / SQLLM_ATTN_PARTITION;
}
static_assert(SQLLM_ATTN_PARTITION == sqllm::kAttnPartition, "the header documents the kernel's partition");

int64_t sqllm_attn_decode_workspace_bytes(int32_t batch, int32_t n_q_heads, int32_t head_dim, int32_t max_blocks, int32_t block_size) {
  if (batch < 1 || n_q_heads < 1 || head_dim < 1 || max_blocks < 1 || block_size < 1) return 0;
  // per (row, query head, partition): acc[head_dim], max, sum -- asked for with one partition too, where nothing is written
  return (int64_t)batch * n_q_heads * attn_parts(max_blocks, block_size) * (head_dim + 2) * 4;
}

// The partitions a window of `window` keys can touch (sqllm_attn_decode_window_*): one more than it fills when it starts inside
// one, never more than the table has.  64-bit: window may be INT32_MAX.
static int64_t attn_window_parts(int32_t max_blocks, int32_t block_size, int32_t window) {
  const int64_t n_parts = attn_parts(max_blocks, block_size);
  const int64_t touched = ((int64_t)window - 1 + SQLLM_ATTN_PARTITION - 1) / SQLLM_ATTN_PARTITION + 1;
  return touched < n_parts ? touched : n_parts;
}

int64_t sqllm_attn_window_workspace_bytes(int32_t batch, int32_t n_q_heads, int32_t head_dim, int32_t max_blocks, int32_t block_size, int32_t window) {
  if (batch < 1 || n_q_heads < 1 || head_dim < 1 || max_blocks < 1 || block_size < 1 || window < 1) return 0;
  // per (row, query head, RELATIVE partition): acc[head_dim], max, sum
  return (int64_t)batch * n_q_heads * attn_window_parts(max_blocks, block_size, window) * (head_dim + 2) * 4;
}

// The twelve attention entries.  The four descriptors begin with the fields of sqllm_attn_decode (`lead`, checked below); what
// follows them is passed on by each entry:
//   `kv_scales` (the fp8 entries): {k_scale, v_scale} of the descriptor -- the caches hold 1-byte e4m3fn elements, their strides
//     and extents count bytes and they need no alignment; the scales are judged last.  NULL: 16-bit caches.
//   `tokens` (sqllm_attn_append_*): lead.batch counts sequences of q_len rows each, `q_lens` (or NULL) their real tokens.  NULL:
//     the one-query entries -- so a q_len below 1 in an append descriptor is a count < 1, never the one-query call.
//   `window` (sqllm_attn_decode_window_*): the keys [max(0, L - *window), L) of every row; a count as the others.  The launch and
//     the workspace are sized by the partitions a window can touch, and the call goes to g_launch_attn_window.  NULL: no window.
struct AttnTokensTail {
  const int32_t* q_lens;
  int32_t q_len;
};
static int launch_attn(const sqllm_attn_decode& lead, sqllm_stream_t stream, bool bf16, const float* kv_scales, const AttnTokensTail* tokens,
                       const int32_t* window = nullptr) {
  const sqllm_attn_decode* const a = &lead;
  const bool append = tokens != nullptr;
  const int32_t q_len = append ? tokens->q_len : 0;
  const int32_t* const q_lens = append ? tokens->q_lens : nullptr;
  const int celem = kv_scales ? 1 : 2;  // bytes per cache element
  if (!a->q || !a->out || !a->k_cache || !a->v_cache || !a->block_table || !a->seq_lens || !a->workspace) return SQLLM_E_NULL;
  const int64_t D = a->head_dim;
  if (a->batch < 1 || a->n_q_heads < 1 || a->n_kv_heads < 1 || D < 1 || a->n_slots < 1 || a->block_size < 1 || a->max_blocks < 1 ||
      a->table_stride < 1 || (append && q_len < 1) || (window && *window < 1))
    return SQLLM_E_SHAPE;
  const int64_t rows = append ? (int64_t)a->batch * q_len : a->batch;  // of q, out and the workspace
  const int64_t width = (int64_t)a->n_q_heads * D;
  if (a->slot_stride < D || a->head_stride < D || a->q_stride < width || a->out_stride < width) return SQLLM_E_SHAPE;
  if (a->max_blocks > a->table_stride) return SQLLM_E_SHAPE;
  // what the kernel serves
  if ((D != 64 && D != 128) || a->n_q_heads % a->n_kv_heads || a->n_q_heads / a->n_kv_heads > 8 || rows > 64 || a->n_q_heads > 65535 ||
      (append && q_len > 16))
    return SQLLM_E_SHAPE;
  // as for sqllm_kv_cache: 32 x 32 -> 64-bit products, and extents that do not wrap
  const int64_t H = a->n_kv_heads;
  if ((a->n_slots > 1 && a->slot_stride >= (1ll << 32)) || (H > 1 && a->head_stride >= (1ll << 32))) return SQLLM_E_SHAPE;
  const unsigned __int128 extent = (unsigned __int128)(a->n_slots - 1) * (uint64_t)a->slot_stride + (unsigned __int128)(H - 1) * (uint64_t)a->head_stride + (uint64_t)D;
  const unsigned __int128 q_extent = (unsigned __int128)(rows - 1) * (uint64_t)a->q_stride + (uint64_t)width;
  const unsigned __int128 out_extent = (unsigned __int128)(rows - 1) * (uint64_t)a->out_stride + (uint64_t)width;
  if (extent >= ((unsigned __int128)1 << 62) || q_extent >= ((unsigned __int128)1 << 62) || out_extent >= ((unsigned __int128)1 << 62)) return SQLLM_E_SHAPE;
  if (!__builtin_isfinite(a->scale)) return SQLLM_E_OPTION;
  const int64_t ws_bytes = window ? sqllm_attn_window_workspace_bytes((int32_t)rows, a->n_q_heads, a->head_dim, a->max_blocks, a->block_size, *window)
                                  : sqllm_attn_decode_workspace_bytes((int32_t)rows, a->n_q_heads, a->head_dim, a->max_blocks, a->block_size);
  const void* const in[6] = {a->q, a->k_cache, a->v_cache, a->block_table, a->seq_lens, q_lens};
  const int64_t in_bytes[6] = {2 * (int64_t)q_extent, celem * (int64_t)extent, celem * (int64_t)extent,
                               4 * ((int64_t)(a->batch - 1) * a->table_stride + a->max_blocks), 4 * (int64_t)a->batch, 4 * (int64_t)a->batch};
  for (int i = 0; i < (q_lens ? 6 : 5); ++i)
    if (ranges_overlap(a->out, 2 * (int64_t)out_extent, in[i], in_bytes[i]) || ranges_overlap(a->workspace, ws_bytes, in[i], in_bytes[i]))
      return SQLLM_E_SHAPE;
  if (ranges_overlap(a->out, 2 * (int64_t)out_extent, a->workspace, ws_bytes)) return SQLLM_E_SHAPE;
  if (((reinterpret_cast<uintptr_t>(a->q) | reinterpret_cast<uintptr_t>(a->out)) & 1u) != 0 ||
      (!kv_scales && ((reinterpret_cast<uintptr_t>(a->k_cache) | reinterpret_cast<uintptr_t>(a->v_cache)) & 1u) != 0) ||
      (reinterpret_cast<uintptr_t>(a->workspace) & 3u) != 0)
    return SQLLM_E_ALIGN;
  float scale = a->scale;
  if (kv_scales) {
    if (!fp8_scale_ok(kv_scales[0]) || !fp8_scale_ok(kv_scales[1])) return SQLLM_E_OPTION;
    scale = a->scale * kv_scales[0];  // (rounded once, here)
    if (!__builtin_isfinite(scale)) return SQLLM_E_OPTION;
  }
  sqllm::AttnCall c;
  c.q = a->q;
  c.out = a->out;
  c.k_cache = a->k_cache;
  c.v_cache = a->v_cache;
  c.block_table = a->block_table;
  c.seq_lens = a->seq_lens;
  c.workspace = a->workspace;
  c.batch = a->batch;
  c.n_q_heads = a->n_q_heads;
  c.n_kv_heads = a->n_kv_heads;
  c.head_dim = a->head_dim;
  c.n_slots = a->n_slots;
  c.block_size = a->block_size;
  c.table_stride = a->table_stride;
  c.capacity = (int)attn_capacity(a->max_blocks, a->block_size);
  c.n_parts = (int)(window ? attn_window_parts(a->max_blocks, a->block_size, *window) : attn_parts(a->max_blocks, a->block_size));
  c.slot_stride = a->slot_stride;
  c.head_stride = a->head_stride;
  c.q_stride = a->q_stride;
  c.out_stride = a->out_stride;
  c.scale = scale;
  c.bf16 = bf16;
  c.fp8 = kv_scales != nullptr;
  c.v_scale = kv_scales ? kv_scales[1] : 1.0f;
  c.q_lens = q_lens;
  c.q_len = q_len;  // (0: one query per sequence; an append call has passed q_len >= 1 above)
  c.window = window ? *window : 0;
  // (a window has a table of its own: a null slot there is an error, never the kernels without a window)
  const sqllm::AttnLauncher launch = window ? sqllm::g_launch_attn_window[c.fp8 ? 1 : 0] : sqllm::g_launch_attn[sqllm::attn_kind(c)];
  return static_cast<int>(launch ? launch(c, static_cast<hipStream_t>(stream)) : hipErrorNotSupported);
}

// every leading field of the three longer descriptors sits where sqllm_attn_decode has it, so its first bytes ARE one
#define SQLLM_ATTN_LEAD_AT(S, F) (offsetof(S, F) == offsetof(sqllm_attn_decode, F) && sizeof(S::F) == sizeof(sqllm_attn_decode::F))
#define SQLLM_ATTN_LEAD(S)                                                                                                        \
  static_assert(SQLLM_ATTN_LEAD_AT(S, q) && SQLLM_ATTN_LEAD_AT(S, out) && SQLLM_ATTN_LEAD_AT(S, k_cache) && SQLLM_ATTN_LEAD_AT(S, v_cache) && \
                    SQLLM_ATTN_LEAD_AT(S, block_table) && SQLLM_ATTN_LEAD_AT(S, seq_lens) && SQLLM_ATTN_LEAD_AT(S, batch) &&       \
                    SQLLM_ATTN_LEAD_AT(S, n_q_heads) && SQLLM_ATTN_LEAD_AT(S, n_kv_heads) && SQLLM_ATTN_LEAD_AT(S, head_dim) &&    \
                    SQLLM_ATTN_LEAD_AT(S, n_slots) && SQLLM_ATTN_LEAD_AT(S, block_size) && SQLLM_ATTN_LEAD_AT(S, max_blocks) &&    \
                    SQLLM_ATTN_LEAD_AT(S, table_stride) && SQLLM_ATTN_LEAD_AT(S, slot_stride) && SQLLM_ATTN_LEAD_AT(S, head_stride) && \
                    SQLLM_ATTN_LEAD_AT(S, q_stride) && SQLLM_ATTN_LEAD_AT(S, out_stride) && SQLLM_ATTN_LEAD_AT(S, scale) &&        \
                    SQLLM_ATTN_LEAD_AT(S, workspace) && offsetof(S, workspace) + sizeof(void*) == sizeof(sqllm_attn_decode),       \
                #S " begins with the fields of sqllm_attn_decode")
SQLLM_ATTN_LEAD(sqllm_attn_decode_fp8);
SQLLM_ATTN_LEAD(sqllm_attn_append);
SQLLM_ATTN_LEAD(sqllm_attn_append_fp8);
#undef SQLLM_ATTN_LEAD
#undef SQLLM_ATTN_LEAD_AT

// the leading fields of a descriptor, by copy (not through a pointer of another struct's type)
extern "C++" template <typename A>
static sqllm_attn_decode attn_lead(const A* p) {
  sqllm_attn_decode lead;
  memcpy(&lead, p, sizeof(lead));
  return lead;
}
extern "C++" template <typename A>
static int launch_attn_fp8(const A* p, sqllm_stream_t stream, bool bf16, const AttnTokensTail* tokens, const int32_t* window = nullptr) {
  const float kv_scales[2] = {p->k_scale, p->v_scale};
  return launch_attn(attn_lead(p), stream, bf16, kv_scales, tokens, window);
}
extern "C++" template <typename A>
static AttnTokensTail attn_tokens(const A* p) { return {p->q_lens, p->q_len}; }

int sqllm_attn_decode_f16(const sqllm_attn_decode* a, sqllm_stream_t stream) {
  return a ? launch_attn(*a, stream, false, nullptr, nullptr) : SQLLM_E_NULL;
}
int sqllm_attn_decode_bf16(const sqllm_attn_decode* a, sqllm_stream_t stream) {
  return a ? launch_attn(*a, stream, true, nullptr, nullptr) : SQLLM_E_NULL;
}
int sqllm_attn_decode_fp8_f16(const sqllm_attn_decode_fp8* a, sqllm_stream_t stream) {
  return a ? launch_attn_fp8(a, stream, false, nullptr) : SQLLM_E_NULL;
}
int sqllm_attn_decode_fp8_bf16(const sqllm_attn_decode_fp8* a, sqllm_stream_t stream) {
  return a ? launch_attn_fp8(a, stream, true, nullptr) : SQLLM_E_NULL;
}
int sqllm_attn_decode_window_f16(const sqllm_attn_decode* a, int32_t window, sqllm_stream_t stream) {
  return a ? launch_attn(*a, stream, false, nullptr, nullptr, &window) : SQLLM_E_NULL;
}
int sqllm_attn_decode_window_bf16(const sqllm_attn_decode* a, int32_t window, sqllm_stream_t stream) {
  return a ? launch_attn(*a, stream, true, nullptr, nullptr, &window) : SQLLM_E_NULL;
}
int sqllm_attn_decode_window_fp8_f16(const sqllm_attn_decode_fp8* a, int32_t window, sqllm_stream_t stream) {
  return a ? launch_attn_fp8(a, stream, false, nullptr, &window) : SQLLM_E_NULL;
}
int sqllm_attn_decode_window_fp8_bf16(const sqllm_attn_decode_fp8* a, int32_t window, sqllm_stream_t stream) {
  return a ? launch_attn_fp8(a, stream, true, nullptr, &window) : SQLLM_E_NULL;
}
static int launch_attn_append(const sqllm_attn_append* a, sqllm_stream_t stream, bool bf16) {
  if (!a) return SQLLM_E_NULL;
  const AttnTokensTail t = attn_tokens(a);
  return launch_attn(attn_lead(a), stream, bf16, nullptr, &t);
}
static int launch_attn_append_fp8(const sqllm_attn_append_fp8* a, sqllm_stream_t stream, bool bf16) {
  if (!a) return SQLLM_E_NULL;
  const AttnTokensTail t = attn_tokens(a);
  return launch_attn_fp8(a, stream, bf16, &t);
}
int sqllm_attn_append_f16(const sqllm_attn_append* a, sqllm_stream_t stream) { return launch_attn_append(a, stream, false); }
int sqllm_attn_append_bf16(const sqllm_attn_append* a, sqllm_stream_t stream) { return launch_attn_append(a, stream, true); }
int sqllm_attn_append_fp8_f16(const sqllm_attn_append_fp8* a, sqllm_stream_t stream) { return launch_attn_append_fp8(a, stream, false); }
int sqllm_attn_append_fp8_bf16(const sqllm_attn_append_fp8* a, sqllm_stream_t stream) { return launch_attn_append_fp8(a, stream, true); }

int sqllm_launch(const sqllm_op* op, sqllm_stream_t stream) {
  return launch_group_with_events(op, 1, stream, nullptr, nullptr);
}

int sqllm_launch_group(const sqllm_op* ops, int32_t n_ops, sqllm_stream_t stream) {
  return launch_group_with_events(ops, n_ops, stream, nullptr, nullptr);
}

int sqllm_launch_groups(const sqllm_op* ops, const int32_t* group_sizes, int32_t n_groups,
                        sqllm_stream_t stream, int32_t* n_done) {
  return launch_groups(ops, nullptr, group_sizes, n_groups, stream, n_done);
}

// what a `_ws` launch of the group can use: the scratch its route asks for (the launch asks the same code)
int64_t sqllm_workspace_bytes(const sqllm_op* ops, int32_t n_ops) {
  if (!ops || n_ops < 1 || ops[0].batch < 2 || ops[0].K <= 0) return 0;  // (batch 1: one kernel, no scratch)
  int64_t need = 0;
  const Route route = route_of(ops, n_ops, false);
  if (route == kFusedSmall) need = SmallScratch::layout(ops, n_ops).total();
  else if (route == kPerOpMfma) need = (int64_t)WideScratch::layout(ops, n_ops, false).total();
  return (need + 255) / 256 * 256;
}

int sqllm_launch_ws(const sqllm_op* op, void* workspace, int64_t workspace_bytes, sqllm_stream_t stream) {
  return launch_group_with_events(op, 1, stream, nullptr, nullptr, nullptr, workspace, workspace_bytes, true);
}

int sqllm_launch_group_ws(const sqllm_op* ops, int32_t n_ops, void* workspace, int64_t workspace_bytes, sqllm_stream_t stream) {
  return launch_group_with_events(ops, n_ops, stream, nullptr, nullptr, nullptr, workspace, workspace_bytes, true);
}

int sqllm_launch_groups_ws(const sqllm_op* ops, const int32_t* group_sizes, int32_t n_groups, void* workspace,
                           int64_t workspace_bytes, sqllm_stream_t stream, int32_t* n_done) {
  return launch_groups(ops, nullptr, group_sizes, n_groups, stream, n_done, workspace, workspace_bytes, true);
}

int sqllm_launch_sequence(const sqllm_op* ops, int32_t n_ops, sqllm_stream_t stream, int32_t* n_done) {
  if (n_done) *n_done = 0;
  if (n_ops < 0 || (n_ops > 0 && !ops)) return SQLLM_E_NULL;
  for (int32_t i = 0; i < n_ops; ++i) {
    int rc = sqllm_launch(&ops[i], stream);
    if (rc != SQLLM_OK) return rc;
    if (n_done) *n_done = i + 1;
  }
  return SQLLM_OK;
}

int sqllm_profile_groups(const sqllm_op* ops, const int32_t* group_sizes, int32_t n_groups,
                         sqllm_stream_t stream, int32_t reps, float* avg_us) {
  return sqllm_profile_groups_ws(ops, group_sizes, n_groups, nullptr, 0, stream, reps, avg_us);
}

int sqllm_profile_groups_ws(const sqllm_op* ops, const int32_t* group_sizes, int32_t n_groups, void* workspace,
                            int64_t workspace_bytes, sqllm_stream_t stream, int32_t reps, float* avg_us) {
  if (n_groups < 0 || reps < 1 || (n_groups > 0 && (!ops || !group_sizes || !avg_us))) return SQLLM_E_NULL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipEvent_t* ev = new hipEvent_t[2 * (size_t)n_groups + 1];
  int rc = SQLLM_OK;
  int made = 0;
  for (; made < 2 * n_groups; ++made)
    if (hipEventCreate(&ev[made]) != hipSuccess) { rc = (int)hipGetLastError(); break; }
  for (int i = 0; i < n_groups; ++i) avg_us[i] = 0.f;
  for (int r = 0; r < reps && rc == SQLLM_OK; ++r) {
    int32_t at = 0;
    for (int g = 0; g < n_groups && rc == SQLLM_OK; ++g) {
      rc = launch_group_with_events(ops + at, group_sizes[g], stream, ev[2 * g], ev[2 * g + 1], nullptr, workspace, workspace_bytes);
      at += group_sizes[g];
    }
    if (rc != SQLLM_OK) break;
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) { rc = (int)e; break; }
    for (int g = 0; g < n_groups; ++g) {
      float ms = 0.f;
      e = hipEventElapsedTime(&ms, ev[2 * g], ev[2 * g + 1]);
      if (e != hipSuccess) { rc = (int)e; break; }
      avg_us[g] += ms * 1000.f;
    }
  }
  for (int g = 0; g < n_groups; ++g) avg_us[g] /= (float)reps;
  for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]);
  delete[] ev;
  return rc;
}

int sqllm_profile_sequence(const sqllm_op* ops, int32_t n_ops, sqllm_stream_t stream, int32_t reps,
                           float* avg_us) {
  if (n_ops < 0) return SQLLM_E_NULL;
  int32_t* ones = new int32_t[n_ops > 0 ? n_ops : 1];
  for (int32_t i = 0; i < n_ops; ++i) ones[i] = 1;
  int rc = sqllm_profile_groups(ops, ones, n_ops, stream, reps, avg_us);
  delete[] ones;
  return rc;
}

// ---- the reference operator names -------------------------------------------------------------

static int named(int bits, int batch, int vec_height, const float* vec, const int32_t* mat,
                 float* mul, const float* lut, int height, int width, const int32_t* rows,
                 const int32_t* cols, const float* vals, int nnz, int num_rows,
                 const float* full_rows, const int32_t* full_idx, int topX, bool has_csr,
                 bool has_topx, sqllm_stream_t stream) {
  if (bits != 3 && bits != 4) return SQLLM_E_BITS;
  if (height <= 0 || width <= 0 || (height % bits) != 0) return SQLLM_E_SHAPE;
  sqllm_op op;
  memset(&op, 0, sizeof(op));
  op.bits = bits;
  op.K = height / bits * 32;  // height = K/32*bits (squeezellm/quant.py:48-51)
  op.N = width;
  op.batch = batch;
  if (batch > 0 && vec_height != op.K) return SQLLM_E_BATCH;
  op.vec = vec;
  op.qweight = mat;
  op.mul = mul;
  op.lookup_table = lut;
  if (has_csr) {
    if (num_rows != width) return SQLLM_E_SPARSE;  // CSR rows are output channels (quant.py:233)
    if (!rows) return SQLLM_E_NULL;
    op.rows = rows;
    op.cols = cols;
    op.vals = vals;
    op.nnz = nnz;
  }
  if (has_topx) {
    if (topX > 0 && !full_rows) return SQLLM_E_NULL;
    op.full_rows = topX > 0 ? full_rows : nullptr;
    op.full_row_indices = full_idx;
    op.topX = topX;
  }
  return sqllm_launch(&op, stream);
}

#define SQLLM_DENSE(BITS)                                                                          \
  int sqllm_vecquant##BITS##matmul_nuq_perchannel(const float* vec, const int32_t* mat, float* mul, \
                                                  const float* lookup_table, int height, int width, \
                                                  sqllm_stream_t stream) {                          \
    return named(BITS, 0, 0, vec, mat, mul, lookup_table, height, width, nullptr, nullptr, nullptr, \
                 0, 0, nullptr, nullptr, 0, false, false, stream);                                  \
  }                                                                                                 \
  int sqllm_vecquant##BITS##matmul_nuq_perchannel_batched(                                          \
      const float* vec, const int32_t* mat, float* mul, const float* lookup_table, int height,      \
      int width, int batch, int vec_height, sqllm_stream_t stream) {                                \
    if (batch < 1) return SQLLM_E_BATCH;                                                            \
    return named(BITS, batch, vec_height, vec, mat, mul, lookup_table, height, width, nullptr,      \
                 nullptr, nullptr, 0, 0, nullptr, nullptr, 0, false, false, stream);                \
  }

#define SQLLM_SPMV(BITS)                                                                            \
  int sqllm_vecquant##BITS##matmul_spmv_nuq_perchannel(                                             \
      const int32_t* rows, const int32_t* cols, const float* mat, const float* vec, float* mul,     \
      int num_rows, const int32_t* matq, const float* lookup_table, int height, int width, int nnz, \
      sqllm_stream_t stream) {                                                                      \
    return named(BITS, 0, 0, vec, matq, mul, lookup_table, height, width, rows, cols, mat, nnz,     \
                 num_rows, nullptr, nullptr, 0, true, false, stream);                               \
  }                                                                                                 \
  int sqllm_vecquant##BITS##matmul_spmv_nuq_perchannel_batched(                                     \
      const int32_t* rows, const int32_t* cols, const float* mat, const float* vec, float* mul,     \
      int num_rows, const int32_t* matq, const float* lookup_table, int height, int width, int nnz, \
      int batch, int vec_height, sqllm_stream_t stream) {                                           \
    if (batch < 1) return SQLLM_E_BATCH;                                                            \
    return named(BITS, batch, vec_height, vec, matq, mul, lookup_table, height, width, rows, cols,  \
                 mat, nnz, num_rows, nullptr, nullptr, 0, true, false, stream);                     \
  }                                                                                                 \
  int sqllm_vecquant##BITS##matmul_spmv_balanced_nuq_perchannel(                                    \
      const int32_t* rows, const int32_t* cols, const int32_t* startrows, const float* mat,         \
      const float* vec, float* mul, const int32_t* matq, const float* lookup_table, int num_rows,   \
      int num_threads, int numvals, int height, int width, sqllm_stream_t stream) {                 \
    (void)startrows;                                                                                \
    (void)num_threads;                                                                              \
    return named(BITS, 0, 0, vec, matq, mul, lookup_table, height, width, rows, cols, mat, numvals, \
                 num_rows, nullptr, nullptr, 0, true, false, stream);                               \
  }

#define SQLLM_HYBRID(BITS)                                                                          \
  int sqllm_vecquant##BITS##matmul_spmv_hybrid_nuq_perchannel(                                      \
      const int32_t* rows, const int32_t* cols, const float* mat, const float* vec,                 \
      const float* full_rows, const int32_t* full_row_indices, float* mul, int num_rows,            \
      const int32_t* matq, const float* lookup_table, int height, int width, int nnz, int topX,     \
      sqllm_stream_t stream) {                                                                      \
    return named(BITS, 0, 0, vec, matq, mul, lookup_table, height, width, rows, cols, mat, nnz,     \
                 num_rows, full_rows, full_row_indices, topX, true, true, stream);                  \
  }                                                                                                 \
  int sqllm_vecquant##BITS##matmul_spmv_hybrid_nuq_perchannel_batched(                              \
      const int32_t* rows, const int32_t* cols, const float* mat, const float* vec,                 \
      const float* full_rows, const int32_t* full_row_indices, float* mul, int num_rows,            \
      const int32_t* matq, const float* lookup_table, int height, int width, int nnz, int topX,     \
      int batch, int vec_height, sqllm_stream_t stream) {                                           \
    if (batch < 1) return SQLLM_E_BATCH;                                                            \
    return named(BITS, batch, vec_height, vec, matq, mul, lookup_table, height, width, rows, cols,  \
                 mat, nnz, num_rows, full_rows, full_row_indices, topX, true, true, stream);        \
  }

SQLLM_DENSE(3)
SQLLM_DENSE(4)
SQLLM_SPMV(3)
SQLLM_SPMV(4)
SQLLM_HYBRID(3)
SQLLM_HYBRID(4)

}  // extern "C"
