// sqllm_kv_compact.hip -- move the K and V rows of an accepted draft path to the front of the tree's slots, in every cache of the
// model at once (include/sqllm_hip.h: sqllm_kv_compact).  Node t of a verified tree was stored as key C_b + t; the accepted path
// path[b, 0 .. a) must become the keys C_b .. C_b + a - 1 before seq_lens = C_b + a holds.  Bytes are copied as bytes: 16-bit and
// e4m3fn caches, paged and head-major static, through the block table.
//
// Split.  One wave per (kv head, cache, sequence) workgroup; grid (n_kv_heads, n_caches, batch); the cache pointers arrive by
// value in the argument block and are picked by blockIdx.y (a scalar load).
//   - Resolve.  Lane j judges element j of the path: its source key C_b + path[b, j], its destination key C_b + j, both slots
//     through the table, and the move bit (sqllm_hip.h's skip rules).  ONE ballot gives the word of moving rows; a workgroup whose
//     word is 0 -- the path that is its own prefix, the common case -- leaves before it touches a cache.
//   - Move.  A row is ROWB = head_dim * elem_bytes bytes; with accesses of VEC bytes ROWB / VEC lanes carry one row, 64 / (ROWB / VEC)
//     rows go in one pass (one row in two halves where ROWB / VEC is 128), and the slots of a pass's rows come from the resolving
//     lanes by a lane shuffle.  With 16-byte accesses ALL loads of the workgroup are issued first and held in registers (at most 64
//     rows x 256 B = 64 VGPRs); the stores follow.  Program order inside the one wave IS the hazard rule -- every source of the
//     sequence is read before any destination is written, the chain path = [1, 2, 3, ...] included: no LDS, no barrier.  Different
//     workgroups touch disjoint bytes (another head, another cache, another sequence's rows).
//   - Narrow accesses (4, 2, 1 bytes: odd base addresses or strides) need up to 64 passes; they go in chunks of 16 passes, loads
//     then stores, the chunks in ascending order of the elements -- which is the same rule, see the kernel.
//   - Passes run over the elements 0 .. (highest moving element), not over a compacted list: a pass without a moving row costs a
//     uniform branch.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 4.4.  No scratch, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sqllm_tree_accept.h"

namespace sqllm {

template <int VEC> struct CompactWord;
typedef uint32_t compact_u32x4 __attribute__((ext_vector_type(4)));
template <> struct CompactWord<16> { typedef compact_u32x4 type; };
template <> struct CompactWord<4> { typedef uint32_t type; };
template <> struct CompactWord<2> { typedef uint16_t type; };
template <> struct CompactWord<1> { typedef uint8_t type; };

// the lane map of a (row bytes, access width) pair
template <int ROWB, int VEC>
struct CompactMap {
  static constexpr int UPR = ROWB / VEC;                  // accesses per row
  static constexpr int HALVES = UPR > 64 ? UPR / 64 : 1;  // ... of one lane
  static constexpr int LPR = UPR / HALVES;                // lanes per row
  static constexpr int RPP = 64 / LPR;                    // rows per pass
  static constexpr int NP = 64 / RPP;                     // passes at most
  static constexpr int CH = NP < 16 ? NP : 16;            // passes whose rows are held in registers at once
  static constexpr int NCH = NP / CH;
  static_assert(UPR >= 4 && UPR <= 128 && LPR * RPP == 64, "the lane map");
};

// Passes P .. CH - 1 of the chunk that begins at element j0, NESTED: pass P loads its rows, the passes behind it run, then pass P
// stores -- so all loads of the chunk stand in front of all its stores, and a row's registers live in one scope (a pair of unrolled
// loops would merge every pass's registers with "not loaded" at each uniform branch).  The stores of a chunk run last pass first;
// they go to different rows.  The lanes of a row that does not move load the last moving row's source instead (`spare`: bytes inside
// the cache that another lane reads anyway) and store nothing: a load under a lane mask would cost a register copy per pass.
template <int ROWB, int VEC, int P>
__device__ __forceinline__ void compact_passes(unsigned char* cache, unsigned long long slot_bytes, int src, int dst, int spare, int j0, int last,
                                               int sub, unsigned at) {
  typedef CompactMap<ROWB, VEC> M;
  typedef typename CompactWord<VEC>::type word_t;
  if constexpr (P < M::CH) {
    if (j0 + P * M::RPP > last) return;  // (uniform)
    const int s = __shfl(src, j0 + P * M::RPP + sub, 64);
    const int d = __shfl(dst, j0 + P * M::RPP + sub, 64);  // (-1 wherever src is)
    const unsigned char* const from = cache + (unsigned long long)(unsigned)(s >= 0 ? s : spare) * slot_bytes + at;
    word_t held[M::HALVES];
#pragma unroll
    for (int e = 0; e < M::HALVES; ++e) held[e] = *reinterpret_cast<const word_t*>(from + e * 64 * VEC);
    compact_passes<ROWB, VEC, P + 1>(cache, slot_bytes, src, dst, spare, j0, last, sub, at);
    if (d >= 0) {
      unsigned char* const to = cache + (unsigned long long)(unsigned)d * slot_bytes + at;
#pragma unroll
      for (int e = 0; e < M::HALVES; ++e) *reinterpret_cast<word_t*>(to + e * 64 * VEC) = held[e];
    }
  }
}

template <int ROWB, int VEC>
__global__ void __launch_bounds__(64) sqllm_kv_compact_kernel(const KvCompactArgs a) {
  typedef CompactMap<ROWB, VEC> M;
  const int lane = threadIdx.x;
  const int h = blockIdx.x, b = blockIdx.z;

  // element `lane` of the sequence's path
  const int T = a.q_len;
  const int n = a.q_lens ? a.q_lens[b] : T;
  const int seq = a.seq_lens[b], alen = a.accept_len[b];
  const long long ctx = (long long)seq - n;
  int src = -1, dst = -1;
  if (n > 0 && n <= T && ctx >= 0 && alen > 0 && alen <= n && lane < alen) {
    const int s = a.path[(long long)b * a.path_stride + lane];
    const long long ks = ctx + s, kd = ctx + lane;
    if (s > lane && s < n && ks < a.capacity) {  // (kd < ks)
      const int* const table = a.block_table + (long long)b * a.table_stride;
      const long long bs = a.block_size;
      const long long ss = (long long)table[ks / bs] * bs + ks % bs, sd = (long long)table[kd / bs] * bs + kd % bs;
      if (ss >= 0 && ss < a.n_slots && sd >= 0 && sd < a.n_slots) {
        src = (int)ss;
        dst = (int)sd;
      }
    }
  }
  const unsigned long long moving = __ballot(src >= 0);
  if (moving == 0ull) return;  // nothing of this sequence moves (uniform): no cache is touched
  const int last = 63 - __builtin_clzll(moving);
  const int spare = __shfl(src, last, 64);  // a slot inside the cache

  unsigned char* const cache = a.caches[blockIdx.y] + (unsigned long long)(unsigned)h * a.head_bytes;
  const int sub = lane / M::LPR;                        // this lane's row of a pass
  const unsigned at = (unsigned)(lane % M::LPR) * VEC;  // ... and its first byte of the row
  // Chunks of CH passes: the loads of a chunk, then its stores.  With 16-byte accesses the whole sequence is ONE chunk.  The narrow
  // accesses of odd alignments take up to four chunks, in ASCENDING order of the elements, which keeps the rule: a moving element j
  // has its source behind it (path[b, j] > j), so the row a chunk writes, key C_b + j, is the source of no element above j -- no
  // later chunk reads what an earlier one wrote.
  for (int c = 0; c < M::NCH; ++c)
    compact_passes<ROWB, VEC, 0>(cache, a.slot_bytes, src, dst, spare, c * M::CH * M::RPP, last, sub, at);
}

template <int ROWB, int VEC>
static hipError_t launch_kv_compact_inst(const KvCompactArgs& k, int n_kv_heads, int n_caches, int batch, hipStream_t stream) {
  hipLaunchKernelGGL((sqllm_kv_compact_kernel<ROWB, VEC>), dim3(n_kv_heads, n_caches, batch), dim3(64), 0, stream, k);
  return hipGetLastError();
}

template <int ROWB>
static hipError_t launch_kv_compact_row(const KvCompactArgs& k, int vec, int n_kv_heads, int n_caches, int batch, hipStream_t stream) {
  switch (vec) {
    case 16: return launch_kv_compact_inst<ROWB, 16>(k, n_kv_heads, n_caches, batch, stream);
    case 4: return launch_kv_compact_inst<ROWB, 4>(k, n_kv_heads, n_caches, batch, stream);
    case 2: return launch_kv_compact_inst<ROWB, 2>(k, n_kv_heads, n_caches, batch, stream);
    case 1: if (ROWB <= 128) return launch_kv_compact_inst<(ROWB <= 128 ? ROWB : 128), 1>(k, n_kv_heads, n_caches, batch, stream);  // (bytes: the e4m3fn caches only)
  }
  return hipErrorInvalidValue;
}

// geometry from HOST fields only; what is not served is an error, never another route
static hipError_t launch_kv_compact(const KvCompactArgs& k, int row_bytes, int vec, int n_kv_heads, int n_caches, int batch, hipStream_t stream) {
  switch (row_bytes) {
    case 64: return launch_kv_compact_row<64>(k, vec, n_kv_heads, n_caches, batch, stream);
    case 128: return launch_kv_compact_row<128>(k, vec, n_kv_heads, n_caches, batch, stream);
    case 256: return launch_kv_compact_row<256>(k, vec, n_kv_heads, n_caches, batch, stream);
  }
  return hipErrorInvalidValue;
}

// the host layer reaches the launcher through its hook (sqllm_tree_accept.h), so that it links without this file too
static const bool g_kv_compact_registered = (g_launch_kv_compact = launch_kv_compact, true);

}  // namespace sqllm
