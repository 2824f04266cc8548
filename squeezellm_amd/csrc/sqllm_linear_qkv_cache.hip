// sqllm_linear_qkv_cache.hip -- the attention front that writes k and v straight into the KV cache, as ONE kernel
// (include/sqllm_hip.h: sqllm_qkv_rope_cache_f16 / _bf16): sqllm_linear_qkv.hip's kernel, statement for statement, with the
// finishing policy RopeCacheFinish (sqllm_cache_finish.h) in the place of RopeFinish.  For row b, s = slots[b], column
// n = h * D + d of member k (resp. v):
//
//     k_cache[s * slot_stride + h * head_stride + d] = the 16 bits out_k[b, n] receives          0 <= s < n_slots
//
// and nothing of row b when s is outside that range.  out_k / out_v may be absent (a null out16 in their segments): the
// cache is then the member's only destination.  q is finished exactly as in the parent.
//
// The values, the walk, the pair exchange and the rotation are the parent's: a finisher of v stores its element a second
// time; the one finisher of a pair of k that completes it stores both elements a second time (both columns of a pair lie
// in one head, so they are the same distance apart in the cache).  The cache's arguments lie behind the rotary ones in the
// kernel-argument segment and are read there by the finisher that needs them (cache_args), for the parent's reason: held
// in SGPRs from the kernel's start they would cost the tiles their VGPR steps.
#include <stddef.h>

#include "sqllm_cache_finish.h"
#include "sqllm_fused.h"

namespace sqllm {

// the kernel's explicit arguments as the ABI lays them out (natural alignment, in order)
struct QkvCacheKernArgs {
  const void* x;
  GroupArgs ga;
  RopeArgs ra;
  KvCacheArgs ca;
};
constexpr unsigned kKvCacheArgsOffset = offsetof(QkvCacheKernArgs, ca);
static_assert(offsetof(QkvCacheKernArgs, ra) == kRopeArgsAt, "rope_args() reads the third argument");
static_assert(kKvCacheArgsOffset == kKvCacheArgsAt, "cache_args() reads the fourth argument");

template <int BITS, int BT, typename OT>
__global__ void __launch_bounds__(kWaves * 64, fused_min_waves(BITS, BT, 0))
sqllm_linear_qkv_cache_kernel(const void* xv, const GroupArgs ga, const RopeArgs ra /* read through rope_args() */,
                              const KvCacheArgs ca /* read through cache_args() */) {
  constexpr int WAVES = kWaves;
  constexpr bool HALF = fused_half_stages(BITS, BT);
  constexpr int T = WAVES * 64;
  constexpr int kLds = lds_floats(Fmt<BITS>::kLut, WAVES, BT, BITS == 3 && BT == 1 && SQLLM_HALF_STAGES && SQLLM_PAIR3);
  __shared__ __attribute__((aligned(16))) float lds[kLds];
  using XT = OT;
  using AT = u64;
  using FIN = RopeCacheFinish<OT>;
  const XT* x = reinterpret_cast<const XT*>(xv);

  // one round of scalar loads for vec's address, the block table and segment 0 (see sqllm_fused_matvec)
  Segment sg;
  const int bid = pick_segment(ga, x, sg);
  const KernelGeom& gm = sg.gm;
  const int b0 = blockIdx.y * BT;
  int nb = gm.batch - b0;
  if (nb > BT) nb = BT;
  // (three segments: the host launches nothing else here)
  const FIN fin{(int)blockIdx.x >= ga.block0[2] ? 2 : (int)blockIdx.x >= ga.block0[1] ? 1 : 0};

  // role by block id within the segment: [sparse | pad | dense] or, with sparse_last, [dense | sparse]
  int d, sp;
  if (gm.sparse_last & 1) {
    d = bid;
    sp = bid - gm.dense_blocks;
  } else {
    d = bid - gm.dense_block0;
    sp = bid < gm.dense_block0 ? bid : -1;
  }
  if (d >= 0 && d < gm.dense_blocks) {
    dense_role<BITS, BT, WAVES, 0, XT, HALF, false, FIN>(x, reinterpret_cast<const u32x4*>(sg.q), sg.y, sg.lut, gm.K, gm.N, b0, nb, d,
                                                         gm.col_tiles, gm.units_total, gm.units_per_wg, lds, sg, &sg, fin);
  } else if (sp >= 0 && sp < gm.csr_blocks) {
    if (gm.dense_prio == 2) __builtin_amdgcn_s_setprio(1);
    csr_role<T, BT, XT, AT, false, false, NoGate, kCsrChunk, FIN>(x, reinterpret_cast<AT*>(sg.y), sg.rows, sg.cols, sg.vals, gm.nnz, gm.K, gm.N,
                                                                  b0, nb, sp, lds, &sg, gm.sparse_last >> 1, nullptr, 0, nullptr, NoGate(), fin);
  } else if (sp >= gm.csr_blocks && sp < gm.csr_blocks + gm.topx_blocks) {
    // (never taken when the plan folds the top-X rows into the dense tiles)
    if (gm.dense_prio == 2) __builtin_amdgcn_s_setprio(1);
    topx_role<T, XT, AT, false, NoGate, BT, FIN>(x, reinterpret_cast<AT*>(sg.y), sg.full_rows, sg.full_idx, gm.topX, gm.K, gm.N, b0, nb,
                                                 sp - gm.csr_blocks, lds);
  }
}

struct QkvCacheFront : FrontTag {
  template <int BITS, int BT, typename OT>
  static auto kernel() { return sqllm_linear_qkv_cache_kernel<BITS, BT, OT>; }
};

// q, k and v (segments 0, 1, 2) over one 16-bit vec (a0.ga; a0.bf16: its type); f.qkv: the rotation; f.kc: the cache
static hipError_t launch_linear_qkv_cache(int bits, const LaunchArgs& a0, const FrontCall& f, hipStream_t stream) {
  if (!f.qkv || !f.kc) return hipErrorInvalidValue;
  const QkvRope& r = *f.qkv;
  const KvCache& kc = *f.kc;
  if (a0.ga.n_seg != 3 || !r.pair_q || !r.pair_k || !r.cos || !r.sin || !r.positions || r.head_dim < 2 || (r.head_dim & 1) || !kc.k_cache ||
      !kc.v_cache || !kc.slots || kc.n_slots < 1 || a0.ga.seg[1].gm.N != a0.ga.seg[2].gm.N || a0.ga.seg[2].gm.N % r.head_dim)
    return hipErrorInvalidValue;
  const LaunchArgs a = without_left_out(a0, kc);
  return launch_front<QkvCacheFront>(bits, a, stream, make_rope_args(a, r), make_kv_cache_args(a, r, kc));
}

// the host layer reaches the launcher through its slot of g_launch_front (sqllm_kernels.h), so that it links without this file too
static const bool g_qkv_cache_registered = (g_launch_front[kFrontQkvCache] = launch_linear_qkv_cache, true);

}  // namespace sqllm
