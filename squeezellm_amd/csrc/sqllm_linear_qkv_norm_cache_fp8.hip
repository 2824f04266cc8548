// sqllm_linear_qkv_norm_cache_fp8.hip -- the attention front with its RMSNorm in front, writing k and v straight into a KV
// cache of 1-byte OCP e4m3fn elements, as ONE kernel (include/sqllm_hip.h: sqllm_qkv_rope_norm_cache_fp8_f16 / _bf16):
// sqllm_linear_qkv_norm_cache.hip's kernel, statement for statement, with the finishing policy RopeCacheFp8Finish
// (sqllm_cache_fp8_finish.h; sqllm_linear_qkv_cache_fp8.hip describes it) in the place of RopeCacheFinish.  The cache's
// arguments lie right behind the rotary ones, where cache_fp8_args() reads them; the norm's arguments stay the kernel's LAST
// argument.
#include <stddef.h>

#include "sqllm_cache_fp8_finish.h"
#include "sqllm_fused.h"
#include "sqllm_norm_front.h"

namespace sqllm {

// the kernel's explicit arguments as the ABI lays them out (natural alignment, in order)
struct QkvNormCacheFp8KernArgs {
  const void* x;
  GroupArgs ga;
  RopeArgs ra;
  KvCacheFp8Args fa;
  NormArgs na;
};
static_assert(offsetof(QkvNormCacheFp8KernArgs, ra) == kRopeArgsAt, "rope_args() reads the third argument");
static_assert(offsetof(QkvNormCacheFp8KernArgs, fa) == kKvCacheFp8ArgsAt, "cache_fp8_args() reads the fourth argument");

template <int BITS, int BT, typename OT>
__global__ void __launch_bounds__(kWaves * 64, norm_min_waves(BITS, BT))
sqllm_linear_qkv_norm_cache_fp8_kernel(const void* xv, const GroupArgs ga, const RopeArgs ra /* read through rope_args() */,
                                       const KvCacheFp8Args fa /* read through cache_fp8_args() */, const NormArgs na) {
  constexpr int WAVES = kWaves;
  constexpr bool HALF = fused_half_stages(BITS, BT);
  constexpr int T = WAVES * 64;
  constexpr bool PAIR3 = BITS == 3 && BT == 1 && SQLLM_HALF_STAGES && SQLLM_PAIR3;
  constexpr int kLds = lds_floats(Fmt<BITS>::kLut, WAVES, BT, PAIR3);
  __shared__ __attribute__((aligned(16))) float lds[kLds];
  using XT = OT;
  using AT = u64;
  using FIN = RopeCacheFp8Finish<OT>;
  using VP = RmsVec<XT, BT>;
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
  VP vp;
  vp.g = reinterpret_cast<const XT*>(na.g);
  static_assert(codebook_floats(BITS, PAIR3) >= kTopxLds && codebook_floats(BITS, PAIR3) + WAVES * BT <= kLds, "norm_rows: where the partial sums lie");
  vp.rv = norm_rows<BT>(x, ga.seg[0].gm.K /* (the members share K) */, b0, nb, na.eps, lds + codebook_floats(BITS, PAIR3));

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
    dense_role<BITS, BT, WAVES, 0, XT, HALF, false, FIN, VP>(x, reinterpret_cast<const u32x4*>(sg.q), sg.y, sg.lut, gm.K, gm.N, b0, nb, d,
                                                             gm.col_tiles, gm.units_total, gm.units_per_wg, lds, sg, &sg, fin, vp);
  } else if (sp >= 0 && sp < gm.csr_blocks) {
    if (gm.dense_prio == 2) __builtin_amdgcn_s_setprio(1);
    csr_role<T, BT, XT, AT, false, false, NoGate, kCsrChunk, FIN, VP>(x, reinterpret_cast<AT*>(sg.y), sg.rows, sg.cols, sg.vals, gm.nnz, gm.K, gm.N,
                                                                      b0, nb, sp, lds, &sg, gm.sparse_last >> 1, nullptr, 0, nullptr, NoGate(), fin, vp);
  } else if (sp >= gm.csr_blocks && sp < gm.csr_blocks + gm.topx_blocks) {
    // (never taken when the plan folds the top-X rows into the dense tiles)
    if (gm.dense_prio == 2) __builtin_amdgcn_s_setprio(1);
    topx_role<T, XT, AT, false, NoGate, BT, FIN, VP>(x, reinterpret_cast<AT*>(sg.y), sg.full_rows, sg.full_idx, gm.topX, gm.K, gm.N, b0, nb,
                                                     sp - gm.csr_blocks, lds, NoGate(), vp);
  }
}

struct QkvNormCacheFp8Front : FrontTag {
  template <int BITS, int BT, typename OT>
  static auto kernel() { return sqllm_linear_qkv_norm_cache_fp8_kernel<BITS, BT, OT>; }
};

// q, k and v (segments 0, 1, 2) over one un-normalised 16-bit vec; f.qkv: the rotation; f.kc: the byte cache and its scales; f.vn: the norm's weight and eps
static hipError_t launch_linear_qkv_norm_cache_fp8(int bits, const LaunchArgs& a0, const FrontCall& f, hipStream_t stream) {
  if (!f.qkv || !f.kc || !f.vn) return hipErrorInvalidValue;
  const QkvRope& r = *f.qkv;
  const KvCache& kc = *f.kc;
  const VecNorm& vn = *f.vn;
  if (a0.ga.n_seg != 3 || !r.pair_q || !r.pair_k || !r.cos || !r.sin || !r.positions || r.head_dim < 2 || (r.head_dim & 1) || !vn.weight ||
      !kc.k_cache || !kc.v_cache || !kc.slots || kc.n_slots < 1 || !kc.fp8 || !kc.scales_ok || a0.ga.seg[1].gm.N != a0.ga.seg[2].gm.N ||
      a0.ga.seg[2].gm.N % r.head_dim)
    return hipErrorInvalidValue;
  const LaunchArgs a = without_left_out(a0, kc);
  const NormArgs na = {vn.weight, vn.eps};
  return launch_front<QkvNormCacheFp8Front>(bits, a, stream, make_rope_args(a, r), make_kv_cache_fp8_args(a, r, kc), na);
}

// the host layer reaches the launcher through its slot of g_launch_front (sqllm_kernels.h), so that it links without this file too
static const bool g_qkv_norm_cache_fp8_registered = (g_launch_front[kFrontQkvNormCacheFp8] = launch_linear_qkv_norm_cache_fp8, true);

}  // namespace sqllm
