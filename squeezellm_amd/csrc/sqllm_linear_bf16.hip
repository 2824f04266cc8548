// sqllm_linear_bf16.hip -- the fused linear with bf16 at its two ends (include/sqllm_hip.h: sqllm_linear_bf16):
//
//     out[b, n] = bf16_rne( bias[n] + sum_k W[n, k] * float(x[b, k]) )
//
// The kernel is the fused batch-tile kernel's skeleton (sqllm_fused.h: pick_segment, role dispatch, dense_role with the
// top-X rows folded in, csr_role, topx_role) instantiated with XT = __bf16, AT = the 64-bit completion word: the same
// fixed-point words, returning atomics, sticky flags and self-cleaning workspace as the fp16 linear, the same order of
// additions inside a contribution.  Three things differ, all of them decided at compile time by the activation type:
//   * every read of vec is a 2-byte load widened by a 16-bit shift ((float)__bf16 is exact);
//   * a finite contribution beyond the word's +-2^17 counts as the infinity of its sign instead of being clamped
//     (sqllm_decode.h: FixRange<__bf16> -- a bf16 result of that size is finite, a clamp would return a wrong number);
//   * the finished column is rounded once to bf16 (v_cvt_pk_bf16_f32: the hardware's round-to-nearest-even) and stored.
// A kernel of its own name: the instantiations of sqllm_fused_matvec (sqllm_kernels.hip) stay the 25 they are.
// Route, planner, geometry and workspace are those of the fp16 linear (sqllm_capi.hip: kFusedLinear).
#include "sqllm_fused.h"

namespace sqllm {

template <int BITS, int BT>
__global__ void __launch_bounds__(kWaves * 64, fused_min_waves(BITS, BT, 0))
sqllm_linear_bf16_kernel(const void* xv, const GroupArgs ga) {
  constexpr int WAVES = kWaves;
  constexpr bool HALF = fused_half_stages(BITS, BT);
  constexpr int T = WAVES * 64;
  constexpr int kLds = lds_floats(Fmt<BITS>::kLut, WAVES, BT, BITS == 3 && BT == 1 && SQLLM_HALF_STAGES && SQLLM_PAIR3);
  __shared__ __attribute__((aligned(16))) float lds[kLds];
  using XT = __bf16;
  using AT = u64;
  const XT* x = reinterpret_cast<const XT*>(xv);

  // one round of scalar loads for vec's address, the block table and segment 0 (see sqllm_fused_matvec)
  Segment sg;
  const int bid = pick_segment(ga, x, sg);
  const KernelGeom& gm = sg.gm;
  const int b0 = blockIdx.y * BT;
  int nb = gm.batch - b0;
  if (nb > BT) nb = BT;

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
    dense_role<BITS, BT, WAVES, 0, XT, HALF, false>(x, reinterpret_cast<const u32x4*>(sg.q), sg.y, sg.lut, gm.K, gm.N, b0, nb, d, gm.col_tiles,
                                                    gm.units_total, gm.units_per_wg, lds, sg, &sg);
  } else if (sp >= 0 && sp < gm.csr_blocks) {
    if (gm.dense_prio == 2) __builtin_amdgcn_s_setprio(1);
    csr_role<T, BT, XT, AT>(x, reinterpret_cast<AT*>(sg.y), sg.rows, sg.cols, sg.vals, gm.nnz, gm.K, gm.N, b0, nb, sp, lds, &sg,
                            gm.sparse_last >> 1, nullptr, 0, nullptr);
  } else if (sp >= gm.csr_blocks && sp < gm.csr_blocks + gm.topx_blocks) {
    // (never taken when the plan folds the top-X rows into the dense tiles)
    if (gm.dense_prio == 2) __builtin_amdgcn_s_setprio(1);
    topx_role<T, XT, AT, false, NoGate, BT>(x, reinterpret_cast<AT*>(sg.y), sg.full_rows, sg.full_idx, gm.topX, gm.K, gm.N, b0, nb,
                                            sp - gm.csr_blocks, lds);
  }
}

// (the kernel has no fp16 form: OT is __bf16 whatever the ladder names, and launch_fused hands over launches with a.bf16 only)
struct LinearBf16Front : FrontTag {
  template <int BITS, int BT, typename OT>
  static auto kernel() { return sqllm_linear_bf16_kernel<BITS, BT>; }
};

// 1..kMaxSegments fused linears over one bf16 vec (a.ga): the batch tiles of launch_fused's linear form
hipError_t launch_linear_bf16(int bits, const LaunchArgs& a, hipStream_t stream) {
  if (!a.bf16) return hipErrorInvalidValue;
  return launch_front<LinearBf16Front>(bits, a, stream);
}

}  // namespace sqllm
