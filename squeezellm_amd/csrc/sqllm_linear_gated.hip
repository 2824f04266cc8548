// sqllm_linear_gated.hip -- the gated front of an MLP as ONE kernel (include/sqllm_hip.h: sqllm_gated_f16 / _bf16):
//
//     g = bias_gate[n] + sum_k Wg[n, k] * float(x[b, k])
//     u = bias_up[n]   + sum_k Wu[n, k] * float(x[b, k])
//     out[b, n] = OT( (g / (1 + exp(-g))) * u )          fp32 throughout, rounded once to OT = the type of x (fp16 or bf16)
//
// The kernel is sqllm_linear_bf16_kernel's skeleton (pick_segment, role dispatch, dense_role with the top-X rows folded in,
// csr_role, topx_role, AT = the 64-bit completion word) launched on a group of exactly two segments, segment 0 = gate and
// segment 1 = up: route, planner, geometry and validation are kFusedLinear's two-op group.  Two things are its own, both
// carried by the finishing policy the roles are instantiated with (PairFinish, sqllm_pair_finish.h; sqllm_decode.h: ColumnStore is the default):
//   * the range rule is the bf16 one for BOTH output types (FixRange<__bf16>: a finite contribution beyond +-2^17 sets the
//     infinity flag of its sign and adds nothing).  The fp16 linear clamps there because such an fp16 result is not finite
//     anyway; here g = 200000, u = 0.05 has a finite fp16 product and a clamp would return a wrong finite number;
//   * the finisher of a member's column does not store.  It forms its fp32 value (flags applied, bias added), re-zeroes its
//     accumulator word, and does ONE returning 64-bit exchange on the PAIR WORD of (b, n) -- a third plane of the workspace,
//     all zero between launches -- depositing kPairTag | bits(v) (the tag, bit 32, tells a deposited 0.0f from an empty
//     word).  An old value of zero: it is the first of the two and leaves.  Otherwise the old value is the other member's
//     result: it computes silu(g) * u (which of the two is g follows from its own segment index), stores OT and exchanges
//     the pair word back to zero.
// Both values travel INSIDE returning agent-scope atomics on one address, so there is no fence (sqllm_decode.h: an
// agent-scope release/acquire pair per workgroup measured +4.5 us per launch), no workgroup waits for another -- no spin, no
// polling, no launch-wide counter: whoever arrives second finishes -- and the result is a function of the operands alone:
// the integer sums commute and the last step sees the same two fp32 values whichever member finishes first.
#include "sqllm_fused.h"
#include "sqllm_pair_finish.h"

namespace sqllm {

template <int BITS, int BT, typename OT>
__global__ void __launch_bounds__(kWaves * 64, fused_min_waves(BITS, BT, 0))
sqllm_linear_gated_kernel(const void* xv, const GroupArgs ga, u64* pair) {
  constexpr int WAVES = kWaves;
  constexpr bool HALF = fused_half_stages(BITS, BT);
  constexpr int T = WAVES * 64;
  constexpr int kLds = lds_floats(Fmt<BITS>::kLut, WAVES, BT, BITS == 3 && BT == 1 && SQLLM_HALF_STAGES && SQLLM_PAIR3);
  __shared__ __attribute__((aligned(16))) float lds[kLds];
  using XT = OT;
  using AT = u64;
  using FIN = PairFinish<OT>;
  const XT* x = reinterpret_cast<const XT*>(xv);

  // one round of scalar loads for vec's address, the block table and segment 0 (see sqllm_fused_matvec)
  Segment sg;
  const int bid = pick_segment(ga, x, sg);
  const KernelGeom& gm = sg.gm;
  const int b0 = blockIdx.y * BT;
  int nb = gm.batch - b0;
  if (nb > BT) nb = BT;
  const FIN fin{pair, (int)blockIdx.x >= ga.block0[1] ? 1 : 0};  // (two segments: the host launches nothing else here)

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

struct GatedFront : FrontTag {
  template <int BITS, int BT, typename OT>
  static auto kernel() { return sqllm_linear_gated_kernel<BITS, BT, OT>; }
  using FrontTag::arg;
  template <typename OT> static u64* arg(void* const& pair) { return static_cast<u64*>(pair); }
};

// gate (segment 0) and up (segment 1) over one 16-bit vec (a.ga; a.bf16: its type), f.pair: the pair plane
static hipError_t launch_linear_gated(int bits, const LaunchArgs& a, const FrontCall& f, hipStream_t stream) {
  if (a.ga.n_seg != 2 || !f.pair) return hipErrorInvalidValue;
  return launch_front<GatedFront>(bits, a, stream, f.pair);
}

// the host layer reaches the launcher through its slot of g_launch_front (sqllm_kernels.h), so that it links without this file too
static const bool g_gated_registered = (g_launch_front[kFrontGated] = launch_linear_gated, true);

}  // namespace sqllm
