// sqllm_linear_qkv.hip -- the attention front as ONE kernel (include/sqllm_hip.h: sqllm_qkv_rope_f16 / _bf16):
//
//     s_m[b, n]  = bias_m[n] + sum_k W_m[n, k] * float(x[b, k])                   m in {q, k, v}
//     out_v[b, n] = OT( s_v[b, n] )
//     for m in {q, k}, head h, j in [0, D/2), p = positions[b], (lo, hi) = the pair's two columns of s_m[b, :]:
//         out_m[b, col_lo] = OT( lo * cos[p, j] - hi * sin[p, j] )
//         out_m[b, col_hi] = OT( hi * cos[p, j] + lo * sin[p, j] )
//
// fp32 throughout, rounded once to OT = the type of x (fp16 or bf16).  The kernel is sqllm_linear_gated.hip's skeleton
// (pick_segment, role dispatch, dense_role with the top-X rows folded in, csr_role, topx_role, AT = the 64-bit completion
// word) launched on a group of exactly three segments, q, k and v: route, planner, geometry and validation are
// kFusedLinear's three-op group.  What is its own is carried by the finishing policy (RopeFinish, sqllm_rope_finish.h):
//   * the range rule is the bf16 one for BOTH output types (a value beyond +-2^17 can rotate to a finite fp16 result);
//   * the finisher of a column of v stores, as the epilogue kernel's identity does.  The finisher of a column of q or k
//     forms its fp32 value, re-zeroes its accumulator word, and does ONE returning 64-bit exchange on the PAIR WORD of
//     (b, h, j) -- a plane of [batch, N / 2] words per rotated member behind the accumulator planes, all zero between
//     launches -- depositing kPairTag | bits(v).  An old value of zero: it is the first of the two and leaves.  Otherwise
//     the old value is its partner column's result: it reads positions[b] and the two table entries, computes BOTH
//     outputs, stores both and exchanges the pair word back to zero.
// Gated pairs a column with the same column of the other member; rotary pairs it with another column of the same member:
// the two finishers may be lanes of one wave (the interleaved layout, or D / 2 < 64) or workgroups apart.  Either way both
// values travel inside returning agent-scope atomics on one address: no fence, nobody waits, and the rotation sees the
// same two fp32 values whichever column finishes first.
//
// Registers.  Everything the rotation needs beyond the member index -- the pair planes, the tables, positions, the
// divisors -- stays in the kernel-argument segment until a finisher asks for it (rope_args): held in SGPRs from the
// kernel's start, those 20 dwords pushed the 2-row and 8-row tiles past their VGPR steps through SGPR parking.  And a
// finisher divides nothing: c / D is a multiply-high by a reciprocal the host supplies, the batch row comes back out of
// at - c = b * N by an fp32 multiply (exact for the sizes the host admits), so the tail unrolled once per batch row of a
// tile is a dozen instructions.
#include <stddef.h>

#include "sqllm_fused.h"
#include "sqllm_rope_finish.h"

namespace sqllm {

// the kernel's explicit arguments as the ABI lays them out (natural alignment, in order)
struct QkvKernArgs {
  const void* x;
  GroupArgs ga;
  RopeArgs ra;
};
constexpr unsigned kRopeArgsOffset = offsetof(QkvKernArgs, ra);
static_assert(kRopeArgsOffset == sizeof(void*) + sizeof(GroupArgs) && sizeof(RopeArgs) == 64, "the descriptor block ends on the next argument's alignment");
static_assert(kRopeArgsOffset == kRopeArgsAt, "rope_args() reads the third argument");

template <int BITS, int BT, typename OT>
__global__ void __launch_bounds__(kWaves * 64, fused_min_waves(BITS, BT, 0))
sqllm_linear_qkv_kernel(const void* xv, const GroupArgs ga, const RopeArgs ra /* read through rope_args() */) {
  constexpr int WAVES = kWaves;
  constexpr bool HALF = fused_half_stages(BITS, BT);
  constexpr int T = WAVES * 64;
  constexpr int kLds = lds_floats(Fmt<BITS>::kLut, WAVES, BT, BITS == 3 && BT == 1 && SQLLM_HALF_STAGES && SQLLM_PAIR3);
  __shared__ __attribute__((aligned(16))) float lds[kLds];
  using XT = OT;
  using AT = u64;
  using FIN = RopeFinish<OT>;
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

struct QkvFront : FrontTag {
  template <int BITS, int BT, typename OT>
  static auto kernel() { return sqllm_linear_qkv_kernel<BITS, BT, OT>; }
};

// q, k and v (segments 0, 1, 2) over one 16-bit vec (a.ga; a.bf16: its type); f.qkv: the host's description of the rotation
static hipError_t launch_linear_qkv(int bits, const LaunchArgs& a, const FrontCall& f, hipStream_t stream) {
  if (!f.qkv) return hipErrorInvalidValue;
  const QkvRope& r = *f.qkv;
  if (a.ga.n_seg != 3 || !r.pair_q || !r.pair_k || !r.cos || !r.sin || !r.positions || r.head_dim < 2 || (r.head_dim & 1))
    return hipErrorInvalidValue;
  return launch_front<QkvFront>(bits, a, stream, make_rope_args(a, r));
}

// the host layer reaches the launcher through its slot of g_launch_front (sqllm_kernels.h), so that it links without this file too
static const bool g_qkv_registered = (g_launch_front[kFrontQkv] = launch_linear_qkv, true);

}  // namespace sqllm
