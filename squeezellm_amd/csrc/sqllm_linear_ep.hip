// sqllm_linear_ep.hip -- the fused linear with an epilogue (include/sqllm_hip.h: sqllm_linear_ep_f16 / _bf16):
//
//     out[b, n] = OT( act(bias[n] + sum_k W[n, k] * float(x[b, k])) + float(residual[b, n]) )
//
// fp32 throughout, rounded once to OT = the type of x (fp16 or bf16).  The kernel is sqllm_linear_bf16_kernel's skeleton
// (pick_segment, role dispatch, dense_role with the top-X rows folded in, csr_role, topx_role, AT = the 64-bit completion
// word) launched on ONE segment: route, planner, geometry, validation and workspace are kFusedLinear's single-op launch.
// What is its own is carried by the finishing policy the roles are instantiated with (EpilogueFinish below; sqllm_decode.h:
// ColumnStore is the default, sqllm_linear_gated.hip: PairFinish the other one):
//   * the range rule is the bf16 one for BOTH output types (FixRange<__bf16>: a finite contribution beyond +-2^17 sets the
//     infinity flag of its sign and adds nothing).  The fp16 linear clamps there because such an fp16 result is not finite
//     anyway; here a contribution of 200000 meets a residual of -180000 and a clamp would return a wrong finite number;
//   * the finisher of a column -- the one thread that holds its final fp32 value -- re-zeroes the accumulator word, applies
//     the activation, adds its residual element and stores.  No new synchronisation, no new workspace: the residual element
//     is read and the output element written by that thread alone, so the residual may BE the output buffer.
// The CSR adds of a long row stay in arrival order (kOrderedCsr = false), as in the linears: the chunk span limit is the
// linears' kCsrSpanMax.  The activation code is a run-time kernel argument: the branch on it is uniform over the launch and
// only finishing lanes reach it (a template parameter would make 80 kernels of these 16).
#include "sqllm_fused.h"

namespace sqllm {

// the codes of include/sqllm_hip.h (SQLLM_ACT_*)
constexpr int kActSilu = 0, kActIdentity = 1, kActRelu = 2, kActGelu = 3, kActGeluTanh = 4;

// OT: the element type of `out` and `residual`; the contributions follow FixRange<__bf16> whatever OT is
template <typename OT>
struct EpilogueFinish {
  const OT* residual;  // [batch, N] or null; may be the output itself
  int act;             // kAct*
  static constexpr bool kOrderedCsr = false;
  template <typename XT> struct Range { using type = __bf16; };
  template <typename RT>
  __device__ __forceinline__ void done(const Segment& sg, u64* word, u64 total, unsigned target, size_t at, int c) const {
    float v;
    if (!column_value(sg, total, target, c, &v)) return;
    atomicExch(word, 0ull);  // result unused: a plain atomic store
    // the formulas of the header's table, in fp32 as written there (their values at +-inf and NaN are the specification)
    switch (act) {
      case kActRelu: v = v > 0.f ? v : (v != v ? v : 0.f); break;  // (not fmaxf: it drops a NaN)
      case kActSilu: v = v / (1.f + expf(-v)); break;
      case kActGelu: v = 0.5f * v * (1.f + erff(v * 0.70710678f)); break;
      case kActGeluTanh: v = 0.5f * v * (1.f + tanhf(0.79788456f * (v + 0.044715f * v * v * v))); break;
      default: break;  // kActIdentity (the host admits nothing else)
    }
    if (residual) v += (float)residual[at];
    reinterpret_cast<OT*>(sg.out16)[at] = (OT)v;
  }
};

template <int BITS, int BT, typename OT>
__global__ void __launch_bounds__(kWaves * 64, fused_min_waves(BITS, BT, 0))
sqllm_linear_ep_kernel(const void* xv, const GroupArgs ga, const OT* residual, int act) {
  constexpr int WAVES = kWaves;
  constexpr bool HALF = fused_half_stages(BITS, BT);
  constexpr int T = WAVES * 64;
  constexpr int kLds = lds_floats(Fmt<BITS>::kLut, WAVES, BT, BITS == 3 && BT == 1 && SQLLM_HALF_STAGES && SQLLM_PAIR3);
  __shared__ __attribute__((aligned(16))) float lds[kLds];
  using XT = OT;
  using AT = u64;
  using FIN = EpilogueFinish<OT>;
  const XT* x = reinterpret_cast<const XT*>(xv);

  // one round of scalar loads for vec's address, the block table and segment 0 (see sqllm_fused_matvec)
  Segment sg;
  const int bid = pick_segment(ga, x, sg);
  const KernelGeom& gm = sg.gm;
  const int b0 = blockIdx.y * BT;
  int nb = gm.batch - b0;
  if (nb > BT) nb = BT;
  const FIN fin{residual, act};

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

struct EpFront : FrontTag {
  template <int BITS, int BT, typename OT>
  static auto kernel() { return sqllm_linear_ep_kernel<BITS, BT, OT>; }
  using FrontTag::arg;
  template <typename OT> static const OT* arg(const void* const& residual) { return static_cast<const OT*>(residual); }
};

// one fused linear over a 16-bit vec (a.ga; a.bf16: its type), finished by act and the optional residual
static hipError_t launch_linear_ep(int bits, const LaunchArgs& a, const FrontCall& f, hipStream_t stream) {
  if (a.ga.n_seg != 1 || f.act < kActSilu || f.act > kActGeluTanh) return hipErrorInvalidValue;
  return launch_front<EpFront>(bits, a, stream, f.residual, f.act);
}

// the host layer reaches the launcher through its slot of g_launch_front (sqllm_kernels.h), so that it links without this file too
static const bool g_ep_registered = (g_launch_front[kFrontEp] = launch_linear_ep, true);

}  // namespace sqllm
