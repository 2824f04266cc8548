// sqllm_norm_front.h -- RMSNorm as a PROLOGUE of a fused kernel (include/sqllm_hip.h: sqllm_gated_norm_* / sqllm_qkv_rope_norm_*):
//
//     ms[b]   = (1 / K) * sum_k float(x[b, k])^2
//     r[b]    = 1.0f / sqrtf(ms[b] + eps)
//     xn[b,k] = float(x[b, k]) * float(g[k]) * r[b]           fp32, never rounded to 16 bits
//
// Every workgroup of every role works out r[] for the rows of its own batch tile at entry (norm_rows below) and hands the
// roles a vec policy (sqllm_roles.h: RmsVec) that scales an element where it is loaded.  Nothing is exchanged between
// workgroups: no workspace, no waiting.  vec is L2-resident (every workgroup of the launch reads the same rows).
//
// The order of the sum, the same in every workgroup of every launch (so every column of a row sees the same r[b] bits):
//   * thread t owns elements [kNormVec * t, + kNormVec) of every round of kNormRound elements and adds their squares in
//     ascending k, round after round, into ONE fp32 accumulator starting at zero (a square of a 16-bit value is exact in fp32);
//   * the 64 lanes of a wave meet in wave_sum's butterfly (lane distances 32, 16, 8, 4, 2, 1);
//   * the eight wave sums are added in wave order, starting at zero.
// The sum is then divided by float(K) and eps is added: one correctly rounded division, addition, square root and division.
// A sum that overflows fp32 gives r = 0; where that happens depends on this order.
#pragma once
#include "sqllm_fused.h"

namespace sqllm {

constexpr int kNormVec = 8;                          // elements of a row a thread squares per round (one 16-byte load where vec is 16-byte aligned)
constexpr int kNormRound = kWaves * 64 * kNormVec;   // elements of a row per round of the pass

// Waves per SIMD the norm fronts' register allocation leaves room for: the counterpart's (fused_min_waves), except the 4-bit
// 2-row tile.  Its counterparts sit at 61 (gated) and 64 (q/k/v) of the 64 registers of the four-workgroup step; the norm
// weight's register across the prefetch and r[] put it 4 (gated) to 9 (q/k/v) registers over, which the allocator spilled.
// It takes the three-workgroup step (80 registers) instead: DESIGN.md 4.4.
constexpr int norm_min_waves(int bits, int bt) { return (bits == 4 && bt == 2) ? 6 : fused_min_waves(bits, bt, 0); }

// by-value kernel argument, the last one
struct NormArgs {
  const void* g;  // 16-bit [K] of vec's type
  float eps;
};

// r[] for the BT rows of the tile, lane b of the result holding r[b] in every wave (RmsVec::rv; rows past nb: the last valid
// row's, worked out from that row again -- the same bits).
// `part`: kWaves * BT floats of LDS that no role writes before its own first barrier (the kernels pass the start of the
// dense role's slabs, behind the codebooks: the CSR role stages behind its two counts, the top-X role's sums lie in front).
// Every thread of the workgroup must call it: one barrier.
template <int BT, typename XT>
__device__ __forceinline__ float norm_rows(const XT* x, int K, int b0, int nb, float eps, float* part) {
  static_assert(sizeof(XT) == 2 && kNormVec * sizeof(XT) == sizeof(u32x4), "eight 16-bit elements are one 16-byte load");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // vec itself need not be aligned beyond its elements (the C ABI asks nothing more); K % 32 == 0, so every row is aligned as
  // the first one is and a thread's eight elements lie inside the row or all behind it.  Both branches add in the same order.
  const bool wide = (reinterpret_cast<uintptr_t>(x) & 15u) == 0;
  float ss[BT];
#pragma unroll
  for (int b = 0; b < BT; ++b) ss[b] = 0.f;
  for (int k = kNormVec * tid; k < K; k += kNormRound) {
#pragma unroll
    for (int b = 0; b < BT; ++b) {
      const XT* p = x + (size_t)(b0 + (b < nb ? b : nb - 1)) * K + k;
      u32x4 e;  // eight elements, two per dword, lower address in the lower half
      if (wide) {
        e = *reinterpret_cast<const u32x4*>(p);
      } else {
        const uint16_t* h = reinterpret_cast<const uint16_t*>(p);
        e = u32x4{h[0] | (uint32_t)h[1] << 16, h[2] | (uint32_t)h[3] << 16, h[4] | (uint32_t)h[5] << 16, h[6] | (uint32_t)h[7] << 16};
      }
      const uint32_t d[4] = {e.x, e.y, e.z, e.w};
#pragma unroll
      for (int j = 0; j < kNormVec; ++j) {
        const float v = (float)__builtin_bit_cast(XT, (uint16_t)(d[j >> 1] >> (16 * (j & 1))));
        ss[b] = __builtin_fmaf(v, v, ss[b]);
      }
    }
  }
#pragma unroll
  for (int b = 0; b < BT; ++b) ss[b] = wave_sum(ss[b]);
  if (lane == 0) {
#pragma unroll
    for (int b = 0; b < BT; ++b) part[wave * BT + b] = ss[b];
  }
  __syncthreads();
  // lane b sums row b's eight wave sums in wave order (lanes past the tile: its last row again)
  const int bl = lane < BT ? lane : BT - 1;
  float s = 0.f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) s += part[w * BT + bl];
  const float ms = s / (float)K;
  const float r = 1.0f / sqrtf(ms + eps);
  // (one row: the same value in every lane -- said out loud, it is a scalar register and the role's v_readlane folds away)
  if constexpr (BT == 1) return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, r)));
  return r;
}

}  // namespace sqllm
