// sqllm_pair_finish.h -- the finishing policy of the gated pair (sqllm_linear_gated.hip describes the scheme; its kernels and
// those of sqllm_linear_gated_norm.hip are instantiated with it).
#pragma once
#include "sqllm_fused.h"

namespace sqllm {

constexpr u64 kPairTag = 1ull << 32;  // a deposited value is never the empty word, whatever its bits

// OT: the element type of `out` (the store); the contributions follow FixRange<__bf16> whatever OT is
template <typename OT>
struct PairFinish {
  u64* pair;   // [batch, N] pair words, all zero between launches
  int member;  // this workgroup's segment: 0 = gate, 1 = up
  static constexpr bool kOrderedCsr = true;  // a CSR chunk's parts of a row meet in wave order: the same fp32 value in every run
  template <typename XT> struct Range { using type = __bf16; };
  template <typename RT>
  __device__ __forceinline__ void done(const Segment& sg, u64* word, u64 total, unsigned target, size_t at, int c) const {
    float v;
    if (!column_value(sg, total, target, c, &v)) return;
    atomicExch(word, 0ull);  // result unused: a plain atomic store
    const u64 mine = kPairTag | (u64)__builtin_bit_cast(uint32_t, v);
    const u64 other = __hip_atomic_exchange(SQLLM_GLOBAL(u64, pair + at), mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (other == 0) return;  // the first of the two: the other member's finisher completes the pair
    const float o = __builtin_bit_cast(float, (uint32_t)other);
    const float g = member ? o : v, u = member ? v : o;
    reinterpret_cast<OT*>(sg.out16)[at] = (OT)((g / (1.f + expf(-g))) * u);
    __hip_atomic_exchange(SQLLM_GLOBAL(u64, pair + at), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (result unused)
  }
};

}  // namespace sqllm
