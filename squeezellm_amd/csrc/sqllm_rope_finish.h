// sqllm_rope_finish.h -- the finishing policy of the attention front and the kernel arguments it reads (sqllm_linear_qkv.hip
// describes the scheme; its kernels and those of sqllm_linear_qkv_norm.hip are instantiated with it).
#pragma once
#include <stddef.h>

#include "sqllm_fused.h"
#include "sqllm_pair_finish.h"  // kPairTag

namespace sqllm {

// by-value kernel argument behind GroupArgs; read through rope_args() only
struct RopeArgs {
  u64* pair_q;           // [batch, N_q / 2] pair words, all zero between launches
  u64* pair_k;           // [batch, N_k / 2]
  const float* cos;      // fp32 [n_pos, D / 2]
  const float* sin;
  const int* positions;  // int32 [batch]
  int n_pos;
  int half;              // D / 2
  uint32_t d_magic;      // floor(2^32 / D) + 1: c / D == mulhi(c, d_magic) for c * D < 2^32 (the host checks N * D)
  int interleaved;       // 0: partner D / 2 away, 1: partner next door
  float inv_nq, inv_nk;  // 1 / N of the member, fp32
};
// where the kernel's third argument lies in the kernel-argument segment: right behind vec's pointer and the descriptor block (each
// kernel file checks it against a mirror struct of its own arguments)
constexpr unsigned kRopeArgsAt = sizeof(void*) + sizeof(GroupArgs);
static_assert(sizeof(RopeArgs) == 64, "the descriptor block ends on the next argument's alignment");

// The rotary arguments, from the kernel-argument segment, no earlier than HERE: the empty asm statement hides where the
// address came from, so the scalar loads through it cannot be scheduled at the kernel's start and held across the walk.
// (The cast back names the constant address space: the loads stay scalar.)
__device__ __forceinline__ const __attribute__((address_space(4))) RopeArgs* rope_args() {
  uintptr_t p = reinterpret_cast<uintptr_t>(__builtin_amdgcn_kernarg_segment_ptr()) + kRopeArgsAt;
  asm volatile("" : "+s"(p));
  return reinterpret_cast<const __attribute__((address_space(4))) RopeArgs*>(p);
}

// Column c of a rotated member: the pair's slot in a row of the pair plane, h * D / 2 + j; *is_hi: c is the pair's upper
// column; *j: the table column; *dist: how far apart the two columns are.  No division: c / D is a multiply-high.
__device__ __forceinline__ uint32_t locate(const __attribute__((address_space(4))) RopeArgs* ra, int c, bool* is_hi, int* j, int* dist) {
  const int half = ra->half;
  const uint32_t h = __umulhi((uint32_t)c, ra->d_magic);
  const int r = c - (int)h * 2 * half;  // c % D
  if (ra->interleaved) {
    *is_hi = c & 1;
    *j = r >> 1;
    *dist = 1;
  } else {
    *is_hi = r >= half;
    *j = *is_hi ? r - half : r;
    *dist = half;
  }
  return h * (uint32_t)half + (uint32_t)*j;
}

// OT: the element type of the outputs; the contributions follow FixRange<__bf16> whatever OT is
template <typename OT>
struct RopeFinish {
  int member;  // this workgroup's segment: 0 = q, 1 = k, 2 = v
  static constexpr bool kOrderedCsr = true;  // a CSR chunk's parts of a row meet in wave order: the same fp32 value in every run
  template <typename XT> struct Range { using type = __bf16; };
  template <typename RT>
  __device__ __forceinline__ void done(const Segment& sg, u64* word, u64 total, unsigned target, size_t at, int c) const {
    float v;
    if (!column_value(sg, total, target, c, &v)) return;
    atomicExch(word, 0ull);  // result unused: a plain atomic store
    OT* out = reinterpret_cast<OT*>(sg.out16);
    if (member == 2) {
      out[at] = (OT)v;
      return;
    }
    const auto* ra = rope_args();
    bool is_hi;
    int j, dist;
    const uint32_t bn = (uint32_t)(at - (size_t)c);  // b * N (N is even)
    u64* pw = (member ? ra->pair_k : ra->pair_q) + ((bn >> 1) + locate(ra, c, &is_hi, &j, &dist));
    const u64 mine = kPairTag | (u64)__builtin_bit_cast(uint32_t, v);
    const u64 other = __hip_atomic_exchange(SQLLM_GLOBAL(u64, pw), mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (other == 0) return;  // the first of the two: the partner column's finisher completes the pair
    const float o = __builtin_bit_cast(float, (uint32_t)other);
    // (located a second time, from a copy of c the compiler cannot see through: four VALU instructions in the one finisher
    // of a pair instead of three registers held by every finisher across its exchange)
    int c2 = c;
    asm volatile("" : "+v"(c2));
    locate(ra, c2, &is_hi, &j, &dist);
    const float lo = is_hi ? o : v, hi = is_hi ? v : o;
    const int b = (int)((float)bn * (member ? ra->inv_nk : ra->inv_nq) + 0.5f);
    const int p = ra->positions[b];
    float cs = __builtin_nanf(""), sn = cs;  // a position outside the tables: NaN, and nothing is read
    if ((unsigned)p < (unsigned)ra->n_pos) {
      const size_t t = (size_t)p * ra->half + j;
      cs = ra->cos[t];
      sn = ra->sin[t];
    }
    const size_t at_lo = is_hi ? at - dist : at;
    out[at_lo] = (OT)(lo * cs - hi * sn);
    out[at_lo + dist] = (OT)(hi * cs + lo * sn);
    __hip_atomic_exchange(SQLLM_GLOBAL(u64, pw), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (result unused)
  }
};

// the kernel argument from the host's description of the rotation (the launchers have checked r)
inline RopeArgs make_rope_args(const LaunchArgs& a, const QkvRope& r) {
  RopeArgs ra;
  ra.pair_q = static_cast<u64*>(r.pair_q);
  ra.pair_k = static_cast<u64*>(r.pair_k);
  ra.cos = r.cos;
  ra.sin = r.sin;
  ra.positions = r.positions;
  ra.n_pos = r.n_pos;
  ra.half = r.head_dim / 2;
  ra.d_magic = (uint32_t)((1ull << 32) / (uint32_t)r.head_dim) + 1u;
  ra.interleaved = r.interleaved ? 1 : 0;
  ra.inv_nq = 1.f / (float)a.ga.seg[0].gm.N;
  ra.inv_nk = 1.f / (float)a.ga.seg[1].gm.N;
  return ra;
}

}  // namespace sqllm
