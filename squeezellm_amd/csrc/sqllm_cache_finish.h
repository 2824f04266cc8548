// sqllm_cache_finish.h -- the attention front's finishing policy that also writes k and v into a KV cache, and the kernel
// argument it reads (sqllm_linear_qkv_cache.hip describes the scheme; its kernels and those of
// sqllm_linear_qkv_norm_cache.hip are instantiated with it).  RopeFinish (sqllm_rope_finish.h) with one more destination:
// the walk, the pair exchange, the rotation and the one rounding are the parent's.
#pragma once
#include <stddef.h>

#include "sqllm_rope_finish.h"

namespace sqllm {

// by-value kernel argument behind RopeArgs; read through cache_args() only
struct KvCacheArgs {
  void* k_cache;         // 16-bit elements of the outputs' type
  void* v_cache;
  const int* slots;      // int32 [batch]
  uint32_t slot_stride;  // elements between consecutive slots (below 2^32: the host checks it; the OFFSETS are 64-bit)
  uint32_t head_skip;    // elements between the end of one kv head of a slot and the start of the next: head_stride - D
  uint32_t n_slots;      // slots[b] outside [0, n_slots): row b writes nothing to either cache
  float inv_nv;          // 1 / N_v, fp32 (N_v == N_k: the host checks it)
};
// where the kernel's fourth argument lies in the kernel-argument segment: right behind the rotary arguments (each kernel
// file checks it against a mirror struct of its own arguments)
constexpr unsigned kKvCacheArgsAt = kRopeArgsAt + sizeof(RopeArgs);
static_assert(sizeof(KvCacheArgs) == 40 && kKvCacheArgsAt % alignof(KvCacheArgs) == 0, "the rotary arguments end on this argument's alignment");

// The cache arguments, from the kernel-argument segment, through the pointer rope_args() returned: no earlier than the
// rotary arguments, for the same reason, and at constant offsets from the SAME base register pair -- an address of their
// own, formed at the kernel's start and held across the walk, is one more pair of SGPRs parked in a VGPR lane.
__device__ __forceinline__ const __attribute__((address_space(4))) KvCacheArgs* cache_args(const __attribute__((address_space(4))) RopeArgs* ra) {
  static_assert(kKvCacheArgsAt - kRopeArgsAt == sizeof(RopeArgs), "directly behind the rotary arguments");
  return reinterpret_cast<const __attribute__((address_space(4))) KvCacheArgs*>(ra + 1);
}

// Where column c of slot s of a cached member goes: base + s * slot_stride + (c / D) * head_stride + c % D, a 64-bit element
// offset out of two 32 x 32 -> 64-bit multiply-adds (strides of 64 bits cost the 4-bit 2-row tile two registers it does not
// have).  c % D is never formed: (c / D) * head_stride + c % D == (c / D) * (head_stride - D) + c, and the host supplies
// head_skip.  The caller has checked s.
template <typename OT>
__device__ __forceinline__ OT* cache_at(const __attribute__((address_space(4))) KvCacheArgs* ca, const __attribute__((address_space(4))) RopeArgs* ra,
                                        void* base, uint32_t s, uint32_t c) {
  const uint32_t h = __umulhi(c, ra->d_magic);
  return reinterpret_cast<OT*>(base) + (int64_t)((uint64_t)s * ca->slot_stride + (uint64_t)h * ca->head_skip + c);
}

// OT: the element type of the outputs and of the caches; the contributions follow FixRange<__bf16> whatever OT is
template <typename OT>
struct RopeCacheFinish {
  int member;  // this workgroup's segment: 0 = q, 1 = k, 2 = v
  static constexpr bool kOrderedCsr = true;  // a CSR chunk's parts of a row meet in wave order: the same fp32 value in every run
  template <typename XT> struct Range { using type = __bf16; };
  template <typename RT>
  __device__ __forceinline__ void done(const Segment& sg, u64* word, u64 total, unsigned target, size_t at, int c) const {
    float v;
    if (!column_value(sg, total, target, c, &v)) return;
    atomicExch(word, 0ull);  // result unused: a plain atomic store
    // null for k or v: only the cache receives that member.  (Through an empty asm statement: whether it is null is then
    // found out here, not at the kernel's start with the answer held in an SGPR pair across the walk.)
    // (A measurement build keeps the pointer in VGPRs, where the statement's scalar operand is not to be had: it does
    // without, and its kernels' register counts are nobody's yardstick.)
    uintptr_t out_at = reinterpret_cast<uintptr_t>(sg.out16);
#ifndef SQLLM_ABLATION_BUILD
    asm volatile("" : "+s"(out_at));
#endif
    OT* out = reinterpret_cast<OT*>(out_at);
    const auto* ra = rope_args();
    const uint32_t bn = (uint32_t)(at - (size_t)c);  // b * N (N is even)
    if (member == 2) {
      const OT r = (OT)v;
      if (out) out[at] = r;
      const auto* ca = cache_args(ra);
      // (one unsigned comparison: negative slots are out of range too)
      const uint32_t s = (uint32_t)ca->slots[(int)((float)bn * ca->inv_nv + 0.5f)];
      if (s < ca->n_slots) *cache_at<OT>(ca, ra, ca->v_cache, s, (uint32_t)c) = r;
      return;
    }
    bool is_hi;
    int j, dist;
    u64* pw = (member ? ra->pair_k : ra->pair_q) + ((bn >> 1) + locate(ra, c, &is_hi, &j, &dist));
    const u64 mine = kPairTag | (u64)__builtin_bit_cast(uint32_t, v);
    const u64 other = __hip_atomic_exchange(SQLLM_GLOBAL(u64, pw), mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (other == 0) return;  // the first of the two: the partner column's finisher completes the pair
    const float o = __builtin_bit_cast(float, (uint32_t)other);
    // (located a second time, as in RopeFinish)
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
    // (the host admits batch * N below 2^31: the element index fits 32 bits, and one register carries it across the loads)
    const uint32_t at_lo = is_hi ? (uint32_t)at - (uint32_t)dist : (uint32_t)at;
    const OT r_lo = (OT)(lo * cs - hi * sn), r_hi = (OT)(hi * cs + lo * sn);
    if (member == 0 || out) {
      out[at_lo] = r_lo;
      out[at_lo + (uint32_t)dist] = r_hi;
    }
    if (member) {  // k: both columns of a pair lie in one head, so the upper one is `dist` elements on in the cache too
      const uint32_t c_lo = is_hi ? (uint32_t)c2 - (uint32_t)dist : (uint32_t)c2;
      const auto* ca = cache_args(ra);
      // (the batch row a second time, out of the two indices that are live anyway)
      const uint32_t s = (uint32_t)ca->slots[(int)((float)(at_lo - c_lo) * ra->inv_nk + 0.5f)];
      if (s < ca->n_slots) {
        OT* dst = cache_at<OT>(ca, ra, ca->k_cache, s, c_lo);
        dst[0] = r_lo;
        dst[dist] = r_hi;
      }
    }
    __hip_atomic_exchange(SQLLM_GLOBAL(u64, pw), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (result unused)
  }
};

// the kernel argument from the host's description of the cache and of the rotation (the launchers have checked both)
inline KvCacheArgs make_kv_cache_args(const LaunchArgs& a, const QkvRope& r, const KvCache& kc) {
  KvCacheArgs ca;
  ca.k_cache = kc.k_cache;
  ca.v_cache = kc.v_cache;
  ca.slots = kc.slots;
  ca.slot_stride = (uint32_t)kc.slot_stride;
  ca.head_skip = (uint32_t)(kc.head_stride - r.head_dim);
  ca.n_slots = (uint32_t)kc.n_slots;
  ca.inv_nv = 1.f / (float)a.ga.seg[2].gm.N;
  return ca;
}

// the launch's operands with the outputs the caller left out taken away (the host layer's validation saw stand-ins)
inline LaunchArgs without_left_out(const LaunchArgs& a, const KvCache& kc) {
  LaunchArgs b = a;
  if (!kc.write_out_k) b.ga.seg[1].out16 = nullptr;
  if (!kc.write_out_v) b.ga.seg[2].out16 = nullptr;
  return b;
}

}  // namespace sqllm
