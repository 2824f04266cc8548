// sqllm_cache_fp8_finish.h -- the attention front's finishing policy that writes k and v into a KV cache of 1-byte OCP
// e4m3fn elements, and the kernel argument it reads (include/sqllm_hip.h, sqllm_kv_cache_fp8: the contract; the kernels of
// sqllm_linear_qkv_cache_fp8.hip and sqllm_linear_qkv_norm_cache_fp8.hip are instantiated with it).  RopeCacheFinish
// (sqllm_cache_finish.h) with another element in the cache: the walk, the pair exchange, the rotation and the one rounding
// of out_k / out_v are the parent's; the cache receives
//
//     byte = e4m3_rne(min(max(x * inv, -448), 448))        inv = 1 / scale, fp32, formed once on the host
//
// of the fp32 value x BEFORE its rounding to 16 bits -- one rounding, straight to fp8.  The clamp is explicit (the result
// does not depend on the conversion instruction's overflow mode), +-inf therefore saturates, and NaN takes its own path
// (fmaxf(NaN, c) is c): exponent and mantissa bits all set.  gfx950's v_cvt_pk_fp8_f32 rounds to nearest even and produces e4m3's subnormals.
#pragma once
#include <stddef.h>

#include "sqllm_cache_finish.h"

namespace sqllm {

// by-value kernel argument behind RopeArgs; read through cache_fp8_args() only.  The 16-bit cache's argument with the two
// reciprocals behind it: two more scalar loads in the finisher that stores, no table and no vector load.  The strides are in
// bytes, which is what elements of one byte make of them.
struct KvCacheFp8Args {
  KvCacheArgs c;
  float inv_k, inv_v;  // 1 / k_scale, 1 / v_scale
};
constexpr unsigned kKvCacheFp8ArgsAt = kRopeArgsAt + sizeof(RopeArgs);
static_assert(sizeof(KvCacheFp8Args) == 48 && offsetof(KvCacheFp8Args, c) == 0 && kKvCacheFp8ArgsAt % alignof(KvCacheFp8Args) == 0,
              "the rotary arguments end on this argument's alignment, and cache_at() reads its head");

// (from the pointer rope_args() returned, at constant offsets from the same base register pair: see cache_args())
__device__ __forceinline__ const __attribute__((address_space(4))) KvCacheFp8Args* cache_fp8_args(const __attribute__((address_space(4))) RopeArgs* ra) {
  static_assert(kKvCacheFp8ArgsAt - kRopeArgsAt == sizeof(RopeArgs), "directly behind the rotary arguments");
  return reinterpret_cast<const __attribute__((address_space(4))) KvCacheFp8Args*>(ra + 1);
}

constexpr float kE4m3Max = 448.0f;

// min(max(x * inv, -448), 448), except that a NaN stays one: fmaxf(NaN, c) is c, so NaN takes its own path, a select between two
// registers.  (Not a constant OR-ed into the byte afterwards: the compiler keeps such a constant in a VGPR across the whole
// walk, and the 4-bit 2-row tile has none to spare.)  x * inv is NaN exactly when x is: inv is finite and positive.
__device__ __forceinline__ float e4m3_clamp(float x, float inv) {
  const float c = __builtin_fminf(__builtin_fmaxf(x * inv, -kE4m3Max), kE4m3Max);
  return x != x ? x : c;
}

// The byte of x * inv in bits 16..23 of `low`, whose bits 0..15 stay (the 16-bit element of the same value rides there: one
// register carries both roundings to their stores).  The conversion turns a NaN into a NaN byte, 0x7f or 0xff.
__device__ __forceinline__ uint32_t e4m3_above(float x, float inv, uint32_t low) {
  const float c = e4m3_clamp(x, inv);
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c, c, (int)low, true);
}
// the bytes of x0 * inv and x1 * inv, in bits 0..7 and bits 16..23 -- the low bytes of the register's two halves, each of which a
// byte store takes without a shift; one value after the other, so that each fp32 value ends with its conversion
__device__ __forceinline__ uint32_t e4m3_pair(float x0, float x1, float inv) {
  const float c0 = e4m3_clamp(x0, inv);
  return e4m3_above(x1, inv, (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(c0, c0, 0, false));
}

// OT: the element type of the outputs; the contributions follow FixRange<__bf16> whatever OT is
template <typename OT>
struct RopeCacheFp8Finish {
  int member;  // this workgroup's segment: 0 = q, 1 = k, 2 = v
  static constexpr bool kOrderedCsr = true;  // a CSR chunk's parts of a row meet in wave order: the same fp32 value in every run
  template <typename XT> struct Range { using type = __bf16; };
  template <typename RT>
  __device__ __forceinline__ void done(const Segment& sg, u64* word, u64 total, unsigned target, size_t at, int c) const {
    float v;
    if (!column_value(sg, total, target, c, &v)) return;
    atomicExch(word, 0ull);  // result unused: a plain atomic store
    // (null for k or v: only the cache receives that member; found out here, as in RopeCacheFinish)
    uintptr_t out_at = reinterpret_cast<uintptr_t>(sg.out16);
#ifndef SQLLM_ABLATION_BUILD
    asm volatile("" : "+s"(out_at));
#endif
    OT* out = reinterpret_cast<OT*>(out_at);
    const auto* ra = rope_args();
    const uint32_t bn = (uint32_t)(at - (size_t)c);  // b * N (N is even)
    if (member == 2) {
      const auto* fa = cache_fp8_args(ra);
      // (both roundings of v into one register, which is what the 16-bit cache's finisher carries to its two stores)
      const uint32_t r = e4m3_above(v, fa->inv_v, (uint32_t)__builtin_bit_cast(unsigned short, (OT)v));
      if (out) reinterpret_cast<unsigned short*>(out)[at] = (unsigned short)r;
      // (one unsigned comparison: negative slots are out of range too)
      const uint32_t s = (uint32_t)fa->c.slots[(int)((float)bn * fa->c.inv_nv + 0.5f)];
      if (s < fa->c.n_slots) *cache_at<uint8_t>(&fa->c, ra, fa->c.v_cache, s, (uint32_t)c) = (uint8_t)(r >> 16);
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
    // Both roundings of the two fp32 values at once, into ONE register: the pair's two 16-bit elements in its halves -- and, for
    // k, the pair's two bytes in a second one.  The fp32 values end here: four results in two registers across the stores, as
    // many as the 16-bit cache's finisher carries (the 4-bit 2-row tile has none to spare).
    uint32_t r16, r8;
    {
      const float f_lo = lo * cs - hi * sn, f_hi = hi * cs + lo * sn;
      r16 = (uint32_t)__builtin_bit_cast(unsigned short, (OT)f_lo) | (uint32_t)__builtin_bit_cast(unsigned short, (OT)f_hi) << 16;
      // (for q too, whose bytes go nowhere: a branch around the conversions costs the 3-bit 1-row norm tile a register)
      r8 = e4m3_pair(f_lo, f_hi, cache_fp8_args(ra)->inv_k);
    }
    asm volatile("" : "+v"(r16), "+v"(r8));
    if (member == 0 || out) {
      unsigned short* o16 = reinterpret_cast<unsigned short*>(out);
      o16[at_lo] = (unsigned short)r16;
      o16[at_lo + (uint32_t)dist] = (unsigned short)(r16 >> 16);
    }
    if (member) {  // k: both columns of a pair lie in one head, so the upper one is `dist` bytes on in the cache too
      const uint32_t c_lo = is_hi ? (uint32_t)c2 - (uint32_t)dist : (uint32_t)c2;
      const auto* fa = cache_fp8_args(ra);
      // (the batch row a second time, out of the two indices that are live anyway)
      const uint32_t s = (uint32_t)fa->c.slots[(int)((float)(at_lo - c_lo) * ra->inv_nk + 0.5f)];
      if (s < fa->c.n_slots) {
        uint8_t* dst = cache_at<uint8_t>(&fa->c, ra, fa->c.k_cache, s, c_lo);
        dst[0] = (uint8_t)r8;
        dst[dist] = (uint8_t)(r8 >> 16);
      }
    }
    // The pair word's address a second time, out of the indices that are live anyway (b * N is at_lo - c_lo): held from the first
    // exchange to here it is two registers across the conversions, which the 4-bit 2-row tile does not have.
    {
      int c3 = c2;
      asm volatile("" : "+v"(c3));
      const uint32_t c_lo = is_hi ? (uint32_t)c3 - (uint32_t)dist : (uint32_t)c3;
      u64* pw2 = (member ? ra->pair_k : ra->pair_q) + (((at_lo - c_lo) >> 1) + locate(ra, c3, &is_hi, &j, &dist));
      __hip_atomic_exchange(SQLLM_GLOBAL(u64, pw2), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (result unused)
    }
  }
};

// the kernel argument from the host's description of the cache and of the rotation (the launchers have checked both)
inline KvCacheFp8Args make_kv_cache_fp8_args(const LaunchArgs& a, const QkvRope& r, const KvCache& kc) {
  KvCacheFp8Args fa;
  fa.c = make_kv_cache_args(a, r, kc);
  fa.inv_k = kc.inv_k_scale;
  fa.inv_v = kc.inv_v_scale;
  return fa;
}

}  // namespace sqllm
