// sqllm_attn_tree64.h -- what the two wide-tree kernel files share (sqllm_attn_tree64.hip: 16-bit caches and the combine;
// sqllm_attn_tree64_fp8.hip: caches of e4m3fn bytes): the kernels' argument and how the host fills it, what the entries serve, a
// row's 64-bit word and its effective length, the attended keys of a key tile as one 64-bit value, one key tile of the compute
// loop (sqllm_attn_prefill.hip's, with the select by bit) and the two ways a workgroup finishes.  NOT shared: everything between
// the cache and LDS, and the walk around it, which stay copies of each other as in the prefill files.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sqllm_attn_prefill.h"

namespace sqllm {

constexpr int kTree64MaxQLen = 64;     // nodes per sequence: the bits of a row's word
static_assert(kTree64Partition % kPrefillTile == 0, "a partition is whole key tiles");

// The prefill kernels' argument, the mask and the partials behind it.  Partial (row, query head, partition) is acc[head_dim] at
// ws_acc[((row * n_q_heads + head) * n_parts + part) * head_dim] and (max, sum) at ws_ml[... * 2]: the combine reads along d.
struct AttnTree64Args : AttnPrefillArgs {
  const int* tree_mask;  // [batch, mask_stride] int32: row (b, t)'s word is words 2 t (low) and 2 t + 1 (high) of sequence b
  long long mask_stride;
  float* ws_acc;
  float* ws_ml;
  int n_q_heads;
  int batch;      // sequences: the combine's grid
  int n_parts;    // ceil(capacity / kTree64Partition); 1: the partial kernel finishes the rows itself
  float v_scale;  // the byte caches' (1 otherwise): once per output element, before the one rounding
};

// what the four entries serve, but for the cache's element type: from HOST fields only
inline bool tree64_served(const AttnCall& c) {
  return (c.head_dim == 64 || c.head_dim == 128) && c.n_kv_heads >= 1 && c.n_kv_heads <= 65535 && c.n_q_heads % c.n_kv_heads == 0 &&
         c.n_q_heads / c.n_kv_heads <= 8 && c.batch >= 1 && c.batch <= kPrefillMaxBatch && c.q_len >= 1 && c.q_len <= kTree64MaxQLen &&
         !c.window && c.tree_mask && c.workspace && c.n_parts >= 1;
}

inline AttnTree64Args make_tree64_args(const AttnCall& c) {
  AttnTree64Args k;
  static_cast<AttnPrefillArgs&>(k) = make_prefill_args(c);
  k.tree_mask = c.tree_mask;
  k.mask_stride = c.mask_stride;
  k.ws_acc = static_cast<float*>(c.workspace);
  k.ws_ml = k.ws_acc + (long long)c.batch * c.q_len * c.n_q_heads * c.n_parts * c.head_dim;
  k.n_q_heads = c.n_q_heads;
  k.batch = c.batch;
  k.n_parts = c.n_parts;
  k.v_scale = c.v_scale;
  return k;
}

// m(b, t): the row's word, two int32 loads (rows of the mask are 4-byte aligned whatever the stride), bits at and above n cleared
__device__ __forceinline__ unsigned long long tree64_word(const AttnTree64Args& a, int b, int t, int n) {
  const int* const p = a.tree_mask + (long long)b * a.mask_stride + 2 * t;
  const unsigned long long w = (unsigned long long)(unsigned)p[0] | ((unsigned long long)(unsigned)p[1] << 32);
  return n >= 64 ? w : n <= 0 ? 0ull : w & ((1ull << n) - 1ull);
}

// Leff(b, t) of include/sqllm_hip.h (sqllm_attn_tree64), tree_row_len of sqllm_attn.h for a 64-bit word `m` = m(b, t): in
// [1, capacity]; 0 for a row that is +0; -1 for a row that is NaN.  The corner rows are judged in the tree entries' order.
__device__ __forceinline__ int tree64_row_len(int n, int seq, int t, int q_len, int capacity, unsigned long long m) {
  if (n > q_len) return -1;
  if (n <= 0) return 0;
  if (seq < n) return -1;
  if (t >= n) return 0;
  const long long len = (long long)seq - n + (m ? 64 - __builtin_clzll(m) : 0);
  if (len == 0) return 0;
  if (len > capacity) return -1;
  return (int)len;
}

// the keys a row attends inside the key tile [key0, key0 + 64), bit i for key key0 + i: the context [0, ctx) and the word shifted to
// the tile's origin (ctx >= 0; a row that attends nothing passes ctx = 0 and word = 0)
__device__ __forceinline__ unsigned long long tree64_tile_bits(int ctx, unsigned long long word, int key0) {
  unsigned long long bits = window_tile_bits(0, ctx, key0);
  if (ctx >= key0) {
    if (ctx - key0 < 64) bits |= word << (ctx - key0);
  } else if (key0 - ctx < 64) {
    bits |= word >> (key0 - ctx);
  }
  return bits;
}

// 16 bytes of fp32 that are aligned to their elements only (the workspace is 4-byte aligned)
struct __attribute__((packed, aligned(4))) Floats4 {
  float v[4];
};

// One key tile of the compute loop of sqllm_attn_prefill.hip, for the wave that calls it: S^T = K Q^T from the staged K, the fp32
// online softmax, out^T += V^T P^T in three planes.  MASKED: score and weight are SELECTED by the lane's bit of `bits` (a masked score
// is -inf, a masked weight 0, whatever bits the key holds); otherwise every key of the tile is every row's.
template <int D, typename OT, bool MASKED>
__device__ __forceinline__ void tree64_tile(const uint16_t* ksb, const uint16_t* vsb, const u32x4 (&qf)[D / 32], unsigned long long bits, float scale,
                                            int l16, int q4, float& m_run, float& l_run, f32x4 (&acc)[D / 16]) {
  constexpr int KROW = D + 8, VROW = kPrefillTile + 8, NDB = D / 16, NQC = D / 32;
  // lane holds query l16, keys key0 + 16 jb + 4 q4 + e
  f32x4 s[4];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {
    s[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NQC; ++c) {
      const u32x4 kf = *reinterpret_cast<const u32x4*>(&ksb[(16 * jb + l16) * KROW + c * 32 + q4 * 8]);
      s[jb] = mfma_16x16x32<OT>(kf, qf[c], s[jb]);
    }
  }
  const unsigned long long mine = bits >> (4 * q4);  // bit 16 jb + e: this lane's key (jb, e)
  float sc[4][4], tmax = -__builtin_inff();
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool on = !MASKED || (mine >> (16 * jb + e) & 1ull);
      sc[jb][e] = on ? scale * s[jb][e] : -__builtin_inff();
      tmax = fmaxf(tmax, sc[jb][e]);
    }
  }
  tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
  tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
  const float m_new = fmaxf(m_run, tmax);
  const float m_use = m_new == -__builtin_inff() ? 0.0f : m_new;  // nothing attended yet: no inf - inf
  const float alpha = expf(m_run - m_use);
  float tsum = 0.0f;
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool on = !MASKED || (mine >> (16 * jb + e) & 1ull);
      sc[jb][e] = on ? expf(sc[jb][e] - m_use) : 0.0f;
      tsum += sc[jb][e];
    }
  }
  tsum += __shfl_xor(tsum, 16, 64);
  tsum += __shfl_xor(tsum, 32, 64);
  l_run = l_run * alpha + tsum;
  m_run = m_new;
#pragma unroll
  for (int db = 0; db < NDB; ++db) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[db][e] *= alpha;
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float w[8] = {sc[2 * c][0], sc[2 * c][1], sc[2 * c][2], sc[2 * c][3], sc[2 * c + 1][0], sc[2 * c + 1][1], sc[2 * c + 1][2], sc[2 * c + 1][3]};
    u32x4 ph, pm, pl;
    weight_planes<OT>(w, ph, pm, pl);
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      const u32x4 vf = *reinterpret_cast<const u32x4*>(&vsb[(16 * db + l16) * VROW + c * 32 + q4 * 8]);
      f32x4 t = acc[db];
      t = mfma_16x16x32<OT>(vf, pl, t);  // small planes first
      t = mfma_16x16x32<OT>(vf, pm, t);
      t = mfma_16x16x32<OT>(vf, ph, t);
      acc[db] = t;
    }
  }
}

// The end of a workgroup, for the lane's row (d = 16 db + 4 q4 .. + 3) of query head `head`, length `len` (tree64_row_len), `fb` the
// first key of this partition with a table entry outside the cache.  One partition: the row itself, as sqllm_attn_prefill.hip
// finishes it (v_scale before the one rounding).  Otherwise the row's partial of partition `part`, which begins at key p0: the
// rows that end at or below p0 have none, the combine writes the +0 and the NaN rows, and a row that meets the bad entry leaves a
// NaN sum behind.  Vector stores only.
template <int D, typename OT>
__device__ __forceinline__ void tree64_finish(const AttnTree64Args& a, long long row, int head, int part, int p0, int len, int fb, int q4, float m_run,
                                              float l_run, const f32x4 (&acc)[D / 16]) {
  constexpr int NDB = D / 16;
  const bool nan_row = len < 0 || len > fb;
  if (a.n_parts == 1) {
    OT* const orow = reinterpret_cast<OT*>(a.out) + row * a.out_stride + (long long)head * D;
    const float denom = std::is_same<OT, __bf16>::value ? l_run : l_run * 32768.0f;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      OT o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float v = 0.0f;
        if (len > 0) v = acc[db][e] / denom * a.v_scale;
        if (nan_row) v = __builtin_nanf("");
        o[e] = (OT)v;
      }
      Packed4 p;
      p.w[0] = (uint32_t)__builtin_bit_cast(unsigned short, o[0]) | ((uint32_t)__builtin_bit_cast(unsigned short, o[1]) << 16);
      p.w[1] = (uint32_t)__builtin_bit_cast(unsigned short, o[2]) | ((uint32_t)__builtin_bit_cast(unsigned short, o[3]) << 16);
      *reinterpret_cast<Packed4*>(orow + 16 * db + 4 * q4) = p;
    }
    return;
  }
  if (len <= p0) return;
  const long long pa = (row * a.n_q_heads + head) * a.n_parts + part;
  const float nan = __builtin_nanf("");
#pragma unroll
  for (int db = 0; db < NDB; ++db) {
    Floats4 f;
#pragma unroll
    for (int e = 0; e < 4; ++e) f.v[e] = nan_row ? nan : acc[db][e];
    *reinterpret_cast<Floats4*>(a.ws_acc + pa * D + 16 * db + 4 * q4) = f;
  }
  if (q4 == 0) {
    a.ws_ml[pa * 2] = nan_row ? 0.0f : m_run;
    a.ws_ml[pa * 2 + 1] = nan_row ? nan : l_run;
  }
}

}  // namespace sqllm
