// sqllm_attn_tree.hip -- decode attention for a TREE of new tokens per sequence in one read of K and V (include/sqllm_hip.h:
// sqllm_attn_tree_f16 / _bf16): the verification step of tree speculation.  Row (b, t) attends the context [0, C_b) and the new
// tokens ("nodes", the keys C_b + j) whose bit j is set in its mask word; with the chain's words (2 << t) - 1 every row holds the
// bits of sqllm_attn_append_*.  The kernel is sqllm_attn_append.hip's -- same grid, same partitions, same lanes, same order of every
// sum -- with a per-head mask over the at most 16 node keys.  A tree differs from a chain only there: a partition wholly below the
// context runs the one-query body, and at most two partitions of a sequence see the mask.
//
// Launch 1 (partials), one workgroup of 256 threads per (partition of kAttnPartition keys, kv head, sequence, chunk of up to 8
// virtual heads), as the sibling:
//   0. (sqllm_attn.h: tree_phase0) the chunk's virtual heads, the keys nv[h] of this partition below each head's Leff and the head's
//      mask word shifted to the partition's origin (both in LDS); ctx, the context's end inside the partition: ONE scalar per
//      workgroup, per sequence and not per head; the slots, once, for the longest head.
//   1. QK for the keys of the longest head.  A score is kept iff the key is below ctx or the head's bit for it is set; every
//      other one is -inf in LDS, whatever the sibling's key holds.
//   2. softmax per head over its nv[h] keys, as the sibling: an excluded key's weight is exp(-inf - m) = +0, stored and added.  No
//      partition below Leff is empty of attended keys (the header says why), so m is a real score.
//   3. PV.  The whole steps below ctx are every head's keys and take the sibling's unrolled loop.  Behind them come at most three
//      steps (16 node keys against steps of 16 or 32, and the step ctx lies in): an excluded key holds a sibling's real data, so it
//      is left out by a SELECT on the accumulator, never by a factor 0.
//   4. the key-lanes meet as there; out (one partition) or the workspace, per virtual head.
// launch 2 (combine), one workgroup of head_dim threads per (query head, row): the sibling's, over ceil(Leff(b, t) / 256) partials;
// it writes the +0 and the NaN rows.
//
// Registers and LDS (the compiler's resource report for gfx950; virtual-head class 1 / 2 / 4 / 8, the larger of the instances of a
// class): 46 / 58 / 77 / 116 VGPRs, 70 / 84 / 88 / 101 SGPRs, 10520 / 19752 / 38216 / 42376 bytes of LDS (the sibling's plus the
// mask words); the combines 12 VGPRs, 34 SGPRs, no LDS.  No scratch and no spills in any instance, and room for two workgroups
// per CU at least, as the sibling's (148 VGPRs and 106 SGPRs at class 8 there).  The per-head words stay in LDS beside nvl: the
// scalar registers are the tight resource (sqllm_attn_append.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sqllm_attn.h"
#include "sqllm_decode.h"
#include "sqllm_kernels.h"

namespace sqllm {

template <int D, int GC, typename OT>
__global__ void __launch_bounds__(kAttnThreads) sqllm_attn_tree_kernel(const AttnTreeArgs a) {
  constexpr int P = kAttnPartition;
  constexpr int LPK = D / 8;         // lanes per key
  constexpr int KPW = 64 / LPK;      // keys per wave instruction
  constexpr int KPS = KPW * 4;       // keys per step of the workgroup
  constexpr int STEPS = P / KPS;
  constexpr int U = kAttnUnroll;
  constexpr int HC = GC < 4 ? GC : 4;  // heads per round of the key-lane exchange
  static_assert(STEPS % U == 0, "whole unrolled rounds");
  __shared__ float sc[GC][P];
  __shared__ int slots[P];
  __shared__ float ml[GC][2];
  __shared__ __attribute__((aligned(16))) float red[KPS][HC][D];
  __shared__ int nvl[GC];
  __shared__ unsigned mwl[GC];
  __shared__ int first_bad;

  const int part = blockIdx.x, hk = blockIdx.y;
  const int chunk = __builtin_amdgcn_readfirstlane(blockIdx.z / a.batch), b = blockIdx.z - chunk * a.batch;  // (a uniform quotient: back to a scalar)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane % LPK, grp = lane / LPK;
  const bool single = a.n_parts == 1;

  // 0. the virtual heads, their mask words and the slots of this partition's keys
  int nv[GC], n_max, ctx;
  if (!tree_phase0<D, GC, OT>(a, part, hk, b, chunk, slots, &first_bad, nvl, mwl, nv, n_max, ctx)) return;
  unsigned live = 0;  // the heads served here, as one scalar: nv[] itself is not held beyond this point (nvl is, in LDS)
#pragma unroll
  for (int h = 0; h < GC; ++h) live |= (nv[h] > 0 ? 1u : 0u) << h;
  const int nsteps = (n_max + KPS - 1) / KPS;
  const unsigned long long head_off = (unsigned long long)(unsigned)hk * a.head_stride + (unsigned)(sub * 8);

  // 1. scores
  {
    float qf[GC][8];
#pragma unroll
    for (int h = 0; h < GC; ++h) {
      if (live >> h & 1) {
        const AppendHead v = append_head(a, hk, b, chunk * GC + h);
        const OT* q = reinterpret_cast<const OT*>(a.q) + (long long)v.row * a.q_stride + (long long)v.head * D + sub * 8;
        widen8<OT>(*reinterpret_cast<const Packed8*>(q), qf[h]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[h][j] = 0.0f;
      }
    }
    const int my_nv = sub < GC ? nvl[sub < GC ? sub : 0] : 0;
    const unsigned my_w = sub < GC ? mwl[sub < GC ? sub : 0] : 0u;
    const OT* kc = reinterpret_cast<const OT*>(a.k_cache);
    for (int s0 = 0; s0 < nsteps; s0 += U) {
      Packed8 kr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        kr[u] = *reinterpret_cast<const Packed8*>(kc + ((unsigned long long)(unsigned)slots[kl] * a.slot_stride + head_off));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        float kf[8];
        widen8<OT>(kr[u], kf);
        float mine = 0.0f;
#pragma unroll
        for (int h = 0; h < GC; ++h) {
          float dot = qf[h][0] * kf[0];
#pragma unroll
          for (int j = 1; j < 8; ++j) dot = fmaf(qf[h][j], kf[j], dot);
          dot = key_sum<LPK>(dot);
          if (sub == h) mine = dot;
        }
        if (sub < GC) sc[sub][kl] = kl < my_nv && tree_key(my_w, kl, ctx) ? a.scale * mine : -__builtin_inff();
      }
    }
  }
  __syncthreads();

  // 2. the partition's softmax, one wave per head over the keys below the head's end (the excluded ones among them: -inf, weight +0)
  for (int h = wave; h < GC; h += 4) {
    const int n_valid = nvl[h];
    if (n_valid == 0) continue;
    float s[P / 64], m = -__builtin_inff();
#pragma unroll
    for (int i = 0; i < P / 64; ++i) {
      const int kl = lane + 64 * i;
      s[i] = kl < n_valid ? sc[h][kl] : -__builtin_inff();
      m = fmaxf(m, s[i]);
    }
    m = wave_max(m);
    float l = 0.0f;
#pragma unroll
    for (int i = 0; i < P / 64; ++i) {
      const int kl = lane + 64 * i;
      const float w = kl < n_valid ? expf(s[i] - m) : 0.0f;
      sc[h][kl] = w;
      l += w;
    }
    l = wave_sum(l);
    if (lane == 0) {
      ml[h][0] = m;
      ml[h][1] = l;
    }
  }
  __syncthreads();

  // 3. PV
  float acc[GC][8];
#pragma unroll
  for (int h = 0; h < GC; ++h)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[h][j] = 0.0f;
  {
    const OT* vc = reinterpret_cast<const OT*>(a.v_cache);
    // the whole steps below the context's end: every key is every head's, and the loop is the sibling's
    const int shared_steps = ctx / KPS;
    for (int s0 = 0; s0 < shared_steps; s0 += U) {
      Packed8 vr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        vr[u] = *reinterpret_cast<const Packed8*>(vc + ((unsigned long long)(unsigned)slots[kl] * a.slot_stride + head_off));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        if (s0 + u >= shared_steps) break;  // (uniform)
        float vf[8];
        widen8<OT>(vr[u], vf);
#pragma unroll
        for (int h = 0; h < GC; ++h) {
          const float w = sc[h][kl];  // (a head that is not served here gathers what nobody reads)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[h][j] = fmaf(w, vf[j], acc[h][j]);
        }
      }
    }
    // the steps behind them, up to nsteps: the step the context ends in and the steps of the 16 node keys, three at the most (a
    // remark on speed, nothing depends on the count).  A key the head's word excludes, or one at or beyond its end, holds another
    // token's real data, with any bits: left out by a SELECT on the accumulator, never by a factor 0
    for (int s0 = shared_steps; s0 < nsteps; ++s0) {
      const int kl = s0 * KPS + wave * KPW + grp;
      const Packed8 vr = *reinterpret_cast<const Packed8*>(vc + ((unsigned long long)(unsigned)slots[kl] * a.slot_stride + head_off));
      float vf[8];
      widen8<OT>(vr, vf);
#pragma unroll
      for (int h = 0; h < GC; ++h) {
        const bool mine = kl < nvl[h] && tree_key(mwl[h], kl, ctx);  // (from LDS: sixteen more scalars held across the loops do not fit)
        const float w = sc[h][kl];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[h][j] = mine ? fmaf(w, vf[j], acc[h][j]) : acc[h][j];
      }
    }
  }

  // 4. the key-lanes meet, HC heads per round, in ascending key-lane order
#pragma unroll
  for (int h0 = 0; h0 < GC; h0 += HC) {
    if (h0) __syncthreads();
#pragma unroll
    for (int hh = 0; hh < HC; ++hh) {
      f32x4* at = reinterpret_cast<f32x4*>(&red[wave * KPW + grp][hh][sub * 8]);
      at[0] = f32x4{acc[h0 + hh][0], acc[h0 + hh][1], acc[h0 + hh][2], acc[h0 + hh][3]};
      at[1] = f32x4{acc[h0 + hh][4], acc[h0 + hh][5], acc[h0 + hh][6], acc[h0 + hh][7]};
    }
    __syncthreads();
    for (int i = tid; i < HC * D; i += kAttnThreads) {
      const int hh = i / D, d = i % D, h = h0 + hh;
      if (nvl[h] == 0) continue;
      const AppendHead v = append_head(a, hk, b, chunk * GC + h);
      float t = red[0][hh][d];
#pragma unroll
      for (int k = 1; k < KPS; ++k) t += red[k][hh][d];
      if (single) {
        reinterpret_cast<OT*>(a.out)[(long long)v.row * a.out_stride + (long long)v.head * D + d] = (OT)(t / ml[h][1]);
      } else {
        const long long pa = ((long long)v.row * a.n_q_heads + v.head) * a.n_parts + part;
        a.ws_acc[pa * D + d] = t;
        if (d == 0) {
          a.ws_ml[pa * 2] = ml[h][0];
          a.ws_ml[pa * 2 + 1] = ml[h][1];
        }
      }
    }
  }
}

template <int D, typename OT>
__global__ void __launch_bounds__(D) sqllm_attn_tree_combine_kernel(const AttnTreeArgs a) {
  const int hq = blockIdx.x, row = blockIdx.y, d = threadIdx.x;
  const int b = row / a.q_len, tok = row - b * a.q_len;
  OT* const out = reinterpret_cast<OT*>(a.out) + (long long)row * a.out_stride + (long long)hq * D;
  const int len = tree_row_len(a.q_lens ? a.q_lens[b] : a.q_len, a.seq_lens[b], tok, a.q_len, a.capacity,
                               a.tree_mask[(long long)b * a.mask_stride + tok]);
  if (len == 0) {
    out[d] = (OT)0.0f;
    return;
  }
  if (len < 0) {
    out[d] = (OT)__builtin_nanf("");
    return;
  }
  const int np = (len + kAttnPartition - 1) / kAttnPartition;
  const long long p0 = ((long long)row * a.n_q_heads + hq) * a.n_parts;
  float m = -__builtin_inff();
  for (int i = 0; i < np; ++i) m = fmaxf(m, a.ws_ml[(p0 + i) * 2]);
  float l = 0.0f, t = 0.0f;
  for (int i = 0; i < np; ++i) {
    const float w = expf(a.ws_ml[(p0 + i) * 2] - m);
    l = fmaf(w, a.ws_ml[(p0 + i) * 2 + 1], l);
    t = fmaf(w, a.ws_acc[(p0 + i) * D + d], t);
  }
  out[d] = (OT)(t / l);
}

struct AttnTreeTag : AttnTreeTokens {
  static constexpr bool fp8 = false;
  template <int D, int GC, typename OT>
  static auto kernel() { return sqllm_attn_tree_kernel<D, GC, OT>; }
  template <int D, typename OT>
  static auto combine_kernel() { return sqllm_attn_tree_combine_kernel<D, OT>; }
};

// the combine alone: behind this file's partials, and behind those of sqllm_attn_tree_fp8.hip
static hipError_t launch_attn_combine_tree(const AttnTreeArgs& k, int head_dim, bool bf16, hipStream_t stream) {
  return launch_attn_combine<AttnTreeTag>(k, head_dim, bf16, dim3(k.n_q_heads, k.batch * k.q_len), stream);
}

// the host layer reaches the launcher through its slot of g_launch_attn_tree (sqllm_kernels.h), so that it links without this file too
static const bool g_attn_tree_registered = (g_launch_attn_tree[0] = launch_attn<AttnTreeTag>, g_launch_attn_tree_combine = launch_attn_combine_tree, true);

}  // namespace sqllm
