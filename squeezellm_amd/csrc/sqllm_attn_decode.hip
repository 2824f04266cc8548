// sqllm_attn_decode.hip -- decode attention (one new query per sequence) over the KV cache the attention front writes
// (include/sqllm_hip.h: sqllm_attn_decode_f16 / _bf16).  A streaming read of K and V: neither the matrix cores nor the softmax
// matter, the loads do.
//
// Launch 1 (partials), one workgroup of 256 threads per (partition of kAttnPartition keys, kv head, row); all the query heads
// of the kv head's group are served from ONE read of K and V:
//   0. thread t resolves key t of the partition to its slot -- one divide and one block-table read per thread, before the
//      stream starts; nothing in the streaming loops depends on the table.  Keys at or beyond seq_lens[b] take the slot of
//      the partition's first key (an attended slot: their loads are in bounds and their values are replaced by zeros), so the
//      loops below have no divergent loads.  An entry that leads outside [0, n_slots) ends the workgroup with a NaN partial
//      before anything of the caches is read.
//   1. QK: head_dim / 8 lanes cover a key with one 16-byte load each, 64 / (head_dim / 8) keys per wave instruction, kAttnUnroll
//      loads in flight before the first use (4 waves x 4 KiB per workgroup); q of the whole group sits in fp32 registers; the
//      dot product meets across the key's lanes in DPP (quad_perm, row_half_mirror, row_mirror: all lanes of a key end with
//      the same bits); scores go to LDS as [group][partition keys].
//   2. softmax of the partition per head, by one wave per head: max, w = expf(s - max) back into LDS, the sum of w.
//   3. PV: the same walk over V; acc[head][8] in fp32 registers; the 16 (head_dim 128) or 32 (head_dim 64) key-lanes of the
//      workgroup meet through LDS at the partition's end, added in ascending key-lane order.
//   4. one partition (max_blocks * block_size <= kAttnPartition): out = round(acc / sum) and that is the whole call.
//      Otherwise (max, sum, acc[head_dim]) go to the workspace in fp32 and
// launch 2 (combine), one workgroup of head_dim threads per (query head, row), folds the partials of the partitions below
// seq_lens[b] in ascending order.  With one partition it multiplies by expf(0) = 1: the bits of (4).
//
// The order of every sum depends on head_dim, the group class and the key's index alone -- not on the block size, the row, the
// batch or on which workgroup ran first: bit-identical run to run, and row by row.
//
// Registers: q (group x 8 fp32) lives in phase 1 only, acc (group x 8 fp32) in phase 3 only; no scratch, no spills
// (tests/test_codegen_attn_decode_cpu.py).  LDS: scores 8 KiB at most, slots 1 KiB, the key-lane exchange 32 KiB at most: three workgroups per CU.
//
// This file holds the two kernels, a tag that names them and one registration line.  The lane helpers and the launch ladder
// (type x head_dim x group class, then the combine) are sqllm_attn.h's, shared with the three sibling files; the kernel BODIES
// of the siblings are copies of the ones here ("Not shared either").
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sqllm_attn.h"
#include "sqllm_decode.h"
#include "sqllm_kernels.h"

namespace sqllm {

// (AttnArgs, the kernels' argument: sqllm_kernels.h; the lane helpers and the launch ladder: sqllm_attn.h)

template <int D, int GC, typename OT>
__global__ void __launch_bounds__(kAttnThreads) sqllm_attn_decode_kernel(const AttnArgs a) {
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

  const int part = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane % LPK, grp = lane / LPK;
  const int g = a.group;
  const bool single = a.n_parts == 1;
  OT* const out = reinterpret_cast<OT*>(a.out) + (long long)b * a.out_stride + (long long)hk * g * D;

  const int len = a.seq_lens[b];
  if (len <= 0 || len > a.capacity) {
    if (single) {  // (otherwise the combine writes these rows)
      const OT c = len <= 0 ? (OT)0.0f : (OT)__builtin_nanf("");
      for (int i = tid; i < g * D; i += kAttnThreads) out[i] = c;
    }
    return;
  }
  const int p0 = part * P;
  if (p0 >= len) return;
  const int n_valid = len - p0 < P ? len - p0 : P;

  // 0. the slots of this partition's keys
  {
    const unsigned p = tid < n_valid ? p0 + tid : p0;
    const unsigned blk = p / (unsigned)a.block_size, off = p - blk * (unsigned)a.block_size;
    const long long s = (long long)a.block_table[(long long)b * a.table_stride + blk] * a.block_size + off;
    const bool bad = s < 0 || s >= a.n_slots;
    slots[tid] = (int)s;
    if (__syncthreads_or(bad)) {  // NaN, and nothing of the caches is read
      const float nan = __builtin_nanf("");
      if (single) {
        for (int i = tid; i < g * D; i += kAttnThreads) out[i] = (OT)nan;
      } else {
        for (int i = tid; i < g * D; i += kAttnThreads) {
          const long long at = ((long long)b * a.n_q_heads + hk * g + i / D) * a.n_parts + part;
          a.ws_acc[at * D + i % D] = nan;
          if (i % D == 0) {
            a.ws_ml[at * 2] = 0.0f;
            a.ws_ml[at * 2 + 1] = nan;
          }
        }
      }
      return;
    }
  }
  const int nsteps = (n_valid + KPS - 1) / KPS;
  const unsigned long long head_off = (unsigned long long)(unsigned)hk * a.head_stride + (unsigned)(sub * 8);

  // 1. scores
  {
    float qf[GC][8];
    const OT* q = reinterpret_cast<const OT*>(a.q) + (long long)b * a.q_stride + (long long)hk * g * D + sub * 8;
#pragma unroll
    for (int h = 0; h < GC; ++h) {
      if (h < g) {
        widen8<OT>(*reinterpret_cast<const Packed8*>(q + h * D), qf[h]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[h][j] = 0.0f;
      }
    }
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
        if (sub < GC) sc[sub][kl] = kl < n_valid ? a.scale * mine : -__builtin_inff();
      }
    }
  }
  __syncthreads();

  // 2. the partition's softmax, one wave per head; every entry of sc[h] is written, whatever phase 1 left there
  for (int h = wave; h < g; h += 4) {
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
    for (int s0 = 0; s0 < nsteps; s0 += U) {
      Packed8 vr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        vr[u] = *reinterpret_cast<const Packed8*>(vc + ((unsigned long long)(unsigned)slots[kl] * a.slot_stride + head_off));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        const bool valid = kl < n_valid;
        if (!valid) {  // (the stand-in slot's values: 0 x NaN would be NaN)
#pragma unroll
          for (int i = 0; i < 4; ++i) vr[u].w[i] = 0u;
        }
        float vf[8];
        widen8<OT>(vr[u], vf);
#pragma unroll
        for (int h = 0; h < GC; ++h) {
          const float w = h < g && valid ? sc[h][kl] : 0.0f;
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[h][j] = fmaf(w, vf[j], acc[h][j]);
        }
      }
    }
  }

  // 4. the key-lanes meet, HC heads per round, in ascending key-lane order
#pragma unroll
  for (int h0 = 0; h0 < GC; h0 += HC) {
    if (h0 >= g) break;  // (uniform)
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
      if (h >= g) break;
      float t = red[0][hh][d];
#pragma unroll
      for (int k = 1; k < KPS; ++k) t += red[k][hh][d];
      if (single) {
        out[h * D + d] = (OT)(t / ml[h][1]);
      } else {
        const long long pa = ((long long)b * a.n_q_heads + hk * g + h) * a.n_parts + part;
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
__global__ void __launch_bounds__(D) sqllm_attn_combine_kernel(const AttnArgs a) {
  const int hq = blockIdx.x, b = blockIdx.y, d = threadIdx.x;
  OT* const out = reinterpret_cast<OT*>(a.out) + (long long)b * a.out_stride + (long long)hq * D;
  const int len = a.seq_lens[b];
  if (len <= 0) {
    out[d] = (OT)0.0f;
    return;
  }
  if (len > a.capacity) {
    out[d] = (OT)__builtin_nanf("");
    return;
  }
  const int np = (len + kAttnPartition - 1) / kAttnPartition;
  const long long p0 = ((long long)b * a.n_q_heads + hq) * a.n_parts;
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

struct AttnDecodeTag : AttnOneQuery {
  static constexpr bool fp8 = false;
  template <int D, int GC, typename OT>
  static auto kernel() { return sqllm_attn_decode_kernel<D, GC, OT>; }
  template <int D, typename OT>
  static auto combine_kernel() { return sqllm_attn_combine_kernel<D, OT>; }
};

// the combine alone: behind this file's partials, and behind those of sqllm_attn_decode_fp8.hip
static hipError_t launch_attn_combine_rows(const AttnArgs& k, int head_dim, bool bf16, int batch, hipStream_t stream) {
  return launch_attn_combine<AttnDecodeTag>(k, head_dim, bf16, dim3(k.n_q_heads, batch), stream);
}

// the host layer reaches the launcher through its slot of g_launch_attn (sqllm_kernels.h), so that it links without this file too
static const bool g_attn_decode_registered = (g_launch_attn[kAttnDecode] = launch_attn<AttnDecodeTag>, g_launch_attn_combine = launch_attn_combine_rows, true);

}  // namespace sqllm
