// sqllm_attn_append.hip -- decode attention for SEVERAL new tokens per sequence in one read of K and V (include/sqllm_hip.h:
// sqllm_attn_append_f16 / _bf16).  Row (b, t) holds the bits sqllm_attn_decode_* gives a row with table row b and length
// L(b, t) = seq_lens[b] - (n_b - 1 - t): the kernel BODIES here are the ones of sqllm_attn_decode.hip, copied, with one change of
// meaning -- a workgroup's heads are VIRTUAL heads, (new token, query head of the kv group) pairs, each with its own length.
// What is still a copy is the bodies alone: the lane helpers, phase 0 and the launch ladder are sqllm_attn.h's, shared by the four files.
//
// Launch 1 (partials), one workgroup of 256 threads per (partition of kAttnPartition keys, kv head, sequence, chunk of up to 8
// virtual heads); the chunks of a (partition, kv head, sequence) read the same keys and are the slowest grid dimension:
//   0. (sqllm_attn.h: append_phase0) the chunk's virtual heads and the keys nv[h] of this partition each of them attends; rows that need no
//      keys; the partition's slots, once, for the longest head.  A head that meets a bad table entry ends as its one-query
//      sibling does, the heads that end below the entry go on.
//   1. QK as there, for the keys of the longest head; a score at or beyond the head's own nv[h] is -inf in LDS.
//   2. softmax per head over its own nv[h] keys.
//   3. PV as there.  The keys below the SHORTEST head's end are all heads' keys: the whole steps of them take the sibling's loop.  In
//      the steps behind them (few: the heads of a sequence end within 15 keys of each other; the loop runs to the longest head's end
//      whatever their number) a key beyond nv[h] holds
//      another token's real data (NaN, inf): it is left out by a SELECT on the accumulator, which is bit for bit what the sibling's
//      fmaf(0, 0, acc) leaves.
//   4. the key-lanes meet as there; out (one partition) or the workspace, per virtual head.
// launch 2 (combine), one workgroup of head_dim threads per (query head, row): the sibling's, over ceil(L(b, t) / 256) partials.
//
// Every sum of a virtual head has the operands and the order its one-query sibling gives that row: the partition of 256 keys,
// the key-to-lane map, ascending key-lanes, ascending partitions.  None of them depends on the sibling's group class, so how
// virtual heads are dealt to workgroups changes no bit.
//
// Registers and LDS as the sibling's, plus nine words of LDS: no scratch, no spills, two workgroups per CU at least
// (tests/test_codegen_attn_append_cpu.py).  The scalar registers are the tight ones (the 8 heads' lengths, the 8 masks of phase 1):
// what is indexed by a head behind phase 1 is read from LDS (nvl), and the corner rows are written by loops that stay loops.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sqllm_attn.h"
#include "sqllm_decode.h"
#include "sqllm_kernels.h"

namespace sqllm {

template <int D, int GC, typename OT>
__global__ void __launch_bounds__(kAttnThreads) sqllm_attn_append_kernel(const AttnAppendArgs a) {
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
  __shared__ int first_bad;

  const int part = blockIdx.x, hk = blockIdx.y;
  const int chunk = __builtin_amdgcn_readfirstlane(blockIdx.z / a.batch), b = blockIdx.z - chunk * a.batch;  // (a uniform quotient: back to a scalar)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int sub = lane % LPK, grp = lane / LPK;
  const bool single = a.n_parts == 1;

  // 0. the virtual heads and the slots of this partition's keys
  int nv[GC], n_max, n_min;
  if (!append_phase0<D, GC, OT>(a, part, hk, b, chunk, slots, &first_bad, nvl, nv, n_max, n_min)) return;
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
        if (sub < GC) sc[sub][kl] = kl < my_nv ? a.scale * mine : -__builtin_inff();
      }
    }
  }
  __syncthreads();

  // 2. the partition's softmax, one wave per head over the head's own keys
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
    // the steps below the SHORTEST head's end: every key is every head's, and the loop is the sibling's (the steps behind them are
    // left out whole, which leaves what its fmaf(0, 0, acc) leaves)
    const int shared_steps = n_min / KPS;
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
    // the steps behind them, up to nsteps (few -- the heads of a sequence end within 15 keys of each other, two whole steps of 16 keys and
    // a partial one at the worst -- which is why one load at a time is affordable: a remark on speed, nothing depends on the count):
    // a key beyond nv[h] holds
    // another token's real data, with any bits, so it is left out by a SELECT on the accumulator, never by a factor 0
    for (int s0 = shared_steps; s0 < nsteps; ++s0) {
      const int kl = s0 * KPS + wave * KPW + grp;
      const Packed8 vr = *reinterpret_cast<const Packed8*>(vc + ((unsigned long long)(unsigned)slots[kl] * a.slot_stride + head_off));
      float vf[8];
      widen8<OT>(vr, vf);
#pragma unroll
      for (int h = 0; h < GC; ++h) {
        const bool mine = kl < nvl[h];  // (from LDS: eight more scalars held across the loops do not fit)
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
__global__ void __launch_bounds__(D) sqllm_attn_append_combine_kernel(const AttnAppendArgs a) {
  const int hq = blockIdx.x, row = blockIdx.y, d = threadIdx.x;
  const int b = row / a.q_len, tok = row - b * a.q_len;
  OT* const out = reinterpret_cast<OT*>(a.out) + (long long)row * a.out_stride + (long long)hq * D;
  const int len = append_row_len(a.q_lens ? a.q_lens[b] : a.q_len, a.seq_lens[b], tok, a.q_len, a.capacity);
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

struct AttnAppendTag : AttnTokens {
  static constexpr bool fp8 = false;
  template <int D, int GC, typename OT>
  static auto kernel() { return sqllm_attn_append_kernel<D, GC, OT>; }
  template <int D, typename OT>
  static auto combine_kernel() { return sqllm_attn_append_combine_kernel<D, OT>; }
};

// the combine alone: behind this file's partials, and behind those of sqllm_attn_append_fp8.hip
static hipError_t launch_attn_combine_tokens(const AttnAppendArgs& k, int head_dim, bool bf16, hipStream_t stream) {
  return launch_attn_combine<AttnAppendTag>(k, head_dim, bf16, dim3(k.n_q_heads, k.batch * k.q_len), stream);
}

// the host layer reaches the launcher through its slot of g_launch_attn (sqllm_kernels.h), so that it links without this file too
static const bool g_attn_append_registered = (g_launch_attn[kAttnAppend] = launch_attn<AttnAppendTag>, g_launch_attn_append_combine = launch_attn_combine_tokens, true);

}  // namespace sqllm
