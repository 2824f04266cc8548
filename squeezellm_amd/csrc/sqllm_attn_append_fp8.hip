// sqllm_attn_append_fp8.hip -- decode attention for several new tokens per sequence over a KV cache of 1-byte OCP e4m3fn elements
// (include/sqllm_hip.h: sqllm_attn_append_fp8_f16 / _bf16; the suffix names the type of q and out).  Row (b, t) holds the bits
// sqllm_attn_decode_fp8_* gives a row with table row b and length L(b, t).  The BODY of the partial kernel of sqllm_attn_decode_fp8.hip,
// copied (the lane helpers, phase 0 and the launch ladder are not copies: sqllm_attn.h), with the virtual heads of sqllm_attn_append.hip (phases 0 to 4 are described there, the lanes and the 16 elements per lane in
// sqllm_attn_decode_fp8.hip); with more than one partition the combine of sqllm_attn_append.hip follows, reached through
// g_launch_attn_append_combine (it does not see the cache).  k_scale is folded into the score's scale on the host; v_scale
// multiplies each partition's sum over the keys once per (virtual head, d).
//
// Registers: q (8 x 16 fp32) lives in phase 1 only, acc (8 x 16 fp32) in phase 3 only; the launch bound asks for two waves per
// SIMD (256 registers); the instance of 8 virtual heads takes 172 (head_dim 64) and 239 (head_dim 128) with the early-out of the
// shared PV loop -- per-step masks there took it beyond 256: no scratch, no spills, two workgroups per CU
// (tests/test_codegen_attn_append_cpu.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sqllm_attn.h"
#include "sqllm_decode.h"
#include "sqllm_kernels.h"

namespace sqllm {

template <int D, int GC, typename OT>
__global__ void __launch_bounds__(kAttnThreads, 2) sqllm_attn_append_fp8_kernel(const AttnAppendArgs a, const float v_scale) {
  constexpr int P = kAttnPartition;
  constexpr int E = 16;              // elements (bytes) per lane and key
  constexpr int LPK = D / E;         // lanes per key
  constexpr int KPW = 64 / LPK;      // keys per wave instruction
  constexpr int KPS = KPW * 4;       // keys per step of the workgroup
  constexpr int STEPS = P / KPS;
  constexpr int U = kAttnUnroll;
  constexpr int HC = GC < 2 ? GC : 2;          // heads per round of the key-lane exchange
  constexpr int R = (GC + LPK - 1) / LPK;      // heads whose score one lane of a key stores
  static_assert(STEPS % U == 0, "whole unrolled rounds");
  static_assert(KPS * HC * D * 4 <= 32 * 1024, "the exchange");
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
  const int nsteps = (n_max + KPS - 1) / KPS;
  const unsigned long long head_off = (unsigned long long)(unsigned)hk * a.head_stride + (unsigned)(sub * E);

  // 1. scores
  {
    float qf[GC][E];
#pragma unroll
    for (int h = 0; h < GC; ++h) {
      if (nv[h] > 0) {
        const AppendHead v = append_head(a, hk, b, chunk * GC + h);
        const OT* q = reinterpret_cast<const OT*>(a.q) + (long long)v.row * a.q_stride + (long long)v.head * D + sub * E;
        widen8<OT>(*reinterpret_cast<const Packed8*>(q), qf[h]);
        widen8<OT>(*reinterpret_cast<const Packed8*>(q + 8), qf[h] + 8);
      } else {
#pragma unroll
        for (int j = 0; j < E; ++j) qf[h][j] = 0.0f;
      }
    }
    const uint8_t* kc = reinterpret_cast<const uint8_t*>(a.k_cache);
    for (int s0 = 0; s0 < nsteps; s0 += U) {
      Bytes16 kr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        kr[u] = *reinterpret_cast<const Bytes16*>(kc + ((unsigned long long)(unsigned)slots[kl] * a.slot_stride + head_off));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        float kf[E];
        widen_e4m3(kr[u], kf);
        float mine[R];
#pragma unroll
        for (int r = 0; r < R; ++r) mine[r] = 0.0f;
#pragma unroll
        for (int h = 0; h < GC; ++h) {
          float dot = qf[h][0] * kf[0];
#pragma unroll
          for (int j = 1; j < E; ++j) dot = fmaf(qf[h][j], kf[j], dot);
          dot = key_sum_fp8<LPK>(dot);
          if (sub == h % LPK) mine[h / LPK] = dot;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int h = sub + r * LPK;
          if (h < GC) sc[h][kl] = kl < nvl[h] ? a.scale * mine[r] : -__builtin_inff();
        }
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
  float acc[GC][E];
#pragma unroll
  for (int h = 0; h < GC; ++h)
#pragma unroll
    for (int j = 0; j < E; ++j) acc[h][j] = 0.0f;
  {
    const uint8_t* vc = reinterpret_cast<const uint8_t*>(a.v_cache);
    // the steps below the SHORTEST head's end: every key is every head's, and the loop is the sibling's (the steps behind them are
    // left out whole, which leaves what its fmaf(0, 0, acc) leaves)
    const int shared_steps = n_min / KPS;
    for (int s0 = 0; s0 < shared_steps; s0 += U) {
      Bytes16 vr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        vr[u] = *reinterpret_cast<const Bytes16*>(vc + ((unsigned long long)(unsigned)slots[kl] * a.slot_stride + head_off));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        if (s0 + u >= shared_steps) break;  // (uniform)
        float vf[E];
        widen_e4m3(vr[u], vf);
#pragma unroll
        for (int h = 0; h < GC; ++h) {
          const float w = sc[h][kl];  // (a head that is not served here gathers what nobody reads)
#pragma unroll
          for (int j = 0; j < E; ++j) acc[h][j] = fmaf(w, vf[j], acc[h][j]);
        }
      }
    }
    // the steps behind them, up to nsteps (few -- the heads of a sequence end within 15 keys of each other -- which is why one load at a
    // time is affordable: a remark on speed, nothing depends on the count): a key beyond nv[h] holds
    // another token's real data, with any bits, so it is left out by a SELECT on the accumulator, never by a factor 0
    for (int s0 = shared_steps; s0 < nsteps; ++s0) {
      const int kl = s0 * KPS + wave * KPW + grp;
      const Bytes16 vr = *reinterpret_cast<const Bytes16*>(vc + ((unsigned long long)(unsigned)slots[kl] * a.slot_stride + head_off));
      float vf[E];
      widen_e4m3(vr, vf);
#pragma unroll
      for (int h = 0; h < GC; ++h) {
        const bool mine = kl < nv[h];
        const float w = sc[h][kl];
#pragma unroll
        for (int j = 0; j < E; ++j) acc[h][j] = mine ? fmaf(w, vf[j], acc[h][j]) : acc[h][j];
      }
    }
  }

  // 4. the key-lanes meet, HC heads per round, in ascending key-lane order; v_scale once per element of the sum
#pragma unroll
  for (int h0 = 0; h0 < GC; h0 += HC) {
    if (h0) __syncthreads();
#pragma unroll
    for (int hh = 0; hh < HC; ++hh) {
      f32x4* at = reinterpret_cast<f32x4*>(&red[wave * KPW + grp][hh][sub * E]);
#pragma unroll
      for (int i = 0; i < E / 4; ++i)
        at[i] = f32x4{acc[h0 + hh][4 * i], acc[h0 + hh][4 * i + 1], acc[h0 + hh][4 * i + 2], acc[h0 + hh][4 * i + 3]};
    }
    __syncthreads();
    for (int i = tid; i < HC * D; i += kAttnThreads) {
      const int hh = i / D, d = i % D, h = h0 + hh;
      if (nvl[h] == 0) continue;
      const AppendHead v = append_head(a, hk, b, chunk * GC + h);
      float t = red[0][hh][d];
#pragma unroll
      for (int k = 1; k < KPS; ++k) t += red[k][hh][d];
      t *= v_scale;
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

struct AttnAppendFp8Tag : AttnTokens {  // (no combine of its own: g_launch_attn_append_combine, the 16-bit file's)
  static constexpr bool fp8 = true;
  template <int D, int GC, typename OT>
  static auto kernel() { return sqllm_attn_append_fp8_kernel<D, GC, OT>; }
};

// the host layer reaches the launcher through its slot of g_launch_attn (sqllm_kernels.h), so that it links without this file too
static const bool g_attn_append_fp8_registered = (g_launch_attn[kAttnAppendFp8] = launch_attn<AttnAppendFp8Tag>, true);

}  // namespace sqllm
