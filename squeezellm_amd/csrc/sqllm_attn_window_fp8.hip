// sqllm_attn_window_fp8.hip -- decode attention over the LAST `window` keys of each row of a KV cache of 1-byte OCP e4m3fn
// elements with one fp32 scale per cache (include/sqllm_hip.h: sqllm_attn_decode_window_fp8_f16 / _bf16; the suffix names the
// type of q and out).  The partial kernel of sqllm_attn_decode_fp8.hip with the lower bound of sqllm_attn_window.hip (its BODY is
// a copy, edited; helpers and the launch ladder are shared: sqllm_attn.h): that file's lanes, loads, scales and reduction order,
// this family's geometry -- win_parts workgroups per (kv head, row), workgroup x on the ABSOLUTE partition lo / 256 + x, phase 0
// over the attended keys only, whole rounds below k_lo skipped, partials at the RELATIVE partition index -- and, with more than
// one partition, the SAME combine kernel as the 16-bit window file behind it, reached through g_launch_attn_window_combine (it
// does not see the cache).
//
// A row with L <= window holds the bits of sqllm_attn_decode_fp8_*; the shift identity holds as for the 16-bit caches.
//
// Registers and LDS as sqllm_attn_decode_fp8.hip: no scratch, no spills, two workgroups per CU at least
// (tests/test_codegen_attn_window_cpu.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sqllm_attn.h"
#include "sqllm_decode.h"
#include "sqllm_kernels.h"

namespace sqllm {

// (the lane helpers of the byte caches and the launch ladder: sqllm_attn.h)

template <int D, int GC, typename OT>
__global__ void __launch_bounds__(kAttnThreads) sqllm_attn_window_fp8_kernel(const AttnWindowArgs a, const float v_scale) {
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

  const int rel = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
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
  const int lo = len > a.window ? len - a.window : 0;  // the first attended key
  const int part = lo / P + rel;                       // the ABSOLUTE partition
  if (part > (len - 1) / P) return;                    // (before part * P: it is below 2^31 from here on)
  const int p0 = part * P;
  const int n_valid = len - p0 < P ? len - p0 : P;
  const int k_lo = lo > p0 ? lo - p0 : 0;  // the keys [k_lo, n_valid) of the partition are attended; k_lo < n_valid

  // 0. the slots of this partition's ATTENDED keys; every other thread takes the first attended key's
  {
    const unsigned p = tid >= k_lo && tid < n_valid ? p0 + tid : p0 + k_lo;
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
          const long long at = ((long long)b * a.n_q_heads + hk * g + i / D) * a.n_parts + rel;
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
  const int s_lo = STEPS > U ? k_lo / (KPS * U) * U : 0;  // whole rounds below k_lo: nothing of them is attended (one round: none)
  const unsigned long long head_off = (unsigned long long)(unsigned)hk * a.head_stride + (unsigned)(sub * E);

  // 1. scores
  {
    float qf[GC][E];
    const OT* q = reinterpret_cast<const OT*>(a.q) + (long long)b * a.q_stride + (long long)hk * g * D + sub * E;
#pragma unroll
    for (int h = 0; h < GC; ++h) {
      if (h < g) {
        widen8<OT>(*reinterpret_cast<const Packed8*>(q + h * D), qf[h]);
        widen8<OT>(*reinterpret_cast<const Packed8*>(q + h * D + 8), qf[h] + 8);
      } else {
#pragma unroll
        for (int j = 0; j < E; ++j) qf[h][j] = 0.0f;
      }
    }
    const uint8_t* kc = reinterpret_cast<const uint8_t*>(a.k_cache);
    for (int s0 = s_lo; s0 < nsteps; s0 += U) {
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
          if (h < GC) sc[h][kl] = kl >= k_lo && kl < n_valid ? a.scale * mine[r] : -__builtin_inff();
        }
      }
    }
  }
  __syncthreads();

  // 2. the partition's softmax, one wave per head; every entry of sc[h] is written, whatever phase 1 left (or skipped) there
  for (int h = wave; h < g; h += 4) {
    float s[P / 64], m = -__builtin_inff();
#pragma unroll
    for (int i = 0; i < P / 64; ++i) {
      const int kl = lane + 64 * i;
      s[i] = kl >= k_lo && kl < n_valid ? sc[h][kl] : -__builtin_inff();
      m = fmaxf(m, s[i]);
    }
    m = wave_max(m);
    float l = 0.0f;
#pragma unroll
    for (int i = 0; i < P / 64; ++i) {
      const int kl = lane + 64 * i;
      const float w = kl >= k_lo && kl < n_valid ? expf(s[i] - m) : 0.0f;
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
    for (int s0 = s_lo; s0 < nsteps; s0 += U) {
      Bytes16 vr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        vr[u] = *reinterpret_cast<const Bytes16*>(vc + ((unsigned long long)(unsigned)slots[kl] * a.slot_stride + head_off));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        const bool valid = kl >= k_lo && kl < n_valid;
        if (!valid) {  // (the stand-in slot's values: 0 x NaN would be NaN; a zero byte is +0)
#pragma unroll
          for (int i = 0; i < 4; ++i) vr[u].w[i] = 0u;
        }
        float vf[E];
        widen_e4m3(vr[u], vf);
#pragma unroll
        for (int h = 0; h < GC; ++h) {
          const float w = h < g && valid ? sc[h][kl] : 0.0f;
#pragma unroll
          for (int j = 0; j < E; ++j) acc[h][j] = fmaf(w, vf[j], acc[h][j]);
        }
      }
    }
  }

  // 4. the key-lanes meet, HC heads per round, in ascending key-lane order; v_scale once per element of the sum
#pragma unroll
  for (int h0 = 0; h0 < GC; h0 += HC) {
    if (h0 >= g) break;  // (uniform)
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
      if (h >= g) break;
      float t = red[0][hh][d];
#pragma unroll
      for (int k = 1; k < KPS; ++k) t += red[k][hh][d];
      t *= v_scale;
      if (single) {
        out[h * D + d] = (OT)(t / ml[h][1]);
      } else {
        const long long pa = ((long long)b * a.n_q_heads + hk * g + h) * a.n_parts + rel;
        a.ws_acc[pa * D + d] = t;
        if (d == 0) {
          a.ws_ml[pa * 2] = ml[h][0];
          a.ws_ml[pa * 2 + 1] = ml[h][1];
        }
      }
    }
  }
}

struct AttnWindowFp8Tag : AttnWindowQuery {  // (no combine of its own: g_launch_attn_window_combine, the 16-bit window file's)
  static constexpr bool fp8 = true;
  template <int D, int GC, typename OT>
  static auto kernel() { return sqllm_attn_window_fp8_kernel<D, GC, OT>; }
};

// the host layer reaches the launcher through its slot of g_launch_attn_window (sqllm_kernels.h), so that it links without this file too
static const bool g_attn_window_fp8_registered = (g_launch_attn_window[1] = launch_attn<AttnWindowFp8Tag>, true);

}  // namespace sqllm
