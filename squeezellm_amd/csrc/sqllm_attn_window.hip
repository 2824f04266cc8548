// sqllm_attn_window.hip -- decode attention (one new query per sequence) over the LAST `window` keys of each row
// (include/sqllm_hip.h: sqllm_attn_decode_window_f16 / _bf16): a row of length L attends the keys [lo, L), lo = max(0, L - window).
// The kernels of sqllm_attn_decode.hip with a lower bound (their BODIES are copies, edited; the lane helpers and the launch
// ladder are shared: sqllm_attn.h), sized by the window and not by the table's capacity.
//
// What differs from sqllm_attn_decode.hip:
//   * the grid has win_parts = min(n_parts, (window - 1 + 255) / 256 + 1) workgroups per (kv head, row) -- all a window can touch
//     -- and workgroup x of row b serves the ABSOLUTE partition lo_b / 256 + x, lo_b read from seq_lens on the device.  The
//     partitions stay the key ranges [256 i, 256 i + 256): the order of every sum depends on head_dim, the group class and the
//     key's index alone, so a row with L <= window holds the bits of sqllm_attn_decode_*, and a row whose lo is a multiple of 256
//     and of block_size those of the shorter row over the advanced table.
//   * k_lo = max(lo - p0, 0) joins n_valid as a uniform value: the keys kl in [k_lo, n_valid) of the partition are attended.
//     Phase 0 resolves table entries for those keys only; every other thread takes the slot of key p0 + k_lo (an attended one),
//     so entries behind the window may hold anything, and every slot the loops load from has passed the [0, n_slots) check.
//     Scores outside the range are -inf, the softmax masks the same range, V loads outside it are zeroed.
//   * whole rounds of kAttnUnroll steps below k_lo are skipped (up to 255 keys of a row's first partition are unattended): acc is
//     +0 there and fmaf(0, 0, +0) is +0, so what remains is bit for bit what the full walk leaves; the key-to-lane map is
//     untouched.
//   * the partials go to the workspace at the RELATIVE partition index x; the combine folds ceil(L / 256) - lo / 256 of them in
//     ascending order and writes the +0 and NaN rows.  With win_parts == 1 (a table of one partition, or window == 1) the partial
//     kernel is the whole call.
//
// Registers and LDS as sqllm_attn_decode.hip: no scratch, no spills, two workgroups per CU at least
// (tests/test_codegen_attn_window_cpu.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sqllm_attn.h"
#include "sqllm_decode.h"
#include "sqllm_kernels.h"

namespace sqllm {

// (AttnWindowArgs, the kernels' argument: sqllm_kernels.h; the lane helpers and the launch ladder: sqllm_attn.h)

template <int D, int GC, typename OT>
__global__ void __launch_bounds__(kAttnThreads) sqllm_attn_window_kernel(const AttnWindowArgs a) {
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
    for (int s0 = s_lo; s0 < nsteps; s0 += U) {
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
        if (sub < GC) sc[sub][kl] = kl >= k_lo && kl < n_valid ? a.scale * mine : -__builtin_inff();
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
  float acc[GC][8];
#pragma unroll
  for (int h = 0; h < GC; ++h)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[h][j] = 0.0f;
  {
    const OT* vc = reinterpret_cast<const OT*>(a.v_cache);
    for (int s0 = s_lo; s0 < nsteps; s0 += U) {
      Packed8 vr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        vr[u] = *reinterpret_cast<const Packed8*>(vc + ((unsigned long long)(unsigned)slots[kl] * a.slot_stride + head_off));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        const bool valid = kl >= k_lo && kl < n_valid;
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

template <int D, typename OT>
__global__ void __launch_bounds__(D) sqllm_attn_window_combine_kernel(const AttnWindowArgs a) {
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
  const int lo = len > a.window ? len - a.window : 0;
  const int np = (len - 1) / kAttnPartition + 1 - lo / kAttnPartition;  // the row's partitions, at most win_parts = a.n_parts
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

struct AttnWindowTag : AttnWindowQuery {
  static constexpr bool fp8 = false;
  template <int D, int GC, typename OT>
  static auto kernel() { return sqllm_attn_window_kernel<D, GC, OT>; }
  template <int D, typename OT>
  static auto combine_kernel() { return sqllm_attn_window_combine_kernel<D, OT>; }
};

// the combine alone: behind this file's partials, and behind those of sqllm_attn_window_fp8.hip
static hipError_t launch_attn_window_combine_rows(const AttnWindowArgs& k, int head_dim, bool bf16, int batch, hipStream_t stream) {
  return launch_attn_combine<AttnWindowTag>(k, head_dim, bf16, dim3(k.n_q_heads, batch), stream);
}

// the host layer reaches the launcher through its slot of g_launch_attn_window (sqllm_kernels.h), so that it links without this file too
static const bool g_attn_window_registered = (g_launch_attn_window[0] = launch_attn<AttnWindowTag>, g_launch_attn_window_combine = launch_attn_window_combine_rows, true);

}  // namespace sqllm
