// sqllm_attn_append.hip -- decode attention for SEVERAL new tokens per sequence in one read of K and V (include/sqllm_hip.h:
// sqllm_attn_append_f16 / _bf16).  Row (b, t) holds the bits sqllm_attn_decode_* gives a row with table row b and length
// L(b, t) = seq_lens[b] - (n_b - 1 - t): the kernels here are the ones of sqllm_attn_decode.hip, copied, with one change of
// meaning -- a workgroup's heads are VIRTUAL heads, (new token, query head of the kv group) pairs, each with its own length.
//
// Launch 1 (partials), one workgroup of 256 threads per (partition of kAttnPartition keys, kv head, sequence, chunk of up to 8
// virtual heads); the chunks of a (partition, kv head, sequence) read the same keys and are the slowest grid dimension:
//   0. (sqllm_attn_append.h) the chunk's virtual heads and the keys nv[h] of this partition each of them attends; rows that need no
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

#include "sqllm_attn_append.h"
#include "sqllm_decode.h"
#include "sqllm_kernels.h"

namespace sqllm {

constexpr int kAppendUnroll = 4;  // 16-byte loads in flight per lane before the first use

// 16 bytes of 16-bit elements that are aligned to their elements only
struct __attribute__((packed, aligned(2))) AppendPacked8 {
  uint32_t w[4];
};

template <typename OT>
__device__ __forceinline__ void append_widen8(const AppendPacked8& p, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (std::is_same<OT, __bf16>::value) {
      f[2 * i] = __builtin_bit_cast(float, p.w[i] << 16);
      f[2 * i + 1] = __builtin_bit_cast(float, p.w[i] & 0xffff0000u);
    } else {
      f[2 * i] = (float)__builtin_bit_cast(_Float16, (unsigned short)(p.w[i] & 0xffffu));
      f[2 * i + 1] = (float)__builtin_bit_cast(_Float16, (unsigned short)(p.w[i] >> 16));
    }
  }
}

// the sum over the LPK lanes of a key, in every one of them (a + b and b + a: the same bits on both sides of each exchange)
template <int LPK>
__device__ __forceinline__ float append_key_sum(float v) {
  v += dpp_f32<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
  v += dpp_f32<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
  v += dpp_f32<0x141, 0xf>(v);  // row_half_mirror: the other quad of the 8 lanes
  if constexpr (LPK == 16) v += dpp_f32<0x140, 0xf>(v);  // row_mirror: the other half of the row
  return v;
}

__device__ __forceinline__ float append_wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

template <int D, int GC, typename OT>
__global__ void __launch_bounds__(kAppendThreads) sqllm_attn_append_kernel(const AttnAppendArgs a) {
  constexpr int P = kAttnPartition;
  constexpr int LPK = D / 8;         // lanes per key
  constexpr int KPW = 64 / LPK;      // keys per wave instruction
  constexpr int KPS = KPW * 4;       // keys per step of the workgroup
  constexpr int STEPS = P / KPS;
  constexpr int U = kAppendUnroll;
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
        append_widen8<OT>(*reinterpret_cast<const AppendPacked8*>(q), qf[h]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[h][j] = 0.0f;
      }
    }
    const int my_nv = sub < GC ? nvl[sub < GC ? sub : 0] : 0;
    const OT* kc = reinterpret_cast<const OT*>(a.k_cache);
    for (int s0 = 0; s0 < nsteps; s0 += U) {
      AppendPacked8 kr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        kr[u] = *reinterpret_cast<const AppendPacked8*>(kc + ((unsigned long long)(unsigned)slots[kl] * a.slot_stride + head_off));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        float kf[8];
        append_widen8<OT>(kr[u], kf);
        float mine = 0.0f;
#pragma unroll
        for (int h = 0; h < GC; ++h) {
          float dot = qf[h][0] * kf[0];
#pragma unroll
          for (int j = 1; j < 8; ++j) dot = fmaf(qf[h][j], kf[j], dot);
          dot = append_key_sum<LPK>(dot);
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
    m = append_wave_max(m);
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
      AppendPacked8 vr[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        vr[u] = *reinterpret_cast<const AppendPacked8*>(vc + ((unsigned long long)(unsigned)slots[kl] * a.slot_stride + head_off));
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kl = (s0 + u) * KPS + wave * KPW + grp;
        if (s0 + u >= shared_steps) break;  // (uniform)
        float vf[8];
        append_widen8<OT>(vr[u], vf);
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
      const AppendPacked8 vr = *reinterpret_cast<const AppendPacked8*>(vc + ((unsigned long long)(unsigned)slots[kl] * a.slot_stride + head_off));
      float vf[8];
      append_widen8<OT>(vr, vf);
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
    for (int i = tid; i < HC * D; i += kAppendThreads) {
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

// the combine alone: behind this file's partials, and behind those of sqllm_attn_append_fp8.hip
static hipError_t launch_attn_append_combine(const AttnAppendArgs& k, int head_dim, bool bf16, hipStream_t stream) {
  if (head_dim != 64 && head_dim != 128) return hipErrorInvalidValue;
  const dim3 grid(k.n_q_heads, k.batch * k.q_len);
  if (head_dim == 64) {
    if (bf16) hipLaunchKernelGGL((sqllm_attn_append_combine_kernel<64, __bf16>), grid, dim3(64), 0, stream, k);
    else hipLaunchKernelGGL((sqllm_attn_append_combine_kernel<64, _Float16>), grid, dim3(64), 0, stream, k);
  } else {
    if (bf16) hipLaunchKernelGGL((sqllm_attn_append_combine_kernel<128, __bf16>), grid, dim3(128), 0, stream, k);
    else hipLaunchKernelGGL((sqllm_attn_append_combine_kernel<128, _Float16>), grid, dim3(128), 0, stream, k);
  }
  return hipGetLastError();
}

// chunks of GC virtual heads: the slowest grid dimension, so that the workgroups which read the same keys lie
// n_parts * n_kv_heads * batch apart in linear id (on one XCD where that product is a multiple of 8: 16 partitions of a 4096-key
// capacity are, 9 partitions of one kv head and one sequence are not; no other order was measured)
template <int D, int GC, typename OT>
static hipError_t launch_append_inst(const AttnAppendArgs& k, int n_kv_heads, bool bf16, hipStream_t stream) {
  const int chunks = (k.q_len * k.group + GC - 1) / GC;
  hipLaunchKernelGGL((sqllm_attn_append_kernel<D, GC, OT>), dim3(k.n_parts, n_kv_heads, k.batch * chunks), dim3(kAppendThreads), 0, stream, k);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || k.n_parts == 1) return e;
  return launch_attn_append_combine(k, D, bf16, stream);
}

template <int D, typename OT>
static hipError_t launch_append_group(const AttnAppendArgs& k, int n_kv_heads, bool bf16, hipStream_t stream) {
  switch (k.q_len * k.group) {  // the virtual heads of a (kv head, sequence)
    case 1: return launch_append_inst<D, 1, OT>(k, n_kv_heads, bf16, stream);
    case 2: return launch_append_inst<D, 2, OT>(k, n_kv_heads, bf16, stream);
    case 3: case 4: return launch_append_inst<D, 4, OT>(k, n_kv_heads, bf16, stream);
    default: return launch_append_inst<D, 8, OT>(k, n_kv_heads, bf16, stream);
  }
}

static hipError_t launch_attn_append(const AttnAppend& p, hipStream_t stream) {
  const AttnDecode& d = p.d;
  if ((d.head_dim != 64 && d.head_dim != 128) || d.n_kv_heads < 1 || d.n_q_heads % d.n_kv_heads || d.n_q_heads / d.n_kv_heads > 8 ||
      d.batch < 1 || d.n_parts < 1 || p.q_len < 1 || p.q_len > 16)
    return hipErrorInvalidValue;
  const AttnAppendArgs k = make_attn_append_args(p);
  if (d.bf16) return d.head_dim == 64 ? launch_append_group<64, __bf16>(k, d.n_kv_heads, true, stream) : launch_append_group<128, __bf16>(k, d.n_kv_heads, true, stream);
  return d.head_dim == 64 ? launch_append_group<64, _Float16>(k, d.n_kv_heads, false, stream) : launch_append_group<128, _Float16>(k, d.n_kv_heads, false, stream);
}

// the host layer reaches the launchers through these hooks (sqllm_kernels.h), so that it links without this file too
static const bool g_attn_append_registered = (g_launch_attn_append = launch_attn_append, g_launch_attn_append_combine = launch_attn_append_combine, true);

}  // namespace sqllm
