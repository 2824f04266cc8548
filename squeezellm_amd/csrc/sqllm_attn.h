// sqllm_attn.h -- what the six decode-attention kernel files share (sqllm_attn_decode.hip, sqllm_attn_decode_fp8.hip,
// sqllm_attn_append.hip, sqllm_attn_append_fp8.hip, sqllm_attn_window.hip, sqllm_attn_window_fp8.hip): the lane helpers for 16-bit elements and for byte caches, the length of an append
// row and phase 0 of the append kernels, and the launch ladder launch_attn<TAG>.  NOT shared: the bodies of the partial kernels
// and of the combines, which stay copies of each other ("Not shared either").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sqllm_decode.h"
#include "sqllm_kernels.h"

namespace sqllm {

constexpr int kAttnThreads = 256;
constexpr int kAttnUnroll = 4;  // 16-byte loads in flight per lane before the first use
static_assert(kAttnPartition == kAttnThreads, "phase 0 resolves one key per thread");

// ------------------------------------------------------------------------------------------------
// 16-bit elements: the caches of the 16-bit files, and q everywhere
// ------------------------------------------------------------------------------------------------
// 16 bytes of 16-bit elements that are aligned to their elements only
struct __attribute__((packed, aligned(2))) Packed8 {
  uint32_t w[4];
};

template <typename OT>
__device__ __forceinline__ void widen8(const Packed8& p, float* f) {  // -> f[0 .. 8)
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
__device__ __forceinline__ float key_sum(float v) {
  v += dpp_f32<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
  v += dpp_f32<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
  v += dpp_f32<0x141, 0xf>(v);  // row_half_mirror: the other quad of the 8 lanes
  if constexpr (LPK == 16) v += dpp_f32<0x140, 0xf>(v);  // row_mirror: the other half of the row
  return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

// ------------------------------------------------------------------------------------------------
// caches of 1-byte e4m3fn elements (q is 16-bit: widen8, twice per lane; the wave's maximum: wave_max)
// ------------------------------------------------------------------------------------------------
// 16 bytes that are aligned to one byte only
struct __attribute__((packed, aligned(1))) Bytes16 {
  uint32_t w[4];
};

// 16 e4m3fn bytes as fp32 (a NaN byte is a NaN)
__device__ __forceinline__ void widen_e4m3(const Bytes16& p, float (&f)[16]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)p.w[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)p.w[i], true);
    f[4 * i] = lo[0];
    f[4 * i + 1] = lo[1];
    f[4 * i + 2] = hi[0];
    f[4 * i + 3] = hi[1];
  }
}

// the sum over the LPK lanes of a key, in every one of them (a + b and b + a: the same bits on both sides of each exchange)
template <int LPK>
__device__ __forceinline__ float key_sum_fp8(float v) {
  static_assert(LPK == 4 || LPK == 8, "head_dim 64 or 128");
  v += dpp_f32<0xB1, 0xf>(v);  // quad_perm [1,0,3,2]
  v += dpp_f32<0x4E, 0xf>(v);  // quad_perm [2,3,0,1]
  if constexpr (LPK == 8) v += dpp_f32<0x141, 0xf>(v);  // row_half_mirror: the other quad of the 8 lanes
  return v;
}

// ------------------------------------------------------------------------------------------------
// several new tokens per sequence (sqllm_attn_append.hip, sqllm_attn_append_fp8.hip)
// ------------------------------------------------------------------------------------------------
// The keys new token t attends, L(b, t) of include/sqllm_hip.h (sqllm_attn_append), in [1, capacity], from the sequence's
// n = q_lens[b] (or q_len) and seq = seq_lens[b]; 0 for a row that is +0 (padding: t >= n; L <= 0); -1 for a row that is NaN
// (n > q_len; L > capacity).  64-bit: seq is any int32.
__device__ __forceinline__ int append_row_len(int n, int seq, int t, int q_len, int capacity) {
  if (n > q_len) return -1;
  if (t >= n) return 0;
  const long long len = (long long)seq - (n - 1 - t);
  if (len <= 0) return 0;
  if (len > capacity) return -1;
  return (int)len;
}

// virtual head vh of (kv head hk, sequence b): new token vh / group, query head vh % group of the kv head's group
struct AppendHead {
  int row, head;  // the row of q / out, the query head
};
__device__ __forceinline__ AppendHead append_head(const AttnAppendArgs& a, int hk, int b, int vh) {
  const int t = (unsigned)vh / (unsigned)a.group;
  return {b * a.q_len + t, hk * a.group + (vh - t * a.group)};
}

// Phase 0 of a partial workgroup: (partition `part`, kv head `hk`, sequence `b`, `chunk` of GC virtual heads).  Virtual head
// chunk * GC + h is (new token t, query head hh of the group), tokens first; it ends up as
//   nv[h]            the keys of THIS partition it attends, 0 when it is not served here: no such token, a +0 or NaN row (with one
//                    partition written here, otherwise the combine's), a row that ends below the partition, or a row that meets
//                    a table entry outside [0, n_slots) in this partition (NaN written here: the one-query kernel's partial).
// slots[0 .. kAttnPartition) are resolved once, for the longest of them; keys at or above n_max take the slot of the partition's
// first key (an attended one).  nvl[h] = nv[h] in LDS, for whoever indexes it by a runtime h.  False: nothing left to do.
template <int D, int GC, typename OT>
__device__ __forceinline__ bool append_phase0(const AttnAppendArgs& a, int part, int hk, int b, int chunk, int* slots, int* first_bad, int* nvl,
                                              int (&nv)[GC], int& n_max, int& n_min) {
  constexpr int P = kAttnPartition;
  const int tid = threadIdx.x, g = a.group, p0 = part * P;
  const bool single = a.n_parts == 1;
  OT* const out = reinterpret_cast<OT*>(a.out);
  const int n = a.q_lens ? a.q_lens[b] : a.q_len, seq = a.seq_lens[b];
  int t = __builtin_amdgcn_readfirstlane(chunk * GC / g), hh = chunk * GC - t * g;  // (a uniform quotient: back to a scalar)
  n_max = 0;
#pragma unroll
  for (int h = 0; h < GC; ++h) {
    nv[h] = 0;
    if (t < a.q_len) {
      const int len = append_row_len(n, seq, t, a.q_len, a.capacity);
      if (len > p0) nv[h] = len - p0 < P ? len - p0 : P;
    }
    n_max = nv[h] > n_max ? nv[h] : n_max;
    if (++hh == g) {
      hh = 0;
      ++t;
    }
  }
  if (single) {  // this launch is the whole call: the +0 and the NaN rows (otherwise the combine writes them).  A loop that
                 // stays a loop: eight heads' addresses at once cost scalar registers the kernels do not have
#pragma unroll 1
    for (int h = 0; h < GC; ++h) {
      const int vh = chunk * GC + h, tok = __builtin_amdgcn_readfirstlane(vh / g);
      if (tok >= a.q_len) break;
      const int len = append_row_len(n, seq, tok, a.q_len, a.capacity);
      if (len > 0) continue;
      const OT c = len == 0 ? (OT)0.0f : (OT)__builtin_nanf("");
      OT* const o = out + (long long)(b * a.q_len + tok) * a.out_stride + (long long)(hk * g + vh - tok * g) * D;
      for (int i = tid; i < D; i += kAttnThreads) o[i] = c;
    }
  }
  if (n_max == 0) return false;

  const unsigned p = tid < n_max ? p0 + tid : p0;
  const unsigned blk = p / (unsigned)a.block_size, off = p - blk * (unsigned)a.block_size;
  const long long s = (long long)a.block_table[(long long)b * a.table_stride + blk] * a.block_size + off;
  const bool bad = s < 0 || s >= a.n_slots;
  slots[tid] = (int)s;
  int fb = P;  // the lowest key of the partition with a bad entry
  if (__syncthreads_or(bad)) {
    if (tid == 0) *first_bad = P;
    __syncthreads();
    if (bad) atomicMin(first_bad, tid < n_max ? tid : 0);
    __syncthreads();
    fb = __builtin_amdgcn_readfirstlane(*first_bad);
  }
  n_max = 0;
  n_min = P;
  unsigned nan_heads = 0;  // the heads that meet the bad entry: NaN, and nothing of the caches is read for them
#pragma unroll
  for (int h = 0; h < GC; ++h) {
    if (nv[h] > fb) {
      nan_heads |= 1u << h;
      nv[h] = 0;
    }
    if (nv[h] > 0) {
      n_max = nv[h] > n_max ? nv[h] : n_max;
      n_min = nv[h] < n_min ? nv[h] : n_min;
    }
    if (tid == h) nvl[h] = nv[h];
  }
#pragma unroll 1
  for (int h = 0; nan_heads >> h; ++h) {  // (a loop that stays a loop, as above)
    if (!(nan_heads >> h & 1)) continue;
    const float nan = __builtin_nanf("");
    const AppendHead v = append_head(a, hk, b, chunk * GC + h);
    if (single) {
      OT* const o = out + (long long)v.row * a.out_stride + (long long)v.head * D;
      for (int i = tid; i < D; i += kAttnThreads) o[i] = (OT)nan;
    } else {
      const long long at = ((long long)v.row * a.n_q_heads + v.head) * a.n_parts + part;
      for (int i = tid; i < D; i += kAttnThreads) {
        a.ws_acc[at * D + i] = nan;
        if (i == 0) {
          a.ws_ml[at * 2] = 0.0f;
          a.ws_ml[at * 2 + 1] = nan;
        }
      }
    }
  }
  if (n_max == 0) return false;
  if (tid >= n_max) slots[tid] = slots[0];  // (n_max <= fb: key 0 of the partition is a good one)
  __syncthreads();
  return true;
}

// ------------------------------------------------------------------------------------------------
// The launch ladder of the six kernel files, written once (as launch_front<TAG> of sqllm_fused.h): {_Float16, __bf16} x head_dim
// 64 / 128 x group class 1 / 2 / 3-4 / 8 -> one instantiation of the partial kernel TAG names; with more than one partition the
// combine behind it.  A kernel file says
//   struct MyAttn : AttnOneQuery {   // or AttnTokens: several new tokens per sequence
//     static constexpr bool fp8 = ...;  // the kernel takes v_scale behind its argument block
//     template <int D, int GC, typename OT> static auto kernel() { return my_kernel<D, GC, OT>; }
//   };
// and registers launch_attn<MyAttn> in its slot of g_launch_attn.  The combines are reached through their hooks by EVERY tag, the
// 16-bit ones too: the hook is not optional for a 16-bit file -- it sets the hook in the same statement as its launcher, so the
// check below is always true for it, and with more than one partition it pays one indirect call and the combine's own
// type x head_dim ladder on the host (it used to launch its combine directly; the device code is the same).  For the byte
// caches a missing combine is an error before anything is launched.
// ------------------------------------------------------------------------------------------------
struct AttnOneQuery {
  typedef AttnArgs Args;
  static bool served(const AttnCall&) { return true; }
  static int heads(const Args& k) { return k.group; }  // the heads a (kv head, row) serves from one read of K and V
  template <int GC>
  static dim3 grid(const Args& k, const AttnCall& c) { return dim3(k.n_parts, c.n_kv_heads, c.batch); }
  static bool has_combine() { return g_launch_attn_combine != nullptr; }
  static hipError_t combine(const Args& k, const AttnCall& c, hipStream_t stream) { return g_launch_attn_combine(k, c.head_dim, c.bf16, c.batch, stream); }
};
struct AttnTokens {
  typedef AttnAppendArgs Args;
  static bool served(const AttnCall& c) { return c.q_len >= 1 && c.q_len <= 16; }
  static int heads(const Args& k) { return k.q_len * k.group; }  // the virtual heads of a (kv head, sequence)
  // chunks of GC virtual heads: the slowest grid dimension, so that the workgroups which read the same keys lie
  // n_parts * n_kv_heads * batch apart in linear id (on one XCD where that product is a multiple of 8: 16 partitions of a 4096-key
  // capacity are, 9 partitions of one kv head and one sequence are not; no other order was measured)
  template <int GC>
  static dim3 grid(const Args& k, const AttnCall& c) { return dim3(k.n_parts, c.n_kv_heads, k.batch * ((k.q_len * k.group + GC - 1) / GC)); }
  static bool has_combine() { return g_launch_attn_append_combine != nullptr; }
  static hipError_t combine(const Args& k, const AttnCall& c, hipStream_t stream) { return g_launch_attn_append_combine(k, c.head_dim, c.bf16, stream); }
};
// one query per sequence over the last `window` keys: win_parts (k.n_parts) workgroups per (kv head, row), the window combine
struct AttnWindowQuery {
  typedef AttnWindowArgs Args;
  static bool served(const AttnCall& c) { return c.window >= 1 && c.q_len == 0; }
  static int heads(const Args& k) { return k.group; }
  template <int GC>
  static dim3 grid(const Args& k, const AttnCall& c) { return dim3(k.n_parts, c.n_kv_heads, c.batch); }
  static bool has_combine() { return g_launch_attn_window_combine != nullptr; }
  static hipError_t combine(const Args& k, const AttnCall& c, hipStream_t stream) { return g_launch_attn_window_combine(k, c.head_dim, c.bf16, c.batch, stream); }
};

template <typename TAG, int D, int GC, typename OT>
inline hipError_t launch_attn_inst(const typename TAG::Args& k, const AttnCall& c, hipStream_t stream) {
  if (k.n_parts > 1 && !TAG::has_combine()) return hipErrorNotSupported;  // (a missing kernel is an error, before anything is launched)
  auto kern = TAG::template kernel<D, GC, OT>();
  if constexpr (TAG::fp8) hipLaunchKernelGGL(kern, TAG::template grid<GC>(k, c), dim3(kAttnThreads), 0, stream, k, c.v_scale);
  else hipLaunchKernelGGL(kern, TAG::template grid<GC>(k, c), dim3(kAttnThreads), 0, stream, k);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || k.n_parts == 1) return e;
  return TAG::combine(k, c, stream);
}

template <typename TAG, int D, typename OT>
inline hipError_t launch_attn_group(const typename TAG::Args& k, const AttnCall& c, hipStream_t stream) {
  switch (TAG::heads(k)) {
    case 1: return launch_attn_inst<TAG, D, 1, OT>(k, c, stream);
    case 2: return launch_attn_inst<TAG, D, 2, OT>(k, c, stream);
    case 3: case 4: return launch_attn_inst<TAG, D, 4, OT>(k, c, stream);
    default: return launch_attn_inst<TAG, D, 8, OT>(k, c, stream);
  }
}

template <typename TAG>
inline hipError_t launch_attn(const AttnCall& c, hipStream_t stream) {
  if ((c.head_dim != 64 && c.head_dim != 128) || c.n_kv_heads < 1 || c.n_q_heads % c.n_kv_heads || c.n_q_heads / c.n_kv_heads > 8 ||
      c.batch < 1 || c.n_parts < 1 || !TAG::served(c))
    return hipErrorInvalidValue;
  const typename TAG::Args k = make_attn_args<typename TAG::Args>(c);
  if (c.bf16) return c.head_dim == 64 ? launch_attn_group<TAG, 64, __bf16>(k, c, stream) : launch_attn_group<TAG, 128, __bf16>(k, c, stream);
  return c.head_dim == 64 ? launch_attn_group<TAG, 64, _Float16>(k, c, stream) : launch_attn_group<TAG, 128, _Float16>(k, c, stream);
}

// The combine alone, behind the partials of either cache type: TAG names the combine kernel template of a 16-bit file
// (template <int D, typename OT> static auto combine_kernel()), `grid` is (query heads, rows).
template <typename TAG>
inline hipError_t launch_attn_combine(const typename TAG::Args& k, int head_dim, bool bf16, dim3 grid, hipStream_t stream) {
  if (head_dim != 64 && head_dim != 128) return hipErrorInvalidValue;
  if (head_dim == 64) {
    if (bf16) hipLaunchKernelGGL((TAG::template combine_kernel<64, __bf16>()), grid, dim3(64), 0, stream, k);
    else hipLaunchKernelGGL((TAG::template combine_kernel<64, _Float16>()), grid, dim3(64), 0, stream, k);
  } else {
    if (bf16) hipLaunchKernelGGL((TAG::template combine_kernel<128, __bf16>()), grid, dim3(128), 0, stream, k);
    else hipLaunchKernelGGL((TAG::template combine_kernel<128, _Float16>()), grid, dim3(128), 0, stream, k);
  }
  return hipGetLastError();
}

}  // namespace sqllm
