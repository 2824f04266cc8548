// sqllm_attn_append.h -- what the kernels of sqllm_attn_append.hip and sqllm_attn_append_fp8.hip share: the length of a row, and
// phase 0 of the partial kernels (the virtual heads of a workgroup, their rows that need no keys, the partition's slots).
#pragma once
#include <hip/hip_runtime.h>

#include "sqllm_kernels.h"

namespace sqllm {

constexpr int kAppendThreads = 256;
static_assert(kAttnPartition == kAppendThreads, "phase 0 resolves one key per thread");

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
      for (int i = tid; i < D; i += kAppendThreads) o[i] = c;
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
      for (int i = tid; i < D; i += kAppendThreads) o[i] = (OT)nan;
    } else {
      const long long at = ((long long)v.row * a.n_q_heads + v.head) * a.n_parts + part;
      for (int i = tid; i < D; i += kAppendThreads) {
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

}  // namespace sqllm
