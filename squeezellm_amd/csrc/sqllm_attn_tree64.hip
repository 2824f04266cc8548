// sqllm_attn_tree64.hip -- decode attention for a TREE of up to 64 new tokens per sequence on the matrix cores, the keys split across
// workgroups (include/sqllm_hip.h: sqllm_attn_tree64_f16 / _bf16): the verification step of EAGLE-2 / Medusa sized trees.  Row (b, t)
// attends the context [0, C_b) and the nodes (keys C_b + j) whose bit j is set in its 64-bit word.  A tree of 64 nodes x a kv group
// is the shape sqllm_attn_prefill.hip was built for -- 64 (token, head of the group) rows against 64 keys per matrix tile -- so the
// lane maps, the LDS layouts (K [key][d] padded, V transposed on the way in), the double buffer with one barrier per key tile, the
// fp32 online softmax and the three 16-bit planes of the weights are THAT file's, described there.  Two things are new.
//
// The mask.  A lane reads its row's word once (tree64_word).  Per key tile the row's attended keys are one 64-bit value,
// tree64_tile_bits: the context part window_tile_bits(0, C_b, key0) and the word shifted by C_b - key0.  A key tile that lies wholly
// inside the context of every live row of a wave takes the loop without a select (tree64_tile<.., false>); only the at most two
// tiles that hold nodes -- and the one the context ends in -- select score and weight by bit, before the exponent: a masked score is
// -inf and a masked weight 0, whatever bits the key holds.
//
// The key split.  Grid x runs over (query tile, partition), y over the kv heads, z over the sequences; 4 waves.  Partition p is the
// ABSOLUTE keys [256 p, 256 p + 256) (kTree64Partition).  A workgroup walks the key tiles of its partition below Lmax, the largest
// Leff of its query tile; one whose partition begins at or beyond Lmax returns before it loads anything of the caches (lengths are
// device data, the grid is not).  With one partition (max_blocks * block_size <= 256) the workgroup finishes its rows itself, as the
// prefill kernel does.  Otherwise every row that reaches into the partition leaves (max, sum, acc[D]) in the workspace with vector
// stores -- a row that attends nothing there leaves (-inf, 0, 0): no inf - inf, the running maximum subtracts 0 until a key is
// attended -- and the combine kernel below, one wave per (row, query head), folds the partials of the partitions below the row's own
// Leff in ascending order, skips the -inf ones, undoes the fp16 planes' 2^15 once, applies v_scale (1 here) and rounds once; it
// writes the +0 and the NaN rows.  sqllm_attn_tree64_fp8.hip reaches it through g_launch_attn_tree64_combine.
//
// Bad table entries.  As the prefill kernel: wave 0 resolves the slots of the next tile, the walk of a partition stops behind the
// tile with the first entry outside [0, n_slots), keys at or beyond it are staged as zeros and never loaded, and a row whose Leff
// lies behind it is NaN (its partial carries a NaN sum).
//
// Bits depend on the row's own operands, its word, its lengths and the shape fields only: partitions and key tiles are absolute,
// the order inside a tile is the lane map's, the fold is ascending.  They are not the bits of the tree, append or prefill entries.
//
// Registers / LDS (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 4.4.  No scratch, two workgroups per CU.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sqllm_attn_tree64.h"

namespace sqllm {

// (built without packed fp32 arithmetic: build.NO_PACKED_FP32)
template <int D, typename OT>
__global__ void __launch_bounds__(kAttnThreads, 2) sqllm_attn_tree64_kernel(const AttnTree64Args a) {
  constexpr int KT = kPrefillTile, P = kTree64Partition;
  constexpr int KROW = D + 8;    // 16-bit elements per staged K row
  constexpr int VROW = KT + 8;   // 16-bit elements per row of V^T
  constexpr int DC = D / 8;      // 16-byte chunks per key row
  constexpr int KIT = KT * DC / kAttnThreads;        // K chunks per thread and tile
  constexpr int VIT = (KT / 2) * DC / kAttnThreads;  // V tasks (two keys x 8 d) per thread and tile
  constexpr int NDB = D / 16, NQC = D / 32;
  static_assert(KIT >= 1 && VIT >= 1 && KT == 64 && kAttnThreads == 256, "the lane maps below");
  __shared__ __attribute__((aligned(16))) uint16_t ks[2][KT * KROW];
  __shared__ __attribute__((aligned(16))) uint16_t vs[2][D * VROW];
  __shared__ int slots[2][KT];
  __shared__ int fb_tile[2];
  __shared__ int wave_len[4];

  const int part = (unsigned)blockIdx.x % (unsigned)a.n_parts;
  const int tile = a.n_tiles - 1 - (int)((unsigned)blockIdx.x / (unsigned)a.n_parts);
  const int hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, q4 = lane >> 4;
  const int g = a.group, T = a.q_len;
  const int p0 = part * P;  // (below the capacity: no overflow)
  // no Leff exceeds seq_lens[b]: most workgroups of a short sequence in a long table leave here, on one scalar load (uniform)
  if (a.n_parts > 1 && p0 >= a.seq_lens[b]) return;

  // this lane's query row: virtual row -> (token, head of the group), its word, its effective length and its context
  const int vrow = tile * KT + wave * 16 + l16;
  const int tok = (unsigned)vrow / (unsigned)g, hh = vrow - tok * g;
  const bool exists = tok < T;
  const int n = a.q_lens ? a.q_lens[b] : T, seq = a.seq_lens[b];
  unsigned long long word = exists ? tree64_word(a, b, tok, n) : 0ull;
  const int my_len = exists ? tree64_row_len(n, seq, tok, T, a.capacity, word) : 0;  // 0: +0 (or no row), -1: NaN
  const int ctx = my_len > 0 ? seq - n : 0;  // (a live row: seq >= n >= 1)
  word = my_len > 0 ? word : 0ull;
  const long long row = (long long)b * T + tok;
  const OT* const qrow = reinterpret_cast<const OT*>(a.q) + row * a.q_stride + (long long)(hk * g + hh) * D;

  int wmax = my_len > 0 ? my_len : 0;        // the wave's longest row
  int wctx = my_len > 0 ? ctx : INT_MAX;     // ... and the shortest context of its live rows
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const int o = __shfl_xor(wmax, s, 64), c = __shfl_xor(wctx, s, 64);
    wmax = o > wmax ? o : wmax;
    wctx = c < wctx ? c : wctx;
  }
  wmax = __builtin_amdgcn_readfirstlane(wmax);
  wctx = __builtin_amdgcn_readfirstlane(wctx);
  if (lane == 0) wave_len[wave] = wmax;
  __syncthreads();
  int lmax = wave_len[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) lmax = wave_len[w] > lmax ? wave_len[w] : lmax;
  lmax = __builtin_amdgcn_readfirstlane(lmax);
  if (a.n_parts > 1 && p0 >= lmax) return;  // nothing of this tile reaches the partition (uniform)

  f32x4 acc[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -__builtin_inff(), l_run = 0.0f;
  int fb = INT_MAX;  // the first key of this partition with a table entry outside the cache

  if (lmax > p0) {
    const int kend = lmax - p0 < P ? lmax : p0 + P;  // the keys [p0, kend) are walked
    // Q^T fragments: query l16, d = 32 c + 8 q4 .. + 7
    u32x4 qf[NQC];
#pragma unroll
    for (int c = 0; c < NQC; ++c) {
      qf[c] = u32x4{0u, 0u, 0u, 0u};
      if (my_len > 0) {
        const Packed8 p = *reinterpret_cast<const Packed8*>(qrow + c * 32 + q4 * 8);
        qf[c] = u32x4{p.w[0], p.w[1], p.w[2], p.w[3]};
      }
    }
    const OT* const kc = reinterpret_cast<const OT*>(a.k_cache);
    const OT* const vc = reinterpret_cast<const OT*>(a.v_cache);
    const unsigned long long head_off = (unsigned long long)(unsigned)hk * a.head_stride;
    const int t0 = p0 / KT;
    int nt = t0 + (kend - p0 + KT - 1) / KT;  // the key tiles [t0, nt)

    // the slots of key tile j, by wave 0: -1 for a key that is staged as zeros
    auto resolve = [&](int j) {
      if (wave != 0) return;
      const int p = j * KT + lane;
      long long s = -1;
      bool bad = false;
      if (p < kend) {
        const unsigned blk = (unsigned)p / (unsigned)a.block_size, off = (unsigned)p - blk * (unsigned)a.block_size;
        s = (long long)a.block_table[(long long)b * a.table_stride + blk] * a.block_size + off;
        bad = s < 0 || s >= a.n_slots;
      }
      const unsigned long long mask = __ballot(bad);
      const int first = mask ? (int)__builtin_ctzll(mask) : KT;
      slots[j & 1][lane] = (p < kend && lane < first) ? (int)s : -1;
      if (lane == 0) fb_tile[j & 1] = mask ? j * KT + first : INT_MAX;
    };

    Packed8 kr[KIT], vr[VIT][2];
    auto fetch = [&](int j) {
      const int* const sl = slots[j & 1];
      const Packed8 zero = {{0u, 0u, 0u, 0u}};
#pragma unroll
      for (int it = 0; it < KIT; ++it) {
        const int c = it * kAttnThreads + tid, key = c / DC, dc = c % DC;
        const int s = sl[key];
        kr[it] = zero;
        if (s >= 0) kr[it] = *reinterpret_cast<const Packed8*>(kc + ((unsigned long long)(unsigned)s * a.slot_stride + head_off + (unsigned)(dc * 8)));
      }
#pragma unroll
      for (int it = 0; it < VIT; ++it) {
        const int c = it * kAttnThreads + tid, kp = c & 31, dc = c >> 5;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int s = sl[2 * kp + e];
          vr[it][e] = zero;
          if (s >= 0) vr[it][e] = *reinterpret_cast<const Packed8*>(vc + ((unsigned long long)(unsigned)s * a.slot_stride + head_off + (unsigned)(dc * 8)));
        }
      }
    };
    auto stage = [&](int buf) {
#pragma unroll
      for (int it = 0; it < KIT; ++it) {
        const int c = it * kAttnThreads + tid, key = c / DC, dc = c % DC;
        *reinterpret_cast<u32x4*>(&ks[buf][key * KROW + dc * 8]) = u32x4{kr[it].w[0], kr[it].w[1], kr[it].w[2], kr[it].w[3]};
      }
#pragma unroll
      for (int it = 0; it < VIT; ++it) {
        const int c = it * kAttnThreads + tid, kp = c & 31, dc = c >> 5;
        const int key = 2 * kp, jb = key >> 4, kq = (key >> 2) & 3, ki = key & 3;
        const int pos = (jb >> 1) * 32 + kq * 8 + (jb & 1) * 4 + ki;  // even: the neighbour key sits at pos + 1
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t lo = vr[it][0].w[j >> 1], hi = vr[it][1].w[j >> 1];
          const uint32_t w = (j & 1) ? __builtin_amdgcn_perm(hi, lo, 0x07060302u) : __builtin_amdgcn_perm(hi, lo, 0x05040100u);
          *reinterpret_cast<uint32_t*>(&vs[buf][(dc * 8 + j) * VROW + pos]) = w;
        }
      }
    };

    resolve(t0);
    __syncthreads();
    if (fb_tile[t0 & 1] != INT_MAX) {
      fb = fb_tile[t0 & 1];
      nt = t0 + 1;
    }
    fetch(t0);
    stage(t0 & 1);
    if (nt > t0 + 1) resolve(t0 + 1);
    __syncthreads();

    for (int i = t0; i < nt; ++i) {
      const int buf = i & 1;
      const bool has_next = i + 1 < nt;
      if (has_next) {
        const int f = fb_tile[buf ^ 1];
        if (f != INT_MAX) {  // (uniform: written before the last barrier)
          fb = f;
          nt = i + 2;
        }
        fetch(i + 1);
      }
      const int key0 = i * KT;
      if (wmax > key0) {
        if (wctx - key0 >= KT)  // the whole tile is context for every live row of the wave
          tree64_tile<D, OT, false>(ks[buf], vs[buf], qf, 0ull, a.scale, l16, q4, m_run, l_run, acc);
        else
          tree64_tile<D, OT, true>(ks[buf], vs[buf], qf, tree64_tile_bits(ctx, word, key0), a.scale, l16, q4, m_run, l_run, acc);
      }
      if (has_next) stage(buf ^ 1);
      if (i + 2 < nt) resolve(i + 2);
      __syncthreads();
    }
  }

  if (!exists) return;
  tree64_finish<D, OT>(a, row, hk * g + hh, part, p0, my_len, fb, q4, m_run, l_run, acc);
}

// The combine: one wave per (row, query head), lane l the elements d = l + 64 e, over the partials of the partitions below the row's
// own Leff, ascending.  A partial with the maximum -inf (the row attends nothing in that partition) is skipped.
template <int D, typename OT>
__global__ void __launch_bounds__(kAttnThreads) sqllm_attn_tree64_combine_kernel(const AttnTree64Args a) {
  constexpr int E = D / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.y;
  const unsigned i = blockIdx.x * 4u + (unsigned)wave;  // (token, query head) of the sequence
  const int tok = i / (unsigned)a.n_q_heads, hq = i - (unsigned)tok * (unsigned)a.n_q_heads;
  if (tok >= a.q_len) return;
  const long long row = (long long)b * a.q_len + tok;
  OT* const out = reinterpret_cast<OT*>(a.out) + row * a.out_stride + (long long)hq * D;
  const int n = a.q_lens ? a.q_lens[b] : a.q_len;
  const int len = tree64_row_len(n, a.seq_lens[b], tok, a.q_len, a.capacity, tree64_word(a, b, tok, n));
  if (len <= 0) {
    const OT c = len == 0 ? (OT)0.0f : (OT)__builtin_nanf("");
#pragma unroll
    for (int e = 0; e < E; ++e) out[lane + 64 * e] = c;
    return;
  }
  const int np = (len - 1) / kTree64Partition + 1;
  const long long pa = (row * a.n_q_heads + hq) * a.n_parts;
  float m = -__builtin_inff();
  for (int p = 0; p < np; ++p) m = fmaxf(m, a.ws_ml[(pa + p) * 2]);
  float l = 0.0f, t[E];
#pragma unroll
  for (int e = 0; e < E; ++e) t[e] = 0.0f;
  for (int p = 0; p < np; ++p) {
    const float mp = a.ws_ml[(pa + p) * 2];
    if (mp == -__builtin_inff()) continue;  // nothing attended there (uniform over the wave)
    const float w = expf(mp - m);
    l = fmaf(w, a.ws_ml[(pa + p) * 2 + 1], l);
#pragma unroll
    for (int e = 0; e < E; ++e) t[e] = fmaf(w, a.ws_acc[(pa + p) * D + lane + 64 * e], t[e]);
  }
  const float denom = std::is_same<OT, __bf16>::value ? l : l * 32768.0f;  // the fp16 planes' 2^15, once
#pragma unroll
  for (int e = 0; e < E; ++e) out[lane + 64 * e] = (OT)(t[e] / denom * a.v_scale);
}

template <int D, typename OT>
static hipError_t launch_attn_tree64_combine_inst(const AttnTree64Args& k, hipStream_t stream) {
  const unsigned per_seq = (unsigned)k.n_q_heads * (unsigned)k.q_len;  // at most 65535 x 64
  hipLaunchKernelGGL((sqllm_attn_tree64_combine_kernel<D, OT>), dim3((per_seq + 3) / 4, k.batch), dim3(kAttnThreads), 0, stream, k);
  return hipGetLastError();
}

// the combine alone: behind this file's partials, and behind those of sqllm_attn_tree64_fp8.hip
static hipError_t launch_attn_tree64_combine(const AttnTree64Args& k, int head_dim, bool bf16, hipStream_t stream) {
  if (bf16) return head_dim == 64 ? launch_attn_tree64_combine_inst<64, __bf16>(k, stream) : launch_attn_tree64_combine_inst<128, __bf16>(k, stream);
  return head_dim == 64 ? launch_attn_tree64_combine_inst<64, _Float16>(k, stream) : launch_attn_tree64_combine_inst<128, _Float16>(k, stream);
}

template <int D, typename OT>
static hipError_t launch_attn_tree64_inst(const AttnTree64Args& k, const AttnCall& c, hipStream_t stream) {
  hipLaunchKernelGGL((sqllm_attn_tree64_kernel<D, OT>), dim3((unsigned)k.n_tiles * (unsigned)k.n_parts, c.n_kv_heads, c.batch), dim3(kAttnThreads), 0, stream, k);
  return hipGetLastError();
}

// geometry from HOST fields only; what is not served is an error, never another kernel
static hipError_t launch_attn_tree64(const AttnCall& c, hipStream_t stream) {
  if (!tree64_served(c) || c.fp8) return hipErrorInvalidValue;  // (byte caches: sqllm_attn_tree64_fp8.hip, a slot of its own)
  const AttnTree64Args k = make_tree64_args(c);
  const hipError_t e = c.bf16 ? (c.head_dim == 64 ? launch_attn_tree64_inst<64, __bf16>(k, c, stream) : launch_attn_tree64_inst<128, __bf16>(k, c, stream))
                              : (c.head_dim == 64 ? launch_attn_tree64_inst<64, _Float16>(k, c, stream) : launch_attn_tree64_inst<128, _Float16>(k, c, stream));
  if (e != hipSuccess || k.n_parts == 1) return e;
  return launch_attn_tree64_combine(k, c.head_dim, c.bf16, stream);
}

// the host layer reaches the launcher through its slot of g_launch_attn_tree64 (sqllm_kernels.h), so that it links without this file too
static const bool g_attn_tree64_registered = (g_launch_attn_tree64[0] = launch_attn_tree64, g_launch_attn_tree64_combine = launch_attn_tree64_combine, true);

}  // namespace sqllm
