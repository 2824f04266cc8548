// sqllm_attn_tree64_fp8.hip -- the wide-tree attention of sqllm_attn_tree64.hip over a paged KV cache of 1-byte OCP e4m3fn elements
// (include/sqllm_hip.h: sqllm_attn_tree64_fp8_f16 / _bf16; the suffix names the type of q and out).  The grid, the partitions, the
// mask, the compute loop (tree64_tile) and both finishes are that file's, and the combine IS that file's kernel, reached through
// g_launch_attn_tree64_combine.  What differs is everything between the cache and LDS, which is sqllm_attn_prefill_fp8.hip's,
// described there: K and V rows leave the cache as bytes with byte alignment only, one tile ahead of the tile being computed; each
// byte is converted ONCE, exactly, to the type of q on its way from the prefetch registers into LDS (pair16), V transposed on the
// bytes before the conversion, so LDS holds the layouts of the 16-bit kernel.
//
// Scales.  The host has folded k_scale into the score scale (rounded once); the matrix instructions see the bytes' own values.
// v_scale multiplies the finished element once, in fp32, before the ONE rounding: in the combine, or in the finishing path of the
// one-partition case.
//
// Registers / LDS (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 4.4.  No scratch, the 16-bit kernel's LDS.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sqllm_attn_tree64.h"

namespace sqllm {

// 8 bytes that are aligned to one byte only
struct __attribute__((packed, aligned(1))) Bytes8 {
  uint32_t w[2];
};
template <int N>
struct BytesOf;
template <>
struct BytesOf<16> { typedef Bytes16 type; };
template <>
struct BytesOf<8> { typedef Bytes8 type; };

// the e4m3fn bytes 0, 1 (HI: 2, 3) of w as one word of two OT elements, the lower byte in the low half; exact, a NaN byte is a NaN
template <typename OT, bool HI>
__device__ __forceinline__ uint32_t pair16(uint32_t w) {
  const f32x2 f = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
  if constexpr (std::is_same<OT, __bf16>::value) {
    const __bf16 lo = (__bf16)f[0], hi = (__bf16)f[1];
    return (uint32_t)__builtin_bit_cast(unsigned short, lo) | ((uint32_t)__builtin_bit_cast(unsigned short, hi) << 16);
  } else {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(f[0], f[1]));
  }
}

// (built without packed fp32 arithmetic: build.NO_PACKED_FP32)
template <int D, typename OT>
__global__ void __launch_bounds__(kAttnThreads, 2) sqllm_attn_tree64_fp8_kernel(const AttnTree64Args a) {
  constexpr int KT = kPrefillTile, P = kTree64Partition;
  constexpr int KROW = D + 8;    // 16-bit elements per staged K row
  constexpr int VROW = KT + 8;   // 16-bit elements per row of V^T
  constexpr int DC = D / 16;     // 16-byte chunks per key row of K
  constexpr int KIT = KT * DC / kAttnThreads;  // K chunks per thread and tile
  constexpr int VE = D / 8;      // bytes (d's) per key of a V task: (KT / 2) key pairs x 8 chunks = 256 tasks, one per thread
  constexpr int VW = VE / 4;     // ... in words
  constexpr int NDB = D / 16, NQC = D / 32;
  typedef typename BytesOf<VE>::type VBytes;
  static_assert(KIT >= 1 && KT == 64 && kAttnThreads == 256 && (KT / 2) * (D / VE) == kAttnThreads, "the lane maps below");
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
    const uint8_t* const kc = reinterpret_cast<const uint8_t*>(a.k_cache);
    const uint8_t* const vc = reinterpret_cast<const uint8_t*>(a.v_cache);
    const unsigned long long head_off = (unsigned long long)(unsigned)hk * a.head_stride;  // (bytes, as slot_stride)
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

    // this thread's V task: keys 2 kp, 2 kp + 1, bytes VE dc .. + VE - 1
    const int kp = tid & 31, dc = tid >> 5;
    Bytes16 kr[KIT];
    VBytes vr[2];
    auto fetch = [&](int j) {
      const int* const sl = slots[j & 1];
#pragma unroll
      for (int it = 0; it < KIT; ++it) {
        const int c = it * kAttnThreads + tid, key = c / DC, kd = c % DC;
        const int s = sl[key];
        kr[it] = Bytes16{{0u, 0u, 0u, 0u}};
        if (s >= 0) kr[it] = *reinterpret_cast<const Bytes16*>(kc + ((unsigned long long)(unsigned)s * a.slot_stride + head_off + (unsigned)(kd * 16)));
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int s = sl[2 * kp + e];
#pragma unroll
        for (int i = 0; i < VW; ++i) vr[e].w[i] = 0u;
        if (s >= 0) vr[e] = *reinterpret_cast<const VBytes*>(vc + ((unsigned long long)(unsigned)s * a.slot_stride + head_off + (unsigned)(dc * VE)));
      }
    };
    auto stage = [&](int buf) {
#pragma unroll
      for (int it = 0; it < KIT; ++it) {
        const int c = it * kAttnThreads + tid, key = c / DC, kd = c % DC;
        uint32_t w[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          w[2 * i] = pair16<OT, false>(kr[it].w[i]);
          w[2 * i + 1] = pair16<OT, true>(kr[it].w[i]);
        }
        u32x4* const at = reinterpret_cast<u32x4*>(&ks[buf][key * KROW + kd * 16]);
        at[0] = u32x4{w[0], w[1], w[2], w[3]};
        at[1] = u32x4{w[4], w[5], w[6], w[7]};
      }
      const int key = 2 * kp, jb = key >> 4, kq = (key >> 2) & 3, ki = key & 3;
      const int pos = (jb >> 1) * 32 + kq * 8 + (jb & 1) * 4 + ki;  // even: the neighbour key sits at pos + 1
#pragma unroll
      for (int i = 0; i < VW; ++i) {
        const uint32_t lo = vr[0].w[i], hi = vr[1].w[i];
        const uint32_t p01 = __builtin_amdgcn_perm(hi, lo, 0x05010400u), p23 = __builtin_amdgcn_perm(hi, lo, 0x07030602u);
        uint16_t* const at = &vs[buf][(dc * VE + 4 * i) * VROW + pos];
        *reinterpret_cast<uint32_t*>(at) = pair16<OT, false>(p01);
        *reinterpret_cast<uint32_t*>(at + VROW) = pair16<OT, true>(p01);
        *reinterpret_cast<uint32_t*>(at + 2 * VROW) = pair16<OT, false>(p23);
        *reinterpret_cast<uint32_t*>(at + 3 * VROW) = pair16<OT, true>(p23);
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
      if (wmax > key0) {  // (scale: the caller's x k_scale)
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

template <int D, typename OT>
static hipError_t launch_attn_tree64_fp8_inst(const AttnTree64Args& k, const AttnCall& c, hipStream_t stream) {
  hipLaunchKernelGGL((sqllm_attn_tree64_fp8_kernel<D, OT>), dim3((unsigned)k.n_tiles * (unsigned)k.n_parts, c.n_kv_heads, c.batch), dim3(kAttnThreads), 0, stream, k);
  return hipGetLastError();
}

// geometry from HOST fields only; what is not served is an error, never another kernel
static hipError_t launch_attn_tree64_fp8(const AttnCall& c, hipStream_t stream) {
  if (!tree64_served(c) || !c.fp8) return hipErrorInvalidValue;
  const AttnTree64Args k = make_tree64_args(c);  // (slot_stride and head_stride count bytes; scale holds scale * k_scale)
  if (k.n_parts > 1 && !g_launch_attn_tree64_combine) return hipErrorNotSupported;  // (before anything is launched)
  const hipError_t e = c.bf16 ? (c.head_dim == 64 ? launch_attn_tree64_fp8_inst<64, __bf16>(k, c, stream) : launch_attn_tree64_fp8_inst<128, __bf16>(k, c, stream))
                              : (c.head_dim == 64 ? launch_attn_tree64_fp8_inst<64, _Float16>(k, c, stream) : launch_attn_tree64_fp8_inst<128, _Float16>(k, c, stream));
  if (e != hipSuccess || k.n_parts == 1) return e;
  return g_launch_attn_tree64_combine(k, c.head_dim, c.bf16, stream);
}

// the host layer reaches the launcher through its slot (sqllm_kernels.h), so that it links without this file too
static const bool g_attn_tree64_fp8_registered = (g_launch_attn_tree64[1] = launch_attn_tree64_fp8, true);

}  // namespace sqllm
