// sqllm_attn_prefill_window_fp8.hip -- SLIDING-WINDOW prefill attention over a paged KV cache of 1-byte OCP e4m3fn elements, on
// the matrix cores (include/sqllm_hip.h: sqllm_attn_prefill_window_fp8_f16 / _fp8_bf16; the suffix names the type of q and out).
// One kernel node, no workspace.  Token t of sequence b attends the keys [lo, L), L = L(b,t), lo = L > W ? L - W : 0.  The body is
// a copy of sqllm_attn_prefill_fp8.hip -- bytes in the prefetch registers, ONE exact conversion per element on the way into LDS
// (pair16), the V transpose on the bytes, k_scale folded into the score's scale by the host and v_scale applied once at the
// finish: all described THERE -- with the walk of sqllm_attn_prefill_window.hip, described there:
//   * the tiles lo_min / 64 .. ceil(lmax / 64) - 1, lo_min the least lo of the workgroup's rows; a wave issues matrix instructions
//     for a tile only if wmax > key0 && wlo < key0 + 64, its barriers are unconditional;
//   * score and weight selected on lo <= kidx && kidx < L;
//   * slots resolved only for the keys lo_min <= p < lmax, everything else staged as ZEROS written here and never loaded, the table
//     entries of blocks wholly below lo_min / block_size never read;
//   * a bad table entry does not stop the walk: its key is staged as zeros, the tile's ballot is kept in LDS and every lane ANDs
//     it with the bits of its own [lo, L): NaN for exactly the rows that attend the key.
//
// Registers / LDS (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 4.4.  No scratch, two workgroups per CU.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sqllm_attn_prefill.h"

namespace sqllm {

// 8 bytes that are aligned to one byte only
struct __attribute__((packed, aligned(1))) WBytes8 {
  uint32_t w[2];
};
template <int N>
struct WBytesOf;
template <>
struct WBytesOf<16> { typedef Bytes16 type; };
template <>
struct WBytesOf<8> { typedef WBytes8 type; };

// the e4m3fn bytes 0, 1 (HI: 2, 3) of w as one word of two OT elements, the lower byte in the low half; exact, a NaN byte is a NaN
template <typename OT, bool HI>
__device__ __forceinline__ uint32_t wpair16(uint32_t w) {
  const f32x2 f = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, HI);
  if constexpr (std::is_same<OT, __bf16>::value) {
    const __bf16 lo = (__bf16)f[0], hi = (__bf16)f[1];
    return (uint32_t)__builtin_bit_cast(unsigned short, lo) | ((uint32_t)__builtin_bit_cast(unsigned short, hi) << 16);
  } else {
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(f[0], f[1]));
  }
}

// (built without packed fp32 arithmetic: build.NO_PACKED_FP32 -- the arithmetic of sqllm_attn_prefill_fp8.hip, for the bit identities)
template <int D, typename OT>
__global__ void __launch_bounds__(kAttnThreads, 2) sqllm_attn_prefill_window_fp8_kernel(const AttnPrefillWindowArgs a, const float v_scale) {
  constexpr int KT = kPrefillTile;
  constexpr int KROW = D + 8;    // 16-bit elements per staged K row
  constexpr int VROW = KT + 8;   // 16-bit elements per row of V^T
  constexpr int DC = D / 16;     // 16-byte chunks per key row of K
  constexpr int KIT = KT * DC / kAttnThreads;  // K chunks per thread and tile
  constexpr int VE = D / 8;      // bytes (d's) per key of a V task: (KT / 2) key pairs x 8 chunks = 256 tasks, one per thread
  constexpr int VW = VE / 4;     // ... in words
  constexpr int NDB = D / 16, NQC = D / 32;
  typedef typename WBytesOf<VE>::type VBytes;
  static_assert(KIT >= 1 && KT == 64 && kAttnThreads == 256 && (KT / 2) * (D / VE) == kAttnThreads, "the lane maps below");
  __shared__ __attribute__((aligned(16))) uint16_t ks[2][KT * KROW];
  __shared__ __attribute__((aligned(16))) uint16_t vs[2][D * VROW];
  __shared__ unsigned long long bad_tile[2];  // per staged tile: bit i, key 64 j + i has a table entry outside the cache
  __shared__ int slots[2][KT];
  __shared__ int wave_len[4], wave_lo[4];

  const int tile = a.n_tiles - 1 - (int)blockIdx.x;  // the heaviest tiles first
  const int hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, q4 = lane >> 4;
  const int g = a.group, T = a.q_len;

  // this lane's query row: virtual row -> (token, head of the group), its length and the first key of its window
  const int vrow = tile * KT + wave * 16 + l16;
  const int tok = (unsigned)vrow / (unsigned)g, hh = vrow - tok * g;
  const bool exists = tok < T;
  const int n = a.q_lens ? a.q_lens[b] : T, seq = a.seq_lens[b];
  const int my_len = exists ? append_row_len(n, seq, tok, T, a.capacity) : 0;  // 0: +0 (or no row), -1: NaN
  const int lo = my_len > a.window ? my_len - a.window : 0;
  const long long row = (long long)b * T + tok;
  const OT* const qrow = reinterpret_cast<const OT*>(a.q) + row * a.q_stride + (long long)(hk * g + hh) * D;
  OT* const orow = reinterpret_cast<OT*>(a.out) + row * a.out_stride + (long long)(hk * g + hh) * D;

  int wmax = my_len > 0 ? my_len : 0;    // the wave's longest row
  int wlo = my_len > 0 ? lo : INT_MAX;   // ... and the earliest key any of its rows attends
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const int o = __shfl_xor(wmax, s, 64), p = __shfl_xor(wlo, s, 64);
    wmax = o > wmax ? o : wmax;
    wlo = p < wlo ? p : wlo;
  }
  wmax = __builtin_amdgcn_readfirstlane(wmax);
  wlo = __builtin_amdgcn_readfirstlane(wlo);
  if (lane == 0) {
    wave_len[wave] = wmax;
    wave_lo[wave] = wlo;
  }
  __syncthreads();
  int lmax = wave_len[0], lo_min = wave_lo[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    lmax = wave_len[w] > lmax ? wave_len[w] : lmax;
    lo_min = wave_lo[w] < lo_min ? wave_lo[w] : lo_min;
  }
  lmax = __builtin_amdgcn_readfirstlane(lmax);
  lo_min = __builtin_amdgcn_readfirstlane(lo_min);  // (below lmax wherever lmax > 0)

  f32x4 acc[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -__builtin_inff(), l_run = 0.0f;
  bool bad_row = false;  // a table entry outside the cache at a key of this row's own [lo, L)

  if (lmax > 0) {
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
    const int i0 = lo_min / KT, nt = (lmax + KT - 1) / KT;  // the tiles i0 .. nt - 1

    // the slots of key tile j, by wave 0: -1 for a key that is staged as zeros (outside [lo_min, lmax), or a bad table entry)
    auto resolve = [&](int j) {
      if (wave != 0) return;
      const int p = j * KT + lane;
      long long s = -1;
      bool bad = false;
      if (p >= lo_min && p < lmax) {
        const unsigned blk = (unsigned)p / (unsigned)a.block_size, off = (unsigned)p - blk * (unsigned)a.block_size;
        s = (long long)a.block_table[(long long)b * a.table_stride + blk] * a.block_size + off;
        bad = s < 0 || s >= a.n_slots;
      }
      const unsigned long long mask = __ballot(bad);
      slots[j & 1][lane] = bad ? -1 : (int)s;
      if (lane == 0) bad_tile[j & 1] = mask;
    };
    // this row against the bad keys of tile j (read behind the barrier that follows resolve(j), before the one in front of
    // resolve(j + 2))
    auto note_bad = [&](int j) { bad_row = bad_row || (bad_tile[j & 1] & window_tile_bits(lo, my_len, j * KT)) != 0ull; };

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
          w[2 * i] = wpair16<OT, false>(kr[it].w[i]);
          w[2 * i + 1] = wpair16<OT, true>(kr[it].w[i]);
        }
        u32x4* const at = reinterpret_cast<u32x4*>(&ks[buf][key * KROW + kd * 16]);
        at[0] = u32x4{w[0], w[1], w[2], w[3]};
        at[1] = u32x4{w[4], w[5], w[6], w[7]};
      }
      const int key = 2 * kp, jb = key >> 4, kq = (key >> 2) & 3, ki = key & 3;
      const int pos = (jb >> 1) * 32 + kq * 8 + (jb & 1) * 4 + ki;  // even: the neighbour key sits at pos + 1
#pragma unroll
      for (int i = 0; i < VW; ++i) {
        const uint32_t b0 = vr[0].w[i], b1 = vr[1].w[i];
        const uint32_t p01 = __builtin_amdgcn_perm(b1, b0, 0x05010400u), p23 = __builtin_amdgcn_perm(b1, b0, 0x07030602u);
        uint16_t* const at = &vs[buf][(dc * VE + 4 * i) * VROW + pos];
        *reinterpret_cast<uint32_t*>(at) = wpair16<OT, false>(p01);
        *reinterpret_cast<uint32_t*>(at + VROW) = wpair16<OT, true>(p01);
        *reinterpret_cast<uint32_t*>(at + 2 * VROW) = wpair16<OT, false>(p23);
        *reinterpret_cast<uint32_t*>(at + 3 * VROW) = wpair16<OT, true>(p23);
      }
    };

    resolve(i0);
    __syncthreads();
    note_bad(i0);
    fetch(i0);
    stage(i0 & 1);
    if (i0 + 1 < nt) resolve(i0 + 1);
    __syncthreads();

    for (int i = i0; i < nt; ++i) {
      const int buf = i & 1;
      const bool has_next = i + 1 < nt;
      if (has_next) {
        note_bad(i + 1);
        fetch(i + 1);
      }
      const int key0 = i * KT;
      if (wmax > key0 && wlo - key0 < KT) {
        // S^T = K Q^T: lane holds query l16, keys key0 + 16 jb + 4 q4 + i
        f32x4 s[4];
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
          s[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int c = 0; c < NQC; ++c) {
            const u32x4 kf = *reinterpret_cast<const u32x4*>(&ks[buf][(16 * jb + l16) * KROW + c * 32 + q4 * 8]);
            s[jb] = mfma_16x16x32<OT>(kf, qf[c], s[jb]);
          }
        }
        float sc[4][4], tmax = -__builtin_inff();
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int kidx = key0 + 16 * jb + 4 * q4 + e;
            sc[jb][e] = (lo <= kidx && kidx < my_len) ? a.scale * s[jb][e] : -__builtin_inff();  // (scale: the caller's x k_scale)
            tmax = fmaxf(tmax, sc[jb][e]);
          }
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float m_new = fmaxf(m_run, tmax);
        const float m_use = m_new == -__builtin_inff() ? 0.0f : m_new;  // nothing attended yet: no inf - inf
        const float alpha = expf(m_run - m_use);
        float tsum = 0.0f;
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int kidx = key0 + 16 * jb + 4 * q4 + e;
            sc[jb][e] = (lo <= kidx && kidx < my_len) ? expf(sc[jb][e] - m_use) : 0.0f;
            tsum += sc[jb][e];
          }
        }
        tsum += __shfl_xor(tsum, 16, 64);
        tsum += __shfl_xor(tsum, 32, 64);
        l_run = l_run * alpha + tsum;
        m_run = m_new;
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[db][e] *= alpha;
        }
        // out^T += V^T P^T, three planes of P
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const float w[8] = {sc[2 * c][0], sc[2 * c][1], sc[2 * c][2], sc[2 * c][3], sc[2 * c + 1][0], sc[2 * c + 1][1], sc[2 * c + 1][2], sc[2 * c + 1][3]};
          u32x4 ph, pm, pl;
          weight_planes<OT>(w, ph, pm, pl);
#pragma unroll
          for (int db = 0; db < NDB; ++db) {
            const u32x4 vf = *reinterpret_cast<const u32x4*>(&vs[buf][(16 * db + l16) * VROW + c * 32 + q4 * 8]);
            f32x4 t = acc[db];
            t = mfma_16x16x32<OT>(vf, pl, t);  // small planes first
            t = mfma_16x16x32<OT>(vf, pm, t);
            t = mfma_16x16x32<OT>(vf, ph, t);
            acc[db] = t;
          }
        }
      }
      if (has_next) stage(buf ^ 1);
      if (i + 2 < nt) resolve(i + 2);
      __syncthreads();
    }
  }

  // finish: this lane's row, d = 16 db + 4 q4 .. + 3; v_scale once per element, before the one rounding
  if (!exists) return;
  const bool nan_row = my_len < 0 || bad_row;
  const float denom = std::is_same<OT, __bf16>::value ? l_run : l_run * 32768.0f;
#pragma unroll
  for (int db = 0; db < NDB; ++db) {
    OT o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = 0.0f;
      if (my_len > 0) v = acc[db][e] / denom * v_scale;
      if (nan_row) v = __builtin_nanf("");
      o[e] = (OT)v;
    }
    Packed4 p;
    p.w[0] = (uint32_t)__builtin_bit_cast(unsigned short, o[0]) | ((uint32_t)__builtin_bit_cast(unsigned short, o[1]) << 16);
    p.w[1] = (uint32_t)__builtin_bit_cast(unsigned short, o[2]) | ((uint32_t)__builtin_bit_cast(unsigned short, o[3]) << 16);
    *reinterpret_cast<Packed4*>(orow + 16 * db + 4 * q4) = p;
  }
}

template <int D, typename OT>
static hipError_t launch_attn_prefill_window_fp8_inst(const AttnPrefillWindowArgs& k, const AttnCall& c, hipStream_t stream) {
  hipLaunchKernelGGL((sqllm_attn_prefill_window_fp8_kernel<D, OT>), dim3(k.n_tiles, c.n_kv_heads, c.batch), dim3(kAttnThreads), 0, stream, k, c.v_scale);
  return hipGetLastError();
}

// geometry from HOST fields only, the grid of the entries without a window; what is not served is an error, never another kernel
static hipError_t launch_attn_prefill_window_fp8(const AttnCall& c, hipStream_t stream) {
  if (!prefill_window_served(c) || !c.fp8) return hipErrorInvalidValue;
  const AttnPrefillWindowArgs k = make_prefill_window_args(c);  // (slot_stride and head_stride count bytes; scale holds scale * k_scale)
  if (c.bf16) return c.head_dim == 64 ? launch_attn_prefill_window_fp8_inst<64, __bf16>(k, c, stream) : launch_attn_prefill_window_fp8_inst<128, __bf16>(k, c, stream);
  return c.head_dim == 64 ? launch_attn_prefill_window_fp8_inst<64, _Float16>(k, c, stream) : launch_attn_prefill_window_fp8_inst<128, _Float16>(k, c, stream);
}

// the host layer reaches the launcher through its slot (sqllm_kernels.h), so that it links without this file too
static const bool g_attn_prefill_window_fp8_registered = (g_launch_attn_prefill_window[1] = launch_attn_prefill_window_fp8, true);

}  // namespace sqllm
