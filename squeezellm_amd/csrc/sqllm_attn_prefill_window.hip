// sqllm_attn_prefill_window.hip -- SLIDING-WINDOW prefill attention over the paged KV cache, on the matrix cores
// (include/sqllm_hip.h: sqllm_attn_prefill_window_f16 / _bf16).  One kernel node, no workspace.  Token t of sequence b attends the
// keys [lo, L), L = L(b,t), lo = L > W ? L - W : 0 -- Mistral's mask, the query's own key included, W keys in all.  The body is a
// copy of sqllm_attn_prefill.hip, edited, the way sqllm_attn_window.hip is a copy of the decode kernels: the work split, the
// staging layouts, S^T = K Q^T and out^T = V^T P^T on v_mfma_f32_16x16x32_{f16,bf16}, the fp32 online softmax, the three weight
// planes and the finish are described THERE.  What differs is the walk.
//
// Range.  Besides the longest row (wmax per wave, lmax per workgroup) the LEAST lo over the rows with L > 0 is reduced, per wave
// (wlo) and per workgroup (lo_min), through the same LDS exchange.  The workgroup walks the absolute key tiles lo_min / 64 ..
// ceil(lmax / 64) - 1: with a window far shorter than the context, W / 64 + 2 tiles or so instead of all of them.  The prologue,
// the prefetch and the slot resolution start at that tile.  A wave issues matrix instructions for a tile only if one of its rows
// can attend it, wmax > key0 && wlo < key0 + 64; its barriers are unconditional.  lo = L - W is taken only where L > W: W may be
// INT32_MAX, and no sum here leaves int.
//
// Mask.  Score and weight are SELECTED on lo <= kidx && kidx < L: a tile a row does not attend leaves its accumulators at +0 and
// its sum at 0 whether it is skipped or walked, so a row with L <= W holds the bits of the entry without a window, and a row
// whose lo is a multiple of 64 and of block_size the bits that entry gives the query over the table advanced to lo.
//
// What is looked at.  Wave 0 resolves a slot only for the keys p of a tile with lo_min <= p < lmax; the others -- the keys of the
// first tile below lo_min as those at or beyond lmax -- are staged as ZEROS written here and never loaded, and the table entries
// of blocks wholly below lo_min / block_size are never read: a rolling buffer may have reused them.
//
// Bad table entries.  With windows the first bad key no longer decides: a bad entry at key p must make NaN exactly the rows with
// lo <= p < L and leave alone the rows of the same tile whose window has passed p.  So the walk does not stop there: such keys are
// staged as zeros (never loaded), the tile's 64-bit ballot is kept in LDS beside the slots, and every lane ANDs it with the bits
// of its own [lo, L) inside that tile (window_tile_bits) -- for every tile walked, skipped by its wave or not.
//
// Registers / LDS (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 4.4.  No scratch, two workgroups per CU.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sqllm_attn_prefill.h"

namespace sqllm {

// (built without packed fp32 arithmetic: build.NO_PACKED_FP32 -- the arithmetic of sqllm_attn_prefill.hip, for the bit identities)
template <int D, typename OT>
__global__ void __launch_bounds__(kAttnThreads, 2) sqllm_attn_prefill_window_kernel(const AttnPrefillWindowArgs a) {
  constexpr int KT = kPrefillTile;
  constexpr int KROW = D + 8;    // 16-bit elements per staged K row
  constexpr int VROW = KT + 8;   // 16-bit elements per row of V^T
  constexpr int DC = D / 8;      // 16-byte chunks per key row
  constexpr int KIT = KT * DC / kAttnThreads;        // K chunks per thread and tile
  constexpr int VIT = (KT / 2) * DC / kAttnThreads;  // V tasks (two keys x 8 d) per thread and tile
  constexpr int NDB = D / 16, NQC = D / 32;
  static_assert(KIT >= 1 && VIT >= 1 && KT == 64 && kAttnThreads == 256, "the lane maps below");
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
    const OT* const kc = reinterpret_cast<const OT*>(a.k_cache);
    const OT* const vc = reinterpret_cast<const OT*>(a.v_cache);
    const unsigned long long head_off = (unsigned long long)(unsigned)hk * a.head_stride;
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
    // this row against the bad keys of tile j (read where the original reads its first bad key: behind the barrier that follows
    // resolve(j), before the one in front of resolve(j + 2))
    auto note_bad = [&](int j) { bad_row = bad_row || (bad_tile[j & 1] & window_tile_bits(lo, my_len, j * KT)) != 0ull; };

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
          const uint32_t lo16 = vr[it][0].w[j >> 1], hi16 = vr[it][1].w[j >> 1];
          const uint32_t word = (j & 1) ? __builtin_amdgcn_perm(hi16, lo16, 0x07060302u) : __builtin_amdgcn_perm(hi16, lo16, 0x05040100u);
          *reinterpret_cast<uint32_t*>(&vs[buf][(dc * 8 + j) * VROW + pos]) = word;
        }
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
            sc[jb][e] = (lo <= kidx && kidx < my_len) ? a.scale * s[jb][e] : -__builtin_inff();
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

  // finish: this lane's row, d = 16 db + 4 q4 .. + 3
  if (!exists) return;
  const bool nan_row = my_len < 0 || bad_row;
  const float denom = std::is_same<OT, __bf16>::value ? l_run : l_run * 32768.0f;
#pragma unroll
  for (int db = 0; db < NDB; ++db) {
    OT o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float v = 0.0f;
      if (my_len > 0) v = acc[db][e] / denom;
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
static hipError_t launch_attn_prefill_window_inst(const AttnPrefillWindowArgs& k, const AttnCall& c, hipStream_t stream) {
  hipLaunchKernelGGL((sqllm_attn_prefill_window_kernel<D, OT>), dim3(k.n_tiles, c.n_kv_heads, c.batch), dim3(kAttnThreads), 0, stream, k);
  return hipGetLastError();
}

// geometry from HOST fields only, the grid of the entries without a window; what is not served is an error, never another kernel
static hipError_t launch_attn_prefill_window(const AttnCall& c, hipStream_t stream) {
  if (!prefill_window_served(c) || c.fp8) return hipErrorInvalidValue;  // (byte caches: sqllm_attn_prefill_window_fp8.hip, slot [1])
  const AttnPrefillWindowArgs k = make_prefill_window_args(c);
  if (c.bf16) return c.head_dim == 64 ? launch_attn_prefill_window_inst<64, __bf16>(k, c, stream) : launch_attn_prefill_window_inst<128, __bf16>(k, c, stream);
  return c.head_dim == 64 ? launch_attn_prefill_window_inst<64, _Float16>(k, c, stream) : launch_attn_prefill_window_inst<128, _Float16>(k, c, stream);
}

// the host layer reaches the launcher through its slot (sqllm_kernels.h), so that it links without this file too
static const bool g_attn_prefill_window_registered = (g_launch_attn_prefill_window[0] = launch_attn_prefill_window, true);

}  // namespace sqllm
