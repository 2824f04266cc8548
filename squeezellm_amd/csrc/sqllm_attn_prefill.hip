// sqllm_attn_prefill.hip -- causal, bottom-right aligned, variable-length PREFILL attention over the paged KV cache, on the matrix
// cores (include/sqllm_hip.h: sqllm_attn_prefill_f16 / _bf16).  One kernel node, no workspace.  The six files beside this one
// are fp32 vector code because one query per key is a gather; a tile of 64 queries against 64 keys is a GEMM.
//
// Work split.  One workgroup of 256 threads (4 waves) per (query tile, kv head, sequence).  A query tile is 64 VIRTUAL ROWS of
// one kv group -- (new token, query head of the group) pairs, tokens first, as in sqllm_attn_append.hip -- so K and V are read once
// for all the query heads of the group.  Wave w owns the virtual rows 16 w .. 16 w + 15 of the tile.  Grid x runs over the tiles,
// the latest tokens (most keys) first; y is the kv head, z the sequence.  A workgroup walks the key tiles [64 i, 64 i + 64) for
// i = 0 .. ceil(Lmax / 64) - 1 in ascending order, Lmax the largest length of its rows: the causal triangle above is skipped, and
// a wave whose rows all end below a key tile skips its matrix instructions (not its barriers).
//
// Staging.  Per key tile the 64 lanes of wave 0 resolve one slot each through the block table; a ballot finds the first entry
// outside [0, n_slots).  Keys at or beyond min(Lmax, first bad key) are staged as ZEROS written here and are never loaded.  All
// threads copy the tile's K and V rows with 16-byte loads of element alignment (Packed8) into registers, one tile AHEAD of the
// tile being computed, and store them into the other of two LDS buffers behind the matrix instructions: one barrier per tile.
//   K  [key][d], rows padded by 16 bytes: the 16-byte fragment reads of 16 consecutive keys fall on all 64 banks.
//   V  TRANSPOSED on the way into LDS, [d][key position], rows padded by 16 bytes.  A thread takes two neighbouring keys x 8 d and
//      writes eight 32-bit words; 32 consecutive lanes fill one row (no conflicts).  Chosen over the transposing LDS reads
//      (ds_read_b64_tr_b16): the write-side transpose needs no instruction whose lane map could only be checked on the device,
//      and the key POSITIONS can be permuted freely (below), which the transposing read does not allow.
//
// Scores, transposed: S^T = K Q^T with v_mfma_f32_16x16x32_{f16,bf16} on the 16-bit operands as stored (products exact, fp32
// accumulation).  A = 16 keys x 32 d from LDS, B = Q^T from registers (a lane's Q fragments are loaded once and stay).  In the
// result lane l holds query l % 16 and the keys 16 jb + 4 (l / 16) + i, i < 4, of each 16-key block jb: 16 scores of ONE query
// row per lane, so the softmax reductions are in-lane plus two cross-lane steps, and the weights are already in operand layout
// for the second product: with key position (jb / 2) * 32 + (l / 16) * 8 + (jb % 2) * 4 + i, a lane's weights of blocks 2c, 2c + 1
// are the 8 consecutive k's of the B operand of chunk c.  V^T is stored in that position order.
//
// Softmax: fp32, online, one running (max, sum, acc) per row; the scale is applied in fp32; the causal / length mask is a SELECT
// by key index (a masked score is -inf, a masked weight 0, whatever bits the key holds).  A row that has attended nothing yet
// subtracts 0 instead of its maximum of -inf: no inf - inf.
//
// PV, transposed: out^T = V^T P^T, so a lane's accumulators belong to its OWN query row (d = 16 db + 4 (l / 16) + i) and the
// rescale by exp(m_old - m_new) needs no exchange.  fp32-class: the fp32 weights are split into three 16-bit planes of the
// value type and three matrix instructions are issued per (d block, chunk) against V as stored, small planes first.
//   bf16: split8 (sqllm_split_common.h), exact: 8 + 8 + 8 significant bits.
//   fp16: w' = w * 2^15 (w <= 1, so w' <= 32768), hi = rn(w'), mid = rn(w' - hi), lo = rn(w' - hi - mid): 11 + 11 + 11 bits, exact
//         while lo stays at or above fp16's subnormal quantum 2^-24, i.e. for w' >= 1/2, w >= 2^-16; below, the loss is at most
//         2^-25 in w', 2^-40 of the row's largest weight.  2^-15 is undone once, in the final division.
// Every product plane x v is exact in fp32 (at most 11 x 11 bits), so the sum differs from an fp32 sum of w * v by accumulation
// order only (DESIGN.md 4.4 has the argument against the gate).
//
// Finish: acc / sum rounded ONCE to the output type; the +0 rows (padding, L <= 0) and the NaN rows (n_b > T, L beyond the table,
// a bad table entry below L) are written by the same kernel.  Bits depend on the row's own operands, L(b,t) and the shape fields
// only: the key tiles are absolute, the order inside a tile is fixed by the lane map.
//
// Registers / LDS (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 4.4.  No scratch; 200 VGPRs and 72216 bytes of
// LDS at head_dim 128 (two workgroups per CU), 112 and 37400 at 64.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "sqllm_attn_prefill.h"

namespace sqllm {

// (the argument, the matrix instruction and the weight planes: sqllm_attn_prefill.h, shared with sqllm_attn_prefill_fp8.hip)
// (built without packed fp32 arithmetic: build.NO_PACKED_FP32)
template <int D, typename OT>
__global__ void __launch_bounds__(kAttnThreads, 2) sqllm_attn_prefill_kernel(const AttnPrefillArgs a) {
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
  __shared__ int slots[2][KT];
  __shared__ int fb_tile[2];
  __shared__ int wave_len[4];

  const int tile = a.n_tiles - 1 - (int)blockIdx.x;  // the heaviest tiles first
  const int hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, q4 = lane >> 4;
  const int g = a.group, T = a.q_len;

  // this lane's query row: virtual row -> (token, head of the group), its length
  const int vrow = tile * KT + wave * 16 + l16;
  const int tok = (unsigned)vrow / (unsigned)g, hh = vrow - tok * g;
  const bool exists = tok < T;
  const int n = a.q_lens ? a.q_lens[b] : T, seq = a.seq_lens[b];
  const int my_len = exists ? append_row_len(n, seq, tok, T, a.capacity) : 0;  // 0: +0 (or no row), -1: NaN
  const long long row = (long long)b * T + tok;
  const OT* const qrow = reinterpret_cast<const OT*>(a.q) + row * a.q_stride + (long long)(hk * g + hh) * D;
  OT* const orow = reinterpret_cast<OT*>(a.out) + row * a.out_stride + (long long)(hk * g + hh) * D;

  int wmax = my_len > 0 ? my_len : 0;  // the wave's longest row
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const int o = __shfl_xor(wmax, s, 64);
    wmax = o > wmax ? o : wmax;
  }
  wmax = __builtin_amdgcn_readfirstlane(wmax);
  if (lane == 0) wave_len[wave] = wmax;
  __syncthreads();
  int lmax = wave_len[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) lmax = wave_len[w] > lmax ? wave_len[w] : lmax;
  lmax = __builtin_amdgcn_readfirstlane(lmax);

  f32x4 acc[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -__builtin_inff(), l_run = 0.0f;
  int fb = INT_MAX;  // the first key with a table entry outside the cache

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
    int nt = (lmax + KT - 1) / KT;

    // the slots of key tile j, by wave 0: -1 for a key that is staged as zeros
    auto resolve = [&](int j) {
      if (wave != 0) return;
      const int p = j * KT + lane;
      long long s = -1;
      bool bad = false;
      if (p < lmax) {
        const unsigned blk = (unsigned)p / (unsigned)a.block_size, off = (unsigned)p - blk * (unsigned)a.block_size;
        s = (long long)a.block_table[(long long)b * a.table_stride + blk] * a.block_size + off;
        bad = s < 0 || s >= a.n_slots;
      }
      const unsigned long long mask = __ballot(bad);
      const int first = mask ? (int)__builtin_ctzll(mask) : KT;
      slots[j & 1][lane] = (p < lmax && lane < first) ? (int)s : -1;
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
          const uint32_t word = (j & 1) ? __builtin_amdgcn_perm(hi, lo, 0x07060302u) : __builtin_amdgcn_perm(hi, lo, 0x05040100u);
          *reinterpret_cast<uint32_t*>(&vs[buf][(dc * 8 + j) * VROW + pos]) = word;
        }
      }
    };

    resolve(0);
    __syncthreads();
    if (fb_tile[0] != INT_MAX) {
      fb = fb_tile[0];
      nt = 1;
    }
    fetch(0);
    stage(0);
    if (nt > 1) resolve(1);
    __syncthreads();

    for (int i = 0; i < nt; ++i) {
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
            sc[jb][e] = kidx < my_len ? a.scale * s[jb][e] : -__builtin_inff();
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
            sc[jb][e] = kidx < my_len ? expf(sc[jb][e] - m_use) : 0.0f;
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
  const bool nan_row = my_len < 0 || my_len > fb;
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
static hipError_t launch_attn_prefill_inst(const AttnPrefillArgs& k, const AttnCall& c, hipStream_t stream) {
  hipLaunchKernelGGL((sqllm_attn_prefill_kernel<D, OT>), dim3(k.n_tiles, c.n_kv_heads, c.batch), dim3(kAttnThreads), 0, stream, k);
  return hipGetLastError();
}

// geometry from HOST fields only; what is not served is an error, never another kernel
static hipError_t launch_attn_prefill(const AttnCall& c, hipStream_t stream) {
  if (!prefill_served(c) || c.fp8) return hipErrorInvalidValue;  // (byte caches: sqllm_attn_prefill_fp8.hip, a slot of its own)
  const AttnPrefillArgs k = make_prefill_args(c);
  if (c.bf16) return c.head_dim == 64 ? launch_attn_prefill_inst<64, __bf16>(k, c, stream) : launch_attn_prefill_inst<128, __bf16>(k, c, stream);
  return c.head_dim == 64 ? launch_attn_prefill_inst<64, _Float16>(k, c, stream) : launch_attn_prefill_inst<128, _Float16>(k, c, stream);
}

// the host layer reaches the launcher through its slot (sqllm_kernels.h), so that it links without this file too
static const bool g_attn_prefill_registered = (g_launch_attn_prefill = launch_attn_prefill, true);

}  // namespace sqllm
