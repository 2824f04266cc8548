// sqllm_select.hip -- outlier selection (include/sqllm_hip.h: sqllm_select, sqllm_outlier_mask): exact order statistics of
// a whole matrix, and the byte mask sqllm_encode takes, without a sort and without a host round trip.
//
// sqllm_select is a most-significant-digit radix select.  Every element becomes an order-preserving unsigned key
// (-0 -> +0 first; negative: all bits flipped, non-negative: sign bit set): 32 bits for fp32, and for fp16 the SAME
// construction on the 16 bits of the half itself (the widening is monotone and exact, so the key of the half orders as
// the key of the float would; the value comes back by widening the half the final key stands for).  The key is consumed
// in digits of 11 + 11 + 10 bits (fp32: three passes over the matrix) or 11 + 5 bits (fp16: two).  Per digit:
//   sqllm_select_hist_kernel   every workgroup (8 waves, at most 512 of them: one resident round) walks its share of the
//     matrix with 16-byte non-temporal loads, four in flight per lane, and counts digits in LDS.  The FIRST digit has one
//     live prefix (the empty one) and every element counts: 2048 bins x 8 copies, one per wave.  The top digit of weight
//     data is skewed; taking 11 bits instead of 8 carries two (fp32) / five (fp16) mantissa bits into it, which spreads
//     each hot exponent over 4 / 32 bins, and the per-wave copies keep the eight waves off each other's counters.  A
//     LATER digit counts only elements whose higher bits equal one of the (at most 8) live prefixes -- one range test
//     against [lowest, highest] prefix rejects what lies outside (for a quartile pair, half the matrix) -- into one
//     histogram per DISTINCT prefix: ranks that share a prefix (the two order statistics either side of a quartile do,
//     down to the last digit) share a histogram.
//     Non-empty bins are added to the 64-bit global counters with integer atomics.
//   sqllm_select_pick_kernel   one workgroup: per live prefix an exclusive scan of its 2048 counters; every rank finds the
//     bin that holds it, extends its prefix by that digit, subtracts what lies below from its remaining rank and adds it
//     to its running `less`; the distinct new prefixes become the next pass's histograms.  After the last digit the prefix
//     IS the key: out[i] is its value, less[i] the running count.
// All state lives in the caller's workspace; the host enqueues one memset node (the counters) and 2 x passes kernels and
// learns nothing in between.  Only integers are counted: the result is a function of the input alone.
//
// sqllm_outlier_mask_kernel: lane = 8 consecutive k's of one channel (one 16-byte load of fp16, two of fp32, per operand),
// mask[n, k] = g > *g_threshold || w >= *w_threshold || w <= -*w_threshold as one 8-byte store; the ones are counted per
// lane, summed over the workgroup and added to *count by one integer atomic per workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sqllm_hip.h"

namespace sqllm {

constexpr int kSelThreads = 512;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelBins = 2048;     // counters per histogram: the widest digit
constexpr int kSelMaxGrid = 512;   // workgroups of the histogram kernel: two of 64 KB LDS per CU, one resident round
constexpr int kSelUnroll = 4;      // 16-byte loads in flight per lane
constexpr int kPickThreads = 256;
constexpr int kPickPer = kSelBins / kPickThreads;
constexpr int kMaskThreads = 256;
constexpr int kMaskMaxRows = 2048;  // workgroup rows of the mask kernel (grid-stride over the channels beyond)
constexpr uint32_t kNoPrefix = 0xffffffffu;  // (a live prefix has at most 22 bits)

static_assert(kSelWaves == SQLLM_SELECT_MAX_RANKS, "the LDS histogram serves 8 per-wave copies or 8 live prefixes");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// what one pass hands to the next (in the workspace, behind the counters); written whole by every pick kernel
struct SelState {
  uint32_t n_groups;
  uint32_t gprefix[SQLLM_SELECT_MAX_RANKS];  // the distinct live prefixes; unused slots hold kNoPrefix
  uint32_t group[SQLLM_SELECT_MAX_RANKS];    // per rank: its prefix's slot
  int64_t rem[SQLLM_SELECT_MAX_RANKS];       // per rank: its position among the elements that share its prefix
  int64_t less[SQLLM_SELECT_MAX_RANKS];      // per rank: elements below its prefix
};

struct HistArgs {
  const void* values;
  int64_t rows, nvec, ld;  // nvec: 16-byte vectors per row
  unsigned long long* hist;  // this pass: [max_groups][kSelBins]
  const SelState* state;
  int shift, bits, max_groups;
};

__device__ __forceinline__ uint32_t key_f32(uint32_t u) {
  u = (u << 1) == 0 ? 0u : u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t key_f16(uint32_t h) {  // h < 2^16
  h = (h & 0x7fffu) == 0 ? 0u : h;
  return (h & 0x8000u) ? (~h & 0xffffu) : (h | 0x8000u);
}

template <bool F16, bool FIRST>
__global__ void __launch_bounds__(kSelThreads) sqllm_select_hist_kernel(const HistArgs a) {
  __shared__ uint32_t h[SQLLM_SELECT_MAX_RANKS * kSelBins];
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  uint32_t gp[SQLLM_SELECT_MAX_RANKS];
  uint32_t gmin = 0, gspan = 0;
  int ng = 1;
  if (!FIRST) {
    ng = min((int)a.state->n_groups, a.max_groups);
    uint32_t gmax = 0;
    gmin = kNoPrefix;
#pragma unroll
    for (int g = 0; g < SQLLM_SELECT_MAX_RANKS; ++g) {
      gp[g] = g < ng ? a.state->gprefix[g] : kNoPrefix;
      if (g < ng) {
        gmin = min(gmin, gp[g]);
        gmax = max(gmax, gp[g]);
      }
    }
    gspan = gmax - gmin;
  }
  const int used = (FIRST ? kSelWaves : ng) * kSelBins;
  for (int i = tid; i < used; i += kSelThreads) h[i] = 0;
  __syncthreads();

  const int shift = a.shift;
  const uint32_t bmask = (1u << a.bits) - 1u;
  uint32_t* mine = h + wave * kSelBins;
  auto count = [&](uint32_t key) {
    if (FIRST) {
      atomicAdd(mine + (key >> shift), 1u);
    } else {
      const uint32_t pfx = (key >> shift) >> a.bits;
      if (pfx - gmin <= gspan) {
        int gi = -1;
#pragma unroll
        for (int g = 0; g < SQLLM_SELECT_MAX_RANKS; ++g) gi = pfx == gp[g] ? g : gi;
        if (gi >= 0) atomicAdd(h + gi * kSelBins + ((key >> shift) & bmask), 1u);
      }
    }
  };

  const int64_t vstride = (int64_t)gridDim.x * kSelThreads;
  for (int64_t r = blockIdx.y; r < a.rows; r += gridDim.y) {
    const u32x4* row = reinterpret_cast<const u32x4*>(static_cast<const char*>(a.values) + r * a.ld * (F16 ? 2 : 4));
    for (int64_t v = (int64_t)blockIdx.x * kSelThreads + tid; v < a.nvec; v += kSelUnroll * vstride) {
      u32x4 x[kSelUnroll];
#pragma unroll
      for (int u = 0; u < kSelUnroll; ++u) {
        const int64_t vu = v + u * vstride;
        x[u] = vu < a.nvec ? __builtin_nontemporal_load(row + vu) : u32x4{0, 0, 0, 0};
      }
#pragma unroll
      for (int u = 0; u < kSelUnroll; ++u) {
        if (v + u * vstride < a.nvec) {
          const uint32_t w[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (F16) {
              count(key_f16(w[j] & 0xffffu));
              count(key_f16(w[j] >> 16));
            } else {
              count(key_f32(w[j]));
            }
          }
        }
      }
    }
  }
  __syncthreads();

  if (FIRST) {
    for (int b = tid; b < kSelBins; b += kSelThreads) {
      uint32_t c = 0;
#pragma unroll
      for (int wv = 0; wv < kSelWaves; ++wv) c += h[wv * kSelBins + b];
      if (c) atomicAdd(a.hist + b, (unsigned long long)c);
    }
  } else {
    for (int i = tid; i < used; i += kSelThreads) {
      const uint32_t c = h[i];
      if (c) atomicAdd(a.hist + i, (unsigned long long)c);
    }
  }
}

struct PickArgs {
  const unsigned long long* hist;  // this pass: [max_groups][kSelBins]
  SelState* state;                 // read (not in the first pass) and rewritten
  int64_t ranks[SQLLM_SELECT_MAX_RANKS];
  float* out;
  int64_t* less;
  int n_ranks, bits, first, last, f16;
};

__global__ void __launch_bounds__(kPickThreads) sqllm_select_pick_kernel(const PickArgs a) {
  __shared__ unsigned long long scan[kPickThreads];
  __shared__ uint32_t s_gp[SQLLM_SELECT_MAX_RANKS], s_grp[SQLLM_SELECT_MAX_RANKS], n_pref[SQLLM_SELECT_MAX_RANKS];
  __shared__ long long s_rem[SQLLM_SELECT_MAX_RANKS], s_less[SQLLM_SELECT_MAX_RANKS], n_rem[SQLLM_SELECT_MAX_RANKS], n_less[SQLLM_SELECT_MAX_RANKS];
  __shared__ int s_ng;
  const int tid = threadIdx.x;
  const int nr = a.n_ranks;
  if (tid < SQLLM_SELECT_MAX_RANKS) {
    if (a.first) {
      s_gp[tid] = tid == 0 ? 0u : kNoPrefix;
      s_grp[tid] = 0;
      s_rem[tid] = a.ranks[tid];
      s_less[tid] = 0;
    } else {
      s_gp[tid] = a.state->gprefix[tid];
      s_grp[tid] = min(a.state->group[tid], (uint32_t)(SQLLM_SELECT_MAX_RANKS - 1));
      s_rem[tid] = a.state->rem[tid];
      s_less[tid] = a.state->less[tid];
    }
  }
  if (tid == 0) s_ng = a.first ? 1 : min((int)a.state->n_groups, nr);
  __syncthreads();
  if (tid < SQLLM_SELECT_MAX_RANKS) {  // (a rank no bin claims -- counts that do not add up: NaN-free input cannot -- keeps bin 0)
    n_pref[tid] = s_gp[s_grp[tid]] << a.bits;
    n_rem[tid] = s_rem[tid];
    n_less[tid] = s_less[tid];
  }
  const int ng = s_ng;
  const int nb = 1 << a.bits;
  for (int g = 0; g < ng; ++g) {
    unsigned long long c[kPickPer], sum = 0;
#pragma unroll
    for (int j = 0; j < kPickPer; ++j) {
      const int b = tid * kPickPer + j;
      c[j] = b < nb ? a.hist[(size_t)g * kSelBins + b] : 0ull;
      sum += c[j];
    }
    scan[tid] = sum;
    __syncthreads();
    for (int off = 1; off < kPickThreads; off <<= 1) {
      const unsigned long long v = tid >= off ? scan[tid - off] : 0ull;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const unsigned long long incl = scan[tid], excl = incl - sum;
    for (int i = 0; i < nr; ++i) {
      if ((int)s_grp[i] != g) continue;  // (uniform: LDS values)
      const unsigned long long rem = (unsigned long long)s_rem[i];
      if (rem >= excl && rem < incl) {
        unsigned long long below = excl;
        int bin = 0;
        bool found = false;
#pragma unroll
        for (int j = 0; j < kPickPer; ++j) {
          if (!found) {
            if (rem < below + c[j]) {
              bin = tid * kPickPer + j;
              found = true;
            } else {
              below += c[j];
            }
          }
        }
        n_pref[i] = (s_gp[g] << a.bits) | (uint32_t)bin;
        n_rem[i] = (long long)(rem - below);
        n_less[i] = s_less[i] + (long long)below;
      }
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid != 0) return;
  if (a.last) {
    for (int i = 0; i < nr; ++i) {
      const uint32_t key = n_pref[i];
      float v;
      if (a.f16) {
        const uint16_t hb = (uint16_t)((key & 0x8000u) ? (key ^ 0x8000u) : (~key & 0xffffu));
        v = (float)__builtin_bit_cast(_Float16, hb);
      } else {
        v = __builtin_bit_cast(float, (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
      }
      a.out[i] = v;
      if (a.less) a.less[i] = n_less[i];
    }
    return;
  }
  // the distinct prefixes, in order of first appearance
  SelState* st = a.state;
  uint32_t n = 0;
  for (int i = 0; i < SQLLM_SELECT_MAX_RANKS; ++i) st->gprefix[i] = kNoPrefix;
  for (int i = 0; i < SQLLM_SELECT_MAX_RANKS; ++i) {
    uint32_t slot = 0;
    if (i < nr) {
      slot = n;
      for (uint32_t j = 0; j < n; ++j)
        if (st->gprefix[j] == n_pref[i]) slot = j;
      if (slot == n) st->gprefix[n++] = n_pref[i];
    }
    st->group[i] = slot;
    st->rem[i] = i < nr ? n_rem[i] : 0;
    st->less[i] = i < nr ? n_less[i] : 0;
  }
  st->n_groups = n;
}

struct MaskArgs {
  const void* weight;
  const void* gradient;
  const float* g_threshold;
  const float* w_threshold;
  uint8_t* mask;
  unsigned long long* count;
  int64_t ld_w, ld_g;
  int K, N;
};

// 8 consecutive elements of a row as fp32
template <bool F16>
__device__ __forceinline__ void load8(const void* base, int64_t off, float (&v)[8]) {
  if (F16) {
    const h8 x = __builtin_bit_cast(h8, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(static_cast<const _Float16*>(base) + off)));
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)x[j];
  } else {
    const u32x4* p = reinterpret_cast<const u32x4*>(static_cast<const float*>(base) + off);
    const f32x4 lo = __builtin_bit_cast(f32x4, __builtin_nontemporal_load(p));
    const f32x4 hi = __builtin_bit_cast(f32x4, __builtin_nontemporal_load(p + 1));
    v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
    v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
  }
}

template <bool WF16, bool GF16>
__global__ void __launch_bounds__(kMaskThreads) sqllm_outlier_mask_kernel(const MaskArgs a) {
  __shared__ uint32_t part[kMaskThreads / 64];
  const int tid = threadIdx.x;
  const bool has_g = a.gradient != nullptr, has_t = a.w_threshold != nullptr;  // (uniform)
  const float gt = has_g ? *a.g_threshold : 0.f;
  const float wt = has_t ? *a.w_threshold : 0.f;
  const int octs = a.K / 8;
  uint32_t ones = 0;
  for (int n = blockIdx.y; n < a.N; n += gridDim.y) {
    for (int o = blockIdx.x * kMaskThreads + tid; o < octs; o += gridDim.x * kMaskThreads) {
      float w[8], g[8];
      load8<WF16>(a.weight, (int64_t)n * a.ld_w + 8 * o, w);
      if (has_g) load8<GF16>(a.gradient, (int64_t)n * a.ld_g + 8 * o, g);
      uint32_t m[2] = {0, 0};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        bool on = false;
        if (has_g) on = g[j] > gt;
        if (has_t) on = on || w[j] >= wt || w[j] <= -wt;
        m[j >> 2] |= (on ? 1u : 0u) << (8 * (j & 3));
      }
      ones += __popc(m[0]) + __popc(m[1]);
      if (a.mask) *reinterpret_cast<uint2*>(a.mask + (size_t)n * a.K + 8 * o) = make_uint2(m[0], m[1]);
    }
  }
  if (!a.count) return;  // (uniform)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ones += __shfl_down(ones, off);
  if ((tid & 63) == 0) part[tid >> 6] = ones;
  __syncthreads();
  if (tid == 0) {
    uint32_t total = 0;
#pragma unroll
    for (int wv = 0; wv < kMaskThreads / 64; ++wv) total += part[wv];
    if (total) atomicAdd(a.count, (unsigned long long)total);
  }
}

static bool known_dtype(int32_t t) { return t == SQLLM_DTYPE_F32 || t == SQLLM_DTYPE_F16; }
static int elems_per_vec(int32_t t) { return t == SQLLM_DTYPE_F16 ? 8 : 4; }
static int select_passes(int32_t t) { return t == SQLLM_DTYPE_F16 ? 2 : 3; }
static bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// everything about a select but its pointers
static int validate_select_shape(const sqllm_select_desc* d) {
  if (!d) return SQLLM_E_NULL;
  if (!known_dtype(d->dtype)) return SQLLM_E_SHAPE;
  if (d->n_ranks < 1 || d->n_ranks > SQLLM_SELECT_MAX_RANKS) return SQLLM_E_SHAPE;
  const int m = elems_per_vec(d->dtype);
  if (d->rows < 1 || d->cols < 1 || (d->cols % m) != 0 || d->ld < d->cols || (d->ld % m) != 0) return SQLLM_E_SHAPE;
  const int64_t lim = (int64_t)1 << 40;
  if (d->rows >= lim || d->cols >= lim || d->ld >= lim || d->rows > (lim - 1) / d->cols) return SQLLM_E_SHAPE;
  const int64_t total = d->rows * d->cols;
  for (int i = 0; i < d->n_ranks; ++i)
    if (d->ranks[i] < 0 || d->ranks[i] >= total) return SQLLM_E_SHAPE;
  return SQLLM_OK;
}

static int64_t select_hist_bytes(const sqllm_select_desc* d) {
  return (int64_t)select_passes(d->dtype) * d->n_ranks * kSelBins * (int64_t)sizeof(unsigned long long);
}

static int validate_outlier(const sqllm_outlier_desc* d) {
  if (!d) return SQLLM_E_NULL;
  if (d->K <= 0 || d->N < 1 || (d->K % 32) != 0) return SQLLM_E_SHAPE;
  // the select's bound.  It keeps the 32-bit counts of a lane and of a workgroup from wrapping: with 64 workgroups across K
  // (K > 63 * 2048) and min(N, 2048) down the channels a workgroup sees about N K / 2^17 elements, or K / 64 < 2^25 of one
  // channel; with fewer across K it sees at most 2048 elements of a channel and ceil(N / 2048) <= 2^20 channels.
  static_assert(kMaskMaxRows == 2048 && kMaskThreads * 8 == 2048, "the bound below is argued for these");
  if ((int64_t)d->N * d->K >= ((int64_t)1 << 40)) return SQLLM_E_SHAPE;
  if (!known_dtype(d->weight_dtype) || (d->gradient && !known_dtype(d->grad_dtype))) return SQLLM_E_SHAPE;
  if (d->ld_w < d->K || (d->ld_w % elems_per_vec(d->weight_dtype)) != 0) return SQLLM_E_SHAPE;
  if (d->gradient && (d->ld_g < d->K || (d->ld_g % elems_per_vec(d->grad_dtype)) != 0)) return SQLLM_E_SHAPE;
  if (!d->weight || (d->gradient != nullptr) != (d->g_threshold != nullptr) || (!d->mask && !d->count)) return SQLLM_E_NULL;
  if (misaligned(d->weight, 16) || misaligned(d->gradient, 16) || misaligned(d->mask, 8) || misaligned(d->count, 8) ||
      misaligned(d->g_threshold, 4) || misaligned(d->w_threshold, 4))
    return SQLLM_E_ALIGN;
  return SQLLM_OK;
}

template <bool F16>
static void launch_hist(bool first, const HistArgs& a, dim3 grid, hipStream_t s) {
  if (first) hipLaunchKernelGGL((sqllm_select_hist_kernel<F16, true>), grid, dim3(kSelThreads), 0, s, a);
  else hipLaunchKernelGGL((sqllm_select_hist_kernel<F16, false>), grid, dim3(kSelThreads), 0, s, a);
}

}  // namespace sqllm

using namespace sqllm;

extern "C" int64_t sqllm_select_workspace_bytes(const sqllm_select_desc* d) {
  const int rc = validate_select_shape(d);
  if (rc != SQLLM_OK) return rc;
  return select_hist_bytes(d) + (int64_t)sizeof(SelState);
}

extern "C" int sqllm_select(const sqllm_select_desc* d, void* workspace, int64_t workspace_bytes, sqllm_stream_t stream) {
  const int rc = validate_select_shape(d);
  if (rc != SQLLM_OK) return rc;
  if (!d->values || !d->out || !workspace) return SQLLM_E_NULL;
  const int64_t hist_bytes = select_hist_bytes(d);
  if (workspace_bytes < hist_bytes + (int64_t)sizeof(SelState)) return SQLLM_E_SHAPE;
  if (misaligned(d->values, 16) || misaligned(workspace, 16) || misaligned(d->out, 4) || misaligned(d->less, 8)) return SQLLM_E_ALIGN;

  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(workspace, 0, (size_t)hist_bytes, s);  // the counters of every pass; the state is written before it is read
  if (e != hipSuccess) return static_cast<int>(e);

  const bool f16 = d->dtype == SQLLM_DTYPE_F16;
  const int passes = select_passes(d->dtype);
  const int digit[3] = {11, f16 ? 5 : 11, 10};
  HistArgs h;
  h.values = d->values;
  // rows without padding are one long row
  const bool flat = d->ld == d->cols;
  h.rows = flat ? 1 : d->rows;
  h.nvec = (flat ? d->rows * d->cols : d->cols) / elems_per_vec(d->dtype);
  h.ld = d->ld;
  h.state = reinterpret_cast<const SelState*>(static_cast<char*>(workspace) + hist_bytes);
  h.max_groups = d->n_ranks;
  const int gy = (int)(h.rows < kSelMaxGrid ? h.rows : kSelMaxGrid);
  const int64_t per = (int64_t)kSelThreads * kSelUnroll;
  int64_t gx = (h.nvec + per - 1) / per;
  if (gx > kSelMaxGrid / gy) gx = kSelMaxGrid / gy;
  const dim3 grid((unsigned)(gx < 1 ? 1 : gx), (unsigned)gy);

  PickArgs p;
  p.state = reinterpret_cast<SelState*>(static_cast<char*>(workspace) + hist_bytes);
  for (int i = 0; i < SQLLM_SELECT_MAX_RANKS; ++i) p.ranks[i] = i < d->n_ranks ? d->ranks[i] : 0;
  p.out = d->out;
  p.less = d->less;
  p.n_ranks = d->n_ranks;
  p.f16 = f16 ? 1 : 0;

  int shift = f16 ? 16 : 32;
  for (int pass = 0; pass < passes; ++pass) {
    shift -= digit[pass];
    h.hist = static_cast<unsigned long long*>(workspace) + (size_t)pass * d->n_ranks * kSelBins;
    h.shift = shift;
    h.bits = digit[pass];
    if (f16) launch_hist<true>(pass == 0, h, grid, s);
    else launch_hist<false>(pass == 0, h, grid, s);
    e = hipGetLastError();
    if (e != hipSuccess) return static_cast<int>(e);
    p.hist = h.hist;
    p.bits = digit[pass];
    p.first = pass == 0;
    p.last = pass == passes - 1;
    hipLaunchKernelGGL(sqllm_select_pick_kernel, dim3(1), dim3(kPickThreads), 0, s, p);
    e = hipGetLastError();
    if (e != hipSuccess) return static_cast<int>(e);
  }
  return SQLLM_OK;
}

extern "C" int sqllm_outlier_mask(const sqllm_outlier_desc* d, sqllm_stream_t stream) {
  const int rc = validate_outlier(d);
  if (rc != SQLLM_OK) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (d->count) {
    const hipError_t e = hipMemsetAsync(d->count, 0, sizeof(int64_t), s);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  MaskArgs a;
  a.weight = d->weight;
  a.gradient = d->gradient;
  a.g_threshold = d->g_threshold;
  a.w_threshold = d->w_threshold;
  a.mask = d->mask;
  a.count = reinterpret_cast<unsigned long long*>(d->count);
  a.ld_w = d->ld_w;
  a.ld_g = d->ld_g;
  a.K = d->K;
  a.N = d->N;
  const int octs = d->K / 8;
  int gx = (octs + kMaskThreads - 1) / kMaskThreads;
  if (gx > 64) gx = 64;
  const dim3 grid(gx, d->N < kMaskMaxRows ? d->N : kMaskMaxRows);
  const bool wf = d->weight_dtype == SQLLM_DTYPE_F16, gf = d->gradient && d->grad_dtype == SQLLM_DTYPE_F16;
  if (wf && gf) hipLaunchKernelGGL((sqllm_outlier_mask_kernel<true, true>), grid, dim3(kMaskThreads), 0, s, a);
  else if (wf) hipLaunchKernelGGL((sqllm_outlier_mask_kernel<true, false>), grid, dim3(kMaskThreads), 0, s, a);
  else if (gf) hipLaunchKernelGGL((sqllm_outlier_mask_kernel<false, true>), grid, dim3(kMaskThreads), 0, s, a);
  else hipLaunchKernelGGL((sqllm_outlier_mask_kernel<false, false>), grid, dim3(kMaskThreads), 0, s, a);
  return static_cast<int>(hipGetLastError());
}
