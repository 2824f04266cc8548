// sqllm_encode.hip -- the dense-to-packed direction (include/sqllm_hip.h: sqllm_encode, sqllm_encode_csr): from a weight
// matrix [N, ld] (k contiguous, nn.Linear.weight) and its per-channel codebooks to the operands the kernels consume,
//     qweight[K/32*bits, N]  (the index of the nearest codebook entry of every weight, as pack2's bit stream),
//     rows[N + 1], cols[nnz], vals[nnz]  (the masked weights that differ from the zero-nearest entry z_n, minus z_n).
// It is sqllm_dequant.hip run backwards: the weights are contiguous along K, the packed words along N, and what is
// transposed is again the PACKED tile (a plain little-endian bit stream per output channel: weight k of a channel sits at
// bit BITS * k of the channel's column of words; for 3 bits that is the 11 + 11 + 10 layout with its two straddlers).
//
// sqllm_encode_kernel: a workgroup (4 waves) owns 64 output channels x 512 k's.
//   1. the 64 codebooks go to LDS; each wave then takes 16 channels, one at a time, lane = 8 k's (fp16: one 16-byte
//      load; fp32: two, 256 k's apart, and one exchange between neighbouring lanes gives every lane 8 consecutive k's).
//      The next channel's weights and mask bytes are requested before this channel's are worked on;
//      Without a mask (a wave-uniform NULL test) the mask bytes are zeros and the same code runs;
//   2. per weight: the first j minimising |w - c_j| in fp32 (strict <, ascending j: nuq.assign_indices), the codebook of
//      the ONE channel a wave is on being wave-uniform.  A masked position gets the index of z_n instead and counts as an
//      outlier iff w != 0 and fl32(w - z_n) != 0 (pack.outliers_to_csr);
//   3. the lane's 8 * BITS bits go into the word tile in LDS, [word row][64 channels], row stride 65 dwords (4 bits: one
//      word per lane; 3 bits: four lanes make three words, each lane gets its neighbour's bits by one shuffle);
//   4. the outliers of the channel's chunk are counted with ballots (integers: no order dependence) and added to
//      rows[n + 1] with one integer atomic per channel and chunk (rows was zero-filled in front of the kernel);
//   5. after one barrier the workgroup stores the tile with lane = channel: 256-byte rows, coalesced along N.
// sqllm_encode_scan_kernel then turns the counts into the exclusive scan in place (one workgroup).
//
// sqllm_encode_csr_kernel: one wave per channel walks the channel's mask row in ascending k, 8 mask bytes per lane and
// step, fetches the weights under non-zero mask bytes, and places every outlier at rows[n] + (its rank within the
// channel) -- a prefix sum over the lanes, no atomics: the output is deterministic and in ascending k.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sqllm_hip.h"

namespace sqllm {

constexpr int kEnThreads = 256;
constexpr int kEnWaves = kEnThreads / 64;
constexpr int kEnTileN = 64;    // output channels per workgroup
constexpr int kEnChunkK = 512;  // k's per workgroup: what one wave reads of one channel per pass
constexpr int kEnStride = 65;   // dwords per row of the word tile (lane = row writes, lane = channel reads: both conflict-free)
constexpr int kScanThreads = 1024;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct EncodeArgs {
  const void* weight;
  const float* lut;
  const uint8_t* mask;
  uint32_t* qweight;
  int* rows;
  int* cols;
  float* vals;
  int64_t ld;
  int K, N, nnz;
};

// what a lane holds of one channel's chunk: fp16, k's 8 lane .. 8 lane + 7 (one load); fp32, k's 4 lane + 256 r .. + 3
template <bool F16>
struct Raw {
  u32x4 w[F16 ? 1 : 2];
  uint32_t m[2];  // mask bytes of the same k's, 4 per word
};

template <bool F16>
__device__ __forceinline__ Raw<F16> load_raw(const EncodeArgs& a, int n, int k0, int kc, int lane) {
  const bool MASK = a.mask != nullptr;  // (wave-uniform)
  Raw<F16> r;
  const int64_t o = (int64_t)n * a.ld + k0;
  const size_t mo = (size_t)n * a.K + k0;
  if (F16) {
    const bool on = 8 * lane < kc;
    r.w[0] = on ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(static_cast<const _Float16*>(a.weight) + o + 8 * lane)) : u32x4{0, 0, 0, 0};
    uint2 m = make_uint2(0, 0);
    if (MASK && on) m = *reinterpret_cast<const uint2*>(a.mask + mo + 8 * lane);
    r.m[0] = m.x;
    r.m[1] = m.y;
  } else {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kl = 4 * lane + 256 * h;
      const bool on = kl < kc;
      r.w[h] = on ? __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(static_cast<const float*>(a.weight) + o + kl)) : u32x4{0, 0, 0, 0};
      r.m[h] = (MASK && on) ? *reinterpret_cast<const uint32_t*>(a.mask + mo + kl) : 0u;
    }
  }
  return r;
}

template <int BITS, bool F16>
__global__ void __launch_bounds__(kEnThreads) sqllm_encode_kernel(const EncodeArgs a) {
  constexpr int E = 1 << BITS;
  constexpr int kRows = kEnChunkK * BITS / 32;  // word rows of a whole chunk
  __shared__ uint32_t wt[kRows * kEnStride];
  __shared__ __attribute__((aligned(16))) float lut_s[kEnTileN * E];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.y * kEnTileN;
  const int k0 = blockIdx.x * kEnChunkK;
  const int K = a.K, N = a.N;
  const int kc = min(kEnChunkK, K - k0);  // k's of this chunk (a multiple of 32)
  const int nrows = kc * BITS / 32;

  Raw<F16> next = {};
  if (n0 + wave < N) next = load_raw<F16>(a, n0 + wave, k0, kc, lane);
  for (int i = tid; i < kEnTileN * E; i += kEnThreads) {
    const size_t g = (size_t)n0 * E + i;
    lut_s[i] = g < (size_t)N * E ? a.lut[g] : 0.f;
  }
  __syncthreads();

  // the octet (8 consecutive k's of the chunk) whose bits this lane ends up with
  const int oct = F16 ? lane : (lane >> 1) + 32 * (lane & 1);
  const bool oct_on = 8 * oct < kc;

#pragma unroll 1
  for (int nl = wave; nl < kEnTileN; nl += kEnWaves) {
    const int n = n0 + nl;
    if (n >= N) break;
    const Raw<F16> cur = next;
    if (nl + kEnWaves < kEnTileN && n + kEnWaves < N) next = load_raw<F16>(a, n + kEnWaves, k0, kc, lane);

    // the channel's codebook (wave-uniform) and its zero-nearest entry (smallest |c|, ties to the lowest index)
    float c[E];
#pragma unroll
    for (int j = 0; j < E; j += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(lut_s + nl * E + j);
      c[j] = v.x; c[j + 1] = v.y; c[j + 2] = v.z; c[j + 3] = v.w;
    }
    float z = c[0];
    uint32_t jz = 0;
    {
      float az = __builtin_fabsf(z);
#pragma unroll
      for (int j = 1; j < E; ++j) {
        const bool u = __builtin_fabsf(c[j]) < az;
        az = u ? __builtin_fabsf(c[j]) : az;
        z = u ? c[j] : z;
        jz = u ? (uint32_t)j : jz;
      }
    }

    float w[8];
    if (F16) {
      const h8 h = __builtin_bit_cast(h8, cur.w[0]);
#pragma unroll
      for (int j = 0; j < 8; ++j) w[j] = (float)h[j];
    } else {
#pragma unroll
      for (int h = 0; h < 2; ++h) {  // (whole-vector casts: element subscripts of the array member read element 0 only)
        const f32x4 f = __builtin_bit_cast(f32x4, cur.w[h]);
        w[4 * h] = f.x; w[4 * h + 1] = f.y; w[4 * h + 2] = f.z; w[4 * h + 3] = f.w;
      }
    }

    // the eight weights side by side, one codebook entry at a time (a scheduling barrier per entry: left to itself the
    // scheduler keeps the compare masks of many entries alive at once and overflows the SGPRs)
    float best[8];
    uint32_t idx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      best[j] = __builtin_fabsf(w[j] - c[0]);
      idx[j] = 0;
    }
#pragma unroll
    for (int e = 1; e < E; ++e) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = __builtin_fabsf(w[j] - c[e]);
        const bool u = d < best[j];
        best[j] = u ? d : best[j];
        idx[j] = u ? (uint32_t)e : idx[j];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    uint32_t part[2] = {0, 0};  // BITS * 4 bits each: the indices of w[0..3] and of w[4..7]
    uint32_t flags = 0;         // bit j: w[j] is an outlier
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      uint32_t ix = idx[j];
      {  // (without a mask the mask bytes are zeros)
        const bool masked = ((cur.m[j >> 2] >> (8 * (j & 3))) & 0xffu) != 0;
        ix = masked ? jz : ix;
        if (masked && w[j] != 0.f && (w[j] - z) != 0.f) flags |= 1u << j;
      }
      part[j >> 2] |= ix << (BITS * (j & 3));
    }

    // the 8 * BITS bits of octet `oct`
    uint32_t b;
    if (F16) {
      b = part[0] | (part[1] << (4 * BITS));
    } else {
      // lanes 2m / 2m + 1 hold the halves of octets m (first load) and 32 + m (second): the even lane keeps the first
      const uint32_t got = (uint32_t)__shfl_xor((int)((lane & 1) ? part[0] : part[1]), 1);
      b = (lane & 1) ? (got | (part[1] << (4 * BITS))) : (part[0] | (got << (4 * BITS)));
    }
    if (BITS == 4) {
      wt[oct * kEnStride + nl] = b;  // (unconditionally: the rows of a short chunk's missing octets are never stored)
    } else {
      // four octets = 96 bits = three words: the lanes of octets 4q, 4q + 1, 4q + 2 write one each
      const uint32_t nb = (uint32_t)__shfl_down((int)b, F16 ? 1 : 2);  // the bits of octet oct + 1
      const int j = oct & 3;
      if (oct_on && j < 3) wt[((oct >> 2) * 3 + j) * kEnStride + nl] = (b >> (8 * j)) | (nb << (24 - 8 * j));
    }

    {
      if (__ballot(flags != 0) != 0) {  // (wave-uniform)
        int total = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) total += __popcll(__ballot((flags >> j) & 1u));
        if (lane == 0) atomicAdd(a.rows + n + 1, total);
      }
    }
  }
  __syncthreads();

  // the tile, lane = channel: 256-byte rows
  if (n0 + lane < N) {
    uint32_t* dst = a.qweight + (size_t)(k0 / 32) * BITS * (size_t)N + n0 + lane;
    for (int r = wave; r < nrows; r += kEnWaves) dst[(size_t)r * N] = wt[r * kEnStride + lane];
  }
}

// rows[1 .. N] holds per-channel counts, rows[0] is 0: make it their running sum, in place
__global__ void __launch_bounds__(kScanThreads) sqllm_encode_scan_kernel(int* __restrict__ rows, int N) {
  __shared__ int part[kScanThreads];
  const int t = threadIdx.x;
  const int seg = (N + kScanThreads - 1) / kScanThreads;
  const int64_t b64 = 1 + (int64_t)t * seg;
  const int b = (int)min(b64, (int64_t)N + 1), e = (int)min(b64 + seg, (int64_t)N + 1);
  int s = 0;
  for (int i = b; i < e; ++i) s += rows[i];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < kScanThreads; off <<= 1) {
    const int v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;
  for (int i = b; i < e; ++i) {
    run += rows[i];
    rows[i] = run;
  }
  if (t == 0) rows[0] = 0;
}

template <bool F16>
__global__ void __launch_bounds__(kEnThreads) sqllm_encode_csr_kernel(const EncodeArgs a, const int E) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int n = blockIdx.x * kEnWaves + wave;
  const int K = a.K;
  if (n >= a.N) return;
  // (rows[] that does not come from sqllm_encode must not send a store outside cols / vals)
  const int base = max(0, min(a.rows[n], a.nnz));
  const int end = max(base, min(a.rows[n + 1], a.nnz));
  if (end <= base) return;

  const float* c = a.lut + (size_t)n * E;
  float z = c[0], az = __builtin_fabsf(z);
  for (int j = 1; j < E; ++j) {
    const float v = c[j];
    if (__builtin_fabsf(v) < az) {
      az = __builtin_fabsf(v);
      z = v;
    }
  }

  const uint8_t* mrow = a.mask + (size_t)n * K;
  const int64_t wo = (int64_t)n * a.ld;
  int pos = base;  // wave-uniform: where the next outlier of the channel goes
  for (int k0 = 0; k0 < K && pos < end; k0 += 8 * 64) {
    const int k = k0 + 8 * lane;
    uint2 m = make_uint2(0, 0);
    if (k < K) m = *reinterpret_cast<const uint2*>(mrow + k);
    if (__ballot((m.x | m.y) != 0) == 0) continue;
    uint32_t flags = 0;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = 0.f;
      if ((((j < 4 ? m.x : m.y) >> (8 * (j & 3))) & 0xffu) != 0) {
        const float w = F16 ? (float)static_cast<const _Float16*>(a.weight)[wo + k + j] : static_cast<const float*>(a.weight)[wo + k + j];
        v[j] = w - z;
        if (w != 0.f && v[j] != 0.f) flags |= 1u << j;
      }
    }
    const int cnt = __popc(flags);
    int incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int up = __shfl_up(incl, off);
      if (lane >= off) incl += up;
    }
    int p = pos + incl - cnt;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if ((flags >> j) & 1u) {
        if (p < end) {
          a.cols[p] = k + j;
          a.vals[p] = v[j];
        }
        ++p;
      }
    }
    pos += __shfl(incl, 63);
  }
}

static int validate_encode(const sqllm_encode_desc* d) {
  if (!d) return SQLLM_E_NULL;
  if (d->bits != 3 && d->bits != 4) return SQLLM_E_BITS;
  if (d->K <= 0 || d->N <= 0 || (d->K % 32) != 0 || (d->N % 4) != 0) return SQLLM_E_SHAPE;
  if (d->weight_dtype != SQLLM_DTYPE_F32 && d->weight_dtype != SQLLM_DTYPE_F16) return SQLLM_E_SHAPE;
  if (d->ld < d->K || (d->ld % (d->weight_dtype == SQLLM_DTYPE_F16 ? 8 : 4)) != 0) return SQLLM_E_SHAPE;
  if ((d->N + kEnTileN - 1) / kEnTileN > 65535) return SQLLM_E_SHAPE;
  if (!d->weight || !d->lookup_table || !d->qweight) return SQLLM_E_NULL;
  if (d->mask && !d->rows) return SQLLM_E_NULL;
  if ((reinterpret_cast<uintptr_t>(d->weight) & 15u) != 0 || (reinterpret_cast<uintptr_t>(d->qweight) & 15u) != 0) return SQLLM_E_ALIGN;
  if ((reinterpret_cast<uintptr_t>(d->mask) & 7u) != 0) return SQLLM_E_ALIGN;
  return SQLLM_OK;
}

static EncodeArgs encode_args(const sqllm_encode_desc* d) {
  EncodeArgs a;
  a.weight = d->weight;
  a.lut = d->lookup_table;
  a.mask = d->mask;
  a.qweight = reinterpret_cast<uint32_t*>(d->qweight);
  a.rows = d->rows;
  a.cols = nullptr;
  a.vals = nullptr;
  a.ld = d->ld;
  a.K = d->K;
  a.N = d->N;
  a.nnz = 0;
  return a;
}

template <int BITS, bool F16>
static void launch_encode(const EncodeArgs& a, dim3 grid, hipStream_t s) {
  hipLaunchKernelGGL((sqllm_encode_kernel<BITS, F16>), grid, dim3(kEnThreads), 0, s, a);
}

}  // namespace sqllm

using namespace sqllm;

extern "C" int sqllm_encode(const sqllm_encode_desc* d, sqllm_stream_t stream) {
  const int rc = validate_encode(d);
  if (rc != SQLLM_OK) return rc;
  const EncodeArgs a = encode_args(d);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (a.mask) {  // the counts are added into rows[1 .. N] by integer atomics: zero in front
    const hipError_t e = hipMemsetAsync(a.rows, 0, ((size_t)a.N + 1) * sizeof(int), s);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  // x: K chunks, y: column tiles
  const dim3 grid((a.K + kEnChunkK - 1) / kEnChunkK, (a.N + kEnTileN - 1) / kEnTileN);
  const bool f16 = d->weight_dtype == SQLLM_DTYPE_F16;
  if (d->bits == 4) {
    if (f16) launch_encode<4, true>(a, grid, s);
    else launch_encode<4, false>(a, grid, s);
  } else {
    if (f16) launch_encode<3, true>(a, grid, s);
    else launch_encode<3, false>(a, grid, s);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return static_cast<int>(e);
  if (a.mask) {
    hipLaunchKernelGGL(sqllm_encode_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, a.rows, a.N);
    e = hipGetLastError();
  }
  return static_cast<int>(e);
}

extern "C" int sqllm_encode_csr(const sqllm_encode_desc* d, int32_t* cols, float* vals, int32_t nnz, sqllm_stream_t stream) {
  const int rc = validate_encode(d);
  if (rc != SQLLM_OK) return rc;
  if (!d->mask || !d->rows || !cols || !vals) return SQLLM_E_NULL;
  if (nnz < 0) return SQLLM_E_SPARSE;
  EncodeArgs a = encode_args(d);
  a.cols = cols;
  a.vals = vals;
  a.nnz = nnz;
  const dim3 grid((a.N + kEnWaves - 1) / kEnWaves);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (d->weight_dtype == SQLLM_DTYPE_F16) hipLaunchKernelGGL((sqllm_encode_csr_kernel<true>), grid, dim3(kEnThreads), 0, s, a, 1 << d->bits);
  else hipLaunchKernelGGL((sqllm_encode_csr_kernel<false>), grid, dim3(kEnThreads), 0, s, a, 1 << d->bits);
  return static_cast<int>(hipGetLastError());
}
