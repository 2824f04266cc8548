// sqllm_dequant.hip -- the packed-to-dense direction (include/sqllm_hip.h: sqllm_dequant): ONE kernel writes
//     W[n, k] = lookup_table[n, idx(k, n)] + sum CSR(n, k) + sum_c [full_row_indices[c] == n] full_rows[k, c]
// as an [N, ld] matrix with k contiguous (nn.Linear.weight), fp32, fp16 or bf16, every element rounded once from its fp32 sum.
//
// The packed words are contiguous along N, the output along K: the kernel is a decode plus a transpose.  What is transposed
// is the PACKED tile (4 bytes per 8 or 10.7 weights), not the decoded one: both formats are a plain little-endian bit
// stream per output channel (weight k of a channel sits at bit BITS * k of the channel's column of words; for 3 bits that
// is exactly the 11 + 11 + 10 layout with its two straddlers), so once a channel's words of a chunk lie in LDS a lane
// cuts the BITS * 8 bits of eight consecutive k's out of two neighbouring words with one 64-bit shift.
//
// A workgroup (4 waves) owns 64 output channels x 512 k's:
//   1. its words (64 or 48 rows of 64 channels) go global -> LDS with lane = channel (256-byte rows, coalesced), row stride
//      65 dwords; the 64 codebooks and rows[n0 .. n0 + 64] go to LDS beside them;
//   2. each wave then takes 16 channels, one at a time, lane = k: word reads at (row, channel) hit 32 different banks per
//      half wave (the rows of a half wave are distinct or equal), the codebook of the ONE channel a wave is on is 8 / 16
//      consecutive dwords, so the lookups are conflict-free too;
//   3. a channel without outliers goes straight from registers to memory.  One with outliers (a CSR row that is not empty, a
//      top-X column whose index is this channel) parks its 512 fp32 values in a wave-private LDS row, the wave walks the
//      channel's CSR row -- its first 64 entries were requested one channel earlier -- and the matching top-X columns and
//      adds what falls into the chunk (CSR: LDS float atomics, lanes may meet on a k; top-X: plain adds, lane = k; one add of
//      one value = the bits of one fp32 add; duplicates accumulate), and the lanes read the row back.  Which channels of the
//      tile have a top-X column at all is marked once per workgroup in step 1.  No workgroup barrier after step 1;
//   4. every store is 16 bytes per lane and a wave's store instruction covers 1024 contiguous bytes of one output row
//      (fp16 / bf16: lane = 8 k's; fp32: lane = 4 k's, twice, 256 k's apart).
// The body is ONE device template over the output type; sqllm_dequant_kernel<BITS, F16> (fp32 / fp16) and
// sqllm_dequant_bf16_kernel<BITS> are its kernels -- the 16-bit paths differ in the final conversion and the type of the
// 16-byte store alone.
// Per weight: BITS / 8 bytes read, 2 or 4 written, one LDS lookup; designed to be bound by the HBM writes (what a
// measurement says about that: DESIGN.md 4.5).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sqllm_hip.h"
#include "sqllm_host.h"

namespace sqllm {

constexpr int kDqThreads = 256;
constexpr int kDqWaves = kDqThreads / 64;
constexpr int kDqTileN = 64;    // output channels per workgroup
constexpr int kDqChunkK = 512;  // k's per workgroup: what one wave writes of one channel per pass
constexpr int kDqStride = 65;   // dwords per row of the word tile (lane = channel writes, lane = row reads: both conflict-free)

struct DequantArgs {
  const uint32_t* qweight;
  const float* lut;
  const int* rows;
  const int* cols;
  const float* vals;
  const float* full_rows;
  const int* full_idx;
  void* out;
  int64_t ld;
  int K, N, nnz, topX;
};

// slot of chunk-local k in a wave's parked row: the lane that owns k reads its values back as whole 16-byte slots,
// consecutive lanes from consecutive slots (fp32 output: a lane owns k's 4 * lane + 256 r: the identity)
template <bool F16>
__device__ __forceinline__ int park_slot(int kl) {
  return F16 ? (((((kl >> 2) & 1) << 6) + (kl >> 3)) << 2) + (kl & 3) : kl;
}

__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// OT: the output element -- float, _Float16 or __bf16 (F16 below: a 16-bit output, eight k's per lane and store)
template <int BITS, typename OT>
__device__ __forceinline__ void dequant_tile(const DequantArgs& a) {
  constexpr bool F16 = sizeof(OT) == 2;
  constexpr int E = 1 << BITS;
  constexpr int kRows = kDqChunkK * BITS / 32;  // word rows of a whole chunk
  __shared__ uint32_t wt[(kRows + 1) * kDqStride];  // (+ 1: the upper word of the last row's 64-bit window is read, never used)
  __shared__ float lut_s[kDqTileN * E];
  __shared__ int rows_s[kDqTileN + 1];
  __shared__ int tx_s[kDqTileN];  // != 0: some top-X column's index is this channel
  __shared__ __attribute__((aligned(16))) float park[kDqWaves][kDqChunkK];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.y * kDqTileN;
  const int k0 = blockIdx.x * kDqChunkK;
  const int K = a.K, N = a.N;
  const int kc = min(kDqChunkK, K - k0);  // k's of this chunk (a multiple of 32)
  const int nrows = kc * BITS / 32;
  const size_t row0 = (size_t)(k0 / 32) * BITS;

  // ---- 1. words, codebooks and row pointers of the tile -> LDS
  if (n0 + lane < N) {
    const uint32_t* src = a.qweight + row0 * (size_t)N + n0 + lane;
#pragma unroll 4
    for (int r = wave; r < nrows; r += kDqWaves) wt[r * kDqStride + lane] = __builtin_nontemporal_load(src + (size_t)r * N);
  }
  for (int i = tid; i < kDqTileN * E; i += kDqThreads) {
    const size_t g = (size_t)n0 * E + i;
    lut_s[i] = g < (size_t)N * E ? a.lut[g] : 0.f;
  }
  if (tid <= kDqTileN) {
    int v = 0;
    if (a.rows) {
      v = a.rows[min(n0 + tid, N)];
      v = max(0, min(v, a.nnz));  // (a malformed rows[] must not send the walk outside cols / vals)
    }
    rows_s[tid] = v;
  }
  // top-X: one pass of the workgroup over the indices marks the channels of this tile that have a column at all
  const int topX = a.full_rows ? a.topX : 0;
  if (tid < kDqTileN) tx_s[tid] = 0;
  __syncthreads();
  for (int c = tid; c < topX; c += kDqThreads) {
    const unsigned nl = (unsigned)(a.full_idx[c] - n0);
    if (nl < (unsigned)kDqTileN) tx_s[nl] = 1;  // (every writer stores the same value)
  }
  __syncthreads();

  // ---- 2.-4. one channel per wave and pass
  float* prow = park[wave];
  int e0 = rows_s[wave], e1 = rows_s[wave + 1];
  int col = -1;
  float val = 0.f;
  if (n0 + wave < N && e0 + lane < e1) {
    col = a.cols[e0 + lane];
    val = a.vals[e0 + lane];
  }
  for (int nl = wave; nl < kDqTileN; nl += kDqWaves) {
    const int n = n0 + nl;
    if (n >= N) break;
    // this channel's first CSR entries are here; request the next channel's
    const int ce0 = e0, ce1 = e1, ccol = col;
    const float cval = val;
    const int nn = nl + kDqWaves;
    col = -1;
    val = 0.f;
    if (nn < kDqTileN && n0 + nn < N) {
      e0 = rows_s[nn];
      e1 = rows_s[nn + 1];
      if (e0 + lane < e1) {
        col = a.cols[e0 + lane];
        val = a.vals[e0 + lane];
      }
    }

    // decode: two runs of 4 k's (fp32 output) or one of 8 (fp16) per lane
    float acc[8];
    const float* lut_n = lut_s + nl * E;
#pragma unroll
    for (int r = 0; r < (F16 ? 1 : 2); ++r) {
      constexpr int R = F16 ? 8 : 4;
      const int kl = F16 ? 8 * lane : 4 * lane + 256 * r;
      const int bit = kl * BITS;
      const uint32_t lo = wt[(bit >> 5) * kDqStride + nl], hi = wt[((bit >> 5) + 1) * kDqStride + nl];
      const uint32_t w = (uint32_t)((((uint64_t)hi << 32) | lo) >> (bit & 31));
#pragma unroll
      for (int j = 0; j < R; ++j) acc[r * R + j] = lut_n[(w >> (BITS * j)) & (E - 1)];
    }

    // outliers of this channel
    const bool has_tx = __builtin_amdgcn_readfirstlane(tx_s[nl]) != 0;
    if (ce1 > ce0 || has_tx) {
      *reinterpret_cast<float4*>(prow + 4 * lane) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      *reinterpret_cast<float4*>(prow + 256 + 4 * lane) = make_float4(acc[4], acc[5], acc[6], acc[7]);
      wave_sync_lds();
      // CSR row: the requested entries, then whatever a long row has beyond them
      {
        const unsigned kl = (unsigned)(ccol - k0);
        if (ccol >= 0 && kl < (unsigned)kc) atomicAdd(prow + park_slot<F16>((int)kl), cval);
      }
      for (int e = ce0 + 64 + lane; e < ce1; e += 64) {
        const unsigned kl = (unsigned)(a.cols[e] - k0);
        if (kl < (unsigned)kc) atomicAdd(prow + park_slot<F16>((int)kl), a.vals[e]);
      }
      // top-X columns whose index is this channel (duplicates accumulate): a lane owns the k's lane + 64 i here, so these
      // are plain adds, ordered behind the CSR atomics of the other lanes by the wave's own LDS order
      if (has_tx) {
        wave_sync_lds();
        for (int base = 0; base < topX; base += 64) {
          uint64_t tx = __ballot(base + lane < topX && a.full_idx[base + lane] == n);
          while (tx) {
            const int c = base + __builtin_ctzll(tx);
            tx &= tx - 1;
            for (int kl = lane; kl < kc; kl += 64) {
              float* p = prow + park_slot<F16>(kl);
              *p = *p + a.full_rows[(size_t)(k0 + kl) * topX + c];
            }
          }
        }
      }
      wave_sync_lds();
      const float4 p0 = *reinterpret_cast<const float4*>(prow + 4 * lane);
      const float4 p1 = *reinterpret_cast<const float4*>(prow + 256 + 4 * lane);
      acc[0] = p0.x; acc[1] = p0.y; acc[2] = p0.z; acc[3] = p0.w;
      acc[4] = p1.x; acc[5] = p1.y; acc[6] = p1.z; acc[7] = p1.w;
      wave_sync_lds();  // (the next channel's parking must not overtake these reads)
    }

    // store: 16 bytes per lane, 1024 contiguous bytes per wave and instruction
    const int64_t o = (int64_t)n * a.ld + k0;
    if (F16) {
      if (8 * lane < kc) {
        typedef OT h8 __attribute__((ext_vector_type(8)));
        h8 h;
#pragma unroll
        for (int j = 0; j < 8; ++j) h[j] = (OT)acc[j];  // (one rounding, to nearest-even, of the fp32 sum)
        *reinterpret_cast<h8*>(static_cast<OT*>(a.out) + o + 8 * lane) = h;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int kl = 4 * lane + 256 * r;
        if (kl < kc)
          *reinterpret_cast<float4*>(static_cast<float*>(a.out) + o + kl) =
              make_float4(acc[4 * r], acc[4 * r + 1], acc[4 * r + 2], acc[4 * r + 3]);
      }
    }
  }
}

template <int BITS, bool F16>
__global__ void __launch_bounds__(kDqThreads) sqllm_dequant_kernel(const DequantArgs a) {
  dequant_tile<BITS, typename std::conditional<F16, _Float16, float>::type>(a);
}

template <int BITS>
__global__ void __launch_bounds__(kDqThreads) sqllm_dequant_bf16_kernel(const DequantArgs a) {
  dequant_tile<BITS, __bf16>(a);
}

}  // namespace sqllm

using namespace sqllm;

extern "C" int sqllm_dequant(const sqllm_dequant_desc* d, sqllm_stream_t stream) {
  if (!d) return SQLLM_E_NULL;
  const sqllm_op* op = &d->op;
  if (op->bits != 3 && op->bits != 4) return SQLLM_E_BITS;
  if (op->K <= 0 || op->N <= 0 || (op->K % 32) != 0 || (op->N % 4) != 0) return SQLLM_E_SHAPE;
  if (d->out_dtype != SQLLM_DTYPE_F32 && d->out_dtype != SQLLM_DTYPE_F16 && d->out_dtype != SQLLM_DTYPE_BF16) return SQLLM_E_SHAPE;
  if (d->ld < op->K || (d->ld % (d->out_dtype == SQLLM_DTYPE_F32 ? 4 : 8)) != 0) return SQLLM_E_SHAPE;
  if (!d->out || !op->qweight || !op->lookup_table) return SQLLM_E_NULL;
  if ((reinterpret_cast<uintptr_t>(op->qweight) & 15u) != 0 || (reinterpret_cast<uintptr_t>(d->out) & 15u) != 0) return SQLLM_E_ALIGN;
  int rc = sqllm_host::validate_sparse(op);
  if (rc != SQLLM_OK) return rc;
  rc = sqllm_host::validate_csr_values(op, stream);  // (option "validate_csr"; a no-op by default)
  if (rc != SQLLM_OK) return rc;

  DequantArgs a;
  a.qweight = reinterpret_cast<const uint32_t*>(op->qweight);
  a.lut = op->lookup_table;
  const bool csr = op->rows && op->nnz > 0;
  a.rows = csr ? op->rows : nullptr;
  a.cols = csr ? op->cols : nullptr;
  a.vals = csr ? op->vals : nullptr;
  a.nnz = csr ? op->nnz : 0;
  const bool topx = op->full_rows && op->topX > 0;
  a.full_rows = topx ? op->full_rows : nullptr;
  a.full_idx = topx ? op->full_row_indices : nullptr;
  a.topX = topx ? op->topX : 0;
  a.out = d->out;
  a.ld = d->ld;
  a.K = op->K;
  a.N = op->N;
  // x: K chunks (neighbouring workgroups share the CSR rows and codebooks of a column tile), y: column tiles
  const dim3 grid((op->K + kDqChunkK - 1) / kDqChunkK, (op->N + kDqTileN - 1) / kDqTileN);
  if (grid.y > 65535u) return SQLLM_E_SHAPE;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool f16 = d->out_dtype == SQLLM_DTYPE_F16;
  if (d->out_dtype == SQLLM_DTYPE_BF16) {
    if (op->bits == 4) hipLaunchKernelGGL((sqllm_dequant_bf16_kernel<4>), grid, dim3(kDqThreads), 0, s, a);
    else hipLaunchKernelGGL((sqllm_dequant_bf16_kernel<3>), grid, dim3(kDqThreads), 0, s, a);
  } else if (op->bits == 4) {
    if (f16) hipLaunchKernelGGL((sqllm_dequant_kernel<4, true>), grid, dim3(kDqThreads), 0, s, a);
    else hipLaunchKernelGGL((sqllm_dequant_kernel<4, false>), grid, dim3(kDqThreads), 0, s, a);
  } else {
    if (f16) hipLaunchKernelGGL((sqllm_dequant_kernel<3, true>), grid, dim3(kDqThreads), 0, s, a);
    else hipLaunchKernelGGL((sqllm_dequant_kernel<3, false>), grid, dim3(kDqThreads), 0, s, a);
  }
  return static_cast<int>(hipGetLastError());
}
