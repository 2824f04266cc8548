// sqllm_nuq.hip -- offline non-uniform quantisation: the exact Fisher-weighted 1-D k-means of every output channel
// (include/sqllm_hip.h: sqllm_nuq_fit).  Replaces the per-row sklearn KMeans of the reference's quantization/nuq.py
// (Lloyd from a k-means++ start: a local optimum) with the global optimum of
//     min over partitions of the sorted row into k contiguous ranges of  sum_r sum_{i in r} w_i (x_i - c_r)^2,
// c_r the weighted mean of range r (1-D optimal clusters are contiguous in sorted order).
//
// Method (Gronlund et al. 2017, "Fast exact k-means, k-medians and Bregman divergence clustering in 1D"):
//   prefix sums W, S, Q of w, w x, w x^2 in fp64 (fp32 cancels in Q - S^2 / W), cost(m, i) of range [m, i) =
//   dQ - dS^2 / dW; D_j(i) = min_m D_{j-1}(m) + cost(m, i); the leftmost argmin is monotone in i, so every level is a
//   divide and conquer over i: O(K log K) per level, O(k K log K) per row; the last level needs i = M only.
//   Equal values are merged first (exact: their weights add), which shrinks fp16-born rows a lot.
//
// Layout: one 256-thread workgroup per row, persistent over rows (grid = min(N, kMaxSlots)).  Each workgroup owns a
// slot of the caller's workspace (prefix sums, two DP rows, the merged boundaries, the k x (K+1) argmin table): K goes
// up to 22016 (65B down_proj), ~880 KB of fp64 per row, more than a CU's LDS.  The divide and conquer runs as passes of
// halving stride (bit-reversed order): in the pass of stride h the items u = h, 3h, 5h, ... (u = i - lo + 1) search
// m between the argmins of u - h and u + h, which earlier passes wrote.  A group of 16 lanes evaluates one item.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sqllm_hip.h"

namespace nuqk {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kGroup = 16;  // lanes per DP item
constexpr int kGroups = kThreads / kGroup;
constexpr int kMaxSlots = 1024;  // persistent workgroups (4 per CU on 256 CUs)
constexpr int kMaxK = 65535;     // argmins are stored as uint16
constexpr int64_t kAlign = 16;

__host__ __device__ inline int64_t align16(int64_t b) { return (b + kAlign - 1) / kAlign * kAlign; }

struct SlotLayout {
  int64_t fp64, bidx, arg, total;  // byte offsets inside one slot, slot size
};

__host__ __device__ inline SlotLayout slot_layout(int K, int k) {
  const int64_t n = int64_t(K) + 1;
  SlotLayout l;
  l.fp64 = 0;                          // W, S, Q, D0, D1: 5 x (K + 1) doubles
  l.bidx = align16(5 * 8 * n);         // int32 [K + 1]: original index where merged element p starts; [M] = K
  l.arg = l.bidx + align16(4 * n);     // uint16 [k][K + 1]: row j - 1 = argmin of level j
  l.total = l.arg + align16(2 * int64_t(k) * n);
  return l;
}

__device__ inline double range_cost(const double* __restrict__ W, const double* __restrict__ S, const double* __restrict__ Q,
                                     int m, int i) {
  const double dw = W[i] - W[m];
  if (!(dw > 0.0)) return 0.0;  // zero total weight: any centroid costs nothing
  const double ds = S[i] - S[m];
  const double c = (Q[i] - Q[m]) - ds * ds / dw;
  return c > 0.0 ? c : 0.0;  // (rounding can take an almost-constant range below 0: a negative cost would attract the DP)
}

// (value, index) minimum, ties to the smaller index, over the `width` lanes of a group
__device__ inline void argmin_reduce(double& v, int& m, int width) {
  for (int off = width / 2; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off, width);
    const int om = __shfl_xor(m, off, width);
    if (ov < v || (ov == v && om < m)) {
      v = ov;
      m = om;
    }
  }
}

__device__ inline double sum_reduce(double v, int width) {
  for (int off = width / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, width);
  return v;
}

struct Shared {
  double wave_tot[2][kWaves][3];  // block scan: per-wave totals (double-buffered across chunks)
  int wave_cnt[2][kWaves];
  double red_v[kWaves];
  int red_m[kWaves];
  int cut[17];                    // range boundaries (merged indices), cut[0] = 0, cut[k] = M
  double cent[16];
  double sse[16];
};

template <int KC>  // KC = 2^bits centroids
__global__ __launch_bounds__(kThreads) void nuq_fit_kernel(const float* __restrict__ values, const float* __restrict__ weights,
                                                           float* __restrict__ centroids, double* __restrict__ cost, int N, int K,
                                                           char* __restrict__ workspace) {
  __shared__ Shared sh;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int glane = tid & (kGroup - 1), group = tid / kGroup;
  const SlotLayout lay = slot_layout(K, KC);
  const int64_t n1 = int64_t(K) + 1;
  char* slot = workspace + int64_t(blockIdx.x) * lay.total;
  double* W = reinterpret_cast<double*>(slot + lay.fp64);
  double* S = W + n1;
  double* Q = S + n1;
  double* Dbuf[2] = {Q + n1, Q + 2 * n1};
  int* bidx = reinterpret_cast<int*>(slot + lay.bidx);
  uint16_t* arg = reinterpret_cast<uint16_t*>(slot + lay.arg);

  for (int row = blockIdx.x; row < N; row += gridDim.x) {
    const float* x = values + int64_t(row) * K;
    const float* wr = weights ? weights + int64_t(row) * K : nullptr;
    // a row whose weights sum to 0 is fitted with unit weights (nuq.py:174-175)
    int any = 0;
    if (wr)
      for (int i = tid; i < K; i += kThreads) any |= wr[i] > 0.f;
    const bool unit = !__syncthreads_or(any);

    // 1. merge equal values and scan: W/S/Q[p] = sums over the original elements before merged element p
    double carry_w = 0.0, carry_s = 0.0, carry_q = 0.0;
    int carry_n = 0;
    for (int c0 = 0, buf = 0; c0 < K; c0 += kThreads, buf ^= 1) {
      const int i = c0 + tid;
      double w = 0.0, xv = 0.0;
      int flag = 0;
      if (i < K) {
        const float xf = x[i];
        xv = xf;
        w = unit ? 1.0 : double(wr[i]);
        flag = (i == 0 || xf != x[i - 1]) ? 1 : 0;
      }
      double sw = w, ss = w * xv, sq = w * xv * xv;
      int sn = flag;
      for (int off = 1; off < 64; off <<= 1) {  // inclusive wave scan
        const double a = __shfl_up(sw, off), b = __shfl_up(ss, off), c = __shfl_up(sq, off);
        const int d = __shfl_up(sn, off);
        if (lane >= off) {
          sw += a;
          ss += b;
          sq += c;
          sn += d;
        }
      }
      if (lane == 63) {
        sh.wave_tot[buf][wave][0] = sw;
        sh.wave_tot[buf][wave][1] = ss;
        sh.wave_tot[buf][wave][2] = sq;
        sh.wave_cnt[buf][wave] = sn;
      }
      __syncthreads();
      double pw = carry_w, ps = carry_s, pq = carry_q;
      int pn = carry_n;
      for (int v = 0; v < kWaves; ++v) {
        if (v < wave) {
          pw += sh.wave_tot[buf][v][0];
          ps += sh.wave_tot[buf][v][1];
          pq += sh.wave_tot[buf][v][2];
          pn += sh.wave_cnt[buf][v];
        }
        carry_w += sh.wave_tot[buf][v][0];
        carry_s += sh.wave_tot[buf][v][1];
        carry_q += sh.wave_tot[buf][v][2];
        carry_n += sh.wave_cnt[buf][v];
      }
      // exclusive prefix: the inclusive one of the lane below (no subtraction: W[i] - W[m] is exactly 0 over zero weights)
      double ew = __shfl_up(sw, 1), es = __shfl_up(ss, 1), eq = __shfl_up(sq, 1);
      if (lane == 0) ew = es = eq = 0.0;
      if (flag) {
        const int p = pn + sn - 1;
        W[p] = pw + ew;
        S[p] = ps + es;
        Q[p] = pq + eq;
        bidx[p] = i;
      }
      // (the other buffer is rewritten next chunk only after that chunk's barrier: every thread has read this one by then)
    }
    const int M = carry_n;
    if (tid == 0) {
      W[M] = carry_w;
      S[M] = carry_s;
      Q[M] = carry_q;
      bidx[M] = K;
    }
    __syncthreads();

    if (M <= KC) {
      // as many ranges as distinct values (or more): one value each, cost 0; empty ranges repeat the last centroid
      if (tid <= KC) sh.cut[tid] = tid < M ? tid : M;
    } else {
      // 2. level 1: D_1(i) = cost(0, i), i in [1, M - KC + 1]
      double* Dp = Dbuf[0];
      for (int i = 1 + tid; i <= M - KC + 1; i += kThreads) Dp[i] = range_cost(W, S, Q, 0, i);
      __syncthreads();
      // 3. levels 2 .. KC - 1: i in [j, M - KC + j], m in [j - 1, i - 1], monotone leftmost argmin
      for (int j = 2; j < KC; ++j) {
        double* Dc = Dbuf[(j - 1) & 1];
        uint16_t* A = arg + int64_t(j - 1) * n1;
        const int lo = j, hi = M - KC + j, n = hi - lo + 1;
        int h = 1;
        while (h * 2 <= n) h *= 2;
        for (; h >= 1; h >>= 1) {
          const int cnt = (n / h + 1) / 2;  // odd multiples of h in [1, n]
          for (int q = group; q < cnt; q += kGroups) {
            const int u = h * (2 * q + 1), i = lo + u - 1;
            const int mlo = u - h == 0 ? j - 1 : int(A[i - h]);
            int mhi = u + h > n ? hi - 1 : int(A[i + h]);
            mhi = mhi < i - 1 ? mhi : i - 1;
            mhi = mhi > mlo ? mhi : mlo;  // (rounding in near-ties can break monotonicity: never search an empty range)
            double best = __builtin_huge_val();
            int bm = mlo;
            for (int m = mlo + glane; m <= mhi; m += kGroup) {
              const double v = Dp[m] + range_cost(W, S, Q, m, i);
              if (v < best) {
                best = v;
                bm = m;
              }
            }
            argmin_reduce(best, bm, kGroup);
            if (glane == 0) {
              Dc[i] = best;
              A[i] = uint16_t(bm);
            }
          }
          __syncthreads();
        }
        Dp = Dc;
      }
      // 4. last level: i = M only, the whole workgroup over m in [KC - 1, M - 1]
      double best = __builtin_huge_val();
      int bm = KC - 1;
      for (int m = KC - 1 + tid; m <= M - 1; m += kThreads) {
        const double v = Dp[m] + range_cost(W, S, Q, m, M);
        if (v < best) {
          best = v;
          bm = m;
        }
      }
      argmin_reduce(best, bm, 64);
      if (lane == 0) {
        sh.red_v[wave] = best;
        sh.red_m[wave] = bm;
      }
      __syncthreads();
      if (tid == 0) {
        double v = sh.red_v[0];
        int m = sh.red_m[0];
        for (int w = 1; w < kWaves; ++w)
          if (sh.red_v[w] < v || (sh.red_v[w] == v && sh.red_m[w] < m)) {
            v = sh.red_v[w];
            m = sh.red_m[w];
          }
        // backtrack
        sh.cut[KC] = M;
        sh.cut[KC - 1] = m;
        for (int jj = KC - 1; jj >= 2; --jj) sh.cut[jj - 1] = arg[int64_t(jj - 1) * n1 + sh.cut[jj]];
        sh.cut[0] = 0;
      }
    }
    __syncthreads();

    // 5. centroids and the exact cost, range by range over the original elements (two passes: no cancellation)
    for (int r = group; r < KC; r += kGroups) {
      const int a = bidx[sh.cut[r]], b = bidx[sh.cut[r + 1]];
      double sw = 0.0, swx = 0.0, sx = 0.0;
      for (int i = a + glane; i < b; i += kGroup) {
        const double xv = x[i], w = unit ? 1.0 : double(wr[i]);
        sw += w;
        swx += w * xv;
        sx += xv;
      }
      sw = sum_reduce(sw, kGroup);
      swx = sum_reduce(swx, kGroup);
      sx = sum_reduce(sx, kGroup);
      // a range of zero total weight: the unweighted mean of its values
      double c = sw > 0.0 ? swx / sw : (b > a ? sx / double(b - a) : 0.0);
      if (sh.cut[r + 1] - sh.cut[r] == 1) c = x[a];  // one distinct value: exactly it (a mean could round off it)
      double e = 0.0;
      for (int i = a + glane; i < b; i += kGroup) {
        const double xv = x[i], w = unit ? 1.0 : double(wr[i]);
        e += w * (xv - c) * (xv - c);
      }
      e = sum_reduce(e, kGroup);
      if (glane == 0) {
        sh.cent[r] = c;
        sh.sse[r] = b > a ? e : -1.0;  // -1: empty (fewer distinct values than centroids)
      }
    }
    __syncthreads();
    if (tid == 0) {
      double total = 0.0, prev = 0.0;
      for (int r = 0; r < KC; ++r) {
        double c = sh.cent[r];
        if (sh.sse[r] < 0.0) {
          c = prev;
        } else {
          total += sh.sse[r];
        }
        prev = c;
        centroids[int64_t(row) * KC + r] = float(c);
      }
      if (cost) cost[row] = total;
    }
    __syncthreads();  // (sh.cut / the slot are reused by the next row)
  }
}

}  // namespace nuqk

using namespace nuqk;

static int nuq_validate(const sqllm_nuq* d) {
  if (!d) return SQLLM_E_NULL;
  if (d->bits != 3 && d->bits != 4) return SQLLM_E_BITS;
  if (d->N < 1 || d->K < (1 << d->bits) || d->K > kMaxK) return SQLLM_E_SHAPE;
  if (!d->values || !d->centroids) return SQLLM_E_NULL;
  return SQLLM_OK;
}

extern "C" int64_t sqllm_nuq_workspace_bytes(const sqllm_nuq* d) {
  // (shapes only: the pointers are not looked at, so a descriptor of shapes sizes the workspace)
  if (!d) return SQLLM_E_NULL;
  if (d->bits != 3 && d->bits != 4) return SQLLM_E_BITS;
  if (d->N < 1 || d->K < (1 << d->bits) || d->K > kMaxK) return SQLLM_E_SHAPE;
  const int slots = d->N < kMaxSlots ? d->N : kMaxSlots;
  return int64_t(slots) * slot_layout(d->K, 1 << d->bits).total + kAlign;  // (+ room to align the base)
}

extern "C" int sqllm_nuq_fit(const sqllm_nuq* d, void* workspace, int64_t workspace_bytes, sqllm_stream_t stream) {
  const int rc = nuq_validate(d);
  if (rc != SQLLM_OK) return rc;
  if (!workspace) return SQLLM_E_NULL;
  if (workspace_bytes < sqllm_nuq_workspace_bytes(d)) return SQLLM_E_SHAPE;
  char* ws = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + kAlign - 1) / kAlign * kAlign);
  const int grid = d->N < kMaxSlots ? d->N : kMaxSlots;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (d->bits == 4)
    hipLaunchKernelGGL(nuq_fit_kernel<16>, dim3(grid), dim3(kThreads), 0, s, d->values, d->weights, d->centroids, d->cost, d->N, d->K, ws);
  else
    hipLaunchKernelGGL(nuq_fit_kernel<8>, dim3(grid), dim3(kThreads), 0, s, d->values, d->weights, d->centroids, d->cost, d->N, d->K, ws);
  return static_cast<int>(hipGetLastError());
}
