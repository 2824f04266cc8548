// launch_recorder.cpp -- the host layer (csrc/sqllm_capi.hip) linked against RECORDING launchers instead of the kernels:
// every function of sqllm_kernels.h that the host layer calls is defined here, notes its arguments and launches nothing.
// Built as plain C++ (no device code) by tests/test_capi_cpu.py::test_plan_query_reports_what_is_launched and run as a
// child process; needs no GPU.  Operand pointers are fake 16-byte-aligned integers: nothing dereferences them.
//
//   main: for single ops over bits x shapes x batches x sparse terms, launched through sqllm_launch_ws with an ample (fake)
//   workspace, one line per case: the geometry of the LAST dense launch and what sqllm_plan_query reports for the same op.
//   -DSQLLM_RECORDER_NO_MAIN leaves main to another file; rec_trace = true then prints every launch with every field.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "sqllm_hip.h"
#include "sqllm_kernels.h"

bool rec_trace = false;       // print every recorded launch
int rec_dense_launches = 0;   // dense launches seen since it was last reset
sqllm::KernelGeom rec_last;   // geometry of the last dense launch's first segment
char rec_last_name[48] = "";

namespace {

void print_geom(const sqllm::KernelGeom& g) {
  printf(" gm{K=%d N=%d batch=%d col_tiles=%d units_total=%d units_per_wg=%d k_slices=%d dense_blocks=%d dense_block0=%d csr_blocks=%d"
         " topx_blocks=%d nnz=%d topX=%d sparse_last=%d fold_csr=%d csr_wide=%d dense_prio=%d}",
         g.K, g.N, g.batch, g.col_tiles, g.units_total, g.units_per_wg, g.k_slices, g.dense_blocks, g.dense_block0, g.csr_blocks,
         g.topx_blocks, g.nnz, g.topX, g.sparse_last, g.fold_csr, g.csr_wide, g.dense_prio);
}

void print_args(const char* name, int bits, const sqllm::LaunchArgs& a) {
  printf("%s bits=%d x=%p linear=%d ev=%p,%p ablate=%d lds_pad=%d xT=%p Bp=%d planes=%p flags=%p wide=%d full_units=%d slabs=%p row_blocks=%d n_seg=%d block0=",
         name, bits, a.x, (int)a.linear, (void*)a.ev_start, (void*)a.ev_stop, a.ablate, a.lds_pad, (const void*)a.xT, a.Bp, a.planes,
         (const void*)a.plane_flags, (int)a.wide, a.wide_full_units, (void*)a.wide_slabs, a.row_blocks, a.ga.n_seg);
  for (int i = 0; i <= sqllm::kMaxSegments; ++i) printf("%s%d", i ? "," : "", a.ga.block0[i]);
  for (int i = 0; i < sqllm::kMaxSegments; ++i) {
    const sqllm::Segment& s = a.ga.seg[i];
    static const sqllm::KernelGeom no_geom = {};
    if (!s.q && !s.y && !s.lut && !s.rows && !s.cols && !s.vals && !s.full_rows && !s.full_idx && !s.bias && !s.out16 &&
        !memcmp(&s.gm, &no_geom, sizeof(no_geom))) {
      printf(" seg%d{0}", i);
      continue;
    }
    printf(" seg%d{q=%p y=%p lut=%p rows=%p cols=%p vals=%p full_rows=%p full_idx=%p bias=%p out16=%p", i, (const void*)s.q, (void*)s.y,
           (const void*)s.lut, (const void*)s.rows, (const void*)s.cols, (const void*)s.vals, (const void*)s.full_rows,
           (const void*)s.full_idx, (const void*)s.bias, s.out16);
    print_geom(s.gm);
    printf("}");
  }
  printf("\n");
}

hipError_t record(const char* name, int bits, const sqllm::LaunchArgs& a, bool dense) {
  if (rec_trace) print_args(name, bits, a);
  if (dense) {
    ++rec_dense_launches;
    rec_last = a.ga.seg[0].gm;
    snprintf(rec_last_name, sizeof(rec_last_name), "%s", name);
  }
  return hipSuccess;
}

}  // namespace

namespace sqllm {

hipError_t launch_fused(int bits, const LaunchArgs& a, hipStream_t) { return record("launch_fused", bits, a, true); }
hipError_t launch_batched_mfma(int bits, const LaunchArgs& a, hipStream_t) { return record("launch_batched_mfma", bits, a, true); }
hipError_t launch_batched_mfma_split(int bits, const LaunchArgs& a, hipStream_t) { return record("launch_batched_mfma_split", bits, a, true); }
hipError_t launch_batched_mfma_split_all(int bits, const LaunchArgs& a, hipStream_t) { return record("launch_batched_mfma_split_all", bits, a, true); }
hipError_t launch_batched_cols(int bits, const LaunchArgs& a, hipStream_t) { return record("launch_batched_cols", bits, a, true); }
hipError_t launch_small_split(int bits, const LaunchArgs& a, hipStream_t) { return record("launch_small_split", bits, a, true); }
hipError_t launch_batched_sparse(const LaunchArgs& a, hipStream_t) { return record("launch_batched_sparse", 0, a, false); }

hipError_t split_vec(const float* x, void* planes, uint32_t* flags, int batch, int K, hipStream_t, hipEvent_t ev) {
  if (rec_trace) printf("split_vec x=%p planes=%p flags=%p batch=%d K=%d ev=%p\n", (const void*)x, planes, (void*)flags, batch, K, (void*)ev);
  return hipSuccess;
}
hipError_t transpose_vec(const float* x, float* xT, int batch, int K, int Bp, hipStream_t, hipEvent_t ev) {
  if (rec_trace) printf("transpose_vec x=%p xT=%p batch=%d K=%d Bp=%d ev=%p\n", (const void*)x, (void*)xT, batch, K, Bp, (void*)ev);
  return hipSuccess;
}
hipError_t transpose_small(const float* x, float* xT, int batch, int K, hipStream_t, hipEvent_t ev) {
  if (rec_trace) printf("transpose_small x=%p xT=%p batch=%d K=%d ev=%p\n", (const void*)x, (void*)xT, batch, K, (void*)ev);
  return hipSuccess;
}
hipError_t prepare_small(const float* x, float* xT, void* planes, int batch, int K, hipStream_t, hipEvent_t ev) {
  if (rec_trace) printf("prepare_small x=%p xT=%p planes=%p batch=%d K=%d ev=%p\n", (const void*)x, (void*)xT, planes, batch, K, (void*)ev);
  return hipSuccess;
}
hipError_t check_csr(const int* rows, int N, int nnz, hipStream_t, int* bad) {
  if (rec_trace) printf("check_csr rows=%p N=%d nnz=%d\n", (const void*)rows, N, nnz);
  *bad = 0;
  return hipSuccess;
}

}  // namespace sqllm

#ifndef SQLLM_RECORDER_NO_MAIN
namespace {
template <class T>
T* fake(uintptr_t v) { return reinterpret_cast<T*>(v); }
}  // namespace

int main() {
  static const int shapes[][2] = {{4096, 4096}, {4096, 11008}, {11008, 4096}, {4096, 12288}, {5120, 5120}, {5120, 13824}, {13824, 5120},
                                  {8192, 8192}, {8192, 22016}, {22016, 8192}, {2560, 10240}, {7168, 28672}, {1024, 776}, {96, 68}, {32, 4}};
  static const int batches[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17, 32, 33, 40, 64, 100, 256, 340, 512, 2048};
  // sparse terms: dense only, 0.45 % CSR + 10 full rows, 2 % CSR + 10 full rows, CSR only, full rows only, 17 full rows (> 16)
  static const struct { double csr; int topX; } sparse[] = {{0, 0}, {0.0045, 10}, {0.02, 10}, {0.0045, 0}, {0, 10}, {0.0045, 17}};
  if (sqllm_set_option("cu_count", 256) != SQLLM_OK) return 2;
  void* const ws = fake<void>(0x40000000);  // ample, never touched: the launchers above launch nothing
  const int64_t ws_bytes = 1ll << 40;
  for (int bits = 3; bits <= 4; ++bits)
    for (const auto& kn : shapes)
      for (int batch : batches)
        for (const auto& sp : sparse) {
          if ((long long)batch * kn[0] >= (1ll << 31)) continue;
          sqllm_op op;
          memset(&op, 0, sizeof(op));
          op.bits = bits;
          op.batch = batch;
          op.K = kn[0];
          op.N = kn[1];
          op.vec = fake<const float>(0x1000);
          op.qweight = fake<const int32_t>(0x2000);
          op.mul = fake<float>(0x3000);
          op.lookup_table = fake<const float>(0x4000);
          if (sp.csr > 0) {
            op.rows = fake<const int32_t>(0x5000);
            op.cols = fake<const int32_t>(0x6000);
            op.vals = fake<const float>(0x7000);
            op.nnz = (int)(sp.csr * kn[0] * kn[1]);
            if (op.nnz < 1) op.nnz = 1;
          }
          if (sp.topX > 0) {
            op.full_rows = fake<const float>(0x8000);
            op.full_row_indices = fake<const int32_t>(0x9000);
            op.topX = sp.topX;
          }
          rec_dense_launches = 0;
          memset(&rec_last, 0, sizeof(rec_last));
          const int rc = sqllm_launch_ws(&op, ws, ws_bytes, nullptr);
          sqllm_plan p;
          memset(&p, 0, sizeof(p));
          const int rp = sqllm_plan_query(&op, &p);
          printf("case bits=%d K=%d N=%d batch=%d nnz=%d topX=%d rc=%d,%d dense_launches=%d via=%s launched=%d,%d,%d,%d,%d,%d plan=%d,%d,%d,%d,%d,%d\n",
                 bits, op.K, op.N, batch, op.nnz, op.topX, rc, rp, rec_dense_launches, rec_last_name, rec_last.col_tiles, rec_last.k_slices,
                 rec_last.units_per_wg, rec_last.dense_blocks, rec_last.csr_blocks, rec_last.topx_blocks, p.col_tiles, p.k_slices,
                 p.groups_per_wave, p.dense_blocks, p.csr_blocks, p.topx_blocks);
        }
  return 0;
}
#endif
