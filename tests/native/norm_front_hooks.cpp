// norm_front_hooks.cpp -- the norm fronts' C entry points on the host layer alone (csrc/sqllm_capi.hip linked against
// tests/native/launch_recorder.cpp with -DSQLLM_RECORDER_NO_MAIN: no device code, nothing is launched, operand pointers are
// fake).  Built and run by tests/test_norm_front_capi_cpu.py; prints one line per step, the test reads them.
//   1. no kernel file is linked in, so every hook is null: a launch that passes validation is an ERROR (hipErrorNotSupported),
//      for the parent entries and the norm entries alike -- never a fallback;
//   2. with recording hooks set, the parent entries reach the parent hooks only, the norm entries the norm hooks only, and the
//      norm hooks receive the weight and eps of the descriptor and the parent's launch arguments.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "sqllm_hip.h"
#include "sqllm_kernels.h"

namespace {

template <class T>
T* fake(uintptr_t v) { return reinterpret_cast<T*>(v); }

int n_gated, n_qkv, n_gated_norm, n_qkv_norm;
sqllm::VecNorm last_vn;
const void* last_x;
void* last_pair;
int last_n_seg;

hipError_t rec_gated(int, const sqllm::LaunchArgs& a, void* pair, hipStream_t) { ++n_gated; last_x = a.x; last_pair = pair; last_n_seg = a.ga.n_seg; return hipSuccess; }
hipError_t rec_qkv(int, const sqllm::LaunchArgs& a, const sqllm::QkvRope& r, hipStream_t) { ++n_qkv; last_x = a.x; last_pair = r.pair_q; last_n_seg = a.ga.n_seg; return hipSuccess; }
hipError_t rec_gated_norm(int, const sqllm::LaunchArgs& a, void* pair, const sqllm::VecNorm& vn, hipStream_t) {
  ++n_gated_norm; last_vn = vn; last_x = a.x; last_pair = pair; last_n_seg = a.ga.n_seg; return hipSuccess;
}
hipError_t rec_qkv_norm(int, const sqllm::LaunchArgs& a, const sqllm::QkvRope& r, const sqllm::VecNorm& vn, hipStream_t) {
  ++n_qkv_norm; last_vn = vn; last_x = a.x; last_pair = r.pair_q; last_n_seg = a.ga.n_seg; return hipSuccess;
}

void fill(sqllm_op* op, int N, uintptr_t base) {
  memset(op, 0, sizeof(*op));
  op->bits = 4; op->batch = 2; op->K = 128; op->N = N;
  op->vec = fake<const float>(0x1000);
  op->qweight = fake<const int32_t>(base);
  op->lookup_table = fake<const float>(base + 0x4000);
}

}  // namespace

int main() {
  if (sqllm_set_option("cu_count", 256) != SQLLM_OK) return 2;
  sqllm_gated g;
  memset(&g, 0, sizeof(g));
  fill(&g.gate, 128, 0x20000);
  fill(&g.up, 128, 0x30000);
  g.out = fake<void>(0x100000);
  g.workspace = fake<void>(0x400000);
  g.act = SQLLM_ACT_SILU;
  sqllm_qkv_rope r;
  memset(&r, 0, sizeof(r));
  fill(&r.q, 256, 0x20000);
  fill(&r.k, 128, 0x30000);
  fill(&r.v, 128, 0x40000);
  r.out_q = fake<void>(0x100000); r.out_k = fake<void>(0x110000); r.out_v = fake<void>(0x120000);
  r.cos = fake<const float>(0x200000); r.sin = fake<const float>(0x210000); r.positions = fake<const int32_t>(0x220000);
  r.n_pos = 16; r.head_dim = 64; r.layout = SQLLM_ROPE_HALF;
  r.workspace = fake<void>(0x400000);
  const sqllm_rmsnorm nm = {fake<const void>(0x300000), 1e-5f};

  printf("nohook gated=%d gated_norm=%d qkv=%d qkv_norm=%d notsupported=%d\n", sqllm_gated_f16(&g, nullptr), sqllm_gated_norm_f16(&g, &nm, nullptr),
         sqllm_qkv_rope_bf16(&r, nullptr), sqllm_qkv_rope_norm_bf16(&r, &nm, nullptr), (int)hipErrorNotSupported);

  sqllm::g_launch_linear_gated = rec_gated;
  sqllm::g_launch_linear_qkv = rec_qkv;
  printf("parenthooks gated=%d gated_norm=%d qkv=%d qkv_norm=%d calls=%d,%d,%d,%d\n", sqllm_gated_bf16(&g, nullptr), sqllm_gated_norm_bf16(&g, &nm, nullptr),
         sqllm_qkv_rope_f16(&r, nullptr), sqllm_qkv_rope_norm_f16(&r, &nm, nullptr), n_gated, n_qkv, n_gated_norm, n_qkv_norm);

  sqllm::g_launch_linear_gated_norm = rec_gated_norm;
  sqllm::g_launch_linear_qkv_norm = rec_qkv_norm;
  n_gated = n_qkv = n_gated_norm = n_qkv_norm = 0;
  int rc = sqllm_gated_f16(&g, nullptr);
  const void* parent_pair = last_pair;
  printf("gated rc=%d calls=%d,%d,%d,%d n_seg=%d\n", rc, n_gated, n_qkv, n_gated_norm, n_qkv_norm, last_n_seg);
  rc = sqllm_gated_norm_f16(&g, &nm, nullptr);
  printf("gated_norm rc=%d calls=%d,%d,%d,%d n_seg=%d weight=%p eps=%.9g x=%p same_pair=%d\n", rc, n_gated, n_qkv, n_gated_norm, n_qkv_norm, last_n_seg,
         last_vn.weight, (double)last_vn.eps, last_x, (int)(last_pair == parent_pair));
  rc = sqllm_qkv_rope_bf16(&r, nullptr);
  parent_pair = last_pair;
  printf("qkv rc=%d calls=%d,%d,%d,%d n_seg=%d\n", rc, n_gated, n_qkv, n_gated_norm, n_qkv_norm, last_n_seg);
  rc = sqllm_qkv_rope_norm_bf16(&r, &nm, nullptr);
  printf("qkv_norm rc=%d calls=%d,%d,%d,%d n_seg=%d weight=%p eps=%.9g x=%p same_pair=%d\n", rc, n_gated, n_qkv, n_gated_norm, n_qkv_norm, last_n_seg,
         last_vn.weight, (double)last_vn.eps, last_x, (int)(last_pair == parent_pair));
  return 0;
}
