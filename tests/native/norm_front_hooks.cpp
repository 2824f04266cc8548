// norm_front_hooks.cpp -- the fronts' C entry points on the host layer alone (csrc/sqllm_capi.hip linked against
// tests/native/launch_recorder.cpp with -DSQLLM_RECORDER_NO_MAIN: no device code, nothing is launched, operand pointers are
// fake).  Built and run by tests/test_norm_front_capi_cpu.py; prints one line per step, the test reads them.
//   1. no kernel file is linked in, so every slot of g_launch_front is null: a launch that passes validation is an ERROR
//      (hipErrorNotSupported), for every one of the 18 front entries -- never a fallback;
//   2. with recording launchers in the parents' slots, the parent entries reach them and the norm entries still fail; with the
//      norm slots set too, the norm entries reach the norm slots only, with the weight and eps of the descriptor and the
//      parent's launch arguments;
//   3. with recording launchers in all nine slots, each of the 18 entries reaches the slot of its own kind and no other, with
//      the VecNorm, KvCache and QkvRope fields of its descriptors.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "sqllm_hip.h"
#include "sqllm_kernels.h"

namespace {

using namespace sqllm;

template <class T>
T* fake(uintptr_t v) { return reinterpret_cast<T*>(v); }

int calls[kFrontKinds];
// what the last launcher saw (the descriptors copied: they live on the host layer's stack)
struct Seen {
  const void* x;
  int n_seg;
  FrontCall f;
  QkvRope qkv;
  VecNorm vn;
  KvCache kc;
} last;

template <int KIND>
hipError_t rec(int, const LaunchArgs& a, const FrontCall& f, hipStream_t) {
  ++calls[KIND];
  memset(&last, 0, sizeof(last));
  last.x = a.x;
  last.n_seg = a.ga.n_seg;
  last.f = f;
  if (f.qkv) last.qkv = *f.qkv;
  if (f.vn) last.vn = *f.vn;
  if (f.kc) last.kc = *f.kc;
  return hipSuccess;
}
const FrontLauncher kRecorders[kFrontKinds] = {rec<0>, rec<1>, rec<2>, rec<3>, rec<4>, rec<5>, rec<6>, rec<7>, rec<8>};

unsigned long long ull(const void* p) { return (unsigned long long)reinterpret_cast<uintptr_t>(p); }
void* last_pair() { return last.f.pair ? last.f.pair : last.qkv.pair_q; }
void reset() { memset(calls, 0, sizeof(calls)); }
// (the four counters of steps 1 and 2, in the order the test has always read them)
void print_calls4() { printf("calls=%d,%d,%d,%d", calls[kFrontGated], calls[kFrontQkv], calls[kFrontGatedNorm], calls[kFrontQkvNorm]); }

void fill(sqllm_op* op, int N, uintptr_t base) {
  memset(op, 0, sizeof(*op));
  op->bits = 4; op->batch = 2; op->K = 128; op->N = N;
  op->vec = fake<const float>(0x1000);
  op->qweight = fake<const int32_t>(base);
  op->lookup_table = fake<const float>(base + 0x4000);
}

sqllm_gated g;
sqllm_linear_ep e;
sqllm_qkv_rope r;
const sqllm_rmsnorm nm = {fake<const void>(0x300000), 1e-5f};
const sqllm_kv_cache c = {fake<void>(0x800000), fake<void>(0x900000), fake<const int32_t>(0x230000), 8, 128, 64};
const sqllm_kv_cache_fp8 c8 = {fake<void>(0x800000), fake<void>(0x900000), fake<const int32_t>(0x230000), 8, 128, 64, 0.5f, 4.0f};

struct Entry {
  const char* name;
  int kind;
  int (*call)();
};
const Entry kEntries[18] = {
    {"sqllm_gated_f16", kFrontGated, [] { return sqllm_gated_f16(&g, nullptr); }},
    {"sqllm_gated_bf16", kFrontGated, [] { return sqllm_gated_bf16(&g, nullptr); }},
    {"sqllm_gated_norm_f16", kFrontGatedNorm, [] { return sqllm_gated_norm_f16(&g, &nm, nullptr); }},
    {"sqllm_gated_norm_bf16", kFrontGatedNorm, [] { return sqllm_gated_norm_bf16(&g, &nm, nullptr); }},
    {"sqllm_linear_ep_f16", kFrontEp, [] { return sqllm_linear_ep_f16(&e, nullptr); }},
    {"sqllm_linear_ep_bf16", kFrontEp, [] { return sqllm_linear_ep_bf16(&e, nullptr); }},
    {"sqllm_qkv_rope_f16", kFrontQkv, [] { return sqllm_qkv_rope_f16(&r, nullptr); }},
    {"sqllm_qkv_rope_bf16", kFrontQkv, [] { return sqllm_qkv_rope_bf16(&r, nullptr); }},
    {"sqllm_qkv_rope_norm_f16", kFrontQkvNorm, [] { return sqllm_qkv_rope_norm_f16(&r, &nm, nullptr); }},
    {"sqllm_qkv_rope_norm_bf16", kFrontQkvNorm, [] { return sqllm_qkv_rope_norm_bf16(&r, &nm, nullptr); }},
    {"sqllm_qkv_rope_cache_f16", kFrontQkvCache, [] { return sqllm_qkv_rope_cache_f16(&r, &c, nullptr); }},
    {"sqllm_qkv_rope_cache_bf16", kFrontQkvCache, [] { return sqllm_qkv_rope_cache_bf16(&r, &c, nullptr); }},
    {"sqllm_qkv_rope_norm_cache_f16", kFrontQkvNormCache, [] { return sqllm_qkv_rope_norm_cache_f16(&r, &nm, &c, nullptr); }},
    {"sqllm_qkv_rope_norm_cache_bf16", kFrontQkvNormCache, [] { return sqllm_qkv_rope_norm_cache_bf16(&r, &nm, &c, nullptr); }},
    {"sqllm_qkv_rope_cache_fp8_f16", kFrontQkvCacheFp8, [] { return sqllm_qkv_rope_cache_fp8_f16(&r, &c8, nullptr); }},
    {"sqllm_qkv_rope_cache_fp8_bf16", kFrontQkvCacheFp8, [] { return sqllm_qkv_rope_cache_fp8_bf16(&r, &c8, nullptr); }},
    {"sqllm_qkv_rope_norm_cache_fp8_f16", kFrontQkvNormCacheFp8, [] { return sqllm_qkv_rope_norm_cache_fp8_f16(&r, &nm, &c8, nullptr); }},
    {"sqllm_qkv_rope_norm_cache_fp8_bf16", kFrontQkvNormCacheFp8, [] { return sqllm_qkv_rope_norm_cache_fp8_bf16(&r, &nm, &c8, nullptr); }},
};

}  // namespace

int main() {
  if (sqllm_set_option("cu_count", 256) != SQLLM_OK) return 2;
  memset(&g, 0, sizeof(g));
  fill(&g.gate, 128, 0x20000);
  fill(&g.up, 128, 0x30000);
  g.out = fake<void>(0x100000);
  g.workspace = fake<void>(0x400000);
  g.act = SQLLM_ACT_SILU;
  memset(&e, 0, sizeof(e));
  fill(&e.lin.op, 128, 0x20000);
  e.lin.op.mul = fake<float>(0x100000);
  e.lin.workspace = fake<void>(0x400000);
  e.residual = fake<const void>(0x500000);
  e.act = SQLLM_ACT_GELU;
  memset(&r, 0, sizeof(r));
  fill(&r.q, 256, 0x20000);
  fill(&r.k, 128, 0x30000);
  fill(&r.v, 128, 0x40000);
  r.out_q = fake<void>(0x100000); r.out_k = fake<void>(0x110000); r.out_v = fake<void>(0x120000);
  r.cos = fake<const float>(0x200000); r.sin = fake<const float>(0x210000); r.positions = fake<const int32_t>(0x220000);
  r.n_pos = 16; r.head_dim = 64; r.layout = SQLLM_ROPE_HALF;
  r.workspace = fake<void>(0x400000);

  // 1. nothing registered
  printf("nohook gated=%d gated_norm=%d qkv=%d qkv_norm=%d notsupported=%d\n", sqllm_gated_f16(&g, nullptr), sqllm_gated_norm_f16(&g, &nm, nullptr),
         sqllm_qkv_rope_bf16(&r, nullptr), sqllm_qkv_rope_norm_bf16(&r, &nm, nullptr), (int)hipErrorNotSupported);
  printf("nohook_all");
  for (const Entry& en : kEntries) printf(" %s=%d", en.name, en.call());
  printf("\n");

  // 2. the parents' slots, then the norm fronts' too
  g_launch_front[kFrontGated] = kRecorders[kFrontGated];
  g_launch_front[kFrontQkv] = kRecorders[kFrontQkv];
  printf("parenthooks gated=%d gated_norm=%d qkv=%d qkv_norm=%d ", sqllm_gated_bf16(&g, nullptr), sqllm_gated_norm_bf16(&g, &nm, nullptr),
         sqllm_qkv_rope_f16(&r, nullptr), sqllm_qkv_rope_norm_f16(&r, &nm, nullptr));
  print_calls4();
  printf("\n");

  g_launch_front[kFrontGatedNorm] = kRecorders[kFrontGatedNorm];
  g_launch_front[kFrontQkvNorm] = kRecorders[kFrontQkvNorm];
  reset();
  int rc = sqllm_gated_f16(&g, nullptr);
  const void* parent_pair = last_pair();
  printf("gated rc=%d ", rc);
  print_calls4();
  printf(" n_seg=%d\n", last.n_seg);
  rc = sqllm_gated_norm_f16(&g, &nm, nullptr);
  printf("gated_norm rc=%d ", rc);
  print_calls4();
  printf(" n_seg=%d weight=%p eps=%.9g x=%p same_pair=%d\n", last.n_seg, last.vn.weight, (double)last.vn.eps, last.x, (int)(last_pair() == parent_pair));
  rc = sqllm_qkv_rope_bf16(&r, nullptr);
  parent_pair = last_pair();
  printf("qkv rc=%d ", rc);
  print_calls4();
  printf(" n_seg=%d\n", last.n_seg);
  rc = sqllm_qkv_rope_norm_bf16(&r, &nm, nullptr);
  printf("qkv_norm rc=%d ", rc);
  print_calls4();
  printf(" n_seg=%d weight=%p eps=%.9g x=%p same_pair=%d\n", last.n_seg, last.vn.weight, (double)last.vn.eps, last.x, (int)(last_pair() == parent_pair));

  // 3. all nine slots: every entry, the slot it reaches and what arrives there
  for (int k = 0; k < kFrontKinds; ++k) g_launch_front[k] = kRecorders[k];
  for (const Entry& en : kEntries) {
    reset();
    memset(&last, 0, sizeof(last));
    rc = en.call();
    printf("reach:%s rc=%d kind=%d calls=", en.name, rc, en.kind);
    for (int k = 0; k < kFrontKinds; ++k) printf("%s%d", k ? "," : "", calls[k]);
    printf(" n_seg=%d x=%#llx pair=%d residual=%#llx act=%d has_qkv=%d has_vn=%d has_kc=%d", last.n_seg, ull(last.x), (int)(last.f.pair != nullptr), ull(last.f.residual),
           last.f.act, (int)(last.f.qkv != nullptr), (int)(last.f.vn != nullptr), (int)(last.f.kc != nullptr));
    printf(" weight=%#llx eps=%.9g", ull(last.vn.weight), (double)last.vn.eps);
    printf(" pair_q=%d pair_k=%d cos=%#llx sin=%#llx positions=%#llx n_pos=%d head_dim=%d interleaved=%d", (int)(last.qkv.pair_q != nullptr),
           (int)(last.qkv.pair_k != nullptr), ull(last.qkv.cos), ull(last.qkv.sin), ull(last.qkv.positions), last.qkv.n_pos,
           last.qkv.head_dim, (int)last.qkv.interleaved);
    printf(" k_cache=%#llx v_cache=%#llx slots=%#llx n_slots=%d slot_stride=%lld head_stride=%lld write_out=%d%d fp8=%d scales_ok=%d inv_k=%.9g inv_v=%.9g\n",
           ull(last.kc.k_cache), ull(last.kc.v_cache), ull(last.kc.slots), last.kc.n_slots, (long long)last.kc.slot_stride, (long long)last.kc.head_stride,
           (int)last.kc.write_out_k, (int)last.kc.write_out_v, (int)last.kc.fp8, (int)last.kc.scales_ok, (double)last.kc.inv_k_scale,
           (double)last.kc.inv_v_scale);
  }
  return 0;
}
