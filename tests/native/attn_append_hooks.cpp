// attn_append_hooks.cpp -- the four sqllm_attn_append_* entries on the host layer alone (csrc/sqllm_capi.hip linked against
// tests/native/launch_recorder.cpp with -DSQLLM_RECORDER_NO_MAIN: no device code, nothing is launched, operand pointers are
// fake).  Built and run by tests/test_attn_append_capi_cpu.py; prints one line per step, the test reads them.
//   1. no kernel file is linked in, so g_launch_attn_append and g_launch_attn_append_fp8 are null: a call that passes validation
//      is an ERROR (hipErrorNotSupported) for each of the four entries -- never a fallback;
//   2. with recording launchers in the two slots each entry reaches the slot of its own cache type and no other, with the
//      sequences, q_len, q_lens, the partitions of the HOST fields, and scale * k_scale / v_scale of the descriptor.
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

int calls[2];
AttnAppend last;

template <int KIND>
hipError_t rec(const AttnAppend& p, hipStream_t) {
  ++calls[KIND];
  last = p;
  return hipSuccess;
}

template <class A>
void fill(A* a) {
  memset(a, 0, sizeof(*a));
  a->q = fake<const void>(0x100000);
  a->out = fake<void>(0x200000);
  a->k_cache = fake<const void>(0x800000);
  a->v_cache = fake<const void>(0x900000);
  a->block_table = fake<const int32_t>(0x300000);
  a->seq_lens = fake<const int32_t>(0x310000);
  a->workspace = fake<void>(0x400000);
  a->q_lens = fake<const int32_t>(0x320000);
  a->q_len = 3;
  a->batch = 2; a->n_q_heads = 4; a->n_kv_heads = 2; a->head_dim = 64;
  a->n_slots = 1024; a->block_size = 16; a->max_blocks = 40; a->table_stride = 48;
  a->slot_stride = 128; a->head_stride = 64; a->q_stride = 256; a->out_stride = 260;
  a->scale = 0.125f;
}

void report(const char* name, int rc) {
  printf("%s rc=%d calls=%d,%d batch=%d q_len=%d q_lens=%llx n_parts=%d capacity=%d bf16=%d scale=%.9g v_scale=%.9g out_stride=%lld\n", name, rc, calls[0],
         calls[1], last.d.batch, last.q_len, (unsigned long long)reinterpret_cast<uintptr_t>(last.q_lens), last.d.n_parts, last.d.capacity,
         (int)last.d.bf16, last.d.scale, last.d.v_scale, (long long)last.d.out_stride);
}

}  // namespace

int main() {
  sqllm_attn_append a;
  sqllm_attn_append_fp8 a8;
  fill(&a);
  fill(&a8);
  a8.k_scale = 0.5f;
  a8.v_scale = 4.0f;
  printf("nohook notsupported=%d f16=%d bf16=%d fp8_f16=%d fp8_bf16=%d\n", (int)hipErrorNotSupported, sqllm_attn_append_f16(&a, nullptr),
         sqllm_attn_append_bf16(&a, nullptr), sqllm_attn_append_fp8_f16(&a8, nullptr), sqllm_attn_append_fp8_bf16(&a8, nullptr));
  g_launch_attn_append = rec<0>;
  printf("half notsupported=%d f16=%d fp8_f16=%d calls=%d,%d\n", (int)hipErrorNotSupported, sqllm_attn_append_f16(&a, nullptr),
         sqllm_attn_append_fp8_f16(&a8, nullptr), calls[0], calls[1]);
  g_launch_attn_append_fp8 = rec<1>;
  memset(calls, 0, sizeof(calls));
  report("f16", sqllm_attn_append_f16(&a, nullptr));
  report("bf16", sqllm_attn_append_bf16(&a, nullptr));
  report("fp8_f16", sqllm_attn_append_fp8_f16(&a8, nullptr));
  report("fp8_bf16", sqllm_attn_append_fp8_bf16(&a8, nullptr));
  a.q_lens = nullptr;
  a.q_len = 1;
  report("null_q_lens", sqllm_attn_append_f16(&a, nullptr));
  return 0;
}
