// attn_hooks.cpp -- the eight decode-attention entries (sqllm_attn_decode_* and sqllm_attn_append_*, 16-bit and fp8 caches) on the
// host layer alone (csrc/sqllm_capi.hip linked against tests/native/launch_recorder.cpp with -DSQLLM_RECORDER_NO_MAIN: no device
// code, nothing is launched, operand pointers are fake).  Built and run by tests/test_attn_append_capi_cpu.py; prints one line per
// step, the test reads them.
//   1. no kernel file is linked in, so every slot of g_launch_attn is null: a call that passes validation is an ERROR
//      (hipErrorNotSupported) for each of the eight entries -- never a fallback;
//   2. with exactly ONE slot filled, each of the four in turn (a 16-bit slot without its fp8 sibling and the other way round),
//      the f16 and the bf16 entry of that slot succeed and the other six entries still fail;
//   3. with recording launchers in the four slots each entry reaches its own slot and no other, with the sequences, q_len,
//      q_lens, the partitions of the HOST fields, and scale * k_scale / v_scale of the descriptor.
// `calls=` counts the two slots of the line's own family (16-bit, fp8); the closing `slots` line counts all four.
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

int calls[kAttnKinds];
AttnCall last;

template <int KIND>
hipError_t rec(const AttnCall& c, hipStream_t) {
  ++calls[KIND];
  last = c;
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
  a->batch = 2; a->n_q_heads = 4; a->n_kv_heads = 2; a->head_dim = 64;
  a->n_slots = 1024; a->block_size = 16; a->max_blocks = 40; a->table_stride = 48;
  a->slot_stride = 128; a->head_stride = 64; a->q_stride = 256; a->out_stride = 260;
  a->scale = 0.125f;
}
template <class A>
void fill_tokens(A* a) {
  fill(a);
  a->q_lens = fake<const int32_t>(0x320000);
  a->q_len = 3;
}

// `first`: the family's 16-bit slot (kAttnDecode or kAttnAppend)
void report(const char* name, int first, int rc) {
  printf("%s rc=%d calls=%d,%d batch=%d q_len=%d q_lens=%llx n_parts=%d capacity=%d bf16=%d scale=%.9g v_scale=%.9g out_stride=%lld\n", name, rc,
         calls[first], calls[first + 1], last.batch, last.q_len, (unsigned long long)reinterpret_cast<uintptr_t>(last.q_lens), last.n_parts,
         last.capacity, (int)last.bf16, last.scale, last.v_scale, (long long)last.out_stride);
}

}  // namespace

int main() {
  static_assert(kAttnDecodeFp8 == kAttnDecode + 1 && kAttnAppendFp8 == kAttnAppend + 1, "a family's fp8 slot follows its 16-bit slot");
  sqllm_attn_decode d;
  sqllm_attn_decode_fp8 d8;
  sqllm_attn_append a;
  sqllm_attn_append_fp8 a8;
  fill(&d);
  fill(&d8);
  fill_tokens(&a);
  fill_tokens(&a8);
  d8.k_scale = a8.k_scale = 0.5f;
  d8.v_scale = a8.v_scale = 4.0f;
  const int ns = (int)hipErrorNotSupported;
  printf("nohook notsupported=%d f16=%d bf16=%d fp8_f16=%d fp8_bf16=%d\n", ns, sqllm_attn_append_f16(&a, nullptr),
         sqllm_attn_append_bf16(&a, nullptr), sqllm_attn_append_fp8_f16(&a8, nullptr), sqllm_attn_append_fp8_bf16(&a8, nullptr));
  printf("nohook_decode notsupported=%d f16=%d bf16=%d fp8_f16=%d fp8_bf16=%d\n", ns, sqllm_attn_decode_f16(&d, nullptr),
         sqllm_attn_decode_bf16(&d, nullptr), sqllm_attn_decode_fp8_f16(&d8, nullptr), sqllm_attn_decode_fp8_bf16(&d8, nullptr));
  // exactly one slot filled, each of the four in turn: the two entries of that slot succeed, the other six still fail
  const AttnLauncher recs[kAttnKinds] = {rec<kAttnDecode>, rec<kAttnDecodeFp8>, rec<kAttnAppend>, rec<kAttnAppendFp8>};
  const char* const names[kAttnKinds] = {"only_decode", "only_decode_fp8", "only_append", "only_append_fp8"};
  for (int k = 0; k < kAttnKinds; ++k) {
    memset(calls, 0, sizeof(calls));
    g_launch_attn[k] = recs[k];
    printf("%s notsupported=%d decode_f16=%d decode_bf16=%d decode_fp8_f16=%d decode_fp8_bf16=%d append_f16=%d append_bf16=%d append_fp8_f16=%d "
           "append_fp8_bf16=%d", names[k], ns, sqllm_attn_decode_f16(&d, nullptr), sqllm_attn_decode_bf16(&d, nullptr),
           sqllm_attn_decode_fp8_f16(&d8, nullptr), sqllm_attn_decode_fp8_bf16(&d8, nullptr), sqllm_attn_append_f16(&a, nullptr),
           sqllm_attn_append_bf16(&a, nullptr), sqllm_attn_append_fp8_f16(&a8, nullptr), sqllm_attn_append_fp8_bf16(&a8, nullptr));
    printf(" calls=%d,%d,%d,%d\n", calls[0], calls[1], calls[2], calls[3]);
    g_launch_attn[k] = nullptr;
  }
  memset(calls, 0, sizeof(calls));
  g_launch_attn[kAttnAppend] = rec<kAttnAppend>;
  printf("half notsupported=%d f16=%d fp8_f16=%d calls=%d,%d\n", ns, sqllm_attn_append_f16(&a, nullptr), sqllm_attn_append_fp8_f16(&a8, nullptr),
         calls[kAttnAppend], calls[kAttnAppendFp8]);
  g_launch_attn[kAttnDecode] = rec<kAttnDecode>;
  g_launch_attn[kAttnDecodeFp8] = rec<kAttnDecodeFp8>;
  g_launch_attn[kAttnAppendFp8] = rec<kAttnAppendFp8>;
  memset(calls, 0, sizeof(calls));
  report("f16", kAttnAppend, sqllm_attn_append_f16(&a, nullptr));
  report("bf16", kAttnAppend, sqllm_attn_append_bf16(&a, nullptr));
  report("fp8_f16", kAttnAppend, sqllm_attn_append_fp8_f16(&a8, nullptr));
  report("fp8_bf16", kAttnAppend, sqllm_attn_append_fp8_bf16(&a8, nullptr));
  a.q_lens = nullptr;
  a.q_len = 1;
  report("null_q_lens", kAttnAppend, sqllm_attn_append_f16(&a, nullptr));
  report("decode_f16", kAttnDecode, sqllm_attn_decode_f16(&d, nullptr));
  report("decode_bf16", kAttnDecode, sqllm_attn_decode_bf16(&d, nullptr));
  report("decode_fp8_f16", kAttnDecode, sqllm_attn_decode_fp8_f16(&d8, nullptr));
  report("decode_fp8_bf16", kAttnDecode, sqllm_attn_decode_fp8_bf16(&d8, nullptr));
  printf("slots decode=%d decode_fp8=%d append=%d append_fp8=%d\n", calls[kAttnDecode], calls[kAttnDecodeFp8], calls[kAttnAppend], calls[kAttnAppendFp8]);
  return 0;
}
