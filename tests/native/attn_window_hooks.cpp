// attn_window_hooks.cpp -- the four sliding-window decode-attention entries (sqllm_attn_decode_window_*, 16-bit and fp8 caches) on
// the host layer alone (csrc/sqllm_capi.hip linked against tests/native/launch_recorder.cpp with -DSQLLM_RECORDER_NO_MAIN: no
// device code, nothing is launched, operand pointers are fake).  Built and run by tests/test_attn_window_capi_cpu.py; prints one
// line per step, the test reads them.
//   1. no kernel file is linked in, so both slots of g_launch_attn_window are null: a call that passes validation is an ERROR
//      (hipErrorNotSupported) for each of the four entries -- also with the four slots of g_launch_attn filled: never a fallback
//      onto the kernels without a window;
//   2. with exactly ONE window slot filled, each in turn, its f16 and bf16 entry succeed and the other two still fail; the eight
//      entries without a window never reach a window slot;
//   3. the recorded call carries the window, and its n_parts is win_parts of the HOST fields.
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

int calls[2], plain_calls;
AttnCall last;

template <int KIND>
hipError_t rec(const AttnCall& c, hipStream_t) {
  ++calls[KIND];
  last = c;
  return hipSuccess;
}
hipError_t rec_plain(const AttnCall& c, hipStream_t) {
  ++plain_calls;
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

void report(const char* name, int rc) {
  printf("%s rc=%d calls=%d,%d plain=%d batch=%d q_len=%d window=%d n_parts=%d capacity=%d bf16=%d fp8=%d scale=%.9g v_scale=%.9g\n", name, rc, calls[0],
         calls[1], plain_calls, last.batch, last.q_len, last.window, last.n_parts, last.capacity, (int)last.bf16, (int)last.fp8, last.scale, last.v_scale);
}

}  // namespace

int main() {
  sqllm_attn_decode d;
  sqllm_attn_decode_fp8 d8;
  sqllm_attn_append a;
  sqllm_attn_append_fp8 a8;
  fill(&d);
  fill(&d8);
  fill(&a);
  fill(&a8);
  a.q_len = a8.q_len = 3;
  d8.k_scale = a8.k_scale = 0.5f;
  d8.v_scale = a8.v_scale = 4.0f;
  const int ns = (int)hipErrorNotSupported;
  printf("nohook notsupported=%d f16=%d bf16=%d fp8_f16=%d fp8_bf16=%d\n", ns, sqllm_attn_decode_window_f16(&d, 100, nullptr),
         sqllm_attn_decode_window_bf16(&d, 100, nullptr), sqllm_attn_decode_window_fp8_f16(&d8, 100, nullptr),
         sqllm_attn_decode_window_fp8_bf16(&d8, 100, nullptr));
  // the four slots without a window filled: still an error, and none of them is called
  for (int k = 0; k < kAttnKinds; ++k) g_launch_attn[k] = rec_plain;
  printf("plainhooks notsupported=%d f16=%d bf16=%d fp8_f16=%d fp8_bf16=%d", ns, sqllm_attn_decode_window_f16(&d, 100, nullptr),
         sqllm_attn_decode_window_bf16(&d, 100, nullptr), sqllm_attn_decode_window_fp8_f16(&d8, 100, nullptr),
         sqllm_attn_decode_window_fp8_bf16(&d8, 100, nullptr));
  printf(" plain=%d\n", plain_calls);
  // exactly one window slot filled, each in turn
  const AttnLauncher recs[2] = {rec<0>, rec<1>};
  const char* const names[2] = {"only_window", "only_window_fp8"};
  for (int k = 0; k < 2; ++k) {
    memset(calls, 0, sizeof(calls));
    plain_calls = 0;
    g_launch_attn_window[k] = recs[k];
    printf("%s notsupported=%d f16=%d bf16=%d fp8_f16=%d fp8_bf16=%d", names[k], ns, sqllm_attn_decode_window_f16(&d, 100, nullptr),
           sqllm_attn_decode_window_bf16(&d, 100, nullptr), sqllm_attn_decode_window_fp8_f16(&d8, 100, nullptr),
           sqllm_attn_decode_window_fp8_bf16(&d8, 100, nullptr));
    printf(" calls=%d,%d plain=%d\n", calls[0], calls[1], plain_calls);
    g_launch_attn_window[k] = nullptr;
  }
  g_launch_attn_window[0] = rec<0>;
  g_launch_attn_window[1] = rec<1>;
  memset(calls, 0, sizeof(calls));
  plain_calls = 0;
  // the eight entries without a window never reach a window slot
  const int rcs[8] = {sqllm_attn_decode_f16(&d, nullptr), sqllm_attn_decode_bf16(&d, nullptr), sqllm_attn_decode_fp8_f16(&d8, nullptr),
                      sqllm_attn_decode_fp8_bf16(&d8, nullptr), sqllm_attn_append_f16(&a, nullptr), sqllm_attn_append_bf16(&a, nullptr),
                      sqllm_attn_append_fp8_f16(&a8, nullptr), sqllm_attn_append_fp8_bf16(&a8, nullptr)};
  int bad = 0;
  for (int i = 0; i < 8; ++i) bad += rcs[i] != 0;
  printf("eight failed=%d calls=%d,%d plain=%d window=%d n_parts=%d\n", bad, calls[0], calls[1], plain_calls, last.window, last.n_parts);
  plain_calls = 0;
  report("f16", sqllm_attn_decode_window_f16(&d, 100, nullptr));
  report("bf16", sqllm_attn_decode_window_bf16(&d, 640, nullptr));
  report("fp8_f16", sqllm_attn_decode_window_fp8_f16(&d8, 1, nullptr));
  report("fp8_bf16", sqllm_attn_decode_window_fp8_bf16(&d8, INT32_MAX, nullptr));
  // validation: the window is a count, judged with the others -- after the NULL checks, before the scale
  d.scale = __builtin_nanf("");
  printf("window0 rc=%d\n", sqllm_attn_decode_window_f16(&d, 0, nullptr));
  printf("windowneg rc=%d\n", sqllm_attn_decode_window_bf16(&d, -1, nullptr));
  printf("window1nan rc=%d\n", sqllm_attn_decode_window_f16(&d, 1, nullptr));
  d.q = nullptr;
  printf("nullq rc=%d calls=%d,%d\n", sqllm_attn_decode_window_f16(&d, 0, nullptr), calls[0], calls[1]);
  return 0;
}
