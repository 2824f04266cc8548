// sqllm_attn_prefill.h -- what the two prefill-attention kernel files share (sqllm_attn_prefill.hip: 16-bit caches;
// sqllm_attn_prefill_fp8.hip: caches of e4m3fn bytes): the kernels' argument and how the host fills it, what the entries serve,
// the matrix instruction and the three planes of the fp32 weights.  NOT shared: the kernels, which differ in everything between
// the cache and LDS and are otherwise copies of each other.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sqllm_attn.h"
#include "sqllm_decode.h"
#include "sqllm_kernels.h"
#include "sqllm_split_common.h"

namespace sqllm {

constexpr int kPrefillTile = 64;      // virtual rows per query tile, keys per key tile
constexpr int kPrefillMaxQLen = 65536;
constexpr int kPrefillMaxBatch = 65535;

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

struct AttnPrefillArgs {
  const void* q;
  void* out;
  const void* k_cache;
  const void* v_cache;
  const int* block_table;  // [batch, table_stride]
  const int* seq_lens;     // [batch]
  const int* q_lens;       // [batch] or null
  long long q_stride, out_stride;
  unsigned slot_stride, head_stride;  // (below 2^32 wherever they are multiplied: checked by the host)
  int group, n_slots, block_size, table_stride;
  int capacity;  // min(max_blocks * block_size, INT32_MAX)
  int q_len;
  int n_tiles;   // ceil(q_len * group / 64)
  float scale;
};

// what both entries serve, but for the cache's element type: from HOST fields only
inline bool prefill_served(const AttnCall& c) {
  return (c.head_dim == 64 || c.head_dim == 128) && c.n_kv_heads >= 1 && c.n_kv_heads <= 65535 && c.n_q_heads % c.n_kv_heads == 0 &&
         c.n_q_heads / c.n_kv_heads <= 8 && c.batch >= 1 && c.batch <= kPrefillMaxBatch && c.q_len >= 1 && c.q_len <= kPrefillMaxQLen && !c.window;
}

inline AttnPrefillArgs make_prefill_args(const AttnCall& c) {
  AttnPrefillArgs k;
  k.q = c.q;
  k.out = c.out;
  k.k_cache = c.k_cache;
  k.v_cache = c.v_cache;
  k.block_table = c.block_table;
  k.seq_lens = c.seq_lens;
  k.q_lens = c.q_lens;
  k.q_stride = c.q_stride;
  k.out_stride = c.out_stride;
  k.slot_stride = (unsigned)c.slot_stride;
  k.head_stride = (unsigned)c.head_stride;
  k.group = c.n_q_heads / c.n_kv_heads;
  k.n_slots = c.n_slots;
  k.block_size = c.block_size;
  k.table_stride = c.table_stride;
  k.capacity = c.capacity;
  k.q_len = c.q_len;
  k.n_tiles = (int)(((long long)c.q_len * k.group + kPrefillTile - 1) / kPrefillTile);
  k.scale = c.scale;
  return k;
}

// The sliding-window prefill kernels (sqllm_attn_prefill_window.hip, sqllm_attn_prefill_window_fp8.hip): the same argument and
// the window behind it, 1 .. INT32_MAX.  Row (b, t) attends the keys [lo, L), lo = L > window ? L - window : 0.
struct AttnPrefillWindowArgs : AttnPrefillArgs {
  int window;
};

// what the window entries serve: the shapes of prefill_served and a window of at least one key
inline bool prefill_window_served(const AttnCall& c) {
  AttnCall plain = c;
  plain.window = 0;
  return c.window >= 1 && prefill_served(plain);
}

inline AttnPrefillWindowArgs make_prefill_window_args(const AttnCall& c) {
  AttnPrefillWindowArgs k;
  static_cast<AttnPrefillArgs&>(k) = make_prefill_args(c);
  k.window = c.window;
  return k;
}

// the keys [lo, len) of a row inside the key tile [key0, key0 + 64) as a 64-bit mask, bit i for key key0 + i (0 <= lo <= len or
// len <= 0; no sum that could leave int)
__device__ __forceinline__ unsigned long long window_tile_bits(int lo, int len, int key0) {
  const int first = lo > key0 ? lo - key0 : 0;
  const int end = len > key0 ? (len - key0 < 64 ? len - key0 : 64) : 0;
  if (end <= first) return 0ull;
  const unsigned long long below_end = end == 64 ? ~0ull : (1ull << end) - 1ull;
  return below_end & ~((1ull << first) - 1ull);  // (first < end <= 64)
}

// 8 bytes of 16-bit elements that are aligned to their elements only
struct __attribute__((packed, aligned(2))) Packed4 {
  uint32_t w[2];
};

template <typename OT>
__device__ __forceinline__ f32x4 mfma_16x16x32(u32x4 a, u32x4 b, f32x4 c) {
  if constexpr (std::is_same<OT, __bf16>::value) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// eight fp32 weights in [0, 1] as three planes of packed 16-bit operands (element 2i in the low half of word i); fp16: of w * 2^15
template <typename OT>
__device__ __forceinline__ void weight_planes(const float (&w)[8], u32x4& h, u32x4& m, u32x4& l) {
  uint32_t hh[4], mm[4], ll[4];
  if constexpr (std::is_same<OT, __bf16>::value) {
    split8(w, hh, mm, ll);
  } else {
    uint32_t hb[8], mb[8], lb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float x = w[i] * 32768.0f;  // exact
      const _Float16 a = (_Float16)x;
      const float r1 = x - (float)a;  // exact
      const _Float16 b = (_Float16)r1;
      const float r2 = r1 - (float)b;  // exact
      const _Float16 c = (_Float16)r2;
      hb[i] = __builtin_bit_cast(unsigned short, a);
      mb[i] = __builtin_bit_cast(unsigned short, b);
      lb[i] = __builtin_bit_cast(unsigned short, c);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hh[i] = hb[2 * i] | (hb[2 * i + 1] << 16);
      mm[i] = mb[2 * i] | (mb[2 * i + 1] << 16);
      ll[i] = lb[2 * i] | (lb[2 * i + 1] << 16);
    }
  }
  h = u32x4{hh[0], hh[1], hh[2], hh[3]};
  m = u32x4{mm[0], mm[1], mm[2], mm[3]};
  l = u32x4{ll[0], ll[1], ll[2], ll[3]};
}

}  // namespace sqllm
