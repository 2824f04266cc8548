// sqllm_tree_accept.h -- what the host layer (sqllm_capi.hip) hands to the two kernels that close the speculative-decoding step
// behind the tree entries: sqllm_tree_accept (sqllm_tree_accept.hip) and sqllm_kv_compact (sqllm_kv_compact.hip).  The entries
// judge their descriptors and reach the launchers through the hooks below, so that the host layer links without the kernel files:
// a null hook is hipErrorNotSupported.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sqllm {

// sqllm_tree_accept_desc as the kernel takes it: every pointer DEVICE memory
struct TreeAcceptArgs {
  const int* parents;
  const int* tree_mask;  // int32 pairs, the low word first
  const int* draft;
  const int* target;
  const int* q_lens;     // or null
  const int* seq_in;     // or null, with seq_out
  int* accept_len;
  int* path;
  int* next_token;
  int* seq_out;
  long long stride, mask_stride;  // int32 words between the sequences' rows
  int q_len, batch;
};
extern hipError_t (*g_launch_tree_accept)(const TreeAcceptArgs& k, hipStream_t stream);

constexpr int kKvCompactMaxCaches = 256;  // SQLLM_KV_COMPACT_MAX_CACHES of include/sqllm_hip.h
// sqllm_kv_compact_desc as the kernel takes it.  The cache pointers travel BY VALUE in the kernel's argument block (2 KiB of the
// 4 KiB there are): a captured graph node owns them, and the host array of the descriptor may go away behind the call.
struct KvCompactArgs {
  unsigned char* caches[kKvCompactMaxCaches];
  const int* block_table;
  const int* seq_lens;
  const int* q_lens;  // or null
  const int* path;
  const int* accept_len;
  long long path_stride;
  unsigned long long slot_bytes, head_bytes;  // the two strides in BYTES (below 2^33 wherever they are multiplied)
  long long capacity;                         // max_blocks * block_size
  int n_slots, block_size, table_stride, q_len;
};
// `row_bytes`: head_dim * elem_bytes, 64 / 128 / 256; `vec`: the access width in bytes, 16 / 4 / 2 / 1, which divides every cache
// pointer and both strides in bytes; the grid is (n_kv_heads, n_caches, batch)
extern hipError_t (*g_launch_kv_compact)(const KvCompactArgs& k, int row_bytes, int vec, int n_kv_heads, int n_caches, int batch, hipStream_t stream);

}  // namespace sqllm
