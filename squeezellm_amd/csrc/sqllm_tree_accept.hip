// sqllm_tree_accept.hip -- greedy acceptance of a verified draft tree (include/sqllm_hip.h: sqllm_tree_accept): which root-to-leaf
// path of up to 64 draft nodes the target model agreed with, how long it is, and the token that follows it.  The step between
// sqllm_attn_tree_* / sqllm_attn_tree64_* (and the caller's argmax) and sqllm_kv_compact.
//
// One wave per sequence, lane t = node t, four sequences per workgroup; no loop over nodes, no LDS, no workspace.
//   - match.  Lane t compares its draft token with the target's token at its parent (a root matches; a parent that is not an earlier
//     node does not).  ONE ballot turns the 64 answers into the word M.
//   - accepted.  Node t is accepted when every node of its closure word w(t) -- the row's 64-bit mask with the own bit set and the
//     bits at and above n_b cleared -- is in M: w & ~M == 0.  The kernel applies the formula, it does not check that w is a closure.
//   - best.  ONE wave reduction (xor butterfly, max) over the key (popcount(w) << 6) | (63 - t): the longest path, the lowest node
//     among equals; -1 for a node that is not accepted.
//   - path.  The best node's word W comes from its lane.  Every lane whose bit is set in W writes its own index at the rank
//     popcount(W & ((1 << t) - 1)); the lanes accept_len <= t < q_len write -1: a scatter, every word of path[b, 0 .. q_len) once.
//   - accept_len, next_token and seq_lens_out are uniform over the wave: lane 0 writes them with ordinary stores, and reads its
//     sequence's seq_lens_in word before it writes seq_lens_out, so the two may be one array.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md 4.4.  No scratch, no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sqllm_tree_accept.h"

namespace sqllm {

constexpr int kAcceptWaves = 4;  // sequences per workgroup

__global__ void __launch_bounds__(64 * kAcceptWaves) sqllm_tree_accept_kernel(const TreeAcceptArgs a) {
  const int t = threadIdx.x & 63;
  const int b = blockIdx.x * kAcceptWaves + (threadIdx.x >> 6);
  if (b >= a.batch) return;  // (uniform over the wave)
  const int T = a.q_len;
  const int n = a.q_lens ? a.q_lens[b] : T;
  const long long row = (long long)b * a.stride;
  const bool served = n > 0 && n <= T;
  const bool node = served && t < n;

  unsigned long long w = 0ull;
  bool match = false;
  if (node) {
    const int* const m = a.tree_mask + (long long)b * a.mask_stride + 2 * t;
    const unsigned long long low = n >= 64 ? ~0ull : (1ull << n) - 1ull;
    w = (((unsigned long long)(unsigned)m[0] | ((unsigned long long)(unsigned)m[1] << 32)) | (1ull << t)) & low;
    const int p = a.parents[row + t];
    match = p < 0 || (p < t && a.draft[row + t] == a.target[row + p]);  // (target is read at an earlier node only)
  }
  const unsigned long long M = __ballot(match);
  const bool accepted = node && (w & ~M) == 0ull;
  const int len = __popcll(w);
  int key = accepted ? (len << 6) | (63 - t) : -1;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const int o = __shfl_xor(key, s, 64);
    key = o > key ? o : key;
  }
  key = __builtin_amdgcn_readfirstlane(key);
  const int best = key < 0 ? 0 : 63 - (key & 63);
  const int alen = key < 0 ? 0 : key >> 6;
  const unsigned lo = __shfl((unsigned)w, best, 64), hi = __shfl((unsigned)(w >> 32), best, 64);
  const unsigned long long W = key < 0 ? 0ull : (unsigned long long)lo | ((unsigned long long)hi << 32);

  if (t >= alen && t < T) a.path[row + t] = -1;
  if (W >> t & 1ull) a.path[row + __popcll(W & ((1ull << t) - 1ull))] = t;  // (ranks below alen: no word is written twice)
  if (t == 0) {
    a.accept_len[b] = alen;
    a.next_token[b] = key < 0 ? -1 : a.target[row + best];
    if (a.seq_out) {
      const int seq = a.seq_in[b];  // (read before the store: seq_in and seq_out may be one array)
      a.seq_out[b] = n > T ? seq : seq - (n > 0 ? n : 0) + alen;
    }
  }
}

static hipError_t launch_tree_accept(const TreeAcceptArgs& k, hipStream_t stream) {
  hipLaunchKernelGGL(sqllm_tree_accept_kernel, dim3((unsigned)(k.batch + kAcceptWaves - 1) / kAcceptWaves), dim3(64 * kAcceptWaves), 0, stream, k);
  return hipGetLastError();
}

// the host layer reaches the launcher through its hook (sqllm_tree_accept.h), so that it links without this file too
static const bool g_tree_accept_registered = (g_launch_tree_accept = launch_tree_accept, true);

}  // namespace sqllm
