// sqllm_stream_api.h -- interface between the measurement library's host code (sqllm_experimental.hip) and its batch-1
// kernels that were measured and not adopted: the streaming kernel (sqllm_stream.hip) and the column-pair-table kernel
// (sqllm_pair.hip).  The product sources do not include this.
#pragma once
#include "sqllm_kernels.h"

namespace sqllm {

// ---- streaming batch-1 kernel (sqllm_stream.hip) ----
constexpr int kStreamPieces4 = 2;  // 64-column tiles one workgroup's range may touch (codebook tables resident at once), 4-bit
constexpr int kStreamPieces3 = 2;  // ... 3-bit (32 KiB pair tables)

struct StreamSeg {  // one op of the launch, dense term only
  const uint32_t* q;
  float* y;
  const float* lut;
  int N;
  int tile0;  // index of the op's first tile in the launch's flattened tile space (INT_MAX: unused slot)
};

// Dense part of a streaming launch: the ops' 64-column tiles back to back, each tile `steps_per_tile`
// steps long (a step = 4 units = what one wave load covers), cut into ranges of `steps_per_wg` steps.
struct StreamArgs {
  const float* x;
  int K;
  int units_total;     // K / 8 (4-bit) or K / 32 (3-bit)
  int steps_per_tile;  // ceil(units_total / 4)
  int steps_per_wg;
  int total_steps;     // tiles of all ops * steps_per_tile
  int dense_block0;    // first dense workgroup id (the sparse-role workgroups come first)
  int n_dense;         // dense workgroups
  int n_seg;
  uint32_t s_magic;    // ceil(2^32 / steps_per_tile): tile of a step = mulhi(step, s_magic)
  StreamSeg seg[kMaxSegments];
  unsigned long long* probe;  // measurement builds: 8 timestamps per workgroup (tools/timeline.py); null otherwise
};

hipError_t launch_pair4(const LaunchArgs& a, hipStream_t stream);  // 4-bit, batch 1, operator launches: column-pair tables, 16-wave workgroups
// `ga`: the sparse roles of the launch (block0[] = prefix over csr + top-X workgroups only)
hipError_t launch_stream(int bits, const StreamArgs& sa, const GroupArgs& ga, hipStream_t stream, hipEvent_t e0, hipEvent_t e1,
                         int ablate);

}  // namespace sqllm
