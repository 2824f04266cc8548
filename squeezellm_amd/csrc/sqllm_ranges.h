// sqllm_ranges.h -- the glue between the planner (sqllm_capi.hip: plan_group, cut_ranges) and the kernels, written once
// for all of them.  Two parts:
//   device side  how a kernel reads the planner's geometry: which op of a multi-op launch a workgroup belongs to
//                (pick_segment), how long a tile is in the flattened (column tile, unit) space (units_stride_of);
//   host side    how the kernel sources launch: launch_kernel (plain, or with the dispatch's events), with_row_blocks
//                (row blocks -> instantiation).  sqllm_mfma_wide.hip includes this header for that part alone.
// Included by the kernel sources only (not by sqllm_capi.hip: sqllm_kernels.h stays plain C++).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <type_traits>

#include "sqllm_kernels.h"

#include "sqllm_decode.h"

namespace sqllm {

// Which op of the launch this workgroup belongs to: workgroup ids [block0[s], block0[s+1]) belong to segment s (1 segment
// = a plain op).  ONE round of scalar loads fetches the block table and -- speculatively -- the whole of segment 0 into
// registers, pinned there together with `x`, the kernel's vec pointer (see sqllm_fused_matvec and SQLLM_SEG_OPERANDS);
// a workgroup of another segment pays a second round for its own descriptor.  Returns the workgroup's id inside its segment.
// (The column-lane kernel, sqllm_fused_cols, keeps a copy of its own: it reloads without readfirstlane and takes its id
// off inside the reload's branch, and its generated code is kept as it was.)
__device__ __forceinline__ int pick_segment(const GroupArgs& ga, const void* x, Segment& sg) {
  sg = ga.seg[0];
  const int n_seg = ga.n_seg, blk1 = ga.block0[1], blk2 = ga.block0[2], blk3 = ga.block0[3];
  asm volatile("" ::SQLLM_SEG_OPERANDS(sg), "s"(x), "s"(n_seg), "s"(blk1), "s"(blk2), "s"(blk3));
  __builtin_amdgcn_sched_barrier(0);  // (or the scheduler starts on the block table after the first few loads, waits, and issues the rest behind that wait)
  int s = 0, base = 0;
  if (n_seg > 1 && (int)blockIdx.x >= blk1) { s = 1; base = blk1; }
  if (n_seg > 2 && (int)blockIdx.x >= blk2) { s = 2; base = blk2; }
  if (n_seg > 3 && (int)blockIdx.x >= blk3) { s = 3; base = blk3; }
  s = __builtin_amdgcn_readfirstlane(s);
  if (s != 0) {
    sg = ga.seg[s];
    asm volatile("" ::SQLLM_SEG_OPERANDS(sg));
  }
  return blockIdx.x - base;
}

// Length of a column tile in the flattened (column tile, unit) space that cut_ranges cuts into equal ranges of
// units_per_wg units, one per dense workgroup.  Two readings of the cut:
//   contiguous    a tile is units_total long; a range that crosses a tile boundary is worked off as two pieces;
//   tile-aligned  every tile is cut into a whole number of ranges (k_slices of them: a tile is k_slices * units_per_wg
//                 >= units_total long, no range crosses, the last one of a tile is short and padding follows it).
// The kernels recognise the tile-aligned cut by dense_blocks == col_tiles * k_slices; a contiguous cut that happens to
// satisfy the same equation is then READ as tile-aligned -- ranges of units_per_wg units that restart at every tile --
// which covers every unit exactly once as well: tests/test_capi_cpu.py fuzzes both readings.
__device__ __forceinline__ int units_stride_of(const KernelGeom& gm) {
  return gm.dense_blocks == gm.col_tiles * gm.k_slices ? gm.k_slices * gm.units_per_wg : gm.units_total;
}

// ---- host side: the launch glue of the kernel sources ----
// One launch: through hipExtLaunchKernelGGL where the caller wants the dispatch's own begin / end timestamps exposed
// through events (profiling aid), plainly otherwise.
template <typename Kernel, typename... Args>
inline hipError_t launch_kernel(Kernel kern, dim3 grid, dim3 block, unsigned lds_bytes, hipStream_t stream,
                                hipEvent_t ev_start, hipEvent_t ev_stop, const Args&... args) {
  if (ev_start || ev_stop) hipExtLaunchKernelGGL(kern, grid, block, lds_bytes, stream, ev_start, ev_stop, 0, args...);
  else hipLaunchKernelGGL(kern, grid, block, lds_bytes, stream, args...);
  return hipGetLastError();
}

// blocks of 16 batch rows per pass of a matrix-core kernel (1, 2 or 4) -> its instantiation: f(integral_constant<int, MB>)
template <typename F>
inline hipError_t with_row_blocks(int row_blocks, F&& f) {
  switch (row_blocks) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

}  // namespace sqllm
