// detect_args.hpp -- what the detection stages share: extrema.hip, scan.hip,
// refine.hip, orient.hip and emit.hip (reference src/sift.cpp:285-577) include
// it and nothing else does.  Output order must equal the reference's (octave
// -> layer -> row -> col -> histogram peak, src/sift.cpp:556-557, 487-491, 525,
// duplicates kept), so no stage appends with atomics: slots come from scans.
#pragma once

#include "common.hpp"

namespace sift {

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// scan.hip.  out[i] = sum(in[0..i)), out[n] = total (also *total_out if
// given).  n from n_dev (clamped to cap) if given, else n_host; tsum is
// [scan_tiles_for(cap)] ints of scratch.
// Per-image offsets from the scan: gout[b] = out[b * stride] (idx == nullptr)
// or out[min(idx[b], n)], b = 0..batch.
struct ScanGather {
  const int* idx;
  int stride, batch;
  int* gout;  // nullptr: no gather
};
void launch_scan(hipStream_t st, const int* in, int* out, const int* n_dev, int n_host, int cap, int* total_out,
                 int* tsum, ScanGather g = ScanGather{nullptr, 0, 0, nullptr});

// The candidate slots and what refinement and orientation read and write
// (launch_refine_orient, refine.hip, fills it in).
struct RefArgs {
  Layout L;
  const float* gpyr;
  const float2* grad;
  const float* dog;
  int dog_from_g;  // 1: DoG values are Gaussian-plane differences (no DoG planes stored)
  const MathConsts* mc;
  const Cand* cands;
  const int* cand_total;
  int cand_cap;
  CandOut* couts;
  int* npeaks;
  // sparse flow (SparseG4 in common.hpp); sparse == 0: the dense flow
  unsigned sparse;
  const float* coef4;
  float* patch;
  int* rstate;
  int* wait;    // two lists of waiting slots, [2][cand_cap]: round k reads (k - 1) & 1, appends to k & 1
  int* g4stat;
};
// orient.hip: the orientation pass over the slots refinement left in A.couts
void launch_orient(hipStream_t st, const RefArgs& A, int batch);

}  // namespace sift
