// block_scan.hpp -- the one-workgroup scan of per-block counts that the ordered
// compactions share (match.hip: the ratio stage; cross_check.hip: the
// cross-check stage), and of the per-cell counts of the windowed matcher's grids
// (match_window.hip, one workgroup per grid).  Device code, included by those
// three files only.
#pragma once

#include "wave_scan.hpp"

namespace sift {

namespace {

// in-place exclusive scan of v[0..n), v[n] = total (one workgroup); workgroup g
// of a larger grid scans the g-th array of n + 1 entries
__global__ __launch_bounds__(1024) void ratio_scan_kernel(int* __restrict__ v, int n) {
  v += (long long)blockIdx.x * (n + 1);
  const int total = wg_scan_chunks<1024>(n, [&](int i) { return v[i]; }, [&](int i, int x) { v[i] = x; });
  if (threadIdx.x == 0) v[n] = total;
}

}  // namespace

}  // namespace sift
