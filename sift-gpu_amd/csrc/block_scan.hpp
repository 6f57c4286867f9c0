// block_scan.hpp -- the one-workgroup scan of per-block counts that the ordered
// compactions share (match.hip: the ratio stage; cross_check.hip: the
// cross-check stage), and of the per-cell counts of the windowed matcher's grids
// (match_window.hip, one workgroup per grid).  Device code, included by those
// three files only.
#pragma once

#include "common.hpp"

namespace sift {

namespace {

// in-place exclusive scan of v[0..n), v[n] = total (one workgroup); workgroup g
// of a larger grid scans the g-th array of n + 1 entries
__global__ __launch_bounds__(1024) void ratio_scan_kernel(int* __restrict__ v, int n) {
  v += (long long)blockIdx.x * (n + 1);
  __shared__ int wsum[16];
  __shared__ int carry_s;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += 1024) {
    const int i = i0 + threadIdx.x;
    const int x = i < n ? v[i] : 0;
    int s = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(s, d);
      if (lane >= d) s += u;
    }
    if (lane == 63) wsum[wv] = s;
    __syncthreads();
    int base = carry_s;
    for (int w = 0; w < wv; ++w) base += wsum[w];
    if (i < n) v[i] = base + s - x;
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = base + s;
    __syncthreads();
  }
  if (threadIdx.x == 0) v[n] = carry_s;
}

}  // namespace

}  // namespace sift
