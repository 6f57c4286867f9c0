// match_seg.hpp -- what the segmented matchers share (match.hip: float
// descriptors, 64-query tiles; match_u8.hip: byte descriptors, 64 x Q-query
// tiles): the clamped device offsets, the segment search and the query-tile
// table.  Device code, included by the matchers and by cross_check.hip (the
// offsets and the search) only.
#pragma once

#include "common.hpp"

namespace sift {

namespace {

// Query rows [qoff[b], qoff[b+1]) are segment b; the offsets live on the device
// (sift_detect_compute_batch's d_img_offsets) and are never read by the host.
// Every bound is clamped to the buffer's row capacity, because the batch call
// leaves the true total in the last offset even when it exceeds kp_cap.
__device__ __forceinline__ int clamp_row(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

// Largest b in [0, n) with clamp(off[b]) <= x; the caller guarantees
// clamp(off[0]) <= x < clamp(off[n]).  Empty segments (equal offsets) are
// skipped: the result's next offset is above x.
__device__ __forceinline__ int seg_of(const int* __restrict__ off, int n, int cap, int x) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (clamp_row(off[mid], cap) <= x) lo = mid; else hi = mid;
  }
  return lo;
}

// Prologue (one workgroup): tile_start[b] = number of kTile-query tiles of the
// segments before b, tile_start[nseg] = all tiles.  A tile never spans two
// segments, so with segmented train it has one train range.
template <int kTile>
__global__ __launch_bounds__(256) void seg_tiles_kernel(const int* __restrict__ qoff, int nseg, int q_cap,
                                                        int* __restrict__ tile_start) {
  __shared__ int wsum[4];
  __shared__ int carry_s;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nseg; b0 += 256) {
    const int b = b0 + threadIdx.x;
    int n = 0;
    if (b < nseg) {
      const int s = clamp_row(qoff[b], q_cap), e = clamp_row(qoff[b + 1], q_cap);
      n = e > s ? (e - s + kTile - 1) / kTile : 0;
    }
    int v = n;  // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(v, d);
      if (lane >= d) v += u;
    }
    if (lane == 63) wsum[wv] = v;
    __syncthreads();
    int base = carry_s;
    for (int w = 0; w < wv; ++w) base += wsum[w];
    if (b < nseg) tile_start[b] = base + v - n;
    __syncthreads();
    if (threadIdx.x == 255) carry_s = base + v;
    __syncthreads();
  }
  if (threadIdx.x == 0) tile_start[nseg] = carry_s;
}

}  // namespace

}  // namespace sift
