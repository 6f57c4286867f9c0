// wave_scan.hpp -- the device scans' one primitive: a wave-inclusive scan, the
// step from it to a workgroup-exclusive offset, and the one-workgroup chunked
// scan with a running carry of scan.hip (scan_tiles_kernel), block_scan.hpp
// (ratio_scan_kernel) and match_seg.hpp (seg_tiles_kernel).  Device code,
// ints only; holds no kernel, so every file may include it.
#pragma once

#include "common.hpp"

namespace sift {

// sum of v over lanes 0..lane of the wave (lane = threadIdx.x & 63)
__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(v, off);
    if (lane >= off) v += t;
  }
  return v;
}

// From every wave's inclusive value to the workgroup (kWaves whole waves, wv =
// threadIdx.x >> 6): before = the sum over the waves before this one, so
// before + incl - v is the thread's exclusive offset; total = the sum over all.
// wsum is kWaves ints of LDS; one barrier, after which wsum is read only --
// the caller synchronises before the next call writes it.
struct WgScan {
  int before, total;
};
template <int kWaves>
__device__ __forceinline__ WgScan wg_scan(int incl, int lane, int wv, int* wsum) {
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  WgScan r{0, 0};
  for (int k = 0; k < kWaves; ++k) {
    r.before += k < wv ? wsum[k] : 0;
    r.total += wsum[k];
  }
  return r;
}

// Exclusive scan of load(0), ..., load(n - 1) by one workgroup of kThreads
// threads, kThreads elements per step with the sum so far carried over:
// store(i, sum of load(0..i)) for every i < n; returns the total to every
// thread.
template <int kThreads, typename Load, typename Store>
__device__ __forceinline__ int wg_scan_chunks(int n, Load load, Store store) {
  __shared__ int wsum[kThreads / 64];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int base = 0; base < n; base += kThreads) {
    const int i = base + tid;
    const int v = i < n ? load(i) : 0;
    const int incl = wave_scan_incl(v, lane);
    const WgScan w = wg_scan<kThreads / 64>(incl, lane, wv, wsum);
    if (i < n) store(i, carry_s + w.before + incl - v);
    __syncthreads();
    if (tid == 0) carry_s += w.total;
    __syncthreads();
  }
  return carry_s;
}

}  // namespace sift
