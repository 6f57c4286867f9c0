// match_seg.hpp -- what the matchers share (match.hip: float L1, 64-query
// tiles; match_u8.hip: byte L1, 64 x Q-query tiles; match_l2_u8.hip: byte
// squared L2, 32 x Q-query tiles; match_window.hip: the three metrics inside a
// search window): the clamped device offsets, the segment search, the clamped
// train range, the query-tile table, and the one top-2 core -- the (distance,
// index) list with its order, its insertion, its write-out and the merge of the
// splits' lists.  Device code, included by the matchers and by cross_check.hip
// (the offsets and the search) only; every translation unit instantiates its
// own copy (anonymous namespace, no relocatable device code).
#pragma once

#include "common.hpp"
#include "wave_scan.hpp"

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

// Segment b's train rows [ts, te): the whole buffer for a shared train set
// (toff null), else the clamped offsets, an inverted pair read as empty.  The
// three dense segmented scoring kernels restate these lines in place: through
// the call their prologue compiles to other code (profiles/match_refactor_isa.txt).
__device__ __forceinline__ void train_range(const int* toff, int b, int t_cap, int& ts, int& te) {
  ts = 0;
  te = t_cap;
  if (toff) {
    ts = clamp_row(toff[b], t_cap);
    te = clamp_row(toff[b + 1], t_cap);
    te = te < ts ? ts : te;
  }
}

// ---- the top-2 list ------------------------------------------------------------
// The two smallest (distance, index) pairs seen so far, distances ascending,
// over float (L1 on float rows) or int (the byte metrics) distances.  An empty
// slot is (kEmptyDist, -1): +inf, or a value above every integer distance.
template <typename D>
constexpr D kEmptyDist = D();
template <>
constexpr float kEmptyDist<float> = INFINITY;
template <>
constexpr int kEmptyDist<int> = 0x7fffffff;

template <typename D>
struct Top2 {
  D d1, d2;
  int i1, i2;
};

template <typename D>
__device__ __forceinline__ Top2<D> top2_empty() {
  return {kEmptyDist<D>, kEmptyDist<D>, -1, -1};
}

// (d, i) < (e, j) lexicographically: an earlier index stays ahead of a later one
// at equal distance (OpenCV's batchDistance insertion, strict '<').  An empty
// slot sorts last via its distance; no index is below -1, so a candidate at the
// empty distance never displaces one: a float row at d = +inf is never a
// neighbour (sift_hip.h).
template <typename D>
__device__ __forceinline__ bool lex_lt(D d, int i, D e, int j) { return d < e || (d == e && i < j); }

template <typename D>
__device__ __forceinline__ void insert(Top2<D>& b, D d, int i) {
  if (lex_lt(d, i, b.d1, b.i1)) {
    b.d2 = b.d1;
    b.i2 = b.i1;
    b.d1 = d;
    b.i1 = i;
  } else if (lex_lt(d, i, b.d2, b.i2)) {
    b.d2 = d;
    b.i2 = i;
  }
}

// The distance as the result holds it: an integer one converted (exact below
// 2^24), +inf beside the index -1.
__device__ __forceinline__ float result_dist(float d, int) { return d; }
__device__ __forceinline__ float result_dist(int d, int i) { return i < 0 ? INFINITY : (float)d; }

// Row qi of idx / dist ([rows][k], k = 1 or 2).
template <typename D>
__device__ __forceinline__ void write_knn(const Top2<D>& b, long long qi, int k, int* idx, float* dist) {
  idx[qi * k] = b.i1;
  dist[qi * k] = result_dist(b.d1, b.i1);
  if (k == 2) {
    idx[qi * k + 1] = b.i2;
    dist[qi * k + 1] = result_dist(b.d2, b.i2);
  }
}

// The splits' lists (part_d / part_i: [splits][q_cap], float2 or int2 distances)
// of the live rows [clamp(qoff[0]), clamp(qoff[nseg])) only, in split order.
template <typename P>
__global__ __launch_bounds__(256) void knn_seg_merge_kernel(const P* __restrict__ part_d,
                                                            const int2* __restrict__ part_i,
                                                            const int* __restrict__ qoff, int nseg, int q_cap,
                                                            int splits, int k, int* __restrict__ idx,
                                                            float* __restrict__ dist) {
  const int qi = blockIdx.x * 256 + threadIdx.x;
  if (qi < clamp_row(qoff[0], q_cap) || qi >= clamp_row(qoff[nseg], q_cap)) return;
  auto best = top2_empty<decltype(P().x)>();
  for (int s = 0; s < splits; ++s) {
    const P d = part_d[(long long)s * q_cap + qi];
    const int2 i = part_i[(long long)s * q_cap + qi];
    insert(best, d.x, i.x);
    insert(best, d.y, i.y);
  }
  write_knn(best, qi, k, idx, dist);
}

// Prologue (one workgroup): tile_start[b] = number of kTile-query tiles of the
// segments before b, tile_start[nseg] = all tiles.  A tile never spans two
// segments, so with segmented train it has one train range.
template <int kTile>
__global__ __launch_bounds__(256) void seg_tiles_kernel(const int* __restrict__ qoff, int nseg, int q_cap,
                                                        int* __restrict__ tile_start) {
  const int total = wg_scan_chunks<256>(
      nseg,
      [&](int b) {
        const int s = clamp_row(qoff[b], q_cap), e = clamp_row(qoff[b + 1], q_cap);
        return e > s ? (e - s + kTile - 1) / kTile : 0;
      },
      [&](int b, int x) { tile_start[b] = x; });
  if (threadIdx.x == 0) tile_start[nseg] = total;
}

}  // namespace

}  // namespace sift
