// cross_check.hip -- cross-check (mutual nearest neighbour) matching for a
// whole batch: cv::BFMatcher(norm, crossCheck = true), which keeps (q, t) only
// if t is q's nearest train row and q is t's nearest query row.
//
// The two directions are two runs of a segmented matcher (match.hip,
// match_u8.hip, match_l2_u8.hip), the second with query and train exchanged;
// this file is the stage that joins the two results on the device and writes
// what the ratio stage (match.hip, ratio_*_kernel) writes: dense records in
// query order, the per-segment offsets and the point pairs.  DESIGN.md §6f.
//
// Shape: the ratio stage's three launches -- kept rows per 256-row block, the
// exclusive scan of the block counts in one workgroup (block_scan.hpp), and the
// emit, which recomputes the flags and ranks them inside the block, with a wave
// per segment boundary for m_offsets.  The order is the row order; no atomic
// takes part.  What differs is the predicate: it needs the row's segment
// (seg_of) and one dependent load from the reverse table, whose address is
// bounded by the segment's clamped train range before the load.  Bound: memory
// latency -- 8 to 16 bytes of the forward tables per row, a binary search over
// the offsets (cached) and one 4-byte gather per row that passes the cheaper
// tests.
#include "common.hpp"
#include "block_scan.hpp"
#include "match_seg.hpp"

namespace sift {

namespace {

constexpr int kCB = 256;  // rows per block of the stage

struct CrossIn {
  const int* idx;     // [q_cap][fk], the forward result (query -> train)
  const float* dist;  // [q_cap][fk]
  const int* ridx;    // [t_cap][rk], the reverse result (train -> query); column 0 is read
  const int* qoff;
  const int* toff;
  int fk, rk;         // row strides of the two tables
  int nseg, q_cap, t_cap;
  double ratio;       // 0: cross-check only
};

// Query row i is kept iff it is live, has a neighbour j, passes the ratio test
// when one is asked for (the ratio stage's expression, src/main.cpp:36-38), j is
// a row of its segment's clamped train range, and that row's nearest query row
// is i.  Rows outside the live range hold whatever the caller left there: none
// of their values is used, and no value of idx reaches an address before it is
// bounded.  b and j are set for a kept row.
__device__ __forceinline__ bool cross_keep(const CrossIn& X, int i, int lo, int hi, int& b, int& j) {
  if (i < lo || i >= hi) return false;
  j = X.idx[(long long)i * X.fk];
  if (j < 0) return false;
  if (X.ratio > 0) {
    if (X.idx[(long long)i * X.fk + 1] < 0) return false;
    if (!((double)X.dist[(long long)i * X.fk] <= X.ratio * (double)X.dist[(long long)i * X.fk + 1])) return false;
  }
  b = seg_of(X.qoff, X.nseg, X.q_cap, i);
  const int tlo = clamp_row(X.toff[b], X.t_cap), thi = clamp_row(X.toff[b + 1], X.t_cap);
  if (j >= thi - tlo) return false;  // tlo + j < thi <= t_cap, without the sum
  return X.ridx[(long long)(tlo + j) * X.rk] == i - clamp_row(X.qoff[b], X.q_cap);
}

__global__ __launch_bounds__(kCB) void cross_count_kernel(CrossIn X, int* __restrict__ blk_cnt) {
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lo = clamp_row(X.qoff[0], X.q_cap), hi = clamp_row(X.qoff[X.nseg], X.q_cap);
  int b, j;
  const bool keep = cross_keep(X, blockIdx.x * kCB + threadIdx.x, lo, hi, b, j);
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wcnt[wv] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
}

struct CrossOut {
  const sift_keypoint* q_kpts;  // nullptr: no point pairs
  const sift_keypoint* t_kpts;
  sift_match* matches;
  float* src_xy;
  float* dst_xy;
  int m_cap;
  int* moff;
};

// Blocks [0, nblk): one row per thread.  Blocks past nblk: one wave per segment
// boundary b computes moff[b] = kept rows below clamp(qoff[b]).
__global__ __launch_bounds__(kCB) void cross_emit_kernel(CrossIn X, const int* __restrict__ blk_pre, int nblk,
                                                         CrossOut O) {
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lo = clamp_row(X.qoff[0], X.q_cap), hi = clamp_row(X.qoff[X.nseg], X.q_cap);
  int b, j;
  if ((int)blockIdx.x >= nblk) {
    const int s = ((int)blockIdx.x - nblk) * 4 + wv;
    if (s > X.nseg) return;
    const int r = clamp_row(X.qoff[s], X.q_cap), blk = r / kCB;  // blk == nblk only with no rows to count
    int cnt = 0;
    for (int i = blk * kCB + lane; i < r; i += 64) cnt += cross_keep(X, i, lo, hi, b, j) ? 1 : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
    if (lane == 0) O.moff[s] = blk_pre[blk] + cnt;
    return;
  }
  const int i = blockIdx.x * kCB + threadIdx.x;
  const bool keep = cross_keep(X, i, lo, hi, b, j);
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wcnt[wv] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int pos = blk_pre[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wv; ++w) pos += wcnt[w];
  if (pos >= O.m_cap) return;
  sift_match rec;
  rec.query = i - clamp_row(X.qoff[b], X.q_cap);
  rec.train = j;
  rec.distance = X.dist[(long long)i * X.fk];
  rec.segment = b;
  O.matches[pos] = rec;
  if (O.q_kpts) {
    const long long tg = (long long)clamp_row(X.toff[b], X.t_cap) + j;  // < t_cap: cross_keep bounded it
    O.src_xy[2ll * pos] = O.q_kpts[i].x;
    O.src_xy[2ll * pos + 1] = O.q_kpts[i].y;
    O.dst_xy[2ll * pos] = O.t_kpts[tg].x;
    O.dst_xy[2ll * pos + 1] = O.t_kpts[tg].y;
  }
}

}  // namespace

int cross_blocks(int q_cap) { return (q_cap + kCB - 1) / kCB; }

void launch_cross_check(hipStream_t st, const int* idx, const float* dist, int fwd_k, const int* qoff, int n_segments,
                        int q_cap, const int* ridx, int rev_k, const int* toff, int t_cap, double ratio,
                        const sift_keypoint* q_kpts, const sift_keypoint* t_kpts, sift_match* matches, float* src_xy,
                        float* dst_xy, int m_cap, int* moff, int* blk_scan) {
  const int nblk = cross_blocks(q_cap);
  const CrossIn X{idx, dist, ridx, qoff, toff, fwd_k, rev_k, n_segments, q_cap, t_cap, ratio};
  const CrossOut O{q_kpts, t_kpts, matches, src_xy, dst_xy, m_cap, moff};
  hipLaunchKernelGGL(cross_count_kernel, dim3(nblk), dim3(kCB), 0, st, X, blk_scan);
  hipLaunchKernelGGL(ratio_scan_kernel, dim3(1), dim3(1024), 0, st, blk_scan, nblk);
  hipLaunchKernelGGL(cross_emit_kernel, dim3(nblk + (n_segments + 1 + 3) / 4), dim3(kCB), 0, st, X, blk_scan, nblk,
                     O);
}

}  // namespace sift
