// match.hip -- brute-force L1 k-nearest-neighbour matching (k <= 2) for gfx950.
//
// The consumer of the descriptors in the reference application:
// `BFMatcher(NORM_L1).knnMatch(descriptors1, descriptors0, matches, 2)` and
// the 0.86 ratio test (src/main.cpp:25-40).  SURVEY.md §8(f) row f2.
//
// Distance: OpenCV's float L1 (normL1_, the x86 SSE3 baseline form): eight
// partial sums p[k] = sum_g |a[8g+k] - b[8g+k]| in g order (two 4-lane
// accumulators over 8-element steps), then q = p[0:4] + p[4:8] and the
// horizontal-add reduction (q0 + q1) + (q2 + q3).  oracle/match.py restates the
// same order; real OpenCV may dispatch a wider SIMD form (different float
// rounding), so parity against OpenCV itself is unpinned.
//
// Order: for each query the two smallest (distance, train index) pairs in
// lexicographic order -- OpenCV's batchDistance insertion keeps an earlier
// train index ahead of a later one at equal distance (strict '<').
//
// Layout: a workgroup owns 64 queries (one per lane, descriptor in VGPRs) and
// one split of the train rows; 64-row train chunks are staged in LDS and each
// of the 4 waves scores every fourth row of a chunk (broadcast ds_read_b128:
// all lanes read the same row).  Bound: VALU -- 2 instructions per element
// pair (v_sub, v_add with |x|), 256 per (query, train) pair; the LDS reads are
// 512 B per row per wave.  The 4 waves' top-2 lists merge in LDS; splits merge
// in knn_merge_kernel.
//
// A whole batch (segments given by device-resident offsets): the same tile in
// knn_l1_seg_kernel, then the ratio test with ordered compaction and the point
// gather of src/main.cpp:28-52 (ratio_*_kernel); DESIGN.md §6a.
#include "common.hpp"
#include "block_scan.hpp"
#include "match_seg.hpp"

#include <float.h>

namespace sift {

namespace {

constexpr int kQT = 64;  // queries per workgroup
constexpr int kTC = 64;  // train rows per LDS chunk
constexpr int kV4 = kDescLen / 4;

using Best2 = Top2<float>;  // match_seg.hpp: the list, its order and insert()

// normL1_ of one query (registers) against one staged train row (LDS, the same
// row for every lane): the summation order of the file comment.
__device__ __forceinline__ float l1_row(const float4* tr, const float4 (&qv)[kV4]) {
  float p[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) p[k] = 0.f;
#pragma unroll
  for (int g = 0; g < kDescLen / 8; ++g) {
    const float4 a = tr[2 * g], b = tr[2 * g + 1];
    const float4 x = qv[2 * g], y = qv[2 * g + 1];
    p[0] = p[0] + fabsf(x.x - a.x);
    p[1] = p[1] + fabsf(x.y - a.y);
    p[2] = p[2] + fabsf(x.z - a.z);
    p[3] = p[3] + fabsf(x.w - a.w);
    p[4] = p[4] + fabsf(y.x - b.x);
    p[5] = p[5] + fabsf(y.y - b.y);
    p[6] = p[6] + fabsf(y.z - b.z);
    p[7] = p[7] + fabsf(y.w - b.w);
  }
  const float q0 = p[0] + p[4], q1 = p[1] + p[5], q2 = p[2] + p[6], q3 = p[3] + p[7];
  return (q0 + q1) + (q2 + q3);
}

__global__ __launch_bounds__(256) void knn_l1_kernel(const float* __restrict__ q, int nq, const float* __restrict__ t,
                                                     int nt, int per_split, float2* __restrict__ part_d,
                                                     int2* __restrict__ part_i) {
  __shared__ float4 tl[kTC * kV4];  // 32 KB
  __shared__ float md[4][2][kQT];
  __shared__ int mi[4][2][kQT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int qi = blockIdx.x * kQT + lane;
  float4 qv[kV4];
  {
    const float4* qp = reinterpret_cast<const float4*>(q + (long long)min(qi, nq - 1) * kDescLen);
#pragma unroll
    for (int v = 0; v < kV4; ++v) qv[v] = qp[v];
  }
  Best2 best = top2_empty<float>();
  const int t0 = blockIdx.y * per_split, t1 = min(nt, t0 + per_split);
  for (int c0 = t0; c0 < t1; c0 += kTC) {
    const int nrow = min(kTC, t1 - c0);
    __syncthreads();
    const float4* src = reinterpret_cast<const float4*>(t + (long long)c0 * kDescLen);
    for (int u = threadIdx.x; u < nrow * kV4; u += 256) tl[u] = src[u];
    __syncthreads();
    for (int r = wv; r < nrow; r += 4) {
      insert(best, l1_row(tl + r * kV4, qv), c0 + r);
    }
  }
  md[wv][0][lane] = best.d1;
  md[wv][1][lane] = best.d2;
  mi[wv][0][lane] = best.i1;
  mi[wv][1][lane] = best.i2;
  __syncthreads();
  if (wv == 0 && qi < nq) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      insert(best, md[w][0][lane], mi[w][0][lane]);
      insert(best, md[w][1][lane], mi[w][1][lane]);
    }
    const long long o = (long long)blockIdx.y * nq + qi;
    part_d[o] = make_float2(best.d1, best.d2);
    part_i[o] = make_int2(best.i1, best.i2);
  }
}

__global__ __launch_bounds__(256) void knn_merge_kernel(const float2* __restrict__ part_d,
                                                        const int2* __restrict__ part_i, int nq, int splits, int k,
                                                        int* __restrict__ idx, float* __restrict__ dist) {
  const int qi = blockIdx.x * 256 + threadIdx.x;
  if (qi >= nq) return;
  Best2 best = top2_empty<float>();
  for (int s = 0; s < splits; ++s) {
    const float2 d = part_d[(long long)s * nq + qi];
    const int2 i = part_i[(long long)s * nq + qi];
    insert(best, d.x, i.x);
    insert(best, d.y, i.y);
  }
  write_knn(best, qi, k, idx, dist);
}

// ---- segmented form: a whole batch in one launch sequence ---------------------
// The clamped offsets (clamp_row), the segment search (seg_of), the query-tile
// table (seg_tiles_kernel, here with 64-query tiles) and the merge of the
// splits' lists (knn_seg_merge_kernel) are match_seg.hpp's, shared with the
// byte matchers.

// knn_l1_kernel's tile (64 queries in VGPRs, 64-row train chunks in LDS,
// broadcast reads) with the bounds taken from the device: grid.x covers the
// most tiles the capacities allow, workgroups past tile_start[nseg] exit.
// grid.y splits every segment's own train range evenly.  Indices are local to
// the train range.  splits == 1 writes idx/dist directly.
__global__ __launch_bounds__(256) void knn_l1_seg_kernel(const float* __restrict__ q, const int* __restrict__ qoff,
                                                         int nseg, int q_cap, const float* __restrict__ t,
                                                         const int* __restrict__ toff, int t_cap,
                                                         const int* __restrict__ tile_start, int splits, int k,
                                                         float2* __restrict__ part_d, int2* __restrict__ part_i,
                                                         int* __restrict__ idx, float* __restrict__ dist) {
  __shared__ float4 tl[kTC * kV4];  // 32 KB
  __shared__ float md[4][2][kQT];
  __shared__ int mi[4][2][kQT];
  const int tile = blockIdx.x;
  if (tile >= tile_start[nseg]) return;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = seg_of(tile_start, nseg, 0x7fffffff, tile);
  const int qe = clamp_row(qoff[b + 1], q_cap);
  const int qi = clamp_row(qoff[b], q_cap) + (tile - tile_start[b]) * kQT + lane;  // < qe for lane 0
  int ts = 0, te = t_cap;  // train_range() of match_seg.hpp, restated (profiles/match_refactor_isa.txt)
  if (toff) {
    ts = clamp_row(toff[b], t_cap);
    te = clamp_row(toff[b + 1], t_cap);
    te = te < ts ? ts : te;
  }
  const int per = (((te - ts) + splits - 1) / splits + kTC - 1) / kTC * kTC;
  const long long t0l = ts + (long long)blockIdx.y * per;
  const int t0 = t0l < te ? (int)t0l : te, t1 = (te - t0) < per ? te : t0 + per;
  float4 qv[kV4];
  {
    const float4* qp = reinterpret_cast<const float4*>(q + (long long)min(qi, qe - 1) * kDescLen);
#pragma unroll
    for (int v = 0; v < kV4; ++v) qv[v] = qp[v];
  }
  Best2 best = top2_empty<float>();
  for (int c0 = t0; c0 < t1; c0 += kTC) {
    const int nrow = min(kTC, t1 - c0);
    __syncthreads();
    const float4* src = reinterpret_cast<const float4*>(t + (long long)c0 * kDescLen);
    for (int u = threadIdx.x; u < nrow * kV4; u += 256) tl[u] = src[u];
    __syncthreads();
    for (int r = wv; r < nrow; r += 4) insert(best, l1_row(tl + r * kV4, qv), c0 + r - ts);
  }
  md[wv][0][lane] = best.d1;
  md[wv][1][lane] = best.d2;
  mi[wv][0][lane] = best.i1;
  mi[wv][1][lane] = best.i2;
  __syncthreads();
  if (wv == 0 && qi < qe) {
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      insert(best, md[w][0][lane], mi[w][0][lane]);
      insert(best, md[w][1][lane], mi[w][1][lane]);
    }
    if (splits == 1) {
      write_knn(best, qi, k, idx, dist);
    } else {
      const long long o = (long long)blockIdx.y * q_cap + qi;
      part_d[o] = make_float2(best.d1, best.d2);
      part_i[o] = make_int2(best.i1, best.i2);
    }
  }
}

// ---- ratio test, ordered compaction, point gather (src/main.cpp:28-52) ---------
// Three launches, like the detect stage's scan: kept rows per 256-row block, an
// exclusive scan of the block counts in one workgroup, and the emit, which
// recomputes the flags and ranks them inside the block.  The order is the row
// order; no atomic takes part.
constexpr int kRB = 256;  // rows per block of the ratio stage

struct RatioIn {
  const int* idx;     // [q_cap][2]
  const float* dist;  // [q_cap][2]
  const int* qoff;
  int nseg, q_cap;
  double ratio;
};

// m1.distance <= ratio * m2.distance in double (src/main.cpp:38); a row without
// a second neighbour is skipped (:36).  Rows outside the live range are never kept.
__device__ __forceinline__ bool ratio_keep(const RatioIn& R, int i, int lo, int hi) {
  if (i < lo || i >= hi) return false;
  if (R.idx[2ll * i + 1] < 0) return false;
  return (double)R.dist[2ll * i] <= R.ratio * (double)R.dist[2ll * i + 1];
}

__global__ __launch_bounds__(kRB) void ratio_count_kernel(RatioIn R, int* __restrict__ blk_cnt) {
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lo = clamp_row(R.qoff[0], R.q_cap), hi = clamp_row(R.qoff[R.nseg], R.q_cap);
  const bool keep = ratio_keep(R, blockIdx.x * kRB + threadIdx.x, lo, hi);
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wcnt[wv] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
}

// the scan of the block counts (ratio_scan_kernel) is block_scan.hpp's, shared
// with the cross-check stage

struct RatioOut {
  const sift_keypoint* q_kpts;  // nullptr: no point pairs
  const sift_keypoint* t_kpts;
  const int* toff;              // nullptr: shared train
  sift_match* matches;
  float* src_xy;
  float* dst_xy;
  int m_cap;
  int* moff;
};

// Blocks [0, nblk): one row per thread.  Blocks past nblk: one wave per segment
// boundary b computes moff[b] = kept rows below clamp(qoff[b]).
__global__ __launch_bounds__(kRB) void ratio_emit_kernel(RatioIn R, const int* __restrict__ blk_pre, int nblk,
                                                         RatioOut O) {
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lo = clamp_row(R.qoff[0], R.q_cap), hi = clamp_row(R.qoff[R.nseg], R.q_cap);
  if ((int)blockIdx.x >= nblk) {
    const int b = ((int)blockIdx.x - nblk) * 4 + wv;
    if (b > R.nseg) return;
    const int r = clamp_row(R.qoff[b], R.q_cap), blk = r / kRB;  // blk == nblk only with no rows to count
    int cnt = 0;
    for (int j = blk * kRB + lane; j < r; j += 64) cnt += ratio_keep(R, j, lo, hi) ? 1 : 0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d);
    if (lane == 0) O.moff[b] = blk_pre[blk] + cnt;
    return;
  }
  const int i = blockIdx.x * kRB + threadIdx.x;
  const bool keep = ratio_keep(R, i, lo, hi);
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wcnt[wv] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int pos = blk_pre[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wv; ++w) pos += wcnt[w];
  if (pos >= O.m_cap) return;
  const int b = seg_of(R.qoff, R.nseg, R.q_cap, i);
  const int tr = R.idx[2ll * i];
  sift_match rec;
  rec.query = i - clamp_row(R.qoff[b], R.q_cap);
  rec.train = tr;
  rec.distance = R.dist[2ll * i];
  rec.segment = b;
  O.matches[pos] = rec;
  if (O.q_kpts) {
    const long long tg = (O.toff ? (long long)O.toff[b] : 0ll) + tr;
    O.src_xy[2ll * pos] = O.q_kpts[i].x;
    O.src_xy[2ll * pos + 1] = O.q_kpts[i].y;
    O.dst_xy[2ll * pos] = O.t_kpts[tg].x;
    O.dst_xy[2ll * pos + 1] = O.t_kpts[tg].y;
  }
}

}  // namespace

int knn_splits(int nq, int nt) {
  const int gx = (nq + kQT - 1) / kQT;
  int s = (2048 + gx - 1) / gx;                  // ~2k workgroups to fill 256 CUs
  const int max_s = (nt + kTC - 1) / kTC;         // at least one chunk per split
  s = s < max_s ? s : max_s;
  return s < 1 ? 1 : s;
}

void launch_knn_l1(hipStream_t st, const float* q, int nq, const float* t, int nt, int k, int splits,
                   float2* part_d, int2* part_i, int* idx, float* dist) {
  if (nq <= 0) return;
  const int per = ((nt + splits - 1) / splits + kTC - 1) / kTC * kTC;
  dim3 grid((nq + kQT - 1) / kQT, splits);
  hipLaunchKernelGGL(knn_l1_kernel, grid, dim3(256), 0, st, q, nq, t, nt, per, part_d, part_i);
  hipLaunchKernelGGL(knn_merge_kernel, dim3((nq + 255) / 256), dim3(256), 0, st, part_d, part_i, nq, splits, k,
                     idx, dist);
}

int knn_seg_max_tiles(int q_cap, int n_segments) { return q_cap / kQT + n_segments; }

int knn_seg_splits(int q_cap, int n_segments, int t_cap, bool seg_train) {
  const int gx = knn_seg_max_tiles(q_cap, n_segments);
  int s = (2048 + gx - 1) / gx;
  // segmented train: an even share of the buffer stands in for the segment size
  const int nt = seg_train ? (t_cap + n_segments - 1) / n_segments : t_cap;
  const int max_s = (nt + kTC - 1) / kTC;
  s = s < max_s ? s : max_s;
  return s < 1 ? 1 : s;
}

void launch_knn_l1_seg(hipStream_t st, const float* q, const int* qoff, int n_segments, int q_cap, const float* t,
                       const int* toff, int t_cap, int k, int splits, int* tile_start, float2* part_d, int2* part_i,
                       int* idx, float* dist) {
  hipLaunchKernelGGL(seg_tiles_kernel<kQT>, dim3(1), dim3(256), 0, st, qoff, n_segments, q_cap, tile_start);
  dim3 grid(knn_seg_max_tiles(q_cap, n_segments), splits);
  hipLaunchKernelGGL(knn_l1_seg_kernel, grid, dim3(256), 0, st, q, qoff, n_segments, q_cap, t, toff, t_cap,
                     tile_start, splits, k, part_d, part_i, idx, dist);
  if (splits > 1)
    hipLaunchKernelGGL(knn_seg_merge_kernel<float2>, dim3((q_cap + 255) / 256), dim3(256), 0, st, part_d, part_i, qoff,
                       n_segments, q_cap, splits, k, idx, dist);
}

int ratio_blocks(int q_cap) { return (q_cap + kRB - 1) / kRB; }

void launch_ratio_matches(hipStream_t st, const int* idx, const float* dist, const int* qoff, int n_segments,
                          int q_cap, double ratio, const sift_keypoint* q_kpts, const sift_keypoint* t_kpts,
                          const int* toff, sift_match* matches, float* src_xy, float* dst_xy, int m_cap, int* moff,
                          int* blk_scan) {
  const int nblk = ratio_blocks(q_cap);
  const RatioIn R{idx, dist, qoff, n_segments, q_cap, ratio};
  const RatioOut O{q_kpts, t_kpts, toff, matches, src_xy, dst_xy, m_cap, moff};
  hipLaunchKernelGGL(ratio_count_kernel, dim3(nblk), dim3(kRB), 0, st, R, blk_scan);
  hipLaunchKernelGGL(ratio_scan_kernel, dim3(1), dim3(1024), 0, st, blk_scan, nblk);
  hipLaunchKernelGGL(ratio_emit_kernel, dim3(nblk + (n_segments + 1 + 3) / 4), dim3(kRB), 0, st, R, blk_scan, nblk,
                     O);
}

}  // namespace sift
