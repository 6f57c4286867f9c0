// match_window.hip -- spatially gated kNN matching (k <= 2) of a whole batch for
// gfx950: the segmented matchers of match.hip (float L1), match_u8.hip (byte
// L1) and match_l2_u8.hip (byte squared L2) with one change -- a train row is a
// candidate for a query only if its keypoint lies in the closed square window
// of half-side `radius` around the query's predicted position
// (sift_knn_match_window_segmented_device, sift_hip.h).  DESIGN.md §6i.
//
// Distances are the dense matchers' own bit for bit: float L1 in the summation
// order of match.hip's l1_row (eight partial sums p[k] over elements 8g + k in
// g order, q = p[0:4] + p[4:8], (q0 + q1) + (q2 + q3)); the byte metrics are
// exact integers in any order.  Selection is the two smallest (distance, local
// train index) pairs, so the result is a function of the candidate SET: the
// order in which the grid hands the candidates over (which the binning's
// atomics leave to the scheduler) reaches no output byte.
//
// Binning (launch_window_bin): per train segment -- once for a shared train
// set -- the keypoints are counted per cell of an nx x ny grid (atomics), the
// counts are scanned by one workgroup per grid (block_scan.hpp), and the local
// train indices and positions are scattered into cell order (atomics on the
// scanned counts, which turn cell c's start into its end).  Rows with a NaN
// coordinate are dropped: no window admits them.  Cells of one grid row are
// adjacent in that order, so the cells [cx0, cx1] of row cy are ONE run.
//
// The cell function is cell(v) = clamp(floor(v * inv_cell), 0, n - 1), monotone
// non-decreasing in v (a float multiply, floor and a clamp each are), -inf and
// +inf included.  For any monotone cell function with border clamping,
// lo <= tx <= hi implies cell(lo) <= cell(tx) <= cell(hi), whatever the grid's
// extent: the image size only shapes the grid, and points outside it fall into
// the border cells.  The window test |tx - px| <= r is evaluated in float, so a
// row may pass it although tx is below the rounded px - r by a rounding error
// of the subtraction; the range is therefore taken from lo = (px - r) - s and
// hi = (px + r) + s with s = 2^-22 (|px| + r), which covers both roundings (the
// test's, relative 2^-24 of about r, and lo's own, relative 2^-24 of at most
// |px| + r).  A NaN bound opens the range to that border.  Every candidate of
// the range then takes the exact test, so the slack admits nothing.
//
// kNN (knn_window_kernel): kWinGroup = 8 lanes per query, 32 queries per
// workgroup.  A group walks its runs eight entries at a time -- one entry's
// position per lane (a coalesced 64-byte read), the exact window test, a ballot
// -- and scores the admitted rows one after the other, all eight lanes on one
// row: lane k forms the partial sum p[k] of the float distance from the dwords
// 8g + k (32 contiguous bytes per group and load) or the sum over bytes
// [16k, 16k + 16) (one 128-byte row per group and load); three lane exchanges
// inside the group finish the sum in l1_row's order, and leave it in all eight
// lanes, which keep identical top-2 lists.  A cell with more entries than a
// group has lanes only takes more steps of eight.  No LDS, no barrier.
#include "common.hpp"
#include "block_scan.hpp"
#include "homography_math.hpp"
#include "match_seg.hpp"
#include "match_window.hpp"

#include <float.h>

namespace sift {

namespace {

// ---- binning -------------------------------------------------------------------
// Workgroups [g * per_grid, (g + 1) * per_grid) walk grid g's train range.
// kScatter false: cell_end[c] += 1 per row of cell c.  kScatter true (after the
// scan): the row takes the next place of its cell's run.  A place is inside the
// train range's own rows of cell_rows / cell_xy as long as the clamped train
// offsets do not decrease (ranges that overlap would share places: the bound
// check keeps that case inside the range, its result unspecified).
template <bool kScatter>
__global__ __launch_bounds__(256) void window_bin_kernel(WindowArgs A, int per_grid) {
  const int g = blockIdx.x / per_grid, blk = blockIdx.x % per_grid;
  int ts, te;
  train_range(A.toff, g, A.t_cap, ts, te);
  int* ce = A.cell_end + (long long)g * (A.nx * A.ny + 1);
  for (long long r = ts + (long long)blk * 256 + threadIdx.x; r < te; r += (long long)per_grid * 256) {
    const float x = A.t_kpts[r].x, y = A.t_kpts[r].y;
    if (x != x || y != y) continue;
    const int c = cell_of(y, A.inv_cell, A.ny) * A.nx + cell_of(x, A.inv_cell, A.nx);
    const int pos = atomicAdd(&ce[c], 1);
    if (kScatter && pos >= 0 && pos < te - ts) {
      A.cell_rows[ts + pos] = (int)(r - ts);
      A.cell_xy[ts + pos] = make_float2(x, y);
    }
  }
}

// ---- gated kNN -----------------------------------------------------------------
// The grid covers q_cap rows; groups outside the live range
// [clamp(qoff[0]), clamp(qoff[nseg])) leave at once.  Control flow is uniform
// inside a group (everything it branches on is the group's query's), so the
// ballot's eight bits and the exchanges inside the group always see all eight
// lanes, however the groups of a wave diverge.
template <int kMetric>
__global__ __launch_bounds__(kWinBlock) void knn_window_kernel(WindowArgs A) {
  const int sub = threadIdx.x & (kWinGroup - 1);
  const long long ql = (long long)blockIdx.x * kWinQueries + (threadIdx.x / kWinGroup);
  if (ql < clamp_row(A.qoff[0], A.q_cap) || ql >= clamp_row(A.qoff[A.nseg], A.q_cap)) return;
  const int qi = (int)ql;
  const int b = seg_of(A.qoff, A.nseg, A.q_cap, qi);
  int ts, te;
  train_range(A.toff, b, A.t_cap, ts, te);
  const int n_cells = A.nx * A.ny;
  const int* ce = A.cell_end + (A.toff ? (long long)b * (n_cells + 1) : 0ll);

  // the predicted position: the query's own, or H[b] applied to it
  float px = A.q_kpts[qi].x, py = A.q_kpts[qi].y;
  if (A.H && !(A.found && A.found[b] == 0)) {
    float o[2];
    hmath::perspective_point(A.H + 9ll * b, px, py, o);
    px = o[0];
    py = o[1];
  }
  Best2 best = top2_empty<float>();
  if (px == px && py == py) {  // a NaN position admits no row
    const float r = A.radius;
    const float sx = kWinSlack * (fabsf(px) + r), sy = kWinSlack * (fabsf(py) + r);
    const int cx0 = cell_lo((px - r) - sx, A.inv_cell, A.nx), cx1 = cell_hi((px + r) + sx, A.inv_cell, A.nx);
    const int cy0 = cell_lo((py - r) - sy, A.inv_cell, A.ny), cy1 = cell_hi((py + r) + sy, A.inv_cell, A.ny);
    Metric<kMetric> M;
    M.load(A.q, qi, sub);
    const int shift = (threadIdx.x & 63) & ~(kWinGroup - 1);  // the group's first lane in the wave
    for (int cy = cy0; cy <= cy1; ++cy) {
      const int c0 = cy * A.nx + cx0, c1 = cy * A.nx + cx1;
      const int s0 = c0 ? ce[c0 - 1] : 0, s1 = min(ce[c1], te - ts);
      for (int s = s0; s < s1; s += kWinGroup) {
        const int e = s + sub;
        bool ok = false;
        int row = 0;
        if (e < s1) {
          const float2 p = A.cell_xy[ts + e];
          ok = fabsf(p.x - px) <= r && fabsf(p.y - py) <= r;
          row = A.cell_rows[ts + e];
        }
        unsigned m = (unsigned)(__ballot(ok) >> shift) & ((1u << kWinGroup) - 1u);
        while (m) {
          const int j = __ffs(m) - 1;
          m &= m - 1;
          const int cand = __shfl(row, j, kWinGroup);
          if ((unsigned)cand >= (unsigned)(te - ts)) continue;  // only with overlapping train ranges (see the binning)
          insert(best, M.score(A.t, (long long)ts + cand, sub), cand);
        }
      }
    }
  }
  if (sub == 0) write_knn(best, qi, A.k, A.idx, A.dist);
}

}  // namespace

hipError_t launch_window_bin(hipStream_t st, const WindowArgs& A) {
  const int n_grids = A.toff ? A.nseg : 1, n_cells = A.nx * A.ny;
  if (hipError_t e = hipMemsetAsync(A.cell_end, 0, (size_t)n_grids * (n_cells + 1) * sizeof(int), st)) return e;
  // about two workgroups' worth of rows per workgroup when the rows are spread evenly; the loop takes the rest
  long long per = ((long long)A.t_cap / n_grids + 511) / 512;
  per = per < 1 ? 1 : (per > 1024 ? 1024 : per);
  const long long max_grid = 0x7fffffffll / 2;
  while (per > 1 && per * n_grids > max_grid) per /= 2;
  const dim3 grid((unsigned)(per * n_grids));
  hipLaunchKernelGGL(window_bin_kernel<false>, grid, dim3(256), 0, st, A, (int)per);
  hipLaunchKernelGGL(ratio_scan_kernel, dim3(n_grids), dim3(1024), 0, st, A.cell_end, n_cells);  // one array per grid
  hipLaunchKernelGGL(window_bin_kernel<true>, grid, dim3(256), 0, st, A, (int)per);
  return hipSuccess;
}

void launch_knn_window(hipStream_t st, const WindowArgs& A) {
  const dim3 grid((unsigned)(((long long)A.q_cap + kWinQueries - 1) / kWinQueries));
  if (A.metric == SIFT_METRIC_L1_F32)
    hipLaunchKernelGGL(knn_window_kernel<SIFT_METRIC_L1_F32>, grid, dim3(kWinBlock), 0, st, A);
  else if (A.metric == SIFT_METRIC_L1_U8)
    hipLaunchKernelGGL(knn_window_kernel<SIFT_METRIC_L1_U8>, grid, dim3(kWinBlock), 0, st, A);
  else
    hipLaunchKernelGGL(knn_window_kernel<SIFT_METRIC_L2SQR_U8>, grid, dim3(kWinBlock), 0, st, A);
}

}  // namespace sift
