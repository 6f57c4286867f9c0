// match_epipolar.hip -- kNN matching (k <= 2) of a whole batch along epipolar
// lines for gfx950: the windowed matcher of match_window.hip around the query's
// own position, with a second gate -- train row t is a candidate for query q of
// segment b only if the pair also passes fmath::is_inlier under the segment's
// fundamental matrix, the estimate's own float test at the limit
// (float)(band * band) (sift_knn_match_epipolar_segmented_device, sift_hip.h).
// DESIGN.md §6o.
//
// Everything but the walk is match_window.hip's: the binning
// (launch_window_bin: train keypoints counted, scanned and scattered into the
// cells of an nx x ny grid, the cells of one grid row adjacent), the Metric<>
// scorers with the dense matchers' bits, the top-2 core, eight lanes per query,
// one entry's position per lane, a ballot, admitted rows scored one after the
// other, no LDS.  The result is a function of the candidate SET alone: neither
// the grid's shape nor the order the binning's atomics left in the cells
// reaches an output byte.
//
// The walk.  The window gives the cell rectangle [cx0, cx1] x [cy0, cy1] as in
// match_window.hip.  With a model, the query's line in the train image is
// l = F [x y 1]^T as is_inlier forms it (emath::dst_line), and for each grid
// row cy the rectangle's run is narrowed to the cells the band
// |aX + bY + c| <= band sqrt(a^2 + b^2) can touch over that row's Y slab
// intersected with the window's own Y range (emath::band_cells, whose file
// comment argues the slack): a near-horizontal line leaves whole-row runs in
// few rows, a near-vertical one a cell or two in every row, and a row whose
// range is empty is skipped before any memory read.  The range only
// over-covers; every candidate of it takes the exact test -- the window's and
// is_inlier's both sides -- so the narrowing admits and rejects nothing.  The
// src-side distance (the query against the train point's line) does not narrow
// the walk: it is a property of the candidate, not of a cell.
#include "common.hpp"
#include "epipolar_math.hpp"
#include "match_seg.hpp"
#include "match_window.hpp"

#include <float.h>

namespace sift {

namespace {

// The grid covers q_cap rows; groups outside the live range leave at once.
// Control flow is uniform inside a group (everything it branches on is the
// group's query's), as in knn_window_kernel.
template <int kMetric>
__global__ __launch_bounds__(kWinBlock) void knn_epipolar_kernel(EpipolarArgs E) {
  const WindowArgs& A = E.W;
  const int sub = threadIdx.x & (kWinGroup - 1);
  const long long ql = (long long)blockIdx.x * kWinQueries + (threadIdx.x / kWinGroup);
  if (ql < clamp_row(A.qoff[0], A.q_cap) || ql >= clamp_row(A.qoff[A.nseg], A.q_cap)) return;
  const int qi = (int)ql;
  const int b = seg_of(A.qoff, A.nseg, A.q_cap, qi);
  int ts, te;
  train_range(A.toff, b, A.t_cap, ts, te);
  const int n_cells = A.nx * A.ny;
  const int* ce = A.cell_end + (A.toff ? (long long)b * (n_cells + 1) : 0ll);

  const float px = A.q_kpts[qi].x, py = A.q_kpts[qi].y;
  const bool model = A.H && !(A.found && A.found[b] == 0);
  float f[9] = {};
  emath::Band band = {0., 0., 0., 0., emath::kAll};
  if (model) {
    fmath::to_float9(A.H + 9ll * b, f);
    float l[3];
    emath::dst_line(f, px, py, l);
    band = emath::band_of(l[0], l[1], l[2], E.limit);
  }
  Best2 best = top2_empty<float>();
  if (px == px && py == py && band.kind != emath::kNone) {  // a NaN position admits no row
    const float r = A.radius;
    const float sx = kWinSlack * (fabsf(px) + r), sy = kWinSlack * (fabsf(py) + r);
    const float wy0 = (py - r) - sy, wy1 = (py + r) + sy;
    const int cx0 = cell_lo((px - r) - sx, A.inv_cell, A.nx), cx1 = cell_hi((px + r) + sx, A.inv_cell, A.nx);
    const int cy0 = cell_lo(wy0, A.inv_cell, A.ny), cy1 = cell_hi(wy1, A.inv_cell, A.ny);
    Metric<kMetric> M;
    M.load(A.q, qi, sub);
    const int shift = (threadIdx.x & 63) & ~(kWinGroup - 1);  // the group's first lane in the wave
    for (int cy = cy0; cy <= cy1; ++cy) {
      int x0 = cx0, x1 = cx1;
      if (band.kind == emath::kStrip) {
        double y0, y1;
        emath::row_slab(cy, A.ny, A.inv_cell, &y0, &y1);
        y0 = fmax(y0, (double)wy0);  // a NaN end of the window's range (inf - inf) leaves the slab's
        y1 = fmin(y1, (double)wy1);
        int bx0, bx1;
        if (!emath::band_cells(band, y0, y1, A.inv_cell, A.nx, &bx0, &bx1)) continue;
        x0 = max(x0, bx0);
        x1 = min(x1, bx1);
        if (x0 > x1) continue;
      }
      const int c0 = cy * A.nx + x0, c1 = cy * A.nx + x1;
      const int s0 = c0 ? ce[c0 - 1] : 0, s1 = min(ce[c1], te - ts);
      for (int s = s0; s < s1; s += kWinGroup) {
        const int e = s + sub;
        bool ok = false;
        int row = 0;
        if (e < s1) {
          const float2 p = A.cell_xy[ts + e];
          ok = fabsf(p.x - px) <= r && fabsf(p.y - py) <= r && (!model || fmath::is_inlier(f, px, py, p.x, p.y, E.limit));
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

void launch_knn_epipolar(hipStream_t st, const EpipolarArgs& E) {
  const dim3 grid((unsigned)(((long long)E.W.q_cap + kWinQueries - 1) / kWinQueries));
  if (E.W.metric == SIFT_METRIC_L1_F32)
    hipLaunchKernelGGL(knn_epipolar_kernel<SIFT_METRIC_L1_F32>, grid, dim3(kWinBlock), 0, st, E);
  else if (E.W.metric == SIFT_METRIC_L1_U8)
    hipLaunchKernelGGL(knn_epipolar_kernel<SIFT_METRIC_L1_U8>, grid, dim3(kWinBlock), 0, st, E);
  else
    hipLaunchKernelGGL(knn_epipolar_kernel<SIFT_METRIC_L2SQR_U8>, grid, dim3(kWinBlock), 0, st, E);
}

}  // namespace sift
