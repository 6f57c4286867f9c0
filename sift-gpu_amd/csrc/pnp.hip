// pnp.hip -- solveP3P and solvePnPRansac for ONE set of 3-D / 2-D rows on the
// host, behind sift_solve_p3p and sift_solve_pnp: host code like fundamental.hip
// and pose.hip, for the same reason.  A batch whose rows are already on the
// device is pnp_batch.hip's; both take every expression from pnp_math.hpp (the
// rule is written out there), and this file keeps only the serial control flow.
#include <string.h>

#include <vector>

#include "common.hpp"
#include "pnp_math.hpp"

namespace sift {

using namespace pnpmath;

int solve_p3p(const double* xyz, const float* xy, const double* K, double* poses) {
  const P2* pix = reinterpret_cast<const P2*>(xy);
  memset(poses, 0, kSolutions * 12 * sizeof(double));
  Calib c;
  if (!calibrate(K, c)) return 0;
  double y[9];
  for (int i = 0; i < 3; ++i) bearing(c.Ki, pix[i], y + 3 * i);
  int count = 0;
  p3p(xyz, y, [&](const double* P) { memcpy(poses + 12 * count++, P, 12 * sizeof(double)); });
  return count;
}

namespace {

// a hypothesis from four rows; a masked-out row: no model
bool fit_rows(const Calib& c, const double* xyz, const P2* pix, const unsigned char* on, const int* idx, double* pose) {
  double x[12];
  P2 p[kModelPoints];
  for (int i = 0; i < kModelPoints; ++i) {
    if (on && !on[idx[i]]) return false;
    memcpy(x + 3 * i, xyz + (size_t)idx[i] * 3, 3 * sizeof(double));
    p[i] = pix[idx[i]];
  }
  return hypothesis(c, x, p, pose);
}

// the 28 sums over the rows of mask, in row order
void refit_sums(const Calib& c, const double* P, const double* xyz, const P2* pix, const unsigned char* mask, int n,
                double* sums) {
  for (int a = 0; a < kRefitSums; ++a) sums[a] = 0;
  for (int i = 0; i < n; ++i) {
    if (!mask[i]) continue;
    double t[kRefitSums];
    refit_terms(c.Ki, P, xyz + (size_t)i * 3, pix[i], t);
    for (int a = 0; a < kRefitSums; ++a) sums[a] += t[a];
  }
}

}  // namespace

int solve_pnp_ransac(const double* xyz, const float* xy, int n, const unsigned char* row_mask, const double* K,
                     double thr, int max_iters, double confidence, double* pose, unsigned char* mask_out,
                     int* n_inliers) {
  constexpr int m = kModelPoints;
  const P2* pix = reinterpret_cast<const P2*>(xy);
  memset(pose, 0, 12 * sizeof(double));
  if (mask_out) memset(mask_out, 0, (size_t)n);
  *n_inliers = 0;
  Calib c;
  if (n < m || !(confidence > 0 && confidence < 1) || max_iters < 1 || !calibrate(K, c)) return 0;
  std::vector<unsigned char> best_mask(n, 0), mask(n);
  double best[12], model[12];
  int max_good = 0;
  if (n == m) {
    const int idx[m] = {0, 1, 2, 3};
    if (!fit_rows(c, xyz, pix, row_mask, idx, best)) return 0;
    best_mask.assign(n, 1);
    max_good = m;
  } else {
    const double t2 = inlier_limit(thr);
    Rng rng{~0ull};
    int niters = max_iters;
    for (int iter = 0; iter < niters; ++iter) {
      int idx[m];
      draw_subset(rng, n, idx);
      if (!fit_rows(c, xyz, pix, row_mask, idx, model)) continue;
      int good = 0;
      for (int i = 0; i < n; ++i) {
        mask[i] = !(row_mask && !row_mask[i]) && is_inlier(c.K, model, xyz + (size_t)i * 3, pix[i], t2);
        good += mask[i];
      }
      if (hmath::wins(good, max_good)) {
        best_mask.swap(mask);
        memcpy(best, model, sizeof(best));
        max_good = good;
        niters = hmath::update_num_iters(confidence, (double)(n - good) / n, m, niters);
      }
    }
    if (max_good <= 0) return 0;
    // the refit over the hypothesis's inliers; the mask stays the hypothesis's
    double cur[12], cand[12], held[kRefitSums], sums[kRefitSums];
    memcpy(cur, best, sizeof(cur));
    refit_sums(c, cur, xyz, pix, best_mask.data(), n, held);
    for (int step = 0; step < kRefitSteps; ++step) {
      if (!refit_candidate(held, cur, cand)) break;
      refit_sums(c, cand, xyz, pix, best_mask.data(), n, sums);
      if (!refit_accept(sums[kRefitSums - 1], held[kRefitSums - 1])) break;
      memcpy(cur, cand, sizeof(cur));
      memcpy(held, sums, sizeof(held));
    }
    if (finite_n(cur, 12)) memcpy(best, cur, sizeof(best));
  }
  memcpy(pose, best, sizeof(best));
  if (mask_out) memcpy(mask_out, best_mask.data(), n);
  *n_inliers = max_good;
  return 1;
}

}  // namespace sift
