// affine.hip -- estimateAffine2D / estimateAffinePartial2D (RANSAC) for ONE set
// of point pairs on the host, behind sift_estimate_affine: host code like
// homography.hip, for the same reason.  A batch whose point pairs are already
// on the device is affine_batch.hip's; both take every expression from
// affine_math.hpp (the rule is written out there), and this file keeps only
// the serial control flow.
#include <string.h>

#include <algorithm>
#include <vector>

#include "affine_math.hpp"
#include "common.hpp"

namespace sift {

namespace {

using namespace amath;

template <int kModel>
int estimate(const P2* s, const P2* d, int n, double thr, int max_iters, double confidence, double* A,
             unsigned char* mask_out) {
  constexpr int m = model_points(kModel);
  if (n < m || !(confidence > 0 && confidence < 1) || max_iters < 1) return 0;
  std::vector<unsigned char> best_mask(n, 0), mask(n);
  double best[6] = {0}, model[6];
  if (n == m) {
    if (!solve_minimal<kModel>(s, d, best)) return 0;
    std::fill(best_mask.begin(), best_mask.end(), 1);
  } else {
    const float t = hmath::inlier_limit(thr);
    Rng rng{~0ull};
    int niters = max_iters, max_good = 0;
    for (int iter = 0; iter < niters; ++iter) {
      int idx[m];
      P2 ms[m], md[m];
      if (!get_subset<kModel>(rng, s, d, n, idx, ms, md)) break;
      if (!solve_minimal<kModel>(ms, md, model)) continue;
      float f[6];
      to_float6(model, f);
      int good = 0;
      for (int i = 0; i < n; ++i) {
        mask[i] = is_inlier(f, s[i].x, s[i].y, d[i].x, d[i].y, t);
        good += mask[i];
      }
      if (wins(good, max_good, m)) {
        best_mask.swap(mask);
        memcpy(best, model, sizeof(best));
        max_good = good;
        niters = hmath::update_num_iters(confidence, (double)(n - good) / n, m, niters);
      }
    }
    if (max_good <= 0) return 0;
    // the least-squares refit on the inliers; the mask stays the hypothesis's
    double c[kRefitCoords] = {0}, S[kRefitSumsMax] = {0}, term[kRefitSumsMax];
    for (int i = 0; i < n; ++i)
      if (best_mask[i])
        for (int a = 0; a < kRefitCoords; ++a) c[a] += refit_coord(s[i], d[i], a);
    for (int a = 0; a < kRefitCoords; ++a) c[a] /= max_good;
    for (int i = 0; i < n; ++i)
      if (best_mask[i]) {
        refit_terms<kModel>(c, s[i], d[i], term);
        for (int a = 0; a < refit_sums(kModel); ++a) S[a] += term[a];
      }
    refit_finish<kModel>(c, S, best);
  }
  memcpy(A, best, sizeof(best));
  if (mask_out) memcpy(mask_out, best_mask.data(), n);
  return 1;
}

}  // namespace

int estimate_affine_ransac(const float* src_xy, const float* dst_xy, int n, int model, double thr, int max_iters,
                           double confidence, double* A, unsigned char* mask_out) {
  const P2* s = reinterpret_cast<const P2*>(src_xy);
  const P2* d = reinterpret_cast<const P2*>(dst_xy);
  if (model == kAffine) return estimate<kAffine>(s, d, n, thr, max_iters, confidence, A, mask_out);
  if (model == kSimilarity) return estimate<kSimilarity>(s, d, n, thr, max_iters, confidence, A, mask_out);
  return 0;
}

}  // namespace sift
