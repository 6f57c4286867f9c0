// fundamental.hip -- findFundamentalMat(FM_RANSAC) for ONE set of point pairs on
// the host, behind sift_find_fundamental: host code like homography.hip and
// affine.hip, for the same reason.  A batch whose point pairs are already on the
// device is fundamental_batch.hip's; both take every expression from
// fundamental_math.hpp (the rule is written out there), and this file keeps
// only the serial control flow.
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.hpp"
#include "fundamental_math.hpp"

namespace sift {

using namespace fmath;

int find_fundamental_ransac(const float* src_xy, const float* dst_xy, int n, double thr, int max_iters,
                            double confidence, double* F, unsigned char* mask_out) {
  constexpr int m = kModelPoints;
  const P2* s = reinterpret_cast<const P2*>(src_xy);
  const P2* d = reinterpret_cast<const P2*>(dst_xy);
  if (n < m || !(confidence > 0 && confidence < 1) || max_iters < 1) return 0;
  std::vector<unsigned char> best_mask(n, 0), mask(n);
  double best[9] = {0}, model[9];
  if (n == m) {
    if (!solve<>(s, d, n, best)) return 0;
    std::fill(best_mask.begin(), best_mask.end(), 1);
  } else {
    const float t = hmath::inlier_limit(thr);
    Rng rng{~0ull};
    int niters = max_iters, max_good = 0;
    for (int iter = 0; iter < niters; ++iter) {
      int idx[m];
      P2 ms[m], md[m];
      if (!get_subset8(rng, s, d, n, idx, ms, md)) break;
      if (!solve<m>(ms, md, m, model)) continue;
      float f[9];
      to_float9(model, f);
      int good = 0;
      for (int i = 0; i < n; ++i) {
        mask[i] = is_inlier(f, s[i].x, s[i].y, d[i].x, d[i].y, t);
        good += mask[i];
      }
      if (wins(good, max_good)) {
        best_mask.swap(mask);
        memcpy(best, model, sizeof(best));
        max_good = good;
        niters = hmath::update_num_iters(confidence, (double)(n - good) / n, m, niters);
      }
    }
    if (max_good <= 0) return 0;
    // the same solve over the inliers, in pair order; the mask stays the hypothesis's
    std::vector<P2> si, di;
    si.reserve(max_good);
    di.reserve(max_good);
    for (int i = 0; i < n; ++i)
      if (best_mask[i]) si.push_back(s[i]), di.push_back(d[i]);
    solve<>(si.data(), di.data(), max_good, best);  // a failed refit leaves best untouched
  }
  memcpy(F, best, sizeof(best));
  if (mask_out) memcpy(mask_out, best_mask.data(), n);
  return 1;
}

}  // namespace sift
