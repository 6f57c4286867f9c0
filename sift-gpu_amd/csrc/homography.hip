// homography.hip -- the reference application's last step,
// host code: findHomography(obj, scene, RANSAC) and perspectiveTransform
// (src/main.cpp:44-62) for ONE pair of images whose points are on the host.  A
// few hundred matches and at most 2000 four-point hypotheses: microseconds of
// CPU work that a GPU launch would only slow down, so the one-pair call stays
// on the host behind the same C ABI.  A batch whose point pairs are already on
// the device is homography_batch.hip's; both take every expression from
// homography_math.hpp, and this file keeps only the serial control flow.
//
// Restated from OpenCV 4.x calib3d (not in this image; parity against it is
// unpinned):
//   * RANSACPointSetRegistrator::run with modelPoints 4, threshold 3,
//     confidence 0.995, maxIters 2000, RNG((uint64)-1) (multiply-with-carry,
//     uniform(a, b) = a + next() % (b - a)), getSubset without partial checks
//     (10000 attempts), RANSACUpdateNumIters after every better model;
//   * HomographyEstimatorCallback: checkSubset (haveCollinearPoints on the last
//     point, the 4-triangle orientation test), runKernel (normalised DLT: the
//     eigenvector of the smallest eigenvalue of LtL, here by cyclic Jacobi),
//     computeError (float reprojection error against threshold^2);
//   * then a DLT refit on the inliers and 10 Levenberg-Marquardt iterations on
//     the 8 free entries (a plain LM here, not OpenCV's LMSolver);
//   * perspectiveTransform: w = h20 x + h21 y + h22, (0, 0) when |w| <= FLT_EPSILON.
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "common.hpp"
#include "homography_math.hpp"

namespace sift {

namespace {

using namespace hmath;

int find_inliers(const P2* s, const P2* d, int n, const double* H, double thr, unsigned char* mask) {
  const float t = inlier_limit(thr);
  int count = 0;
  for (int i = 0; i < n; ++i) {
    mask[i] = is_inlier(H, s[i], d[i], t);
    count += mask[i];
  }
  return count;
}

void refine_lm(const P2* s, const P2* d, int n, double* H) {
  double lambda = kLmLambda0;
  auto cost = [&](const double* h) {
    double c = 0;
    for (int i = 0; i < n; ++i) c += lm_cost_term(h, s[i], d[i]);
    return c;
  };
  double c0 = cost(H);
  for (int it = 0; it < kLmSteps; ++it) {
    double JtJ[8][8] = {}, Jtr[8] = {};
    for (int i = 0; i < n; ++i) {
      double Jx[8], Jy[8], rx, ry;
      lm_rows(H, s[i], d[i], Jx, Jy, rx, ry);
      for (int a = 0; a < 8; ++a) {
        Jtr[a] += lm_jtr(Jx, Jy, a, rx, ry);
        for (int b = 0; b < 8; ++b) JtJ[a][b] += lm_jtj(Jx, Jy, a, b);
      }
    }
    double A[8 * 9], dx[8], Hn[9];
    if (!lm_solve(&JtJ[0][0], Jtr, lambda, A, dx)) break;
    lm_candidate(H, dx, Hn);
    const double c1 = cost(Hn);
    const bool accepted = lm_accept(c1, c0);
    if (accepted) {
      memcpy(H, Hn, sizeof(Hn));
      c0 = c1;
    }
    lambda = lm_lambda_next(lambda, accepted);
  }
}

}  // namespace

int find_homography_ransac(const float* src_xy, const float* dst_xy, int n, double thr, int max_iters,
                           double confidence, double* H, unsigned char* mask_out) {
  if (n < 4 || !(confidence > 0 && confidence < 1) || max_iters < 1) return 0;
  const P2* s = reinterpret_cast<const P2*>(src_xy);
  const P2* d = reinterpret_cast<const P2*>(dst_xy);
  std::vector<unsigned char> best_mask(n, 0), mask(n);
  double best[9] = {0}, model[9];
  bool result = false;
  if (n == 4) {
    if (!run_kernel<4>(s, d, 4, best)) return 0;
    std::fill(best_mask.begin(), best_mask.end(), 1);
    result = true;
  } else {
    Rng rng{~0ull};
    int niters = max_iters, max_good = 0;
    for (int iter = 0; iter < niters; ++iter) {
      int idx[4];
      P2 ms[4], md[4];
      if (!get_subset(rng, s, d, n, idx, ms, md)) {
        if (iter == 0) return 0;
        break;
      }
      if (!run_kernel<4>(ms, md, 4, model)) continue;
      const int good = find_inliers(s, d, n, model, thr, mask.data());
      if (wins(good, max_good)) {
        best_mask.swap(mask);
        memcpy(best, model, sizeof(best));
        max_good = good;
        niters = update_num_iters(confidence, (double)(n - good) / n, 4, niters);
      }
    }
    result = max_good > 0;
  }
  if (!result) return 0;
  if (n > 4) {  // refit on the inliers, then LM (findHomography, fundam.cpp)
    std::vector<P2> si, di;
    for (int i = 0; i < n; ++i)
      if (best_mask[i]) {
        si.push_back(s[i]);
        di.push_back(d[i]);
      }
    if (!si.empty()) {
      double refit[9];
      if (run_kernel(si.data(), di.data(), (int)si.size(), refit)) memcpy(best, refit, sizeof(best));
      refine_lm(si.data(), di.data(), (int)si.size(), best);
    }
  }
  normalise_h(best, H);
  if (mask_out) memcpy(mask_out, best_mask.data(), n);
  return 1;
}

void perspective_transform(const double* H, const float* xy, int n, float* out) {
  for (int i = 0; i < n; ++i) perspective_point(H, xy[2 * i], xy[2 * i + 1], out + 2 * i);
}

}  // namespace sift
