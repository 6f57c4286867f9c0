// affine_math.hpp -- the arithmetic of estimateAffine2D / estimateAffinePartial2D
// (RANSAC), stated once for the host path (affine.hip, one pair set) and the
// kernel (affine_batch.hip, every segment of a batch), in the manner of
// homography_math.hpp, whose Rng, P2, det3, inlier_limit, update_num_iters and
// collinearity expression it reuses.  Every function is __host__ __device__ and
// inline; the library is built -ffp-contract=off and double + - * / are IEEE on
// gfx950 as on x86-64, so the same statement gives the same bits on either
// side.  The one libm-dependent site is again update_num_iters.
//
// Two models of m model points, both kept as the six doubles of a row-major
// 2x3 (x' = A0 x + A1 y + A2, y' = A3 x + A4 y + A5):
//   SIFT_MODEL_AFFINE      m = 3   (a b tx; c d ty)
//   SIFT_MODEL_SIMILARITY  m = 2   (a -b tx; b a ty)
// The loop is RANSACPointSetRegistrator::run with m in place of 4: n < m none;
// n == m a direct fit without a subset check; else Rng{~0}, subsets of m
// distinct rows until check_subset accepts one (kSubsetAttempts), a hypothesis
// wins iff good > max(max_good, m - 1), and after a win niters =
// update_num_iters(confidence, (n - good) / n, m, niters).
//
// The final model is the ordinary least-squares fit of the model to the best
// hypothesis's inliers: double sums in pair order over coordinates centred on
// the inliers' centroids, solved in closed form.  The residual is linear in
// the parameters, so this is the minimum that OpenCV's 10 LMSolver iterations
// (refineIters) look for: there is no refineIters argument and no LM here.  A
// singular or non-finite refit leaves the RANSAC model standing.  The result is
// the library's own rule, not bit-compatible with OpenCV.
#pragma once

#include "homography_math.hpp"

namespace sift {
namespace amath {

using hmath::P2;
using hmath::Rng;

constexpr int kAffine = 0, kSimilarity = 1;  // SIFT_MODEL_AFFINE, SIFT_MODEL_SIMILARITY
constexpr int model_points(int model) { return model == kAffine ? 3 : 2; }

SIFT_HD bool finite6(const double* A) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 6; ++k) ok &= fabs(A[k]) <= DBL_MAX;  // false for NaN and inf
  return ok;
}

// haveCollinearPoints on the last of 3: homography_math.hpp's expression.
SIFT_HD bool collinear3(const P2* p) {
  const double dx1 = p[1].x - p[2].x, dy1 = p[1].y - p[2].y;
  const double dx2 = p[0].x - p[2].x, dy2 = p[0].y - p[2].y;
  return fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2));
}

template <int kModel>
SIFT_HD bool check_subset(const P2* s, const P2* d) {
  if (kModel == kAffine) return !collinear3(s) && !collinear3(d);
  return !(s[0].x == s[1].x && s[0].y == s[1].y);
}

// getSubset for m rows: hmath::get_subset with the model's count and check.
template <int kModel>
SIFT_HD bool get_subset(Rng& rng, const P2* s, const P2* d, int n, int* idx, P2* ms, P2* md) {
  constexpr int m = model_points(kModel);
  for (int attempts = 0; attempts < hmath::kSubsetAttempts; ++attempts) {
#pragma unroll
    for (int i = 0; i < m; ++i) {
      for (;;) {
        idx[i] = rng.uniform(0, n);
        bool seen = false;
#pragma unroll
        for (int j = 0; j < i; ++j) seen |= idx[i] == idx[j];
        if (!seen) break;
      }
      ms[i] = s[idx[i]];
      md[i] = d[idx[i]];
    }
    if (check_subset<kModel>(ms, md)) return true;
  }
  return false;
}

// | a0 a1 a2 ; b0 b1 b2 ; c0 c1 c2 |, expanded along the first row
SIFT_HD double det3c(double a0, double a1, double a2, double b0, double b1, double b2, double c0, double c1,
                     double c2) {
  return a0 * (b1 * c2 - c1 * b2) - a1 * (b0 * c2 - c0 * b2) + a2 * (b0 * c1 - b1 * c0);
}

// The minimal solve on the first m points, in double from the float
// coordinates.  false: a zero determinant / denominator or a non-finite
// coefficient.
template <int kModel>
SIFT_HD bool solve_minimal(const P2* s, const P2* d, double* A) {
  if (kModel == kAffine) {  // Cramer on [x y 1] (a b tx)^T = X, [x y 1] (c d ty)^T = Y
    const double x0 = s[0].x, y0 = s[0].y, x1 = s[1].x, y1 = s[1].y, x2 = s[2].x, y2 = s[2].y;
    const double X0 = d[0].x, Y0 = d[0].y, X1 = d[1].x, Y1 = d[1].y, X2 = d[2].x, Y2 = d[2].y;
    const double det = hmath::det3(x0, y0, x1, y1, x2, y2);
    if (det == 0) return false;
    A[0] = hmath::det3(X0, y0, X1, y1, X2, y2) / det;
    A[1] = hmath::det3(x0, X0, x1, X1, x2, X2) / det;
    A[2] = det3c(x0, y0, X0, x1, y1, X1, x2, y2, X2) / det;
    A[3] = hmath::det3(Y0, y0, Y1, y1, Y2, y2) / det;
    A[4] = hmath::det3(x0, Y0, x1, Y1, x2, Y2) / det;
    A[5] = det3c(x0, y0, Y0, x1, y1, Y1, x2, y2, Y2) / det;
  } else {  // the complex quotient (P1 - P0) / (p1 - p0) = a + i b
    const double x0 = s[0].x, y0 = s[0].y, X0 = d[0].x, Y0 = d[0].y;
    const double dx = s[1].x - x0, dy = s[1].y - y0, dX = d[1].x - X0, dY = d[1].y - Y0;
    const double den = dx * dx + dy * dy;
    if (den == 0) return false;
    const double a = (dX * dx + dY * dy) / den, b = (dY * dx - dX * dy) / den;
    A[0] = a, A[1] = -b, A[2] = X0 - (a * x0 - b * y0);
    A[3] = b, A[4] = a, A[5] = Y0 - (b * x0 + a * y0);
  }
  return finite6(A);
}

// Affine2DEstimatorCallback::computeError + the inlier test: the coefficients
// as floats, unfused float arithmetic left to right, error <= (float)(thr^2).
// A NaN error is never an inlier.
SIFT_HD void to_float6(const double* A, float* f) {
#pragma unroll
  for (int k = 0; k < 6; ++k) f[k] = (float)A[k];
}
SIFT_HD bool is_inlier(const float* f, float x, float y, float X, float Y, float t) {
  const float a = f[0] * x + f[1] * y + f[2] - X;
  const float b = f[3] * x + f[4] * y + f[5] - Y;
  return a * a + b * b <= t;
}

SIFT_HD bool wins(int good, int max_good, int m) { return good > (max_good < m - 1 ? m - 1 : max_good); }

// ---- the least-squares refit on the inliers ----------------------------------
// c[] are the centroids {src x, src y, dst x, dst y}: sums of the float
// coordinates in pair order, divided by the inlier count.
SIFT_HD double refit_coord(P2 s, P2 d, int a) { return a == 0 ? s.x : a == 1 ? s.y : a == 2 ? d.x : d.y; }
constexpr int kRefitCoords = 4;
constexpr int kRefitSumsMax = 7;
constexpr int refit_sums(int model) { return model == kAffine ? 7 : 3; }

// One pair's terms of the model's sums over centred coordinates:
//   affine      uu uv vv uU vU uV vV
//   similarity  uu + vv,  uU + vV,  uV - vU
template <int kModel>
SIFT_HD void refit_terms(const double* c, P2 s, P2 d, double* out) {
  const double u = s.x - c[0], v = s.y - c[1], U = d.x - c[2], V = d.y - c[3];
  if (kModel == kAffine) {
    out[0] = u * u, out[1] = u * v, out[2] = v * v, out[3] = u * U, out[4] = v * U, out[5] = u * V, out[6] = v * V;
  } else {
    out[0] = u * u + v * v, out[1] = u * U + v * V, out[2] = u * V - v * U;
  }
}

// The closed-form solve; false (A untouched): singular or non-finite.
template <int kModel>
SIFT_HD bool refit_finish(const double* c, const double* S, double* A) {
  double R[6];
  if (kModel == kAffine) {
    const double det = S[0] * S[2] - S[1] * S[1];
    if (det == 0) return false;
    R[0] = (S[3] * S[2] - S[4] * S[1]) / det;
    R[1] = (S[0] * S[4] - S[1] * S[3]) / det;
    R[3] = (S[5] * S[2] - S[6] * S[1]) / det;
    R[4] = (S[0] * S[6] - S[1] * S[5]) / det;
  } else {
    if (S[0] == 0) return false;
    const double a = S[1] / S[0], b = S[2] / S[0];
    R[0] = a, R[1] = -b, R[3] = b, R[4] = a;
  }
  R[2] = c[2] - (R[0] * c[0] + R[1] * c[1]);
  R[5] = c[3] - (R[3] * c[0] + R[4] * c[1]);
  if (!finite6(R)) return false;
#pragma unroll
  for (int k = 0; k < 6; ++k) A[k] = R[k];
  return true;
}

}  // namespace amath
}  // namespace sift
