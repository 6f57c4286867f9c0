// fundamental_math.hpp -- the arithmetic of findFundamentalMat(FM_RANSAC),
// stated once for the host path (fundamental.hip, one pair set) and the kernel
// (fundamental_batch.hip, every segment of a batch), in the manner of
// affine_math.hpp.  It reuses homography_math.hpp's Rng, P2, mat3mul,
// inlier_limit, update_num_iters, kSubsetAttempts, its collinearity expression
// and its Jacobi (smallest_eigvec, at N = 9 and N = 3).  Every function is
// __host__ __device__ and inline; the library is built -ffp-contract=off and
// double + - * / and sqrt are IEEE on gfx950 as on x86-64, so the same
// statement gives the same bits on either side.  The one libm-dependent site is
// again update_num_iters.
//
// Convention (OpenCV's): [dst; 1]^T F [src; 1] = 0, F row-major, 9 doubles.
//
// The loop is RANSACPointSetRegistrator::run with m = 8: n < 8 none; n == 8 a
// direct fit without a subset check and a mask of ones (none if the solve
// fails); else Rng{~0}, subsets of 8 distinct rows until check_subset accepts
// one (the last drawn point collinear with no two earlier ones, in src and in
// dst; kSubsetAttempts draws), a hypothesis wins iff good > max(max_good, 7),
// and after a win niters = update_num_iters(confidence, (n - good) / n, 8,
// niters).
//
// The solve (solve<>, for a hypothesis and for the refit) is the normalised
// 8-point algorithm, every sum a double chain in pair order:
//   * per image the centroid (the float coordinates summed, divided by the
//     count) and the scale sqrt(2) / (mean of sqrt(dx^2 + dy^2)); a mean below
//     DBL_EPSILON or a non-finite one fails the solve;
//   * the nine-term row [X x, X y, X, Y x, Y y, Y, x, y, 1] over normalised
//     coordinates (x, y src; X, Y dst) and the 45 sums of A^T A's upper
//     triangle, mirrored afterwards;
//   * f, the eigenvector of A^T A's smallest eigenvalue (Jacobi, N = 9);
//   * rank 2: F0 <- F0 - (F0 v) v^T with v the eigenvector of the smallest
//     eigenvalue of F0^T F0 (the same Jacobi, N = 3).  (F0 v) v^T is the
//     sigma_3 u_3 v_3^T term of F0's SVD, so this is the SVD truncation without
//     an SVD routine or a libm call;
//   * F = T_dst^T F0 T_src, divided by F[8] when |F[8]| > FLT_EPSILON; a
//     non-finite entry fails the solve.
//
// The final model is the same solve over the best hypothesis's inliers; a
// failed refit leaves the RANSAC model standing, and the mask is the best
// hypothesis's, taken before the refit.  No LM / Sampson refinement, and no
// 7-point solver (its cubic needs cbrt / acos, which would break host / device
// bit equality).  The library's own rule, not bit-compatible with OpenCV.
#pragma once

#include "homography_math.hpp"

namespace sift {
namespace fmath {

using hmath::P2;
using hmath::Rng;

constexpr int kModelPoints = 8;
constexpr int kCoords = 4;     // centroid sums: src x, src y, dst x, dst y
constexpr int kDists = 2;      // distance sums: src, dst
constexpr int kProducts = 45;  // A^T A's upper triangle, row by row
constexpr double kSqrt2 = 1.4142135623730951;  // sqrt(2.), correctly rounded

SIFT_HD bool finite9(const double* F) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 9; ++k) ok &= fabs(F[k]) <= DBL_MAX;  // false for NaN and inf
  return ok;
}

// haveCollinearPoints on the last of kCount: homography_math.hpp's expression.
template <int kCount>
SIFT_HD bool collinear_last(const P2* p) {
  constexpr int i = kCount - 1;
#pragma unroll
  for (int j = 0; j < i; ++j) {
    const double dx1 = p[j].x - p[i].x, dy1 = p[j].y - p[i].y;
#pragma unroll
    for (int k = 0; k < j; ++k) {
      const double dx2 = p[k].x - p[i].x, dy2 = p[k].y - p[i].y;
      if (fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2)))
        return true;
    }
  }
  return false;
}

SIFT_HD bool check_subset8(const P2* s, const P2* d) {
  return !collinear_last<kModelPoints>(s) && !collinear_last<kModelPoints>(d);
}

// getSubset for 8 rows: hmath::get_subset with this model's count and check (the names carry
// an 8 because P2 is hmath's: an unqualified call would find both).
SIFT_HD bool get_subset8(Rng& rng, const P2* s, const P2* d, int n, int* idx, P2* ms, P2* md) {
  for (int attempts = 0; attempts < hmath::kSubsetAttempts; ++attempts) {
#pragma unroll
    for (int i = 0; i < kModelPoints; ++i) {
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
    if (check_subset8(ms, md)) return true;
  }
  return false;
}

// ---- run8Point, in its steps --------------------------------------------------
// c[] are the centroids {src x, src y, dst x, dst y}, k[] the scales {src, dst}.
struct Norm {
  double c[kCoords], k[kDists];
};

SIFT_HD double coord(P2 s, P2 d, int a) { return a == 0 ? s.x : a == 1 ? s.y : a == 2 ? d.x : d.y; }

// One pair's distances to the two centroids.
SIFT_HD void dist_terms(const double* c, P2 s, P2 d, double* out) {
  const double u = s.x - c[0], v = s.y - c[1], U = d.x - c[2], V = d.y - c[3];
  out[0] = sqrt(u * u + v * v);
  out[1] = sqrt(U * U + V * V);
}

// false: a degenerate or non-finite point set; else k becomes sqrt(2) / mean distance
SIFT_HD bool scale_finish(const double* dist_sum, int count, double* k) {
  const double m0 = dist_sum[0] / count, m1 = dist_sum[1] / count;
  if (!(m0 >= DBL_EPSILON && m0 <= DBL_MAX && m1 >= DBL_EPSILON && m1 <= DBL_MAX)) return false;
  k[0] = kSqrt2 / m0;
  k[1] = kSqrt2 / m1;
  return true;
}

SIFT_HD void row(const Norm& n, P2 s, P2 d, double* r) {
  const double x = (s.x - n.c[0]) * n.k[0], y = (s.y - n.c[1]) * n.k[0];
  const double X = (d.x - n.c[2]) * n.k[1], Y = (d.y - n.c[3]) * n.k[1];
  r[0] = X * x, r[1] = X * y, r[2] = X, r[3] = Y * x, r[4] = Y * y, r[5] = Y, r[6] = x, r[7] = y, r[8] = 1;
}

// One pair's terms of A^T A's upper triangle, row by row: out[kProducts].
SIFT_HD void product_terms(const Norm& n, P2 s, P2 d, double* out) {
  double r[9];
  row(n, s, d, r);
  int t = 0;
#pragma unroll
  for (int j = 0; j < 9; ++j)
#pragma unroll
    for (int k = j; k < 9; ++k) out[t++] = r[j] * r[k];
}

// A^T A's upper triangle is summed: mirror it, take f, enforce rank 2, undo the
// normalisation, scale.  false (F untouched): a non-finite entry.
SIFT_HD bool finish(const Norm& n, double AtA[9][9], double* F) {
#pragma unroll
  for (int j = 0; j < 9; ++j)
#pragma unroll
    for (int k = 0; k < j; ++k) AtA[j][k] = AtA[k][j];
  double f[9];
  hmath::smallest_eigvec(AtA, f);
  double G[3][3], v[3], w[3], F0[9];  // G = F0^T F0
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) G[i][j] = f[i] * f[j] + f[3 + i] * f[3 + j] + f[6 + i] * f[6 + j];
  hmath::smallest_eigvec(G, v);
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] = f[i * 3] * v[0] + f[i * 3 + 1] * v[1] + f[i * 3 + 2] * v[2];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) F0[i * 3 + j] = f[i * 3 + j] - w[i] * v[j];
  const double TdT[9] = {n.k[1], 0, 0, 0, n.k[1], 0, -n.c[2] * n.k[1], -n.c[3] * n.k[1], 1};
  const double Ts[9] = {n.k[0], 0, -n.c[0] * n.k[0], 0, n.k[0], -n.c[1] * n.k[0], 0, 0, 1};
  double T[9], R[9];
  hmath::mat3mul(TdT, F0, T);
  hmath::mat3mul(T, Ts, R);
  if (fabs(R[8]) > FLT_EPSILON) {
    const double r8 = R[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = R[i] / r8;
  }
  if (!finite9(R)) return false;
#pragma unroll
  for (int i = 0; i < 9; ++i) F[i] = R[i];
  return true;
}

// The steps above in pair order.  kCount > 0 fixes the count at compile time
// (the 8-point hypotheses of the kernel).
template <int kCount = 0>
SIFT_HD bool solve(const P2* s, const P2* d, int count_arg, double* F) {
  const int count = kCount ? kCount : count_arg;
  Norm n = {};
#pragma unroll 8
  for (int i = 0; i < count; ++i)
#pragma unroll
    for (int a = 0; a < kCoords; ++a) n.c[a] += coord(s[i], d[i], a);
#pragma unroll
  for (int a = 0; a < kCoords; ++a) n.c[a] /= count;
  double dist[kDists] = {0, 0};
#pragma unroll 8
  for (int i = 0; i < count; ++i) {
    double t[kDists];
    dist_terms(n.c, s[i], d[i], t);
    dist[0] += t[0];
    dist[1] += t[1];
  }
  if (!scale_finish(dist, count, n.k)) return false;
  double AtA[9][9];
#pragma unroll
  for (int j = 0; j < 9; ++j)
#pragma unroll
    for (int k = 0; k < 9; ++k) AtA[j][k] = 0;
#pragma unroll 8
  for (int i = 0; i < count; ++i) {
    double r[9];
    row(n, s[i], d[i], r);
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
      for (int k = j; k < 9; ++k) AtA[j][k] += r[j] * r[k];
  }
  return finish(n, AtA, F);
}

// FMEstimatorCallback::computeError + the inlier test: the coefficients as
// floats, unfused float arithmetic left to right.  The error is
// max(d_dst^2 s_dst, d_src^2 s_src), the squared distances of each point to the
// other's epipolar line with s = 1 / (a^2 + b^2); max(..) <= t is taken as
// both terms <= t, so a NaN in either is never an inlier.
SIFT_HD void to_float9(const double* F, float* f) {
#pragma unroll
  for (int k = 0; k < 9; ++k) f[k] = (float)F[k];
}
SIFT_HD bool is_inlier(const float* f, float x, float y, float X, float Y, float t) {
  float a = f[0] * x + f[1] * y + f[2], b = f[3] * x + f[4] * y + f[5], c = f[6] * x + f[7] * y + f[8];
  const float s_dst = 1.f / (a * a + b * b);
  const float d_dst = X * a + Y * b + c;
  a = f[0] * X + f[3] * Y + f[6], b = f[1] * X + f[4] * Y + f[7], c = f[2] * X + f[5] * Y + f[8];
  const float s_src = 1.f / (a * a + b * b);
  const float d_src = x * a + y * b + c;
  return d_dst * d_dst * s_dst <= t && d_src * d_src * s_src <= t;
}

SIFT_HD bool wins(int good, int max_good) {
  return good > (max_good < kModelPoints - 1 ? kModelPoints - 1 : max_good);
}

}  // namespace fmath
}  // namespace sift
