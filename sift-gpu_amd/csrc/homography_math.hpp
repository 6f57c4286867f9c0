// homography_math.hpp -- the arithmetic of findHomography(RANSAC), stated once
// for the host path (homography.hip, one pair) and the kernels
// (homography_batch.hip, every segment of a batch).  Every function is
// __host__ __device__ and inline; the library is built -ffp-contract=off and
// double + - * / and sqrt are IEEE on gfx950 as on x86-64, so the same
// statement gives the same bits on either side.  Where the host walks points
// serially and the kernels walk them one accumulator per lane, both add the
// same per-point term (dlt_product, lm_jtj, lm_jtr, lm_cost_term) to the same
// accumulator in the same point order.
//
// The one libm-dependent site is update_num_iters (pow, log): the device's
// and the host's libm may differ by an ulp there.  Its results reach the
// output only through lrint(num / denom) and the two comparisons
// (denom < DBL_MIN, -num >= max_iters * -denom); the exact cases (ep == 0:
// pow(1, 4) = 1, denom 0, result 0; ep == 1: pow(0, 4) = 0, log(1) = 0, result
// max_iters) are exact in any libm.  An ulp elsewhere moves a result only when
// num / denom lies within an ulp of a half-integer.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SIFT_HD __host__ __device__ inline
#else
#define SIFT_HD inline
#endif

namespace sift {
namespace hmath {

constexpr int kSubsetAttempts = 10000;  // getSubset's limit per hypothesis

struct Rng {  // cv::RNG
  uint64_t state;
  SIFT_HD unsigned next() {
    state = (uint64_t)(unsigned)state * 4164903690u + (unsigned)(state >> 32);
    return (unsigned)state;
  }
  SIFT_HD int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a)) + a; }
};

struct P2 {
  float x, y;
};

SIFT_HD bool collinear_last(const P2* p) {  // haveCollinearPoints on the last of 4
  const int i = 3;
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

SIFT_HD double det3(double a0, double a1, double b0, double b1, double c0, double c1) {
  // | a0 a1 1 ; b0 b1 1 ; c0 c1 1 |
  return a0 * (b1 - c1) - a1 * (b0 - c0) + (b0 * c1 - b1 * c0);
}

SIFT_HD bool orientation_flips(const P2* s, const P2* d, int t0, int t1, int t2) {
  const double A = det3(s[t0].x, s[t0].y, s[t1].x, s[t1].y, s[t2].x, s[t2].y);
  const double B = det3(d[t0].x, d[t0].y, d[t1].x, d[t1].y, d[t2].x, d[t2].y);
  return A * B < 0;
}

SIFT_HD bool check_subset(const P2* s, const P2* d) {
  if (collinear_last(s) || collinear_last(d)) return false;
  const int negative = (int)orientation_flips(s, d, 0, 1, 2) + (int)orientation_flips(s, d, 1, 2, 3) +
                       (int)orientation_flips(s, d, 0, 2, 3) + (int)orientation_flips(s, d, 0, 1, 3);
  return negative == 0 || negative == 4;
}

// getSubset without partial checks: 4 distinct rows drawn until check_subset
// accepts them, at most kSubsetAttempts times.  false: no subset was accepted.
SIFT_HD bool get_subset(Rng& rng, const P2* s, const P2* d, int n, int* idx, P2* ms, P2* md) {
  for (int attempts = 0; attempts < kSubsetAttempts; ++attempts) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
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
    if (check_subset(ms, md)) return true;
  }
  return false;
}

// Symmetric N x N eigen decomposition (cyclic Jacobi); returns the eigenvector
// of the smallest eigenvalue.  Every index is a compile-time constant once the
// loops are unrolled, so on the device A and V live in registers.  N is deduced
// from A: 9 for the DLT and the 8-point solve, 3 for the latter's rank-2 step
// (fundamental_math.hpp); the statements are the same for every N.
template <int N>
SIFT_HD void smallest_eigvec(double A[N][N], double* v) {
  double V[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) V[i][j] = i == j;
#pragma unroll 1
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = i + 1; j < N; ++j) off += A[i][j] * A[i][j];
    if (off < 1e-300) break;
#pragma unroll
    for (int p = 0; p < N; ++p)
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        if (fabs(A[p][q]) < 1e-300) continue;
        const double th = (A[q][q] - A[p][p]) / (2 * A[p][q]);
        const double t = (th >= 0 ? 1 : -1) / (fabs(th) + sqrt(th * th + 1));
        const double c = 1 / sqrt(t * t + 1), s = t * c;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  // the first smallest diagonal entry's column, picked without a run-time index
  double least = A[0][0];
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = V[k][0];
#pragma unroll
  for (int i = 1; i < N; ++i)
    if (A[i][i] < least) {
      least = A[i][i];
#pragma unroll
      for (int k = 0; k < N; ++k) v[k] = V[k][i];
    }
}

// smallest_eigvec's sibling for a caller that needs every eigenpair
// (pose_math.hpp): the same sweeps, statement for statement, then all of V
// (eigenvectors in columns) and A's diagonal in d, unordered.  A function of
// its own, so that smallest_eigvec keeps the statements its tests pin.
template <int N>
SIFT_HD void sym_eig(double A[N][N], double V[N][N], double* d) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) V[i][j] = i == j;
#pragma unroll 1
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int j = i + 1; j < N; ++j) off += A[i][j] * A[i][j];
    if (off < 1e-300) break;
#pragma unroll
    for (int p = 0; p < N; ++p)
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        if (fabs(A[p][q]) < 1e-300) continue;
        const double th = (A[q][q] - A[p][p]) / (2 * A[p][q]);
        const double t = (th >= 0 ? 1 : -1) / (fabs(th) + sqrt(th * th + 1));
        const double c = 1 / sqrt(t * t + 1), s = t * c;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) d[i] = A[i][i];
}

SIFT_HD void mat3mul(const double* a, const double* b, double* c) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
}

// ---- HomographyEstimatorCallback::runKernel, in its steps --------------------
// c[] / s[] are {m.x, m.y, M.x, M.y}: m the dst points, M the src points.
struct Norm {
  double c[4], s[4];
};

SIFT_HD float norm_coord(P2 M, P2 m, int a) { return a == 0 ? m.x : a == 1 ? m.y : a == 2 ? M.x : M.y; }
SIFT_HD void centroid_add(double& c, float v) { c += v; }
SIFT_HD void centroid_finish(double& c, int count) { c /= count; }
SIFT_HD void spread_add(double& s, float v, double c) { s += fabs(v - c); }
// false: a degenerate point set; else s becomes the scale count / s
SIFT_HD bool spread_finish(Norm& n, int count) {
  if (fabs(n.s[0]) < DBL_EPSILON || fabs(n.s[1]) < DBL_EPSILON || fabs(n.s[2]) < DBL_EPSILON ||
      fabs(n.s[3]) < DBL_EPSILON)
    return false;
#pragma unroll
  for (int a = 0; a < 4; ++a) n.s[a] = count / n.s[a];
  return true;
}

SIFT_HD void dlt_rows(const Norm& n, P2 M, P2 m, double* Lx, double* Ly) {
  const double cmx = n.c[0], cmy = n.c[1], cMx = n.c[2], cMy = n.c[3];
  const double smx = n.s[0], smy = n.s[1], sMx = n.s[2], sMy = n.s[3];
  const double x = (m.x - cmx) * smx, y = (m.y - cmy) * smy;
  const double X = (M.x - cMx) * sMx, Y = (M.y - cMy) * sMy;
  Lx[0] = X, Lx[1] = Y, Lx[2] = 1, Lx[3] = 0, Lx[4] = 0, Lx[5] = 0, Lx[6] = -x * X, Lx[7] = -x * Y, Lx[8] = -x;
  Ly[0] = 0, Ly[1] = 0, Ly[2] = 0, Ly[3] = X, Ly[4] = Y, Ly[5] = 1, Ly[6] = -y * X, Ly[7] = -y * Y, Ly[8] = -y;
}

// One point's term of LtL[j][k], j <= k.
SIFT_HD double dlt_product(const double* Lx, const double* Ly, int j, int k) { return Lx[j] * Lx[k] + Ly[j] * Ly[k]; }
constexpr int kDltSums = 45;  // the upper triangle, row by row

// LtL's upper triangle is summed: mirror it, take the eigenvector, undo the
// normalisation, divide by H[2][2].
SIFT_HD bool dlt_finish(const Norm& n, double LtL[9][9], double* H) {
  const double cmx = n.c[0], cmy = n.c[1], cMx = n.c[2], cMy = n.c[3];
  const double smx = n.s[0], smy = n.s[1], sMx = n.s[2], sMy = n.s[3];
  const double invHnorm[9] = {1. / smx, 0, cmx, 0, 1. / smy, cmy, 0, 0, 1};
  const double Hnorm2[9] = {sMx, 0, -cMx * sMx, 0, sMy, -cMy * sMy, 0, 0, 1};
#pragma unroll
  for (int j = 0; j < 9; ++j)
#pragma unroll
    for (int k = 0; k < j; ++k) LtL[j][k] = LtL[k][j];
  double H0[9], T[9], R[9];
  smallest_eigvec(LtL, H0);
  mat3mul(invHnorm, H0, T);
  mat3mul(T, Hnorm2, R);
  if (fabs(R[8]) < DBL_MIN) return false;
#pragma unroll
  for (int i = 0; i < 9; ++i) H[i] = R[i] / R[8];
  return true;
}

// The steps above in point order: H mapping M (src) to m (dst).  kCount > 0
// fixes the count at compile time (the 4-point hypotheses of the kernels).
template <int kCount = 0>
SIFT_HD bool run_kernel(const P2* M, const P2* m, int count_arg, double* H) {
  const int count = kCount ? kCount : count_arg;
  Norm n = {};
#pragma unroll 4
  for (int i = 0; i < count; ++i)
#pragma unroll
    for (int a = 0; a < 4; ++a) centroid_add(n.c[a], norm_coord(M[i], m[i], a));
#pragma unroll
  for (int a = 0; a < 4; ++a) centroid_finish(n.c[a], count);
#pragma unroll 4
  for (int i = 0; i < count; ++i)
#pragma unroll
    for (int a = 0; a < 4; ++a) spread_add(n.s[a], norm_coord(M[i], m[i], a), n.c[a]);
  if (!spread_finish(n, count)) return false;
  double LtL[9][9];
#pragma unroll
  for (int j = 0; j < 9; ++j)
#pragma unroll
    for (int k = 0; k < 9; ++k) LtL[j][k] = 0;
#pragma unroll 4
  for (int i = 0; i < count; ++i) {
    double Lx[9], Ly[9];
    dlt_rows(n, M[i], m[i], Lx, Ly);
#pragma unroll
    for (int j = 0; j < 9; ++j)
#pragma unroll
      for (int k = j; k < 9; ++k) LtL[j][k] += dlt_product(Lx, Ly, j, k);
  }
  return dlt_finish(n, LtL, H);
}

// computeError + the inlier test: float reprojection error <= (float)(thr^2).
SIFT_HD float inlier_limit(double thr) { return (float)(thr * thr); }
SIFT_HD bool is_inlier(const double* H, P2 s, P2 d, float t) {
  const float ww = 1.f / (H[6] * s.x + H[7] * s.y + 1.f);
  const float dx = (H[0] * s.x + H[1] * s.y + H[2]) * ww - d.x;
  const float dy = (H[3] * s.x + H[4] * s.y + H[5]) * ww - d.y;
  const float e = dx * dx + dy * dy;
  return e <= t;
}

// A hypothesis with `good` inliers replaces the best so far:
SIFT_HD bool wins(int good, int max_good) { return good > (max_good < 3 ? 3 : max_good); }

// RANSACUpdateNumIters; the libm-dependent site (see the top of the file).
SIFT_HD int update_num_iters(double p, double ep, int model_points, int max_iters) {
  p = p < 0. ? 0. : p;  // std::min(std::max(p, 0.), 1.)
  p = 1. < p ? 1. : p;
  ep = ep < 0. ? 0. : ep;
  ep = 1. < ep ? 1. : ep;
  double num = 1. - p < DBL_MIN ? DBL_MIN : 1. - p;
  double denom = 1. - pow(1. - ep, (double)model_points);
  if (denom < DBL_MIN) return 0;
  num = log(num);
  denom = log(denom);
  return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)lrint(num / denom);
}

// ---- 10 Levenberg-Marquardt iterations on h[0..7] (h[8] = 1) -----------------
// residuals (H s)_xy / (H s)_z - d over the inliers
SIFT_HD double lm_cost_term(const double* h, P2 s, P2 d) {
  const double w = h[6] * s.x + h[7] * s.y + 1;
  const double ex = (h[0] * s.x + h[1] * s.y + h[2]) / w - d.x;
  const double ey = (h[3] * s.x + h[4] * s.y + h[5]) / w - d.y;
  return ex * ex + ey * ey;
}

SIFT_HD void lm_rows(const double* H, P2 s, P2 d, double* Jx, double* Jy, double& rx, double& ry) {
  const double X = s.x, Y = s.y;
  const double w = H[6] * X + H[7] * Y + 1, iw = 1 / w;
  const double u = (H[0] * X + H[1] * Y + H[2]) * iw, v = (H[3] * X + H[4] * Y + H[5]) * iw;
  Jx[0] = X * iw, Jx[1] = Y * iw, Jx[2] = iw, Jx[3] = 0, Jx[4] = 0, Jx[5] = 0, Jx[6] = -X * u * iw, Jx[7] = -Y * u * iw;
  Jy[0] = 0, Jy[1] = 0, Jy[2] = 0, Jy[3] = X * iw, Jy[4] = Y * iw, Jy[5] = iw, Jy[6] = -X * v * iw, Jy[7] = -Y * v * iw;
  rx = u - d.x;
  ry = v - d.y;
}
SIFT_HD double lm_jtr(const double* Jx, const double* Jy, int a, double rx, double ry) { return Jx[a] * rx + Jy[a] * ry; }
SIFT_HD double lm_jtj(const double* Jx, const double* Jy, int a, int b) { return Jx[a] * Jx[b] + Jy[a] * Jy[b]; }
constexpr int kLmSums = 72;  // JtJ row by row, then Jtr
constexpr int kLmSteps = 10;
constexpr double kLmLambda0 = 1e-3;

// (JtJ + lambda diag(JtJ)) dx = -Jtr by Gaussian elimination with partial
// pivoting; A is 8 x 9 of work space.  false: a pivot below 1e-300.
SIFT_HD bool lm_solve(const double* JtJ /* [8][8] */, const double* Jtr, double lambda, double* A /* [8][9] */,
                      double* dx) {
  for (int a = 0; a < 8; ++a) {
    for (int b = 0; b < 8; ++b) A[a * 9 + b] = JtJ[a * 8 + b] + (a == b ? lambda * JtJ[a * 8 + a] : 0);
    A[a * 9 + 8] = -Jtr[a];
  }
  for (int c = 0; c < 8; ++c) {
    int piv = c;
    for (int r = c + 1; r < 8; ++r)
      if (fabs(A[r * 9 + c]) > fabs(A[piv * 9 + c])) piv = r;
    if (fabs(A[piv * 9 + c]) < 1e-300) return false;
    if (piv != c)
      for (int k = 0; k < 9; ++k) {
        const double t = A[c * 9 + k];
        A[c * 9 + k] = A[piv * 9 + k];
        A[piv * 9 + k] = t;
      }
    for (int r = c + 1; r < 8; ++r) {
      const double f = A[r * 9 + c] / A[c * 9 + c];
      for (int k = c; k < 9; ++k) A[r * 9 + k] -= f * A[c * 9 + k];
    }
  }
  for (int c = 7; c >= 0; --c) {
    double v = A[c * 9 + 8];
    for (int k = c + 1; k < 8; ++k) v -= A[c * 9 + k] * dx[k];
    dx[c] = v / A[c * 9 + c];
  }
  return true;
}

SIFT_HD void lm_candidate(const double* H, const double* dx, double* Hn) {
  for (int k = 0; k < 8; ++k) Hn[k] = H[k] + dx[k];
  Hn[8] = 1;
}
// the step after a candidate of cost c1 against the held cost c0
SIFT_HD bool lm_accept(double c1, double c0) { return c1 < c0; }
SIFT_HD double lm_lambda_next(double lambda, bool accepted) {
  return accepted ? (lambda * 0.1 < 1e-12 ? 1e-12 : lambda * 0.1) : lambda * 10;
}

SIFT_HD void normalise_h(const double* best, double* H) {
  for (int i = 0; i < 9; ++i) H[i] = best[i] / best[8];
}

// perspectiveTransform of one point: (0, 0) when |w| <= FLT_EPSILON.
SIFT_HD void perspective_point(const double* H, float xf, float yf, float* out) {
  const double x = xf, y = yf;
  const double w = H[6] * x + H[7] * y + H[8];
  if (fabs(w) > FLT_EPSILON) {
    const double iw = 1. / w;
    out[0] = (float)((H[0] * x + H[1] * y + H[2]) * iw);
    out[1] = (float)((H[3] * x + H[4] * y + H[5]) * iw);
  } else {
    out[0] = out[1] = 0.f;
  }
}

}  // namespace hmath
}  // namespace sift
