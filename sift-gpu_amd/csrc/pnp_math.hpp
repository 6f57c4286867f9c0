// pnp_math.hpp -- the arithmetic of solvePnPRansac with a P3P minimal solver,
// stated once for the host path (pnp.hip, one row set) and the kernel
// (pnp_batch.hip, every segment of a batch), in the manner of
// fundamental_math.hpp and pose_math.hpp.  It reuses pose_math.hpp's invert3,
// normalise and finite_n and homography_math.hpp's Rng, P2, sym_eig (at N = 3),
// wins and update_num_iters.  Every function is __host__ __device__ and inline;
// the library is built -ffp-contract=off and double + - * / and sqrt are IEEE on
// gfx950 as on x86-64, so the same statement gives the same bits on either side.
// Every loop has a fixed iteration count.  The one libm-dependent site is again
// update_num_iters.
//
// Convention: X_cam = R X + t; a pose is the twelve doubles of [R | t] by rows,
// what sift_recover_pose* writes; K is row-major, 9 doubles.
//
//   1. Calibration (calibrate): K^-1 by pmath::invert3; a singular or non-finite
//      K: no model.  A pixel's normalised point (u, v) is pmath::normalise's, its
//      bearing (u, v, 1) / sqrt(u u + v v + 1).
//   2. P3P (p3p), the Lambda-Twist route (Persson & Nordberg, ECCV 2018), which
//      needs neither cbrt nor acos.  With a_ij = |x_i - x_j|^2 and b_ij = y_i . y_j
//      the depths L satisfy L^T M_ij L = a_ij.  D1 = a23 M12 - a12 M23 and
//      D2 = a23 M13 - a13 M23 are homogeneous in L.  det(D1 + g D2) = c3 g^3 +
//      c2 g^2 + c1 g + c0 with c0 = det D1, c1 = tr(adj(D1) D2), c2 = tr(adj(D2)
//      D1), c3 = det D2.  c3 == 0 (or NaN): no solution.  The cubic divided by c3
//      is bisected for 64 steps on [-B, B], B = 1 + max |coefficient| (f < 0 moves
//      the lower end), then takes 2 Newton steps (skipped where f' == 0).  The
//      eigenpairs of D0 = D1 + g D2 by hmath::sym_eig<3>; the eigenvalue of
//      smallest magnitude (the first such) is taken as the zero one; the other
//      two must be s1 > 0 > s2, else no solution; s = sqrt(-s2 / s1).  For each
//      line w = e1 + s e2, then w = e1 - s e2: l1 = p l2 + q l3 with p = -w1 / w0,
//      q = -w2 / w0; L = (p + q tau, 1, tau) in L^T D1 L = 0 is a quadratic in
//      tau, roots (+sqrt(disc) - b) / 2a then (-sqrt(disc) - b) / 2a, none when
//      disc < 0; a root is kept iff tau > 0, p + q tau > 0 and den = 1 + tau^2 -
//      2 b23 tau > 0; l2 = sqrt(a23 / den), l3 = tau l2, l1 = (p + q tau) l2; five
//      Gauss-Newton steps on the three constraints (adjugate solve, a zero
//      determinant ends them); R = Y X^-1 with X = [x1 - x2, x1 - x3, their cross
//      product] (inverse by adjugate / determinant) and Y the same of l_i y_i;
//      t = l1 y1 - R x1.  A non-finite entry drops the solution.  At most four,
//      in the order (line +, line -) x (root +, root -).
//   3. A hypothesis (hypothesis) is 4 rows: P3P on the first three, then the
//      first solution with the smallest squared error on the fourth row in
//      normalised coordinates, among those that put it at z > 0 with an error
//      below +inf; none: no model.
//   4. Inlier test (is_inlier), no division: p = K (R x + t), ex = p0 - x_pix p2,
//      ey = p1 - y_pix p2; inlier iff p2 > 0 && ex ex + ey ey <= (thr thr)(p2 p2).
//   5. The loop is RANSACPointSetRegistrator::run with m = 4 (pnp.hip).
//   6. Refit: five Gauss-Newton steps on (rotation, translation) over the best
//      hypothesis's inliers, residuals in normalised coordinates; per row the
//      28 terms of refit_terms (J^T J's upper triangle row by row, J^T r, the
//      cost), summed in row order; the 6 x 6 solve is Gaussian elimination with
//      partial pivoting; R <- R C(d) with the Cayley transform C = ((1 - a.a) I +
//      2 a a^T + 2 [a]x) / (1 + a.a), a = d / 2 (rational, orthogonal), t <- t + dt.
//      A step is kept iff the cost fell, else the loop ends.
//
// The library's own rule, not bit-compatible with OpenCV.
#pragma once

#include "pose_math.hpp"

namespace sift {
namespace pnpmath {

using hmath::P2;
using hmath::Rng;
using pmath::finite_n;

constexpr int kModelPoints = 4;
constexpr int kSolutions = 4;
constexpr int kBisectSteps = 64;
constexpr int kNewtonSteps = 2;
constexpr int kDepthSteps = 5;
constexpr int kRefitSteps = 5;
constexpr int kRefitSums = 28;  // J^T J's upper triangle (21), J^T r (6), the cost

struct Calib {
  double K[9], Ki[9];
};

// false: K is singular or non-finite
SIFT_HD bool calibrate(const double* K, Calib& c) {
#pragma unroll
  for (int k = 0; k < 9; ++k) c.K[k] = K[k];
  return pmath::invert3(K, c.Ki);
}

SIFT_HD void bearing(const double* Ki, P2 p, double* y) {
  double u, v;
  pmath::normalise(Ki, p, u, v);
  const double nrm = sqrt(u * u + v * v + 1);
  y[0] = u / nrm;
  y[1] = v / nrm;
  y[2] = 1 / nrm;
}

SIFT_HD double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

SIFT_HD void cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// the adjugate of a 3 x 3 (invert3's cofactors) and the determinant along row 0
SIFT_HD void adj3(const double* A, double* c) {
  c[0] = A[4] * A[8] - A[5] * A[7], c[1] = A[2] * A[7] - A[1] * A[8], c[2] = A[1] * A[5] - A[2] * A[4];
  c[3] = A[5] * A[6] - A[3] * A[8], c[4] = A[0] * A[8] - A[2] * A[6], c[5] = A[2] * A[3] - A[0] * A[5];
  c[6] = A[3] * A[7] - A[4] * A[6], c[7] = A[1] * A[6] - A[0] * A[7], c[8] = A[0] * A[4] - A[1] * A[3];
}
SIFT_HD double det3(const double* A, const double* c) { return A[0] * c[0] + A[1] * c[3] + A[2] * c[6]; }

SIFT_HD double trace_product(const double* a, const double* b) {
  double s = a[0] * b[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) s += a[k] * b[k];
  return s;
}

SIFT_HD double cubic(double g, double k2, double k1, double k0) { return ((g + k2) * g + k1) * g + k0; }

// Step 2.  x: three 3-D points (x[3 i + k]), y: their bearings; sink(pose) is
// called once per solution, in order.
template <class Sink>
SIFT_HD void p3p(const double* x, const double* y, Sink&& sink) {
  double d12[3], d13[3], d23[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d12[k] = x[k] - x[3 + k];
    d13[k] = x[k] - x[6 + k];
    d23[k] = x[3 + k] - x[6 + k];
  }
  const double a12 = dot3(d12, d12), a13 = dot3(d13, d13), a23 = dot3(d23, d23);
  const double b12 = dot3(y, y + 3), b13 = dot3(y, y + 6), b23 = dot3(y + 3, y + 6);
  const double D1[9] = {a23, -a23 * b12, 0, -a23 * b12, a23 - a12, a12 * b23, 0, a12 * b23, -a12};
  const double D2[9] = {a23, 0, -a23 * b13, 0, -a13, a13 * b23, -a23 * b13, a13 * b23, a23 - a13};
  double A1[9], A2[9];
  adj3(D1, A1);
  adj3(D2, A2);
  const double c0 = det3(D1, A1), c3 = det3(D2, A2);
  const double c1 = trace_product(A1, D2), c2 = trace_product(A2, D1);
  if (!(fabs(c3) > 0)) return;
  const double k2 = c2 / c3, k1 = c1 / c3, k0 = c0 / c3;
  double big = fabs(k2);
  if (fabs(k1) > big) big = fabs(k1);
  if (fabs(k0) > big) big = fabs(k0);
  double lo = -(1 + big), hi = 1 + big;
#pragma unroll 1
  for (int it = 0; it < kBisectSteps; ++it) {
    const double mid = (lo + hi) / 2;
    if (cubic(mid, k2, k1, k0) < 0)
      lo = mid;
    else
      hi = mid;
  }
  double g = (lo + hi) / 2;
#pragma unroll 1
  for (int it = 0; it < kNewtonSteps; ++it) {
    const double f = cubic(g, k2, k1, k0), df = (3 * g + 2 * k2) * g + k1;
    if (fabs(df) > 0) g = g - f / df;
  }
  double A[3][3], V[3][3], d[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A[i][j] = D1[i * 3 + j] + g * D2[i * 3 + j];
  hmath::sym_eig(A, V, d);
  int z = 0;
  double least = fabs(d[0]);
  if (fabs(d[1]) < least) least = fabs(d[1]), z = 1;
  if (fabs(d[2]) < least) z = 2;
  const double da = z == 0 ? d[1] : d[0], db = z == 2 ? d[1] : d[2];
  double ea[3], eb[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ea[i] = z == 0 ? V[i][1] : V[i][0];
    eb[i] = z == 2 ? V[i][1] : V[i][2];
  }
  const bool ab = da > 0 && db < 0, ba = db > 0 && da < 0;
  if (!ab && !ba) return;
  const double s = ab ? sqrt(-db / da) : sqrt(-da / db);
  double e1[3], e2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    e1[i] = ab ? ea[i] : eb[i];
    e2[i] = ab ? eb[i] : ea[i];
  }
  // X^-1, shared by every solution
  double X[9], Xa[9], Xi[9], cr[3];
  cross3(d12, d13, cr);
#pragma unroll
  for (int i = 0; i < 3; ++i) X[i * 3] = d12[i], X[i * 3 + 1] = d13[i], X[i * 3 + 2] = cr[i];
  adj3(X, Xa);
  const double dx = det3(X, Xa);
#pragma unroll
  for (int k = 0; k < 9; ++k) Xi[k] = Xa[k] / dx;

#pragma unroll 1
  for (int line = 0; line < 2; ++line) {
    const double sg = line ? -s : s;
    const double w0 = e1[0] + sg * e2[0], w1 = e1[1] + sg * e2[1], w2 = e1[2] + sg * e2[2];
    const double p = -w1 / w0, q = -w2 / w0;
    const double qa = D1[0] * q * q + D1[8];
    const double qb = 2 * (D1[0] * p * q + D1[1] * q + D1[5]);
    const double qc = D1[0] * p * p + 2 * D1[1] * p + D1[4];
    const double disc = qb * qb - 4 * qa * qc;
    if (!(disc >= 0)) continue;
    const double sq = sqrt(disc);
#pragma unroll 1
    for (int root = 0; root < 2; ++root) {
      const double tau = ((root ? -sq : sq) - qb) / (2 * qa);
      const double l1r = p + q * tau, den = 1 + tau * tau - 2 * b23 * tau;
      if (!(tau > 0 && l1r > 0 && den > 0)) continue;
      double l2 = sqrt(a23 / den);
      double l3 = tau * l2, l1 = l1r * l2;
#pragma unroll 1
      for (int it = 0; it < kDepthSteps; ++it) {
        const double r0 = l1 * l1 + l2 * l2 - 2 * b12 * l1 * l2 - a12;
        const double r1 = l1 * l1 + l3 * l3 - 2 * b13 * l1 * l3 - a13;
        const double r2 = l2 * l2 + l3 * l3 - 2 * b23 * l2 * l3 - a23;
        const double J[9] = {2 * l1 - 2 * b12 * l2, 2 * l2 - 2 * b12 * l1, 0, 2 * l1 - 2 * b13 * l3, 0,
                             2 * l3 - 2 * b13 * l1, 0, 2 * l2 - 2 * b23 * l3, 2 * l3 - 2 * b23 * l2};
        double Ja[9];
        adj3(J, Ja);
        const double dj = det3(J, Ja);
        if (dj == 0) break;
        l1 = l1 - (Ja[0] * r0 + Ja[1] * r1 + Ja[2] * r2) / dj;
        l2 = l2 - (Ja[3] * r0 + Ja[4] * r1 + Ja[5] * r2) / dj;
        l3 = l3 - (Ja[6] * r0 + Ja[7] * r1 + Ja[8] * r2) / dj;
      }
      double f1[3], f2[3], fc[3], Y[9], R[9], pose[12];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        f1[k] = l1 * y[k] - l2 * y[3 + k];
        f2[k] = l1 * y[k] - l3 * y[6 + k];
      }
      cross3(f1, f2, fc);
#pragma unroll
      for (int i = 0; i < 3; ++i) Y[i * 3] = f1[i], Y[i * 3 + 1] = f2[i], Y[i * 3 + 2] = fc[i];
      hmath::mat3mul(Y, Xi, R);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        pose[i * 4] = R[i * 3], pose[i * 4 + 1] = R[i * 3 + 1], pose[i * 4 + 2] = R[i * 3 + 2];
        pose[i * 4 + 3] = l1 * y[i] - (R[i * 3] * x[0] + R[i * 3 + 1] * x[1] + R[i * 3 + 2] * x[2]);
      }
      if (finite_n(pose, 12)) sink(pose);
    }
  }
}

// R x + t for a pose of twelve doubles
SIFT_HD void transform(const double* P, const double* x, double* pc) {
#pragma unroll
  for (int i = 0; i < 3; ++i) pc[i] = P[i * 4] * x[0] + P[i * 4 + 1] * x[1] + P[i * 4 + 2] * x[2] + P[i * 4 + 3];
}

// Step 3.  x: four 3-D points, pix: their pixels.  false: no model (pose is then unspecified).
SIFT_HD bool hypothesis(const Calib& c, const double* x, const P2* pix, double* pose) {
  double y[9], u, v;
#pragma unroll
  for (int i = 0; i < 3; ++i) bearing(c.Ki, pix[i], y + 3 * i);
  pmath::normalise(c.Ki, pix[3], u, v);
  double best = __builtin_inf();
  bool has = false;
  p3p(x, y, [&](const double* P) {
    double pc[3];
    transform(P, x + 9, pc);
    const double ex = pc[0] / pc[2] - u, ey = pc[1] / pc[2] - v;
    const double e = ex * ex + ey * ey;
    if (pc[2] > 0 && e < best) {
      best = e;
      has = true;
#pragma unroll
      for (int k = 0; k < 12; ++k) pose[k] = P[k];
    }
  });
  return has;
}

SIFT_HD double inlier_limit(double thr) { return thr * thr; }

// Step 4.
SIFT_HD bool is_inlier(const double* K, const double* P, const double* x, P2 pix, double t2) {
  double pc[3];
  transform(P, x, pc);
  const double p0 = K[0] * pc[0] + K[1] * pc[1] + K[2] * pc[2];
  const double p1 = K[3] * pc[0] + K[4] * pc[1] + K[5] * pc[2];
  const double p2 = K[6] * pc[0] + K[7] * pc[1] + K[8] * pc[2];
  const double ex = p0 - pix.x * p2, ey = p1 - pix.y * p2;
  return p2 > 0 && ex * ex + ey * ey <= t2 * (p2 * p2);
}

// Step 6: one row's 28 terms under the pose P.
SIFT_HD void refit_terms(const double* Ki, const double* P, const double* x, P2 pix, double* out) {
  double u, v, pc[3], Jx[6], Jy[6];
  pmath::normalise(Ki, pix, u, v);
  transform(P, x, pc);
  const double iz = 1 / pc[2];
  const double px = pc[0] * iz, py = pc[1] * iz;
  const double rx = px - u, ry = py - v;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    // column j of -R [x]x
    const int a = (j + 1) % 3, b = (j + 2) % 3;
    const double g0 = P[b] * x[a] - P[a] * x[b], g1 = P[4 + b] * x[a] - P[4 + a] * x[b],
                 g2 = P[8 + b] * x[a] - P[8 + a] * x[b];
    Jx[j] = iz * g0 - px * iz * g2;
    Jy[j] = iz * g1 - py * iz * g2;
  }
  Jx[3] = iz, Jx[4] = 0, Jx[5] = -px * iz;
  Jy[3] = 0, Jy[4] = iz, Jy[5] = -py * iz;
  int t = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) out[t++] = Jx[a] * Jx[b] + Jy[a] * Jy[b];
#pragma unroll
  for (int a = 0; a < 6; ++a) out[t++] = Jx[a] * rx + Jy[a] * ry;
  out[t] = rx * rx + ry * ry;
}

// J^T J d = -J^T r by Gaussian elimination with partial pivoting (every index a
// constant once unrolled), then the candidate Pn = (R C(d), t + dt).  false: a
// pivot below 1e-300.
SIFT_HD bool refit_candidate(const double* sums, const double* P, double* Pn) {
  double A[6][7], d[6];
  int t = 0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = a; b < 6; ++b) A[a][b] = A[b][a] = sums[t++];
#pragma unroll
  for (int a = 0; a < 6; ++a) A[a][6] = -sums[21 + a];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    int piv = c;
    double most = fabs(A[c][c]);
#pragma unroll
    for (int r = c + 1; r < 6; ++r)
      if (fabs(A[r][c]) > most) most = fabs(A[r][c]), piv = r;
    if (most < 1e-300) return false;
#pragma unroll
    for (int r = c + 1; r < 6; ++r)
      if (r == piv) {
#pragma unroll
        for (int k = 0; k < 7; ++k) {
          const double tmp = A[c][k];
          A[c][k] = A[r][k];
          A[r][k] = tmp;
        }
      }
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      const double f = A[r][c] / A[c][c];
#pragma unroll
      for (int k = c; k < 7; ++k) A[r][k] -= f * A[c][k];
    }
  }
#pragma unroll
  for (int c = 5; c >= 0; --c) {
    double v = A[c][6];
#pragma unroll
    for (int k = c + 1; k < 6; ++k) v -= A[c][k] * d[k];
    d[c] = v / A[c][c];
  }
  const double a[3] = {d[0] / 2, d[1] / 2, d[2] / 2};
  const double aa = dot3(a, a), den = 1 + aa;
  const double C[9] = {((1 - aa) + 2 * a[0] * a[0]) / den, (2 * a[0] * a[1] - 2 * a[2]) / den,
                       (2 * a[0] * a[2] + 2 * a[1]) / den, (2 * a[1] * a[0] + 2 * a[2]) / den,
                       ((1 - aa) + 2 * a[1] * a[1]) / den, (2 * a[1] * a[2] - 2 * a[0]) / den,
                       (2 * a[2] * a[0] - 2 * a[1]) / den, (2 * a[2] * a[1] + 2 * a[0]) / den,
                       ((1 - aa) + 2 * a[2] * a[2]) / den};
  const double R[9] = {P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]};
  double Rn[9];
  hmath::mat3mul(R, C, Rn);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    Pn[i * 4] = Rn[i * 3], Pn[i * 4 + 1] = Rn[i * 3 + 1], Pn[i * 4 + 2] = Rn[i * 3 + 2];
    Pn[i * 4 + 3] = P[i * 4 + 3] + d[3 + i];
  }
  return true;
}

// a candidate of cost c1 against the held cost c0
SIFT_HD bool refit_accept(double c1, double c0) { return c1 < c0; }

// 4 distinct rows of n (n > 4); no check on the subset: a degenerate one gives no model
SIFT_HD void draw_subset(Rng& rng, int n, int* idx) {
#pragma unroll
  for (int i = 0; i < kModelPoints; ++i) {
    for (;;) {
      idx[i] = rng.uniform(0, n);
      bool seen = false;
#pragma unroll
      for (int j = 0; j < i; ++j) seen |= idx[i] == idx[j];
      if (!seen) break;
    }
  }
}

}  // namespace pnpmath
}  // namespace sift
