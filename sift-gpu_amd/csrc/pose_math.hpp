// pose_math.hpp -- the arithmetic of recoverPose and triangulatePoints, stated
// once for the host path (pose.hip, one pair set) and the kernels
// (pose_batch.hip, every segment of a batch), in the manner of
// fundamental_math.hpp.  It reuses homography_math.hpp's P2, mat3mul and its
// Jacobi (smallest_eigvec at N = 4, sym_eig at N = 3).  Every function is
// __host__ __device__ and inline; the library is built -ffp-contract=off and
// double + - * / and sqrt are IEEE on gfx950 as on x86-64, so the same
// statement gives the same bits on either side.  There is no libm call.
//
// Convention (OpenCV's): src is image 1, dst image 2, [dst; 1]^T F [src; 1] = 0,
// X_dst = R X_src + t, E ~ [t]x R.  Matrices are row-major doubles; a camera P is
// 3 x 4, twelve doubles.
//
//   1. Calibration (invert3): K^-1 = adj(K) / det(K).  A zero or non-finite
//      determinant or a non-finite entry of the inverse: no pose.  A pixel
//      (x, y) becomes K^-1 (x, y, 1)^T divided by its third component
//      (normalise).
//   2. Essential matrix (decompose): E0 = K_dst^T (F K_src); sym_eig on E0^T E0;
//      the eigenpairs ordered sigma_1^2 >= sigma_2^2 >= sigma_3^2 by three
//      compare-exchanges (a later pair moves ahead only when strictly larger); a
//      non-finite sigma^2 or sigma_2^2 <= 0: no pose (a zero F, an exactly rank-1 E0).
//      u1 = E0 v1 / sigma_1, u2 = E0 v2 / sigma_2, u3 = u1 x u2; v3 is negated
//      when det [v1 v2 v3] < 0.  The reported E is ((sigma_1 + sigma_2) / 2)
//      (u1 v1^T + u2 v2^T), the nearest essential matrix (H&Z 9.6).
//   3. Candidates: with W = [0 -1 0; 1 0 0; 0 0 1], R1 = U W V^T, R2 = U W^T V^T,
//      t = u3, in cv::decomposeEssentialMat's order inside recoverPose:
//      (R1, +t), (R2, +t), (R1, -t), (R2, -t).  A non-finite entry: no pose.
//   4. Triangulation (triangulate, cv::triangulatePoints): for points (x, y) and
//      (X, Y) and cameras P_src, P_dst the rows x P_src[2] - P_src[0],
//      y P_src[2] - P_src[1], X P_dst[2] - P_dst[0], Y P_dst[2] - P_dst[1]; the
//      ten sums of A^T A's upper triangle, each row 0 + row 1 + row 2 + row 3,
//      mirrored; Q = smallest_eigvec<4>.
//   5. Cheirality (good_point, cv::recoverPose with distanceThresh): with
//      Q /= Q[3], a row is good iff 0 < z < distance_thresh for z = Q[2] and for
//      z = P_dst[2] . Q, in double (a NaN is never good).  The winner is the first
//      candidate with the largest count of good rows among the rows considered.
//
// The library's own rule, not bit-compatible with OpenCV (which uses an SVD).
#pragma once

#include "homography_math.hpp"

namespace sift {
namespace pmath {

using hmath::P2;

constexpr int kCandidates = 4;

SIFT_HD bool finite_n(const double* a, int n) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < n; ++k) ok &= fabs(a[k]) <= DBL_MAX;  // false for NaN and inf
  return ok;
}

// false: K is singular or non-finite
SIFT_HD bool invert3(const double* K, double* Ki) {
  const double c[9] = {K[4] * K[8] - K[5] * K[7], K[2] * K[7] - K[1] * K[8], K[1] * K[5] - K[2] * K[4],
                       K[5] * K[6] - K[3] * K[8], K[0] * K[8] - K[2] * K[6], K[2] * K[3] - K[0] * K[5],
                       K[3] * K[7] - K[4] * K[6], K[1] * K[6] - K[0] * K[7], K[0] * K[4] - K[1] * K[3]};
  const double det = K[0] * c[0] + K[1] * c[3] + K[2] * c[6];
  if (!(fabs(det) > 0 && fabs(det) <= DBL_MAX)) return false;
#pragma unroll
  for (int k = 0; k < 9; ++k) Ki[k] = c[k] / det;
  return finite_n(Ki, 9);
}

SIFT_HD void normalise(const double* Ki, P2 p, double& x, double& y) {
  const double px = p.x, py = p.y;
  const double w = Ki[6] * px + Ki[7] * py + Ki[8];
  x = (Ki[0] * px + Ki[1] * py + Ki[2]) / w;
  y = (Ki[3] * px + Ki[4] * py + Ki[5]) / w;
}

// What a segment's rows share: both inverse calibrations, the reported E and
// the four candidate cameras [R | t].
struct Decomp {
  double Kis[9], Kid[9], E[9], P[kCandidates][12];
};

// compare-exchange of eigenpairs a < b: pair b moves ahead when strictly larger
SIFT_HD void order_pair(double& da, double& db, double* va, double* vb) {
  if (db > da) {
    const double t = da;
    da = db;
    db = t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double u = va[k];
      va[k] = vb[k];
      vb[k] = u;
    }
  }
}

// Steps 1 to 3.  false: no pose (D is then unspecified).
SIFT_HD bool decompose(const double* F, const double* Ks, const double* Kd, Decomp& D) {
  if (!invert3(Ks, D.Kis) || !invert3(Kd, D.Kid)) return false;
  double T[9], E0[9], G[3][3], V[3][3], d[3];
  hmath::mat3mul(F, Ks, T);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) E0[i * 3 + j] = Kd[i] * T[j] + Kd[3 + i] * T[3 + j] + Kd[6 + i] * T[6 + j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) G[i][j] = E0[i] * E0[j] + E0[3 + i] * E0[3 + j] + E0[6 + i] * E0[6 + j];
  hmath::sym_eig(G, V, d);
  double v1[3] = {V[0][0], V[1][0], V[2][0]}, v2[3] = {V[0][1], V[1][1], V[2][1]}, v3[3] = {V[0][2], V[1][2], V[2][2]};
  order_pair(d[0], d[1], v1, v2);
  order_pair(d[1], d[2], v2, v3);
  order_pair(d[0], d[1], v1, v2);
  if (!finite_n(d, 3) || !(d[1] > 0)) return false;
  const double s1 = sqrt(d[0]), s2 = sqrt(d[1]);
  double u1[3], u2[3], u3[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    u1[i] = (E0[i * 3] * v1[0] + E0[i * 3 + 1] * v1[1] + E0[i * 3 + 2] * v1[2]) / s1;
    u2[i] = (E0[i * 3] * v2[0] + E0[i * 3 + 1] * v2[1] + E0[i * 3 + 2] * v2[2]) / s2;
  }
  u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
  u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
  u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  const double det = v1[0] * (v2[1] * v3[2] - v2[2] * v3[1]) - v1[1] * (v2[0] * v3[2] - v2[2] * v3[0]) +
                     v1[2] * (v2[0] * v3[1] - v2[1] * v3[0]);
  if (det < 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v3[k] = -v3[k];
  }
  const double half = (s1 + s2) / 2;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      D.E[i * 3 + j] = half * (u1[i] * v1[j] + u2[i] * v2[j]);
      // U W = [u2 -u1 u3], U W^T = [-u2 u1 u3]
      const double r1 = u2[i] * v1[j] - u1[i] * v2[j] + u3[i] * v3[j];
      const double r2 = u1[i] * v2[j] - u2[i] * v1[j] + u3[i] * v3[j];
      D.P[0][i * 4 + j] = D.P[2][i * 4 + j] = r1;
      D.P[1][i * 4 + j] = D.P[3][i * 4 + j] = r2;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    D.P[0][i * 4 + 3] = D.P[1][i * 4 + 3] = u3[i];
    D.P[2][i * 4 + 3] = D.P[3][i * 4 + 3] = -u3[i];
  }
  return finite_n(D.E, 9) && finite_n(D.P[0], 12) && finite_n(D.P[1], 12);
}

// Step 4 for one pair: Q[4], homogeneous, not divided.
SIFT_HD void triangulate(const double* Ps, const double* Pd, double x, double y, double X, double Y, double* Q) {
  double a[4][4], A[4][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    a[0][k] = x * Ps[8 + k] - Ps[k];
    a[1][k] = y * Ps[8 + k] - Ps[4 + k];
    a[2][k] = X * Pd[8 + k] - Pd[k];
    a[3][k] = Y * Pd[8 + k] - Pd[4 + k];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = j; k < 4; ++k)
      A[j][k] = A[k][j] = a[0][j] * a[0][k] + a[1][j] * a[1][k] + a[2][j] * a[2][k] + a[3][j] * a[3][k];
  hmath::smallest_eigvec(A, Q);
}

SIFT_HD void identity_camera(double* P) {
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = k == 0 || k == 5 || k == 10;
}

// Steps 4 and 5 for one pair under the camera P_dst = P (P_src = [I | 0]):
// xyz is Q[0..2] / Q[3].
SIFT_HD bool good_point(const Decomp& D, const double* P, P2 s, P2 d, double thresh, double* xyz) {
  double Ps[12], Q[4], x, y, X, Y;
  identity_camera(Ps);
  normalise(D.Kis, s, x, y);
  normalise(D.Kid, d, X, Y);
  triangulate(Ps, P, x, y, X, Y, Q);
  xyz[0] = Q[0] / Q[3];
  xyz[1] = Q[1] / Q[3];
  xyz[2] = Q[2] / Q[3];
  const double z2 = P[8] * xyz[0] + P[9] * xyz[1] + P[10] * xyz[2] + P[11];
  return xyz[2] > 0 && xyz[2] < thresh && z2 > 0 && z2 < thresh;
}

// The winner of four counts: the first candidate with the largest.
SIFT_HD int winner(const int* count) {
  int w = 0, most = count[0];
#pragma unroll
  for (int c = 1; c < kCandidates; ++c)
    if (count[c] > most) most = count[c], w = c;
  return w;
}

SIFT_HD bool thresh_ok(double thresh) { return thresh > 0; }  // false for NaN; +inf passes

}  // namespace pmath
}  // namespace sift
