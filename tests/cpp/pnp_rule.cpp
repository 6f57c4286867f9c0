// The host path of sift_solve_p3p and sift_solve_pnp (sift-gpu_amd/csrc/pnp.hip
// over pnp_math.hpp) as a stand-alone program: it is linked with pnp.hip alone,
// built with the address and undefined-behaviour sanitizers, and run on the CPU
// (tests/test_pnp.py::test_pnp_rule_program).
//
//   1. a calibrated view of 200 points under a planted pose, pixels rounded to
//      float: P3P on the first three rows returns the planted pose among its
//      solutions; RANSAC without outliers and with 30 % outliers returns it,
//      with every planted inlier in the mask and no planted outlier;
//   2. the degenerate inputs: n = 0, 3 and 4, NULL optional buffers, a row mask
//      of zeros and one with a zero among four rows, rows behind the camera,
//      all-zero 3-D rows, NaN and infinite rows, coincident 3-D points and
//      bearings, collinear points, a singular and a non-finite K, thresholds of
//      0, -8, NaN and +inf, max_iters 0 and 1, confidence 0 and 1.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

namespace sift {
int solve_p3p(const double* xyz, const float* xy, const double* K, double* poses);
int solve_pnp_ransac(const double* xyz, const float* xy, int n, const unsigned char* row_mask, const double* K,
                     double thr, int max_iters, double confidence, double* pose, unsigned char* mask_out,
                     int* n_inliers);
}  // namespace sift

static void fail(const char* what) {
  fprintf(stderr, "FAIL: %s\n", what);
  exit(1);
}

static double pose_error(const double* pose, const double* R, const double* t) {
  double e = 0;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) e = fmax(e, fabs(pose[i * 4 + j] - R[i * 3 + j]));
    e = fmax(e, fabs(pose[i * 4 + 3] - t[i]));
  }
  return e;
}

int main() {
  const int n = 200;
  const double f = 800, cx = 320, cy = 240, ay = 0.4, ax = -0.25;
  const double K[9] = {f, 1.5, cx, 0, f + 10, cy, 0, 0, 1};
  const double Ry[9] = {cos(ay), 0, sin(ay), 0, 1, 0, -sin(ay), 0, cos(ay)};
  const double Rx[9] = {1, 0, 0, 0, cos(ax), -sin(ax), 0, sin(ax), cos(ax)};
  double R[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = Ry[i * 3] * Rx[j] + Ry[i * 3 + 1] * Rx[3 + j] + Ry[i * 3 + 2] * Rx[6 + j];
  const double t[3] = {0.7, -1.1, 2.0};
  std::vector<double> X(3 * n);
  std::vector<float> xy(2 * n), noisy;
  std::vector<unsigned char> planted(n, 1);
  unsigned lcg = 4242u;
  auto unit = [&]() {
    lcg = lcg * 1664525u + 1013904223u;
    return (lcg >> 8) / 16777216.0;
  };
  for (int i = 0; i < n; ++i) {
    // a point in front of the camera, expressed in the world frame: X = R^T (Xc - t)
    const double c[3] = {-1.5 + 3 * unit() - t[0], -1 + 2 * unit() - t[1], 2 + 8 * unit() - t[2]};
    for (int k = 0; k < 3; ++k) X[3 * i + k] = R[k] * c[0] + R[3 + k] * c[1] + R[6 + k] * c[2];
    const double xc = c[0] + t[0], yc = c[1] + t[1], zc = c[2] + t[2];
    xy[2 * i] = (float)((K[0] * xc + K[1] * yc) / zc + K[2]);
    xy[2 * i + 1] = (float)(K[4] * yc / zc + K[5]);
  }

  double poses[48], pose[12];
  const int ns = sift::solve_p3p(X.data(), xy.data(), K, poses);
  if (ns < 1 || ns > 4) fail("P3P: no solution for a general triple");
  double best = 1e9;
  for (int s = 0; s < ns; ++s) best = fmin(best, pose_error(poses + 12 * s, R, t));
  if (!(best < 1e-4)) fail("P3P: the planted pose is not among the solutions");
  for (int k = 12 * ns; k < 48; ++k)
    if (poses[k] != 0) fail("P3P: an unused slot is not zero");

  std::vector<unsigned char> mask(n, 9);
  int good = -1;
  if (!sift::solve_pnp_ransac(X.data(), xy.data(), n, nullptr, K, 8.0, 100, 0.99, pose, mask.data(), &good))
    fail("no model without outliers");
  if (good != n || !(pose_error(pose, R, t) < 1e-5)) fail("the planted pose does not come back");
  noisy = xy;
  for (int i = 0; i < n; i += 3) {  // a third of the rows: 40 px and more away
    noisy[2 * i] += (float)(40 + 200 * unit());
    noisy[2 * i + 1] -= (float)(40 + 100 * unit());
    planted[i] = 0;
  }
  if (!sift::solve_pnp_ransac(X.data(), noisy.data(), n, nullptr, K, 8.0, 100, 0.99, pose, mask.data(), &good))
    fail("no model with outliers");
  if (!(pose_error(pose, R, t) < 1e-5)) fail("the planted pose does not come back with outliers");
  for (int i = 0; i < n; ++i)
    if (mask[i] != planted[i]) fail("the mask is not the planted one");
  // optional buffers NULL, a row mask
  if (!sift::solve_pnp_ransac(X.data(), noisy.data(), n, planted.data(), K, 8.0, 100, 0.99, pose, nullptr, &good))
    fail("no model under a row mask");

  // the degenerate inputs: every one returns, none touches memory it does not own
  auto none = [&](const double* x, const float* p, int cnt, const unsigned char* rm, const double* Km, double thr,
                  int iters, double conf, const char* what) {
    double q[12];
    int g = -1;
    memset(q, 0x55, sizeof(q));
    std::vector<unsigned char> m(cnt + 1, 7);
    if (sift::solve_pnp_ransac(x, p, cnt, rm, Km, thr, iters, conf, q, m.data(), &g)) fail(what);
    for (double v : q)
      if (v != 0) fail(what);
    if (g != 0 || m[cnt] != 7) fail(what);
    for (int i = 0; i < cnt; ++i)
      if (m[i] != 0) fail(what);
  };
  const std::vector<unsigned char> zeros(n, 0);
  const unsigned char one_out[4] = {1, 1, 0, 1};
  const double Ksing[9] = {f, 0, cx, 0, f, cy, 2 * f, 0, 2 * cx};
  double Knan[9];
  memcpy(Knan, K, sizeof(K));
  Knan[4] = NAN;
  none(X.data(), xy.data(), 0, nullptr, K, 8.0, 100, 0.99, "a model from no rows");
  none(X.data(), xy.data(), 3, nullptr, K, 8.0, 100, 0.99, "a model from three rows");
  none(X.data(), xy.data(), 4, one_out, K, 8.0, 100, 0.99, "a model from four rows with one masked out");
  none(X.data(), xy.data(), n, zeros.data(), K, 8.0, 100, 0.99, "a model from a mask of zeros");
  none(X.data(), xy.data(), n, nullptr, Ksing, 8.0, 100, 0.99, "a model from a singular K");
  none(X.data(), xy.data(), n, nullptr, Knan, 8.0, 100, 0.99, "a model from a NaN K");
  none(X.data(), xy.data(), n, nullptr, K, NAN, 100, 0.99, "a model at threshold NaN");
  none(X.data(), xy.data(), n, nullptr, K, 8.0, 0, 0.99, "a model from no iterations");
  none(X.data(), xy.data(), n, nullptr, K, 8.0, 100, 0.0, "a model at confidence 0");
  none(X.data(), xy.data(), n, nullptr, K, 8.0, 100, 1.0, "a model at confidence 1");
  if (!sift::solve_pnp_ransac(X.data(), xy.data(), 4, nullptr, K, 8.0, 100, 0.99, pose, mask.data(), &good) ||
      good != 4 || !mask[0] || !mask[3])
    fail("no direct fit from four rows");
  if (!sift::solve_pnp_ransac(X.data(), xy.data(), n, nullptr, K, -8.0, 1, 0.99, pose, mask.data(), &good) || good != n)
    fail("threshold -8 with one iteration does not behave as 8");
  if (!sift::solve_pnp_ransac(X.data(), noisy.data(), n, nullptr, K, INFINITY, 100, 0.99, pose, mask.data(), &good))
    fail("no model at threshold +inf");
  // these return whatever the rule gives; they must only run clean
  sift::solve_pnp_ransac(X.data(), xy.data(), n, nullptr, K, 0.0, 100, 0.99, pose, mask.data(), &good);
  std::vector<double> Y = X;
  std::vector<float> q = xy;
  for (int i = 0; i < n; i += 4) Y[3 * i] = Y[3 * i + 1] = Y[3 * i + 2] = 0;           // all-zero rows
  for (int i = 1; i < n; i += 8)                                                      // rows behind the camera
    for (int k = 0; k < 3; ++k) Y[3 * i + k] = -X[3 * i + k] - 2 * (R[k] * t[0] + R[3 + k] * t[1] + R[6 + k] * t[2]);
  Y[3 * 6 + 1] = NAN, Y[3 * 10] = INFINITY, q[2 * 14] = NAN, q[2 * 18 + 1] = -INFINITY;
  if (!sift::solve_pnp_ransac(Y.data(), q.data(), n, nullptr, K, 8.0, 100, 0.99, pose, mask.data(), &good))
    fail("no model among zero, mirrored, NaN and infinite rows");
  for (double v : pose)
    if (!(fabs(v) <= 1e300)) fail("a non-finite pose");
  if (mask[0] || mask[6] || mask[10] || mask[14] || mask[18]) fail("a zero, NaN or infinite row is an inlier");
  // P3P: coincident points, coincident bearings, collinear points, non-finite input, bad K
  double T3[9];
  float p3[6];
  memcpy(T3, X.data(), sizeof(T3)), memcpy(p3, xy.data(), sizeof(p3));
  memcpy(T3 + 6, T3 + 3, 3 * sizeof(double));
  sift::solve_p3p(T3, p3, K, poses);
  memcpy(T3, X.data(), sizeof(T3));
  p3[2] = p3[0], p3[3] = p3[1];
  sift::solve_p3p(T3, p3, K, poses);
  memcpy(p3, xy.data(), sizeof(p3));
  for (int k = 0; k < 3; ++k) T3[6 + k] = T3[k] + 2.5 * (T3[3 + k] - T3[k]);
  if (sift::solve_p3p(T3, p3, K, poses) != 0) fail("P3P: a solution from collinear points");
  memcpy(T3, X.data(), sizeof(T3));
  T3[4] = NAN;
  if (sift::solve_p3p(T3, p3, K, poses) != 0) fail("P3P: a solution from a NaN point");
  T3[4] = INFINITY;
  sift::solve_p3p(T3, p3, K, poses);
  memcpy(T3, X.data(), sizeof(T3));
  if (sift::solve_p3p(T3, p3, Ksing, poses) != 0 || sift::solve_p3p(T3, p3, Knan, poses) != 0)
    fail("P3P: a solution from a singular or NaN K");
  printf("pnp rule ok\n");
  return 0;
}
