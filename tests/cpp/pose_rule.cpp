// The host path of sift_recover_pose and sift_triangulate_points
// (sift-gpu_amd/csrc/pose.hip over pose_math.hpp) as a stand-alone program: it is
// linked with pose.hip alone, built with the address and undefined-behaviour
// sanitizers, and run on the CPU (tests/test_pose.py::test_pose_rule_program).
//
//   1. two calibrated views of 50 points: the planted rotation and baseline come
//      back, every row is good, and the points are the planted ones; the same
//      through sift_triangulate_points with the returned camera;
//   2. the degenerate inputs: n = 0 and n = 1, NULL optional outputs, a mask of
//      zeros, a NaN row, a singular and a non-finite K, F of zeros, of rank 1 and
//      non-finite, and distance thresholds of 0, -1, NaN and +inf.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

namespace sift {
int recover_pose(const double* F, const double* K_src, const double* K_dst, const float* src_xy, const float* dst_xy,
                 int n, const unsigned char* mask_in, double distance_thresh, double* pose, double* E,
                 unsigned char* mask_out, double* xyz, int* n_good);
void triangulate_points(const double* P_src, const double* P_dst, const float* src_xy, const float* dst_xy, int n,
                        double* xyzw);
}  // namespace sift

static void fail(const char* what) {
  fprintf(stderr, "FAIL: %s\n", what);
  exit(1);
}

static void mul3(const double* a, const double* b, double* c) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
}

int main() {
  const int n = 50;
  const double f = 800, cx = 320, cy = 240, ang = 0.15;
  double t[3] = {-1.0, 0.1, 0.2};
  const double tn = sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  for (double& v : t) v /= tn;
  const double R[9] = {cos(ang), 0, sin(ang), 0, 1, 0, -sin(ang), 0, cos(ang)};
  const double Tx[9] = {0, -t[2], t[1], t[2], 0, -t[0], -t[1], t[0], 0};
  const double K[9] = {f, 0, cx, 0, f, cy, 0, 0, 1};
  const double Ki[9] = {1 / f, 0, -cx / f, 0, 1 / f, -cy / f, 0, 0, 1};
  const double KiT[9] = {1 / f, 0, 0, 0, 1 / f, 0, -cx / f, -cy / f, 1};
  double E0[9], A[9], F[9];
  mul3(Tx, R, E0);
  mul3(KiT, E0, A);
  mul3(A, Ki, F);
  for (double& v : F) v *= -1e4;  // any scale and sign
  std::vector<float> src(2 * n), dst(2 * n);
  std::vector<double> X(3 * n);
  unsigned lcg = 4242u;
  auto unit = [&]() {
    lcg = lcg * 1664525u + 1013904223u;
    return (lcg >> 8) / 16777216.0;
  };
  for (int i = 0; i < n; ++i) {
    const double x = -2 + 4 * unit(), y = -1.5 + 3 * unit(), z = 4 + 6 * unit();
    const double xc = R[0] * x + R[1] * y + R[2] * z + t[0], yc = R[3] * x + R[4] * y + R[5] * z + t[1],
                 zc = R[6] * x + R[7] * y + R[8] * z + t[2];
    X[3 * i] = x, X[3 * i + 1] = y, X[3 * i + 2] = z;
    src[2 * i] = (float)(f * x / z + cx), src[2 * i + 1] = (float)(f * y / z + cy);
    dst[2 * i] = (float)(f * xc / zc + cx), dst[2 * i + 1] = (float)(f * yc / zc + cy);
  }

  double pose[12], E[9];
  std::vector<unsigned char> mask(n, 9);
  std::vector<double> xyz(3 * n, 5.0), xyzw(4 * n);
  int good = -1;
  if (!sift::recover_pose(F, K, K, src.data(), dst.data(), n, nullptr, 50.0, pose, E, mask.data(), xyz.data(), &good))
    fail("no pose");
  if (good != n) fail("not every row is good");
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      if (!(fabs(pose[i * 4 + j] - R[i * 3 + j]) < 1e-12)) fail("the rotation is not the planted one");
    if (!(fabs(pose[i * 4 + 3] - t[i]) < 1e-12)) fail("the baseline is not the planted one");
  }
  for (int i = 0; i < n; ++i) {
    if (mask[i] != 1) fail("a planted row is not in the mask");
    for (int k = 0; k < 3; ++k)
      if (!(fabs(xyz[3 * i + k] - X[3 * i + k]) < 5e-3)) fail("a point is not the planted one");
  }
  // the same points through triangulate_points: cameras K [I | 0] and K [R | t] on the pixels
  double Ps[12], Pd[12];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      Ps[i * 4 + j] = j < 3 ? K[i * 3 + j] : 0;
      Pd[i * 4 + j] = K[i * 3] * pose[j] + K[i * 3 + 1] * pose[4 + j] + K[i * 3 + 2] * pose[8 + j];
    }
  sift::triangulate_points(Ps, Pd, src.data(), dst.data(), n, xyzw.data());
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k)
      if (!(fabs(xyzw[4 * i + k] / xyzw[4 * i + 3] - X[3 * i + k]) < 5e-3)) fail("triangulate_points disagrees");
  sift::triangulate_points(Ps, Pd, src.data(), dst.data(), 0, nullptr);

  // the degenerate inputs: every one returns, none touches memory it does not own
  auto none = [&](const double* Fm, const double* Ks, const double* Kd, int cnt, const unsigned char* mi, double thr,
                  const char* what) {
    double p[12], e[9];
    int g = -1;
    memset(p, 0x55, sizeof(p));
    if (sift::recover_pose(Fm, Ks, Kd, src.data(), dst.data(), cnt, mi, thr, p, e, mask.data(), xyz.data(), &g)) fail(what);
    for (double v : p)
      if (v != 0) fail(what);
    if (g != 0) fail(what);
    for (int i = 0; i < cnt; ++i)
      if (mask[i] != 0 || xyz[3 * i] != 0) fail(what);
  };
  const double zero[9] = {0}, rank1[9] = {1, 2, 3, 2, 4, 6, 3, 6, 9};
  const double Ksing[9] = {f, 0, cx, 0, f, cy, 2 * f, 0, 2 * cx};
  double Knan[9], Fnan[9], Finf[9];
  memcpy(Knan, K, sizeof(K)), memcpy(Fnan, F, sizeof(F)), memcpy(Finf, F, sizeof(F));
  Knan[4] = NAN, Fnan[5] = NAN, Finf[0] = INFINITY;
  const std::vector<unsigned char> zeros(n, 0);
  none(F, K, K, 0, nullptr, 50.0, "a pose from no rows");
  none(F, K, K, n, zeros.data(), 50.0, "a pose from a mask of zeros");
  none(F, Ksing, K, n, nullptr, 50.0, "a pose from a singular K_src");
  none(F, K, zero, n, nullptr, 50.0, "a pose from a zero K_dst");
  none(F, Knan, K, n, nullptr, 50.0, "a pose from a NaN K");
  none(zero, K, K, n, nullptr, 50.0, "a pose from a zero F");
  none(Fnan, K, K, n, nullptr, 50.0, "a pose from a NaN F");
  none(Finf, K, K, n, nullptr, 50.0, "a pose from an infinite F");
  none(F, K, K, n, nullptr, 0.0, "a pose at threshold 0");
  none(F, K, K, n, nullptr, -1.0, "a pose at threshold -1");
  none(F, K, K, n, nullptr, NAN, "a pose at threshold NaN");
  // these return whatever the rule gives; they must only run clean
  sift::recover_pose(rank1, K, K, src.data(), dst.data(), n, nullptr, 50.0, pose, E, mask.data(), xyz.data(), &good);
  if (!sift::recover_pose(F, K, K, src.data(), dst.data(), 1, nullptr, 50.0, pose, nullptr, nullptr, nullptr, &good) ||
      good != 1)
    fail("no pose from one row");
  if (!sift::recover_pose(F, K, K, src.data(), dst.data(), n, nullptr, INFINITY, pose, E, nullptr, xyz.data(), &good) ||
      good != n)
    fail("no pose at threshold +inf");
  src[10] = NAN, dst[31] = INFINITY;
  if (!sift::recover_pose(F, K, K, src.data(), dst.data(), n, nullptr, 50.0, pose, E, mask.data(), nullptr, &good) ||
      good != n - 2 || mask[5] || mask[15])
    fail("a NaN row and an infinite row are not simply left out");
  printf("pose rule ok\n");
  return 0;
}
