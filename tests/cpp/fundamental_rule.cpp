// The host path of sift_find_fundamental (sift-gpu_amd/csrc/fundamental.hip over
// fundamental_math.hpp) on two fixed inputs, as a stand-alone program: it is
// linked with fundamental.hip alone, built with the address and
// undefined-behaviour sanitizers, and run on the CPU
// (tests/test_fundamental.py::test_fundamental_rule_program).
//
//   1. two views of 60 points with depth spread, every fourth pair an outlier
//      moved 120 px off its epipolar line: a model is found, the mask is the
//      planted inlier set, every inlier lies within 3 px of its epipolar lines
//      under the returned F, and det F is that of a rank-2 matrix;
//   2. the first 8 pairs alone (the direct fit, a mask of ones), the same with a
//      NaN row (none: F untouched by the core), and 7 pairs (none).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

namespace sift {
int find_fundamental_ransac(const float* src_xy, const float* dst_xy, int n, double thr, int max_iters,
                            double confidence, double* F, unsigned char* mask_out);
}

static void fail(const char* what) {
  fprintf(stderr, "FAIL: %s\n", what);
  exit(1);
}

// distance of (X, Y) to the line F (x, y, 1), and of (x, y) to F^T (X, Y, 1)
static double epipolar(const double* F, double x, double y, double X, double Y) {
  const double a = F[0] * x + F[1] * y + F[2], b = F[3] * x + F[4] * y + F[5], c = F[6] * x + F[7] * y + F[8];
  const double A = F[0] * X + F[3] * Y + F[6], B = F[1] * X + F[4] * Y + F[7], C = F[2] * X + F[5] * Y + F[8];
  const double d2 = fabs(X * a + Y * b + c) / sqrt(a * a + b * b), d1 = fabs(x * A + y * B + C) / sqrt(A * A + B * B);
  return d1 > d2 ? d1 : d2;
}

int main() {
  const int n = 60;
  const double f = 800, cx = 320, cy = 240, ang = 0.15, tx = -1.0, ty = 0.1, tz = 0.2;
  // F = K^-T [t]x R K^-1 for K = (f 0 cx; 0 f cy; 0 0 1), R a rotation about y
  const double R[9] = {cos(ang), 0, sin(ang), 0, 1, 0, -sin(ang), 0, cos(ang)};
  const double Tx[9] = {0, -tz, ty, tz, 0, -tx, -ty, tx, 0};
  double E[9], Ft[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) E[i * 3 + j] = Tx[i * 3] * R[j] + Tx[i * 3 + 1] * R[3 + j] + Tx[i * 3 + 2] * R[6 + j];
  const double Ki[9] = {1 / f, 0, -cx / f, 0, 1 / f, -cy / f, 0, 0, 1};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double v = 0;
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) v += Ki[a * 3 + i] * E[a * 3 + b] * Ki[b * 3 + j];
      Ft[i * 3 + j] = v;
    }
  std::vector<float> src(2 * n), dst(2 * n);
  std::vector<unsigned char> planted(n), mask(n, 9);
  unsigned lcg = 12345u;
  auto unit = [&]() {
    lcg = lcg * 1664525u + 1013904223u;
    return (lcg >> 8) / 16777216.0;
  };
  for (int i = 0; i < n; ++i) {
    const double X = -2 + 4 * unit(), Y = -1.5 + 3 * unit(), Z = 4 + 6 * unit();
    const double x = f * X / Z + cx, y = f * Y / Z + cy;
    const double Xc = R[0] * X + R[1] * Y + R[2] * Z + tx, Yc = R[3] * X + R[4] * Y + R[5] * Z + ty,
                 Zc = R[6] * X + R[7] * Y + R[8] * Z + tz;
    double u = f * Xc / Zc + cx, v = f * Yc / Zc + cy;
    planted[i] = i % 4 != 3;
    if (!planted[i]) {  // 120 px along the normal of the point's true epipolar line
      const double a = Ft[0] * x + Ft[1] * y + Ft[2], b = Ft[3] * x + Ft[4] * y + Ft[5], h = sqrt(a * a + b * b);
      u += 120 * a / h, v += 120 * b / h;
    }
    src[2 * i] = (float)x, src[2 * i + 1] = (float)y, dst[2 * i] = (float)u, dst[2 * i + 1] = (float)v;
  }

  double F[9];
  if (!sift::find_fundamental_ransac(src.data(), dst.data(), n, 3.0, 1000, 0.99, F, mask.data())) fail("no model");
  for (int i = 0; i < n; ++i) {
    if (mask[i] != planted[i]) fail("the mask is not the planted inlier set");
    if (planted[i] && !(epipolar(F, src[2 * i], src[2 * i + 1], dst[2 * i], dst[2 * i + 1]) < 3.0))
      fail("an inlier lies 3 px or more from its epipolar line");
  }
  double norm = 0;
  for (int k = 0; k < 9; ++k) norm += F[k] * F[k];
  const double det = F[0] * (F[4] * F[8] - F[5] * F[7]) - F[1] * (F[3] * F[8] - F[5] * F[6]) +
                     F[2] * (F[3] * F[7] - F[4] * F[6]);
  if (!(fabs(det) <= 1e-12 * norm * sqrt(norm))) fail("F is not of rank 2");

  // the first eight inliers: the direct fit
  std::vector<float> s8, d8;
  for (int i = 0; i < n && s8.size() < 16; ++i)
    if (planted[i]) {
      s8.insert(s8.end(), {src[2 * i], src[2 * i + 1]});
      d8.insert(d8.end(), {dst[2 * i], dst[2 * i + 1]});
    }
  unsigned char m8[8] = {0};
  double F8[9];
  if (!sift::find_fundamental_ransac(s8.data(), d8.data(), 8, 3.0, 1000, 0.99, F8, m8)) fail("no direct fit");
  for (int i = 0; i < 8; ++i)
    if (m8[i] != 1) fail("the direct fit's mask is not all ones");
  for (int k = 0; k < 9; ++k)
    if (!(fabs(F8[k]) <= 1e300)) fail("a non-finite direct fit");
  if (sift::find_fundamental_ransac(s8.data(), d8.data(), 7, 3.0, 1000, 0.99, F8, m8)) fail("a model from 7 pairs");
  s8[5] = NAN;
  if (sift::find_fundamental_ransac(s8.data(), d8.data(), 8, 3.0, 1000, 0.99, F8, m8)) fail("a model from a NaN row");
  printf("fundamental rule ok\n");
  return 0;
}
