// undistort_math.hpp -- the arithmetic of sift_undistort[_batch_device] and
// sift_undistort_points[_segmented[_device]], stated once for the host
// (undistort.hip's point loop, the stand-alone tests/cpp/undistort_rule.cpp)
// and the kernels (undistort.hip).  Every function is __host__ __device__ and
// inline; the library is built -ffp-contract=off and double + - * /, rint and
// the float multiply and add are IEEE on gfx950 as on x86-64, so the same
// statement gives the same bits on either side.  There is no libm call.
//
// It is the library's own statement of
//     cv::undistort(src, dst, K, dist, newK)            INTER_LINEAR, BORDER_CONSTANT 0
//     cv::undistortPoints(src, dst, K, dist, noArray(), P)
// for OpenCV's 8-coefficient rational model, dist = (k1, k2, p1, p2, k3, k4, k5, k6)
// (restated in numpy in tests/undistort_oracle.py; written out in
// include/sift_hip.h).  The library's own rule, not bit-compatible with OpenCV
// (whose undistort goes through float maps and whose undistortPoints stops on a
// reprojection criterion): parity is by construction and unpinned.
//
// The inverse of a calibration is pose_math.hpp's invert3 (adj / det); the
// second half of a destination pixel (NaN -> 0, clamp, rint, the split into
// sample and fraction, samples outside are 0 and never read, the blends) is
// warp_math.hpp's, unchanged.
#pragma once

#include "pose_math.hpp"
#include "warp_math.hpp"

namespace sift {
namespace umath {

using pmath::finite_n;
using pmath::invert3;
using wmath::Coord;

// For normalised (x, y): the forward model's terms.
//   xx = x x, yy = y y, r2 = xx + yy
//   num = 1 + ((k3 r2 + k2) r2 + k1) r2,  den = 1 + ((k6 r2 + k5) r2 + k4) r2
//   dx = ((2 p1) x) y + p2 (r2 + 2 xx),  dy = p1 (r2 + 2 yy) + ((2 p2) x) y
struct Terms {
  double num, den, dx, dy;
};
SIFT_HD Terms terms(const double* d, double x, double y) {
  const double xx = x * x, yy = y * y, r2 = xx + yy;
  Terms t;
  t.num = 1.0 + ((d[4] * r2 + d[1]) * r2 + d[0]) * r2;
  t.den = 1.0 + ((d[7] * r2 + d[6]) * r2 + d[5]) * r2;
  t.dx = ((2.0 * d[2]) * x) * y + d[3] * (r2 + 2.0 * xx);
  t.dy = d[2] * (r2 + 2.0 * yy) + ((2.0 * d[3]) * x) * y;
  return t;
}

// Forward (distort): s = num / den, xd = x s + dx, yd = y s + dy.
SIFT_HD void distort(const double* d, double x, double y, double& xd, double& yd) {
  const Terms t = terms(d, x, y);
  const double s = t.num / t.den;
  xd = x * s + t.dx;
  yd = y * s + t.dy;
}

// (X, Y, W) = A (u, v, 1), each row (a u + b v) + c; the point is (X / W, Y / W).
SIFT_HD void project(const double* A, double u, double v, double& x, double& y) {
  const double X = (A[0] * u + A[1] * v) + A[2];
  const double Y = (A[3] * u + A[4] * v) + A[5];
  const double W = (A[6] * u + A[7] * v) + A[8];
  x = X / W;
  y = Y / W;
}

// ---- images ----
// What the pixels of an image share: newK^-1, K and the coefficients.
struct ImageCam {
  double Ni[9], K[9], d[8];
};
// false: the image undistorts to zeros -- K or newK singular or not finite, or a
// coefficient not finite (C is then unspecified).  newK may be null: K.
SIFT_HD bool image_camera(const double* K, const double* dist, const double* newK, ImageCam& C) {
  double Ki[9];
  if (!finite_n(K, 9) || !finite_n(dist, 8) || !invert3(K, Ki)) return false;
  if (newK) {
    if (!finite_n(newK, 9) || !invert3(newK, C.Ni)) return false;
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) C.Ni[i] = Ki[i];
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) C.K[i] = K[i];
#pragma unroll
  for (int i = 0; i < 8; ++i) C.d[i] = dist[i];
  return true;
}

// The source position of destination pixel (u, v):
//   (x, y) = project(newK^-1, u, v); (xd, yd) = distort(x, y);
//   Wd = (K6 xd + K7 yd) + K8
//   fX = (32 ((K0 xd + K1 yd) + K2)) / Wd,  fY = (32 ((K3 xd + K4 yd) + K5)) / Wd
// and from there warp_math.hpp's split_coord.
SIFT_HD Coord source_coord(const ImageCam& C, int u, int v) {
  double x, y, xd, yd;
  project(C.Ni, (double)u, (double)v, x, y);
  distort(C.d, x, y, xd, yd);
  const double Wd = (C.K[6] * xd + C.K[7] * yd) + C.K[8];
  const double fX = (32.0 * ((C.K[0] * xd + C.K[1] * yd) + C.K[2])) / Wd;
  const double fY = (32.0 * ((C.K[3] * xd + C.K[4] * yd) + C.K[5])) / Wd;
  return wmath::split_coord(fX, fY);
}

// A Coord in two ints: X = 32 sx + ax, Y = 32 sy + ay.  A pixel that is 0 (a NaN
// coordinate, a camera that undistorts to zeros) is (INT_MIN, INT_MIN): every
// sample then lies outside any image, is never read, and both blends of four
// zeros give the same +0 / 0 that the rule gives.
struct Packed {
  int X, Y;
};
SIFT_HD Packed pack(const Coord& c) {
  if (!c.valid) return {(int)0x80000000u, (int)0x80000000u};
  return {c.sx * 32 + c.ax, c.sy * 32 + c.ay};
}
SIFT_HD Coord unpack(const Packed& p) { return {p.X >> 5, p.Y >> 5, p.X & 31, p.Y & 31, true}; }

// ---- points ----
constexpr int kMaxIters = 100;

// What the rows of a segment share: K^-1, the coefficients and P.
struct PointCam {
  double Ki[9], d[8], P[9];
  int has_P;
};
// false: the segment's rows are zeros -- K singular or not finite, a
// coefficient or an entry of P not finite.  P may be null: the identity,
// which is not multiplied by.
SIFT_HD bool point_camera(const double* K, const double* dist, const double* P, PointCam& C) {
  if (!finite_n(K, 9) || !finite_n(dist, 8) || !invert3(K, C.Ki)) return false;
  if (P && !finite_n(P, 9)) return false;
#pragma unroll
  for (int i = 0; i < 8; ++i) C.d[i] = dist[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) C.P[i] = P ? P[i] : 0.0;
  C.has_P = P != nullptr;
  return true;
}

// One row: (x0, y0) = project(K^-1, u, v), x = x0, y = y0; iters times, with the
// terms taken at (x, y): icd = den / num, x = (x0 - dx) icd, y = (y0 - dy) icd;
// then project(P, x, y) where there is a P; then one rounding to float.
SIFT_HD void undistort_point(const PointCam& C, int iters, float u, float v, float& ou, float& ov) {
  double x0, y0;
  project(C.Ki, (double)u, (double)v, x0, y0);
  double x = x0, y = y0;
  for (int j = 0; j < iters; ++j) {
    const Terms t = terms(C.d, x, y);
    const double icd = t.den / t.num;
    x = (x0 - t.dx) * icd;
    y = (y0 - t.dy) * icd;
  }
  if (C.has_P) {
    double X, Y;
    project(C.P, x, y, X, Y);
    x = X;
    y = Y;
  }
  ou = (float)x;
  ov = (float)y;
}

SIFT_HD bool iters_ok(int iters) { return iters >= 0 && iters <= kMaxIters; }
SIFT_HD bool stride_ok(unsigned long long stride) { return stride >= 8 && stride % 4 == 0; }

}  // namespace umath
}  // namespace sift
