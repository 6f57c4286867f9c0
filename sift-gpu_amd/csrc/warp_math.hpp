// warp_math.hpp -- the arithmetic of sift_warp_perspective[_segmented_device],
// stated once for the host (apps.hip's absent-segment check, the stand-alone
// tests/cpp/warp_rule.cpp) and the kernel (warp.hip).  Every function is
// __host__ __device__ and inline; the library is built -ffp-contract=off and
// double + - * /, rint and the float multiply and add are IEEE on gfx950 as on
// x86-64, so the same statement gives the same bits on either side.
//
// It is the library's own statement of
//     cv::warpPerspective(src, dst, H, dsize, INTER_LINEAR [| WARP_INVERSE_MAP],
//                         BORDER_CONSTANT, 0)
// (restated in numpy in tests/warp_inputs.py).  Parity against OpenCV itself is
// by construction and unpinned, exactly as for sift_upsample2x and the
// homography: no OpenCV here.  The rule is written out in include/sift_hip.h.
#pragma once

#include <float.h>
#include <math.h>

#if defined(__HIPCC__)
#define SIFT_WARP_HD __host__ __device__ inline
#define SIFT_WARP_UNROLL _Pragma("unroll")
#else
#define SIFT_WARP_HD inline
#define SIFT_WARP_UNROLL
#endif

namespace sift {
namespace wmath {

SIFT_WARP_HD bool finite(double v) { return fabs(v) <= DBL_MAX; }  // false for NaN and infinities

SIFT_WARP_HD bool finite9(const double* a) {
  bool ok = true;
  SIFT_WARP_UNROLL
  for (int i = 0; i < 9; ++i) ok = ok && finite(a[i]);
  return ok;
}

// The matrix M that maps a destination pixel to its source position.
// inverse_map: M = H.  Otherwise M = adj(H) * (1 / det(H)): det by cofactors
// along row 0, the nine cofactors in this order, each entry one multiply by the
// reciprocal.  false: the segment warps to nothing (a non-finite entry of H or
// of M, det zero or non-finite) and M is nine zeros.
SIFT_WARP_HD bool warp_matrix(const double* H, bool inverse_map, double* M) {
  bool ok = finite9(H);
  if (inverse_map) {
  SIFT_WARP_UNROLL
    for (int i = 0; i < 9; ++i) M[i] = H[i];
  } else {
    const double c0 = H[4] * H[8] - H[5] * H[7];
    const double c1 = H[5] * H[6] - H[3] * H[8];
    const double c2 = H[3] * H[7] - H[4] * H[6];
    const double det = (H[0] * c0 + H[1] * c1) + H[2] * c2;
    const double r = 1.0 / det;
    M[0] = c0 * r;
    M[1] = (H[2] * H[7] - H[1] * H[8]) * r;
    M[2] = (H[1] * H[5] - H[2] * H[4]) * r;
    M[3] = c1 * r;
    M[4] = (H[0] * H[8] - H[2] * H[6]) * r;
    M[5] = (H[2] * H[3] - H[0] * H[5]) * r;
    M[6] = c2 * r;
    M[7] = (H[1] * H[6] - H[0] * H[7]) * r;
    M[8] = (H[0] * H[4] - H[1] * H[3]) * r;
    ok = ok && det != 0.0 && finite(det) && finite9(M);
  }
  if (!ok) {
  SIFT_WARP_UNROLL
    for (int i = 0; i < 9; ++i) M[i] = 0.0;
  }
  return ok;
}

// The terms of a destination row y that do not depend on x.
struct RowTerms {
  double m1y, m4y, m7y;
};
SIFT_WARP_HD RowTerms row_terms(const double* M, int y) {
  const double yd = (double)y;
  return {M[1] * yd, M[4] * yd, M[7] * yd};
}

// The source position of destination pixel (x, y) in 1/32 pixel units, split
// into the sample (sx, sy) and the fractions (ax, ay) in 0..31.
struct Coord {
  int sx, sy, ax, ay;
  bool valid;  // false: a NaN coordinate, the pixel is 0
};
SIFT_WARP_HD double clamp_int(double v) {
  return v < -2147483648.0 ? -2147483648.0 : (v > 2147483647.0 ? 2147483647.0 : v);
}
// (fX, fY) in 1/32 pixel units to a Coord: the half sift_undistort* shares (undistort_math.hpp).
SIFT_WARP_HD Coord split_coord(double fX, double fY) {
  Coord c{0, 0, 0, 0, !(fX != fX || fY != fY)};
  if (c.valid) {
    const int X = (int)rint(clamp_int(fX)), Y = (int)rint(clamp_int(fY));  // ties to even
    c.sx = X >> 5;  // arithmetic shifts
    c.ax = X & 31;
    c.sy = Y >> 5;
    c.ay = Y & 31;
  }
  return c;
}
SIFT_WARP_HD Coord source_coord(const double* M, const RowTerms& R, int x) {
  const double xd = (double)x;
  const double Wd = (M[6] * xd + R.m7y) + M[8];
  const double W = Wd != 0.0 ? 32.0 / Wd : 0.0;
  const double fX = ((M[0] * xd + R.m1y) + M[2]) * W;
  const double fY = ((M[3] * xd + R.m4y) + M[5]) * W;
  return split_coord(fX, fY);
}

// A sample outside [0, rows) x [0, cols) is the value 0 and is never read.
SIFT_WARP_HD bool inside(int sy, int sx, int rows, int cols) {
  return sy >= 0 && sy < rows && sx >= 0 && sx < cols;
}

// Four multiplies and three adds in this order, never fused; the weights are
// exact multiples of 1/1024.  A NaN or infinite sample propagates at weight 0.
SIFT_WARP_HD float blend_f32(float v00, float v01, float v10, float v11, int ax, int ay) {
  const float fx = (float)ax * 0.03125f, fy = (float)ay * 0.03125f;
  const float w00 = (1.f - fy) * (1.f - fx), w01 = (1.f - fy) * fx, w10 = fy * (1.f - fx), w11 = fy * fx;
  return ((v00 * w00 + v01 * w01) + v10 * w10) + v11 * w11;
}

// OpenCV's 15-bit coefficient table with the common factor 32 taken out.
SIFT_WARP_HD unsigned char blend_u8(int v00, int v01, int v10, int v11, int ax, int ay) {
  const int k00 = (32 - ay) * (32 - ax), k01 = (32 - ay) * ax, k10 = ay * (32 - ax), k11 = ay * ax;
  return (unsigned char)((v00 * k00 + v01 * k01 + v10 * k10 + v11 * k11 + 512) >> 10);
}

// One destination pixel of an f32 image; S rows are pitch bytes apart.
SIFT_WARP_HD float pixel_f32(const unsigned char* S, int rows, int cols, long long pitch, const Coord& c) {
  if (!c.valid) return 0.f;
  const long long o = (long long)c.sy * pitch + (long long)c.sx * 4;
  const float v00 = inside(c.sy, c.sx, rows, cols) ? *reinterpret_cast<const float*>(S + o) : 0.f;
  const float v01 = inside(c.sy, c.sx + 1, rows, cols) ? *reinterpret_cast<const float*>(S + o + 4) : 0.f;
  const float v10 = inside(c.sy + 1, c.sx, rows, cols) ? *reinterpret_cast<const float*>(S + o + pitch) : 0.f;
  const float v11 = inside(c.sy + 1, c.sx + 1, rows, cols) ? *reinterpret_cast<const float*>(S + o + pitch + 4) : 0.f;
  return blend_f32(v00, v01, v10, v11, c.ax, c.ay);
}

// One destination pixel of a u8 image of CH interleaved channels, each channel alone.
template <int CH>
SIFT_WARP_HD void pixel_u8(const unsigned char* S, int rows, int cols, long long pitch, const Coord& c,
                           unsigned char* out) {
  const bool i00 = c.valid && inside(c.sy, c.sx, rows, cols), i01 = c.valid && inside(c.sy, c.sx + 1, rows, cols);
  const bool i10 = c.valid && inside(c.sy + 1, c.sx, rows, cols), i11 = c.valid && inside(c.sy + 1, c.sx + 1, rows, cols);
  const long long o = (long long)c.sy * pitch + (long long)c.sx * CH;
  SIFT_WARP_UNROLL
  for (int k = 0; k < CH; ++k) {
    const int v00 = i00 ? S[o + k] : 0, v01 = i01 ? S[o + CH + k] : 0;
    const int v10 = i10 ? S[o + pitch + k] : 0, v11 = i11 ? S[o + pitch + CH + k] : 0;
    out[k] = c.valid ? blend_u8(v00, v01, v10, v11, c.ax, c.ay) : (unsigned char)0;
  }
}

}  // namespace wmath
}  // namespace sift
