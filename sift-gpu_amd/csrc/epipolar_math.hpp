// epipolar_math.hpp -- which cells of one grid row the epipolar band of a query
// can touch: the range computation of match_epipolar.hip's walk, stated once
// for the kernel and for tests/cpp/epipolar_cover.cpp.  Every function is
// __host__ __device__ and inline, in the manner of fundamental_math.hpp, whose
// is_inlier stays the one exact test: nothing here admits or rejects a row.  The
// range may only over-cover -- every candidate of it still takes the exact
// test -- so this file has one duty: a train point (X, Y) that passes the
// dst-side half of is_inlier for the line (a, b, c) must lie in a cell of the
// range returned for its grid row.
//
// The exact test, in float, unfused, left to right (u = 2^-24):
//   d = (X * a + Y * b) + c,  s = 1 / (a * a + b * b),  (d * d) * s <= t.
// Away from underflow and overflow, s is 1 / n2 within 3 roundings
// (n2 = a^2 + b^2 in reals) and the product adds 2, so a passing point has
// |d| <= sqrt(t n2) (1 + 2.6 u); and d differs from the real value
// D = aX + bY + c by at most 3.01 u (|aX| + |bY| + |c|) (three roundings on the
// products' path, one on c's).  With |aX| <= |D| + |bY| + |c| that gives
//   |D| (1 - 3.01 u) <= sqrt(t n2) (1 + 2.6 u) + 6.02 u (|bY| + |c|).
// The strip walked is |D| <= w with
//   w = (sqrt(tt n2) (1 + 2^-21) + 1e-18 + 2^-21 (|b| Ymax + |c|)) (1 + 2^-21),
// Ymax the slab's largest |Y|: 2^-21 = 8 u covers 6.02 u with 2 u to spare,
// which also pays for this file's own double roundings (2^-53 each) and for the
// final division by a.  The remaining cases, each made to over-cover:
//   * t = +inf (band = +inf, or a band whose square overflows float): every
//     non-NaN error passes, a = b = 0 included (c^2 * inf = inf <= inf), so
//     nothing is narrowed: kAll.
//   * d * d underflows below 2^-126 only for |d| < 2^-63 < 1e-18, the absolute
//     term of w; a product (d * d) * s in the subnormal range means a real
//     error below 1.2e-38, which tt = max(t, 1e-30) admits whatever t is.
//   * n2 outside [1e-30, 1e37] (a * a underflows or overflows in float, s is
//     inf, subnormal or 0): no claim is made, kAll.  n2 = 0 with a finite t is
//     the one exception: s = +inf, the error is +inf or NaN, no row passes:
//     kNone, as for a non-finite coefficient (a NaN or infinite a, b or c makes
//     d or s non-finite, and the error +inf or NaN).
//   * an infinite slab end (a border row: the binning clamps outside points
//     into it) with b != 0 makes w infinite: the whole row.
// The X range [lo / a, hi / a] is cast to float (round to nearest is monotone,
// and X is a float, so lo <= X implies (float)lo <= X) and then to cells by the
// binning's own monotone cell function, restated here for both sides.
//
// A grid row's Y slab: row cy holds the Y with floorf(Y * inv_cell) = cy after
// clamping, so an interior boundary cy / inv_cell is met within one rounding of
// the product (relative 2^-24); the slab is widened by 2^-22 of the boundary,
// and the border rows extend to -inf and +inf.
#pragma once

#include "fundamental_math.hpp"

namespace sift {
namespace emath {

constexpr double kRel = 1. / 2097152.;  // 2^-21, see the file comment
constexpr double kAbs = 1e-18;
constexpr double kSlab = 1. / 4194304.;  // 2^-22

// The binning's cell function (match_window.hpp's cell_of / cell_lo / cell_hi), for both sides.
SIFT_HD int cell_of(float v, float inv_cell, int n) {
  const float f = floorf(v * inv_cell);
  return (int)fminf(fmaxf(f, 0.f), (float)(n - 1));
}
SIFT_HD int cell_hi(float v, float inv_cell, int n) { return v != v ? n - 1 : cell_of(v, inv_cell, n); }

// The dst-side line of is_inlier for the query (x, y): its first statement.
SIFT_HD void dst_line(const float* f, float x, float y, float* l) {
  l[0] = f[0] * x + f[1] * y + f[2];
  l[1] = f[3] * x + f[4] * y + f[5];
  l[2] = f[6] * x + f[7] * y + f[8];
}

enum Kind { kNone = 0, kAll = 1, kStrip = 2 };

// One query's band: the line and the part of w that no slab changes.
struct Band {
  double a, b, c, w0;
  int kind;
};

SIFT_HD Band band_of(float a, float b, float c, float t) {
  Band B = {a, b, c, 0., kAll};
  if (!(t < INFINITY)) return B;  // +inf (or NaN): the exact test decides alone
  const bool finite = fabsf(a) <= FLT_MAX && fabsf(b) <= FLT_MAX && fabsf(c) <= FLT_MAX;
  const double n2 = B.a * B.a + B.b * B.b;
  if (!finite || n2 == 0.) {
    B.kind = kNone;
    return B;
  }
  if (!(n2 >= 1e-30 && n2 <= 1e37)) return B;
  const double tt = t > 1e-30f ? (double)t : 1e-30;
  B.w0 = sqrt(tt * n2) * (1. + kRel) + kAbs + kRel * fabs(B.c);
  B.kind = kStrip;
  return B;
}

// Grid row cy of ny: the closed Y interval that covers every point binned into it.
SIFT_HD void row_slab(int cy, int ny, float inv_cell, double* y0, double* y1) {
  *y0 = -INFINITY;
  *y1 = INFINITY;
  if (cy > 0) {
    const double v = (double)cy / (double)inv_cell;  // ny > 1: inv_cell > 0
    *y0 = v - kSlab * v;
  }
  if (cy < ny - 1) {
    const double v = (double)(cy + 1) / (double)inv_cell;
    *y1 = v + kSlab * v;
  }
}

// The cells [*cx0, *cx1] of a grid row of nx cells that a point of the slab
// y0 <= Y <= y1 (either end may be infinite) passing the exact test can lie in.
// false: none (an empty slab included).
SIFT_HD bool band_cells(const Band& B, double y0, double y1, float inv_cell, int nx, int* cx0, int* cx1) {
  *cx0 = 0;
  *cx1 = nx - 1;
  if (B.kind == kNone || !(y0 <= y1)) return false;
  if (B.kind == kAll) return true;
  double bmin = 0., bmax = 0., w = B.w0;
  if (B.b != 0.) {
    const double p = B.b * y0, q = B.b * y1, ymax = fmax(fabs(y0), fabs(y1));
    bmin = fmin(p, q);
    bmax = fmax(p, q);
    w = w + kRel * (fabs(B.b) * ymax);
  }
  w = w * (1. + kRel);
  if (!(w < INFINITY)) return true;  // a border row under a sloped line
  const double lo = (-w - B.c) - bmax, hi = (w - B.c) - bmin;  // lo <= a X <= hi
  if (B.a == 0.) return lo <= 0. && 0. <= hi;
  const double x0 = (B.a > 0. ? lo : hi) / B.a, x1 = (B.a > 0. ? hi : lo) / B.a;
  *cx0 = cell_of((float)x0, inv_cell, nx);
  *cx1 = cell_hi((float)x1, inv_cell, nx);
  return true;
}

}  // namespace emath
}  // namespace sift
