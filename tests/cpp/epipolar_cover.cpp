// The one duty of sift-gpu_amd/csrc/epipolar_math.hpp, checked without a GPU: a
// train point that passes the exact float test for a line lies in a cell of
// the range band_cells returns for the point's grid row -- so the walk of
// match_epipolar.hip, which visits those cells only, can lose no admissible
// row.  Lines: horizontal, vertical, +-45 degrees, slopes 1e-6 and 1e6, one
// that misses the extent, one through a corner, c at 1e7, and seeded random
// ones; limits from band 0 to 1e4; grids from 1 x 1 to the cell cap; points on
// the band's two edges within a few float ulps (both sides), inside, far
// outside and at +-inf; the slab also intersected with a window's Y range, as
// the kernel does.  The whole of fmath::is_inlier is run as well, over random
// fundamental matrices, with the line from dst_line.  a = b = 0 and non-finite
// coefficients give an empty range at a finite limit; a +inf limit narrows
// nothing.  The binning's cell function is restated here.
#include <stdio.h>

#include <random>

#include "../../sift-gpu_amd/csrc/epipolar_math.hpp"

using namespace sift;

static int failures = 0;
static long long passed_points = 0, tested_points = 0;
#define CHECK(cond, ...)                \
  do {                                  \
    if (!(cond)) {                      \
      if (++failures <= 20) {           \
        printf("FAIL: ");               \
        printf(__VA_ARGS__);            \
        printf(" [%s]\n", #cond);       \
      }                                 \
    }                                   \
  } while (0)

// match_window.hpp's cell_of, as the binning applies it
static int bin_cell(float v, float inv_cell, int n) {
  const float f = floorf(v * inv_cell);
  return (int)fminf(fmaxf(f, 0.f), (float)(n - 1));
}

// the dst-side half of fmath::is_inlier, in its order
static bool dst_test(float a, float b, float c, float X, float Y, float t) {
  const float s_dst = 1.f / (a * a + b * b);
  const float d_dst = X * a + Y * b + c;
  return d_dst * d_dst * s_dst <= t;
}

struct Grid { int nx, ny; float inv_cell; };
static const Grid kGrids[] = {{1, 1, 0.f},          {2, 1, 1.f / 48.f},  {1, 2, 1.f / 32.f},   {6, 4, 1.f / 16.f},
                              {60, 34, 1.f / 32.f}, {64, 64, 1.f / 3.f}, {4096, 1, 1.f},       {1, 4096, 1.f},
                              {96, 42, 1.f / 20.273f}, {3, 3, 1.f / 1e6f}};

// One point against one line on every grid: if it passes, its cell is in its row's range.
static void cover(float a, float b, float c, float t, float X, float Y, bool passes) {
  ++tested_points;
  if (!passes) return;
  ++passed_points;
  const emath::Band B = emath::band_of(a, b, c, t);
  for (const Grid& g : kGrids) {
    const int cx = bin_cell(X, g.inv_cell, g.nx), cy = bin_cell(Y, g.inv_cell, g.ny);
    double y0, y1;
    emath::row_slab(cy, g.ny, g.inv_cell, &y0, &y1);
    CHECK(y0 <= (double)Y && (double)Y <= y1, "Y=%.9g is outside the slab [%.17g, %.17g] of row %d, grid %d x %d", Y,
          y0, y1, cy, g.nx, g.ny);
    for (int win = 0; win < 2; ++win) {
      double s0 = y0, s1 = y1;
      if (win) {  // a window's Y range that holds Y, as the kernel intersects it
        s0 = fmax(s0, (double)Y - 0.5);
        s1 = fmin(s1, (double)Y + 2.5);
      }
      int cx0 = -1, cx1 = -1;
      const bool any = emath::band_cells(B, s0, s1, g.inv_cell, g.nx, &cx0, &cx1);
      CHECK(any && cx0 <= cx && cx <= cx1 && cx0 >= 0 && cx1 < g.nx,
            "line (%.9g, %.9g, %.9g) t=%.9g point (%.9g, %.9g) cell %d of row %d, grid %d x %d win %d: range %s [%d, %d]",
            a, b, c, t, X, Y, cx, cy, g.nx, g.ny, win, any ? "" : "EMPTY", cx0, cx1);
    }
  }
}

static float nudge(float v, int ulps) {
  for (; ulps > 0; --ulps) v = nextafterf(v, INFINITY);
  for (; ulps < 0; ++ulps) v = nextafterf(v, -INFINITY);
  return v;
}

// Points around the line: on both edges of the band within a few ulps, inside, outside, at +-inf.
static void sweep_line(float a, float b, float c, float band, std::mt19937& rng) {
  const float t = (float)((double)band * band);
  const double n = sqrt((double)a * a + (double)b * b);
  std::uniform_real_distribution<double> U(-200., 2200.);
  const float inf = INFINITY;
  for (int i = 0; i < 400; ++i) {
    // a point of the line, solved for the axis the line crosses
    double X = U(rng), Y = U(rng);
    const double off = (i % 5 == 0 ? 0. : i % 5 == 1 ? band : i % 5 == 2 ? -(double)band : i % 5 == 3 ? 0.5 * band : 4. * band + 1.) * n;
    if (fabs(b) >= fabs(a))
      Y = (off - c - a * X) / b;
    else
      X = (off - c - b * Y) / a;
    for (int u = -3; u <= 3; ++u) {
      const float fx = fabs(b) >= fabs(a) ? (float)X : nudge((float)X, u);
      const float fy = fabs(b) >= fabs(a) ? nudge((float)Y, u) : (float)Y;
      cover(a, b, c, t, fx, fy, dst_test(a, b, c, fx, fy, t));
    }
  }
  const float far[][2] = {{inf, 10.f}, {-inf, 10.f}, {10.f, inf}, {10.f, -inf}, {inf, inf}, {-inf, inf},
                          {1e30f, -1e30f}, {-1e30f, 3.f}, {0.f, 0.f}, {-0.f, 1e-30f}, {1920.f, 1080.f}};
  for (const auto& p : far) cover(a, b, c, t, p[0], p[1], dst_test(a, b, c, p[0], p[1], t));
}

int main() {
  std::mt19937 rng(20240611);
  const float inf = INFINITY, nan = NAN;
  const float bands[] = {0.f, 1e-3f, 1.f, 3.f, 8.f, 1e4f};
  // crafted lines over a 1920 x 1080 extent: a X + b Y + c = 0
  const float lines[][3] = {{0.f, 1.f, -540.f},          // horizontal
                            {0.f, -2.5f, 100.f},
                            {1.f, 0.f, -960.f},          // vertical
                            {-3e-4f, 0.f, 0.25f},
                            {1.f, 1.f, -1500.f},         // -45 degrees
                            {1.f, -1.f, 0.f},            // +45 degrees, through the corner (0, 0)
                            {1e-6f, -1.f, 500.f},        // slope 1e-6
                            {1e6f, -1.f, -9e8f},         // slope 1e6
                            {1.f, 2.f, 50000.f},         // misses the extent
                            {-1080.f, -1920.f, 1080.f * 1920.f},  // through the corners (1920, 0) and (0, 1080)
                            {0.5f, 0.25f, 1e7f},         // c at 1e7
                            {3.f, -4.f, -1e7f},
                            {1e-12f, 1e-12f, -1e-9f},    // tiny coefficients: no claim, the whole row
                            {1e15f, -1e15f, 1e17f},
                            {1e19f, 1e19f, 0.f}};        // a * a overflows float: the whole row
  for (const auto& l : lines)
    for (float band : bands) sweep_line(l[0], l[1], l[2], band, rng);
  // seeded random lines through the extent, every direction
  std::uniform_real_distribution<double> ang(0., 6.283185307179586), px(0., 1920.), py(0., 1080.), mag(-6., 3.);
  for (int i = 0; i < 300; ++i) {
    const double th = ang(rng), m = pow(10., mag(rng)), x = px(rng), y = py(rng);
    const float a = (float)(m * cos(th)), b = (float)(m * sin(th)), c = (float)(-(m * cos(th) * x + m * sin(th) * y));
    sweep_line(a, b, c, bands[i % 6], rng);
  }
  CHECK(passed_points > 20000 && tested_points - passed_points > 20000, "the sweep has both kinds: %lld of %lld pass",
        passed_points, tested_points);

  // the whole of is_inlier over random fundamental matrices (rank 2 not needed for the claim)
  long long inliers = 0;
  std::uniform_real_distribution<double> cf(-1., 1.);
  for (int i = 0; i < 200; ++i) {
    double F[9];
    for (int k = 0; k < 9; ++k) F[k] = cf(rng) * (k % 3 == 2 || k >= 6 ? (k == 8 ? 100. : 1.) : 1e-3);
    float f[9], l[3];
    fmath::to_float9(F, f);
    const float x = (float)px(rng), y = (float)py(rng), t = 9.f;
    emath::dst_line(f, x, y, l);
    for (int j = 0; j < 400; ++j) {
      double X = px(rng), Y = py(rng);
      const double off = cf(rng) * 4. * sqrt((double)l[0] * l[0] + (double)l[1] * l[1]);
      if (fabs(l[1]) >= fabs(l[0]))
        Y = (off - l[2] - l[0] * X) / l[1];
      else
        X = (off - l[2] - l[1] * Y) / l[0];
      const bool in = fmath::is_inlier(f, x, y, (float)X, (float)Y, t);
      if (in) CHECK(dst_test(l[0], l[1], l[2], (float)X, (float)Y, t), "dst_line restates is_inlier's first line");
      inliers += in;
      cover(l[0], l[1], l[2], t, (float)X, (float)Y, in);
    }
  }
  CHECK(inliers > 1000, "is_inlier admitted %lld pairs", inliers);

  // nothing can pass: an empty range in every row; a +inf limit narrows nothing
  const float none[][3] = {{0.f, 0.f, 1.f},  {0.f, -0.f, 0.f}, {nan, 1.f, 0.f},  {1.f, nan, 0.f}, {1.f, 1.f, nan},
                           {inf, 1.f, 0.f},  {1.f, -inf, 0.f}, {1.f, 1.f, inf},  {inf, inf, inf}, {nan, nan, nan}};
  for (const auto& l : none)
    for (const Grid& g : kGrids) {
      const emath::Band B = emath::band_of(l[0], l[1], l[2], 9.f);
      CHECK(B.kind == emath::kNone, "(%g, %g, %g) is no line", l[0], l[1], l[2]);
      for (int cy = 0; cy < g.ny; cy += (g.ny > 8 ? g.ny / 8 : 1)) {
        double y0, y1;
        int cx0, cx1;
        emath::row_slab(cy, g.ny, g.inv_cell, &y0, &y1);
        CHECK(!emath::band_cells(B, y0, y1, g.inv_cell, g.nx, &cx0, &cx1), "(%g, %g, %g): row %d is not empty", l[0],
              l[1], l[2], cy);
      }
      // and indeed no point passes the exact test
      for (float X : {0.f, 1.f, -5.f, inf}) CHECK(!dst_test(l[0], l[1], l[2], X, 2.f, 9.f), "a point passed");
      const emath::Band A = emath::band_of(l[0], l[1], l[2], inf);
      int cx0, cx1;
      CHECK(A.kind == emath::kAll && emath::band_cells(A, -inf, inf, g.inv_cell, g.nx, &cx0, &cx1) && cx0 == 0 &&
                cx1 == g.nx - 1,
            "a +inf limit leaves the whole row");
    }
  {
    // an empty slab is empty; a horizontal line leaves rows far from it empty, and the rows it crosses whole
    const emath::Band B = emath::band_of(0.f, 1.f, -540.f, 9.f);
    int cx0, cx1;
    CHECK(!emath::band_cells(B, 5., 4., 1.f / 32.f, 60, &cx0, &cx1), "an inverted slab");
    CHECK(!emath::band_cells(B, 0., 500., 1.f / 32.f, 60, &cx0, &cx1), "a slab 37 px above the line");
    CHECK(emath::band_cells(B, 520., 545., 1.f / 32.f, 60, &cx0, &cx1) && cx0 == 0 && cx1 == 59, "the line's own row");
    // a vertical line: one or two cells in every row
    const emath::Band V = emath::band_of(1.f, 0.f, -960.f, 9.f);
    CHECK(emath::band_cells(V, -INFINITY, INFINITY, 1.f / 32.f, 60, &cx0, &cx1) && cx0 == 29 && cx1 == 30,
          "x = 960 +- 3 touches cells 29 and 30: [%d, %d]", cx0, cx1);
  }
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("epipolar cover ok: %lld of %lld points pass the exact test, %lld is_inlier pairs\n", passed_points,
         tested_points, inliers);
  return 0;
}
