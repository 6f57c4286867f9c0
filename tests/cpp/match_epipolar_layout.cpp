// The scratch layout of the epipolar matcher's host form and its search grid
// (sift-gpu_amd/csrc/scratch.hpp: epipolar_grid, epipolar_host_layout; the
// device form carves window_layout, which match_window_layout.cpp checks), in
// the manner of match_window_layout.cpp: each piece starts on a 256-byte
// boundary, pieces are pairwise disjoint and lie inside the measured total, the
// measuring pass agrees with the pass on a real block, and every piece is
// written end to end.  The grid: at least one cell, never more than the cap,
// one cell when radius and band are both +inf, a cell no narrower than the
// scaled min(radius, band) otherwise, and window_grid's own grid when the band
// is +inf and the scale 1.
#include <limits.h>
#include "layout_check.hpp"

int main() {
  char what[200];
  const float inf = HUGE_VALF;
  struct G { float radius; double band; int rows, cols, t_cap, n_grids; };
  const G grids[] = {{inf, 3., 1080, 1920, 13000 * 64, 64},   {128.f, 3., 1080, 1920, 13000 * 64, 64},
                     {128.f, 1., 1080, 1920, 13000 * 64, 64}, {inf, 8., 1080, 1920, 13000, 1},
                     {inf, HUGE_VAL, 1080, 1920, 13000, 1},   {2.f, 50., 64, 96, 700, 7},
                     {16.f, 3., 64, 96, 0, 1},                {16.f, 0., 64, 96, 1, 1},
                     {0.f, 0., 64, 96, 1, 40},                {1e-30f, 1e-300, 1, 1, 5, 1},
                     {0.f, 1e300, INT_MAX, INT_MAX, INT_MAX, 1}, {3e9f, 4e9, INT_MAX, INT_MAX, INT_MAX, 1},
                     {inf, 1., 1, INT_MAX, 1 << 20, 1},       {1.f, HUGE_VAL, INT_MAX, 1, 1 << 20, 3}};
  for (const G& g : grids) {
    snprintf(what, sizeof(what), "grid radius=%g band=%g rows=%d cols=%d t_cap=%d n_grids=%d", g.radius, g.band, g.rows,
             g.cols, g.t_cap, g.n_grids);
    const int cap = window_cell_cap(g.t_cap, g.n_grids);
    const WindowGrid w = epipolar_grid(g.radius, g.band, g.rows, g.cols, g.t_cap, g.n_grids);
    const double side = (g.band < g.radius ? g.band : (double)g.radius) * kEpipolarCellScale;
    CHECK(w.nx >= 1 && w.ny >= 1 && (long long)w.nx * w.ny <= cap, "%d x %d cells, cap %d", w.nx, w.ny, cap);
    CHECK(w.inv_cell >= 0.f && w.inv_cell <= 1.f, "cells are at least a pixel wide: 1 / side = %g", w.inv_cell);
    if (side > 2e9) CHECK(w.nx == 1 && w.ny == 1 && w.inv_cell == 0.f, "one cell");
    if (side >= 1. && side < 2e9)
      CHECK(1.f / w.inv_cell >= side * 0.999, "a cell is no narrower than min(radius, band): %g", 1.f / w.inv_cell);
    if (g.band == HUGE_VAL && kEpipolarCellScale == 1.) {
      const WindowGrid v = window_grid(g.radius, g.rows, g.cols, g.t_cap, g.n_grids);
      CHECK(v.nx == w.nx && v.ny == w.ny && v.inv_cell == w.inv_cell, "no band: the windowed matcher's grid");
    }
  }
  for (int t_cap : {0, 1, 7})
    for (int n_grids : {1, 3})
      for (int n_cells : {1, 4, kWindowMaxCells})
        for (size_t row : {(size_t)128, (size_t)512})
          for (int k : {1, 2})
            for (int opt = 0; opt < 8; ++opt)
              for (int q_cap : {1, 5}) {
                const bool t_off = opt & 1, has_F = opt & 2, has_found = opt & 4;
                const int n_seg = t_off ? n_grids : 2;
                snprintf(what, sizeof(what), "epipolar host t_cap=%d n_grids=%d n_cells=%d row=%zu k=%d opt=%d q_cap=%d",
                         t_cap, n_grids, n_cells, row, k, opt, q_cap);
                run(what, 13, [&](Carver& a, char* base) {
                  const EpipolarHost s = epipolar_host_layout(a, n_seg, q_cap, t_cap, row, t_off, has_F, has_found, k,
                                                              t_off ? n_grids : 1, n_cells);
                  AT(s.query, 0);
                  AT(s.train, 1);
                  AT(s.q_kpts, 2);
                  AT(s.t_kpts, 3);
                  AT(s.idx, 4);
                  AT(s.dist, 5);
                  AT(s.q_off, 6);
                  if (t_off) AT(s.t_off, 7);
                  if (has_F) AT(s.F, 8);
                  if (has_found) AT(s.found, 9);
                  CHECK((t_off || !s.t_off) && (has_F || !s.F) && (has_found || !s.found), "absent inputs are null");
                  AT(s.win.cell_end, 10);
                  AT(s.win.cell_rows, 11);
                  AT(s.win.cell_xy, 12);
                  CHECK(a.pieces[0].bytes == (size_t)q_cap * row && a.pieces[1].bytes == (size_t)(t_cap ? t_cap : 1) * row,
                        "rows of the metric's width, the train rows keep one element");
                  CHECK(a.pieces[2].bytes == (size_t)q_cap * 28 && a.pieces[3].bytes == (size_t)(t_cap ? t_cap : 1) * 28,
                        "keypoints are 28 bytes");
                  CHECK(a.pieces[4].bytes == (size_t)q_cap * k * 4 && a.pieces[5].bytes == a.pieces[4].bytes, "results");
                  CHECK(a.pieces[8].bytes == (size_t)n_seg * 72 && a.pieces[9].bytes == (size_t)n_seg * 4,
                        "F is nine doubles per segment, found one int");
                  // piece for piece the windowed matcher's host layout
                  Carver w(nullptr);
                  window_host_layout(w, n_seg, q_cap, t_cap, row, t_off, has_F, has_found, k, t_off ? n_grids : 1, n_cells);
                  CHECK(w.n_pieces == a.n_pieces && w.bytes() == a.bytes(), "the windowed matcher's layout");
                  for (int i = 0; i < w.n_pieces && i < a.n_pieces; ++i)
                    CHECK(w.pieces[i].off == a.pieces[i].off && w.pieces[i].bytes == a.pieces[i].bytes, "piece %d", i);
                });
              }
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("match epipolar layouts ok\n");
  return 0;
}
