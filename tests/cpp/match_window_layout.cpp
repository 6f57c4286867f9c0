// The scratch layouts of the windowed matcher's entry points
// (sift-gpu_amd/csrc/scratch.hpp: window_grid, window_layout,
// window_host_layout) at their smallest and degenerate counts, without a GPU,
// in the manner of match_u8_layout.cpp: each piece starts on a 256-byte
// boundary, pieces are pairwise disjoint and lie inside the measured total, and
// the measuring pass (null base) agrees with the pass on a real block.  The
// block is a heap allocation of exactly the measured size and every piece is
// written end to end, so an address sanitizer build also sees any piece that
// leaves it.  The search grid: at least one cell, never more than the cap, one
// cell for an infinite radius, a finite positive cell side otherwise.
#include <limits.h>
#include "layout_check.hpp"

int main() {
  char what[200];
  // ---- the search grid ----
  const float inf = HUGE_VALF;
  struct G { float radius; int rows, cols, t_cap, n_grids; };
  const G grids[] = {{32.f, 1080, 1920, 13000 * 64, 64}, {8.f, 1080, 1920, 13000 * 64, 64},
                     {128.f, 1080, 1920, 13000 * 64, 64}, {0.f, 1080, 1920, 13000, 1},
                     {inf, 1080, 1920, 13000, 1},          {16.f, 64, 96, 700, 7},
                     {16.f, 64, 96, 0, 1},                 {16.f, 64, 96, 1, 1},
                     {16.f, 64, 96, 1, 40},                {1e-30f, 1, 1, 5, 1},
                     {0.f, INT_MAX, INT_MAX, INT_MAX, 1},  {3e9f, INT_MAX, INT_MAX, INT_MAX, 1},
                     {1.f, 1, INT_MAX, 1 << 20, 1},        {1.f, INT_MAX, 1, 1 << 20, 3}};
  for (const G& g : grids) {
    snprintf(what, sizeof(what), "grid radius=%g rows=%d cols=%d t_cap=%d n_grids=%d", g.radius, g.rows, g.cols,
             g.t_cap, g.n_grids);
    const int cap = window_cell_cap(g.t_cap, g.n_grids);
    const WindowGrid w = window_grid(g.radius, g.rows, g.cols, g.t_cap, g.n_grids);
    CHECK(cap >= 1 && cap <= kWindowMaxCells, "cap %d", cap);
    CHECK(w.nx >= 1 && w.ny >= 1 && (long long)w.nx * w.ny <= cap, "%d x %d cells, cap %d", w.nx, w.ny, cap);
    CHECK(w.inv_cell >= 0.f && w.inv_cell <= 1.f, "cells are at least a pixel wide: 1 / side = %g", w.inv_cell);
    if (g.radius > 2e9f) CHECK(w.nx == 1 && w.ny == 1 && w.inv_cell == 0.f, "one cell");
    if (g.radius >= 1.f && g.radius < 2e9f)
      CHECK(1.f / w.inv_cell >= g.radius * 0.999f, "a cell is no narrower than the radius: %g", 1.f / w.inv_cell);
  }
  {
    snprintf(what, sizeof(what), "grid at 1080p");
    const WindowGrid w = window_grid(32.f, 1080, 1920, 13000 * 64, 64);
    CHECK(w.nx == 60 && w.ny == 34 && w.inv_cell == 1.f / 32.f, "radius 32 fits uncapped: %d x %d", w.nx, w.ny);
    CHECK(window_cell_cap(0, 1) == 1 && window_cell_cap(1, 1) == 4 && window_cell_cap(1, 40) == 4 &&
              window_cell_cap(1 << 20, 1) == kWindowMaxCells && window_cell_cap(INT_MAX, 1) == kWindowMaxCells,
          "the cap: four cells per row of an even share, at most kWindowMaxCells");
  }
  // ---- the layouts ----
  for (int t_cap : {0, 1, 7})
    for (int n_grids : {1, 3})
      for (int n_cells : {1, 4, kWindowMaxCells}) {
        snprintf(what, sizeof(what), "window t_cap=%d n_grids=%d n_cells=%d", t_cap, n_grids, n_cells);
        run(what, 3, [&](Carver& a, char* base) {
          const WindowParts s = window_layout(a, n_grids, n_cells, t_cap);
          AT(s.cell_end, 0);
          AT(s.cell_rows, 1);
          AT(s.cell_xy, 2);
          CHECK(a.pieces[0].bytes == (size_t)n_grids * (n_cells + 1) * 4, "a count per cell and a total, per grid");
          CHECK(a.pieces[1].bytes == (size_t)(t_cap ? t_cap : 1) * 4 && a.pieces[2].bytes == 2 * a.pieces[1].bytes,
                "one index and one position per train row, one element kept at t_cap 0");
        });
        for (size_t row : {(size_t)128, (size_t)512})
          for (int k : {1, 2})
            for (int opt = 0; opt < 8; ++opt)
              for (int q_cap : {1, 5}) {
                const bool t_off = opt & 1, has_H = opt & 2, has_found = opt & 4;
                const int n_seg = t_off ? n_grids : 2;
                snprintf(what, sizeof(what), "window host t_cap=%d n_grids=%d n_cells=%d row=%zu k=%d opt=%d q_cap=%d",
                         t_cap, n_grids, n_cells, row, k, opt, q_cap);
                run(what, 13, [&](Carver& a, char* base) {
                  const WindowHost s = window_host_layout(a, n_seg, q_cap, t_cap, row, t_off, has_H, has_found, k,
                                                          t_off ? n_grids : 1, n_cells);
                  AT(s.query, 0);
                  AT(s.train, 1);
                  AT(s.q_kpts, 2);
                  AT(s.t_kpts, 3);
                  AT(s.idx, 4);
                  AT(s.dist, 5);
                  AT(s.q_off, 6);
                  if (t_off) AT(s.t_off, 7);
                  if (has_H) AT(s.H, 8);
                  if (has_found) AT(s.found, 9);
                  CHECK((t_off || !s.t_off) && (has_H || !s.H) && (has_found || !s.found), "absent inputs are null");
                  AT(s.win.cell_end, 10);
                  AT(s.win.cell_rows, 11);
                  AT(s.win.cell_xy, 12);
                  CHECK(a.pieces[0].bytes == (size_t)q_cap * row && a.pieces[1].bytes == (size_t)(t_cap ? t_cap : 1) * row,
                        "rows of the metric's width, the train rows keep one element");
                  CHECK(a.pieces[2].bytes == (size_t)q_cap * 28 && a.pieces[3].bytes == (size_t)(t_cap ? t_cap : 1) * 28,
                        "keypoints are 28 bytes");
                  CHECK(a.pieces[4].bytes == (size_t)q_cap * k * 4 && a.pieces[5].bytes == a.pieces[4].bytes, "results");
                  CHECK(a.pieces[8].bytes == (size_t)n_seg * 72 && a.pieces[9].bytes == (size_t)n_seg * 4,
                        "H is nine doubles per segment, found one int");
                });
              }
      }
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("match window layouts ok\n");
  return 0;
}
