// The scratch layouts of the cross-check entry points
// (sift-gpu_amd/csrc/scratch.hpp: cross_layout, cross_host_layout and the three
// cross_match_*_layout of the one-call form) over a sweep of capacities,
// without a GPU, in the manner of match_l2_u8_layout.cpp: each piece starts on
// a 256-byte boundary, pieces are pairwise disjoint and lie inside the
// measured total, and the measuring pass (null base) agrees with the pass on a
// real block.  The block is a heap allocation of exactly the measured size and
// every piece is written end to end, so an address sanitizer build also sees
// any piece that leaves it.  The one-call layouts must hold the matchers' own
// device layouts unchanged: each pass's pieces have the sizes that matcher's
// layout gives on its own.
#include "layout_check.hpp"

// Pieces [first, first + n) of a have the sizes of the pieces of a matcher layout carved on its own.
template <typename F>
static void same_sizes(const char* what, const Carver& a, int first, int n, F&& own) {
  Carver m(nullptr);
  own(m);
  CHECK(m.n_pieces == n, "the matcher's own layout has %d pieces, expected %d", m.n_pieces, n);
  for (int i = 0; i < n && i < m.n_pieces; ++i)
    CHECK(a.pieces[first + i].bytes == m.pieces[i].bytes, "piece %d: %zu bytes, the matcher's own %zu", first + i,
          a.pieces[first + i].bytes, m.pieces[i].bytes);
}

static void tables(const char* what, const Carver& a, char* base, const CrossTables& t, int q_cap, int t_cap, int k,
                   int blocks) {
  AT(t.idx, 0);
  AT(t.dist, 1);
  AT(t.ridx, 2);
  AT(t.rdist, 3);
  AT(t.blk_scan, 4);
  CHECK(a.pieces[0].bytes == (size_t)q_cap * k * 4 && a.pieces[1].bytes == a.pieces[0].bytes, "forward tables");
  CHECK(a.pieces[2].bytes == (size_t)(t_cap ? t_cap : 1) * 4 && a.pieces[3].bytes == a.pieces[2].bytes,
        "reverse tables keep one element");
  CHECK(a.pieces[4].bytes == (size_t)(blocks + 1) * 4, "one count per block and the total");
}

int main() {
  char what[200];
  for (int q_cap : {1, 255, 256, 257, 4097}) {
    const int blocks = (q_cap + 255) / 256;  // cross_check.hip's cross_blocks()
    snprintf(what, sizeof(what), "stage q_cap=%d", q_cap);
    run(what, 1, [&](Carver& a, char* base) {
      AT(cross_layout(a, blocks), 0);
      CHECK(a.pieces[0].bytes == (size_t)(blocks + 1) * 4, "one count per block and the total");
    });
    for (int t_cap : {0, 7, 300})
      for (int n_seg : {1, 3, 257})
        for (int fk : {1, 2}) {
          for (int rk : {1, 2})
            for (int m_cap : {0, 5, q_cap})
              for (bool pairs : {false, true}) {
                snprintf(what, sizeof(what), "host n_seg=%d q_cap=%d t_cap=%d fk=%d rk=%d m_cap=%d pairs=%d", n_seg,
                         q_cap, t_cap, fk, rk, m_cap, pairs);
                run(what, pairs ? 12 : 8, [&](Carver& a, char* base) {
                  const CrossHost s = cross_host_layout(a, n_seg, q_cap, fk, t_cap, rk, m_cap, pairs, blocks);
                  int i = 0;
                  AT(s.idx, i++);
                  AT(s.dist, i++);
                  AT(s.ridx, i++);
                  AT(s.q_off, i++);
                  AT(s.t_off, i++);
                  AT(s.m_off, i++);
                  if (pairs) {
                    AT(s.q_kpts, i++);
                    AT(s.t_kpts, i++);
                  }
                  AT(s.matches, i++);
                  if (pairs) {
                    AT(s.src_xy, i++);
                    AT(s.dst_xy, i++);
                  }
                  AT(s.blk_scan, i++);
                  CHECK(pairs || (!s.q_kpts && !s.t_kpts && !s.src_xy && !s.dst_xy), "pair buffers without pairs");
                  CHECK(a.pieces[0].bytes == (size_t)q_cap * fk * 4 && a.pieces[1].bytes == a.pieces[0].bytes,
                        "forward tables");
                  CHECK(a.pieces[2].bytes == (size_t)(t_cap ? t_cap : 1) * rk * 4, "reverse table keeps one row");
                  CHECK(a.pieces[3].bytes == (size_t)(n_seg + 1) * 4 && a.pieces[4].bytes == a.pieces[3].bytes &&
                            a.pieces[5].bytes == a.pieces[3].bytes,
                        "three offset arrays");
                  CHECK(a.pieces[pairs ? 8 : 6].bytes == (size_t)(m_cap ? m_cap : 1) * 16, "records keep one element");
                  if (pairs)
                    CHECK(a.pieces[6].bytes == (size_t)q_cap * 28 && a.pieces[7].bytes == (size_t)(t_cap ? t_cap : 1) * 28,
                          "keypoints");
                });
              }
          for (int fs : {1, 4})
            for (int rs : {1, 3}) {
              snprintf(what, sizeof(what), "one call n_seg=%d q_cap=%d t_cap=%d fk=%d splits=%d/%d", n_seg, q_cap,
                       t_cap, fk, fs, rs);
              run(what, 11, [&](Carver& a, char* base) {
                const CrossMatch<SegParts> s = cross_match_layout(a, n_seg, q_cap, t_cap, fk, fs, rs, blocks);
                tables(what, a, base, s.tab, q_cap, t_cap, fk, blocks);
                AT(s.fwd.tile_start, 5);
                AT(s.fwd.parts.dist, 6);
                AT(s.fwd.parts.idx, 7);
                AT(s.rev.tile_start, 8);
                AT(s.rev.parts.dist, 9);
                AT(s.rev.parts.idx, 10);
                same_sizes(what, a, 5, 3, [&](Carver& m) { seg_layout(m, n_seg, q_cap, fs); });
                same_sizes(what, a, 8, 3, [&](Carver& m) { seg_layout(m, n_seg, t_cap, rs); });
              });
              run(what, 11, [&](Carver& a, char* base) {
                const CrossMatch<SegPartsU8> s = cross_match_u8_layout(a, n_seg, q_cap, t_cap, fk, fs, rs, blocks);
                tables(what, a, base, s.tab, q_cap, t_cap, fk, blocks);
                AT(s.fwd.tile_start, 5);
                AT(s.fwd.parts.dist, 6);
                AT(s.fwd.parts.idx, 7);
                AT(s.rev.tile_start, 8);
                AT(s.rev.parts.dist, 9);
                AT(s.rev.parts.idx, 10);
                same_sizes(what, a, 5, 3, [&](Carver& m) { seg_u8_layout(m, n_seg, q_cap, fs); });
                same_sizes(what, a, 8, 3, [&](Carver& m) { seg_u8_layout(m, n_seg, t_cap, rs); });
              });
              run(what, 15, [&](Carver& a, char* base) {
                const CrossMatch<SegPartsL2U8> s =
                    cross_match_l2_u8_layout(a, n_seg, q_cap, t_cap, fk, fs, rs, blocks);
                tables(what, a, base, s.tab, q_cap, t_cap, fk, blocks);
                AT(s.fwd.tile_start, 5);
                AT(s.fwd.q_norm, 6);
                AT(s.fwd.t_norm, 7);
                AT(s.fwd.parts.dist, 8);
                AT(s.fwd.parts.idx, 9);
                AT(s.rev.tile_start, 10);
                AT(s.rev.q_norm, 11);
                AT(s.rev.t_norm, 12);
                AT(s.rev.parts.dist, 13);
                AT(s.rev.parts.idx, 14);
                same_sizes(what, a, 5, 5, [&](Carver& m) { seg_l2_u8_layout(m, n_seg, q_cap, t_cap, fs); });
                same_sizes(what, a, 10, 5, [&](Carver& m) { seg_l2_u8_layout(m, n_seg, t_cap, q_cap, rs); });
                CHECK(a.pieces[11].bytes == (size_t)t_cap * 4 && a.pieces[12].bytes == (size_t)(q_cap + 32) * 4,
                      "the reverse pass's norms have the capacities exchanged");
              });
            }
        }
  }
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("cross check layouts ok\n");
  return 0;
}
