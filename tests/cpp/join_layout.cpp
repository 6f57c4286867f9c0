// The scratch layouts of the match-join entry points
// (sift-gpu_amd/csrc/scratch.hpp: join_layout and join_host_layout) over a sweep
// of capacities, without a GPU, in the manner of cross_check_layout.cpp: each
// piece starts on a 256-byte boundary, pieces are pairwise disjoint and lie
// inside the measured total, and the measuring pass (null base) agrees with the
// pass on a real block.  The block is a heap allocation of exactly the measured
// size and every piece is written end to end, so an address sanitizer build
// also sees any piece that leaves it.  The host layout must hold the device
// layout unchanged, and a buffer the caller left out keeps its place and is null.
#include "layout_check.hpp"

static void parts(const char* what, const Carver& a, char* base, const JoinParts& p, int first, int n_seg, int key_cap,
                  int b_cap) {
  AT(p.lookup, first);
  AT(p.a_tiles, first + 1);
  AT(p.b_tiles, first + 2);
  AT(p.blk_scan, first + 3);
  CHECK(a.pieces[first].bytes == (size_t)(key_cap ? key_cap : 1) * 8, "one 64-bit entry per key, one kept");
  CHECK(a.pieces[first + 1].bytes == (size_t)(n_seg + 1) * 4 && a.pieces[first + 2].bytes == a.pieces[first + 1].bytes,
        "two tile tables");
  CHECK(a.pieces[first + 3].bytes == (size_t)(b_cap / 256 + n_seg + 1) * 4, "one count per block and the total");
}

int main() {
  char what[200];
  for (int n_seg : {1, 3, 257})
    for (int b_cap : {1, 255, 256, 257, 4097})
      for (int key_cap : {0, 7, 5000}) {
        snprintf(what, sizeof(what), "device n_seg=%d b_cap=%d key_cap=%d", n_seg, b_cap, key_cap);
        CHECK(join_max_tiles(b_cap, n_seg) == b_cap / kJoinRows + n_seg && kJoinRows == 256, "the grid's size");
        run(what, 4, [&](Carver& a, char* base) {
          parts(what, a, base, join_layout(a, n_seg, key_cap, b_cap), 0, n_seg, key_cap, b_cap);
        });
        for (int a_cap : {0, 300})
          for (int j_cap : {0, 5, b_cap})
            for (int mask = 0; mask < 4; ++mask) {
              // mask bit 0: the caller passes the masks and the gathered rows; bit 1: the row outputs
              const bool in = mask & 1, out = mask & 2;
              const JoinHostHas has{in, in, in, in, out, out, out, out, out};
              snprintf(what, sizeof(what), "host n_seg=%d a_cap=%d b_cap=%d key_cap=%d j_cap=%d in=%d out=%d", n_seg,
                       a_cap, b_cap, key_cap, j_cap, in, out);
              run(what, 19, [&](Carver& a, char* base) {
                const JoinHost s = join_host_layout(a, n_seg, a_cap, b_cap, key_cap, j_cap, has);
                const size_t na = a_cap ? a_cap : 1, nj = j_cap ? j_cap : 1, offs = (size_t)(n_seg + 1) * 4;
                AT(s.a, 0);
                AT(s.a_off, 1);
                AT(s.b, 4);
                AT(s.b_off, 5);
                AT(s.key_off, 8);
                AT(s.j_off, 14);
                if (in) {
                  AT(s.a_mask, 2);
                  AT(s.a_xyz, 3);
                  AT(s.b_mask, 6);
                  AT(s.b_xy, 7);
                } else {
                  CHECK(!s.a_mask && !s.a_xyz && !s.b_mask && !s.b_xy, "an input the caller left out is not null");
                }
                if (out) {
                  AT(s.xyz_out, 9);
                  AT(s.xy_out, 10);
                  AT(s.a_row, 11);
                  AT(s.b_row, 12);
                  AT(s.b_joined, 13);
                } else {
                  CHECK(!s.xyz_out && !s.xy_out && !s.a_row && !s.b_row && !s.b_joined,
                        "an output the caller left out is not null");
                }
                CHECK(a.pieces[0].bytes == na * 16 && a.pieces[4].bytes == (size_t)b_cap * 16, "records are 16 bytes");
                CHECK(a.pieces[1].bytes == offs && a.pieces[5].bytes == offs && a.pieces[8].bytes == offs &&
                          a.pieces[14].bytes == offs,
                      "four offset arrays");
                CHECK(a.pieces[2].bytes == na && a.pieces[3].bytes == na * 24, "A's mask and 3-D points");
                CHECK(a.pieces[6].bytes == (size_t)b_cap && a.pieces[7].bytes == (size_t)b_cap * 8, "B's mask and pixels");
                CHECK(a.pieces[9].bytes == nj * 24 && a.pieces[10].bytes == nj * 8 && a.pieces[11].bytes == nj * 4 &&
                          a.pieces[12].bytes == nj * 4,
                      "the joined rows keep one element");
                CHECK(a.pieces[13].bytes == (size_t)b_cap, "one byte per B row");
                parts(what, a, base, s.parts, 15, n_seg, key_cap, b_cap);
              });
            }
      }
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("join layouts ok\n");
  return 0;
}
