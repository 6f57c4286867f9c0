// The scratch layouts of the 8-bit descriptor entry points
// (sift-gpu_amd/csrc/scratch.hpp: seg_u8_layout, seg_u8_host_layout,
// quant_u8_host_layout) at their smallest and degenerate counts, without a GPU,
// in the manner of scratch_layout.cpp: each piece starts on a 256-byte
// boundary, pieces are pairwise disjoint and lie inside the measured total, and
// the measuring pass (null base) agrees with the pass on a real block.  The
// block is a heap allocation of exactly the measured size and every piece is
// written end to end, so an address sanitizer build also sees any piece that
// leaves it.
#include "layout_check.hpp"

int main() {
  char what[160];
  for (int splits : {1, 4})
    for (int k : {1, 2})
      for (int t_cap : {0, 7})
        for (bool t_off : {false, true})
          for (int n_seg : {1, 3})
            for (int q_cap : {1, 5, 257}) {
              snprintf(what, sizeof(what), "seg u8 n_seg=%d q_cap=%d t_cap=%d t_off=%d k=%d splits=%d", n_seg, q_cap,
                       t_cap, t_off, k, splits);
              run(what, 3, [&](Carver& a, char* base) {
                const SegPartsU8 s = seg_u8_layout(a, n_seg, q_cap, splits);
                AT(s.tile_start, 0);
                AT(s.parts.dist, 1);
                AT(s.parts.idx, 2);
                CHECK(a.pieces[0].bytes == (size_t)(n_seg + 1) * 4, "one tile count per segment and the total");
                CHECK(a.pieces[1].bytes == (splits > 1 ? (size_t)splits * q_cap * 8 : 0) &&
                          a.pieces[2].bytes == a.pieces[1].bytes,
                      "partials only above one split");
              });
              run(what, 9, [&](Carver& a, char* base) {
                const SegHostU8 s = seg_u8_host_layout(a, n_seg, q_cap, t_cap, t_off, k, splits);
                AT(s.query, 0);
                AT(s.train, 1);
                AT(s.idx, 2);
                AT(s.dist, 3);
                AT(s.q_off, 4);
                if (t_off) AT(s.t_off, 5);
                CHECK(t_off || s.t_off == nullptr, "t_off without train offsets");
                AT(s.seg.tile_start, 6);
                AT(s.seg.parts.dist, 7);
                AT(s.seg.parts.idx, 8);
                CHECK(a.pieces[0].bytes == (size_t)q_cap * 128, "query rows are 128 bytes");
                CHECK(a.pieces[1].bytes == (size_t)(t_cap ? t_cap : 1) * 128, "train rows keep one element");
                CHECK(a.pieces[2].bytes == (size_t)q_cap * k * 4 && a.pieces[3].bytes == (size_t)q_cap * k * 4,
                      "results");
              });
            }
  for (int n : {1, 3}) {
    snprintf(what, sizeof(what), "quantiser n=%d", n);
    run(what, 2, [&](Carver& a, char* base) {
      const QuantHostU8 s = quant_u8_host_layout(a, n);
      AT(s.desc, 0);
      AT(s.out, 1);
      CHECK(a.pieces[0].bytes == (size_t)n * 512 && a.pieces[1].bytes == (size_t)n * 128, "float rows, byte rows");
    });
  }
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("match u8 layouts ok\n");
  return 0;
}
