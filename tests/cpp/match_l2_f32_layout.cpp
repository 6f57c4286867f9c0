// The scratch layouts of the squared-L2 float matcher's entry points
// (sift-gpu_amd/csrc/scratch.hpp: seg_l2_f32_layout, seg_l2_f32_host_layout) at
// their smallest and degenerate counts, without a GPU, in the manner of
// match_l2_u8_layout.cpp: each piece starts on a 256-byte boundary, pieces are
// pairwise disjoint and lie inside the measured total, and the measuring pass
// (null base) agrees with the pass on a real block.  The block is a heap
// allocation of exactly the measured size and every piece is written end to
// end, so an address sanitizer build also sees any piece that leaves it.
#include "layout_check.hpp"

int main() {
  char what[160];
  for (int splits : {1, 4})
    for (int k : {1, 2})
      for (int t_cap : {0, 7, 65})
        for (bool t_off : {false, true})
          for (int n_seg : {1, 3})
            for (int q_cap : {1, 5, 257}) {
              snprintf(what, sizeof(what), "seg l2 f32 n_seg=%d q_cap=%d t_cap=%d t_off=%d k=%d splits=%d", n_seg,
                       q_cap, t_cap, t_off, k, splits);
              run(what, 5, [&](Carver& a, char* base) {
                const SegPartsL2F32 s = seg_l2_f32_layout(a, n_seg, q_cap, t_cap, splits);
                AT(s.tile_start, 0);
                AT(s.q_norm, 1);
                AT(s.t_norm, 2);
                AT(s.parts.dist, 3);
                AT(s.parts.idx, 4);
                CHECK(a.pieces[0].bytes == (size_t)(n_seg + 1) * 4, "one tile count per segment and the total");
                CHECK(a.pieces[1].bytes == (size_t)q_cap * 4, "one norm per query row");
                CHECK(a.pieces[2].bytes == (size_t)(t_cap + 64) * 4, "one norm per train row and a step of padding");
                CHECK(a.pieces[3].bytes == (splits > 1 ? (size_t)splits * q_cap * 8 : 0) &&
                          a.pieces[4].bytes == a.pieces[3].bytes,
                      "partials only above one split");
              });
              run(what, 11, [&](Carver& a, char* base) {
                const SegHostL2F32 s = seg_l2_f32_host_layout(a, n_seg, q_cap, t_cap, t_off, k, splits);
                AT(s.query, 0);
                AT(s.train, 1);
                AT(s.idx, 2);
                AT(s.dist, 3);
                AT(s.q_off, 4);
                if (t_off) AT(s.t_off, 5);
                CHECK(t_off || s.t_off == nullptr, "t_off without train offsets");
                AT(s.seg.tile_start, 6);
                AT(s.seg.q_norm, 7);
                AT(s.seg.t_norm, 8);
                AT(s.seg.parts.dist, 9);
                AT(s.seg.parts.idx, 10);
                CHECK(a.pieces[0].bytes == (size_t)q_cap * 512, "query rows are 512 bytes");
                CHECK(a.pieces[1].bytes == (size_t)(t_cap ? t_cap : 1) * 512, "train rows keep one element");
                CHECK(a.pieces[2].bytes == (size_t)q_cap * k * 4 && a.pieces[3].bytes == (size_t)q_cap * k * 4,
                      "results");
                CHECK(a.pieces[8].bytes == (size_t)(t_cap + 64) * 4, "train norms and their padding");
              });
            }
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("match l2 f32 layouts ok\n");
  return 0;
}
