// The scratch layout of the segmented affine / similarity estimate
// (sift-gpu_amd/csrc/scratch.hpp: affine_host_layout) at its smallest and some
// odd counts, without a GPU: each piece starts on a 256-byte boundary, pieces
// are pairwise disjoint and lie inside the measured total, the measuring pass
// (null base) agrees with the pass on a real block, and every field is the
// piece it should be and holds what the host form stages: m_cap point pairs on
// either side, n_seg + 1 offsets, nine doubles and one flag per segment, one
// mask byte per pair row.  The device form carves nothing: a round's
// kAffineRound subsets and counts live in LDS.  The block is a heap allocation
// of exactly the measured size and every piece is written end to end, so an
// address sanitizer build also sees any piece that leaves it.
#include "layout_check.hpp"

int main() {
  char what[160];
  static_assert(kAffineRound % 64 == 0 && kAffineRound <= 1024, "a round is whole waves of one workgroup");
  for (int n_seg : {1, 3, 63, 300})
    for (int m_cap : {1, 2, 3, 257, 4099}) {
      snprintf(what, sizeof(what), "affine n_seg=%d m_cap=%d", n_seg, m_cap);
      run(what, 6, [&](Carver& a, char* base) {
        const AffineHost s = affine_host_layout(a, n_seg, m_cap);
        AT(s.src_xy, 0);
        AT(s.dst_xy, 1);
        AT(s.m_off, 2);
        AT(s.H, 3);
        AT(s.found, 4);
        AT(s.mask, 5);
        CHECK(a.pieces[0].bytes == (size_t)m_cap * 8 && a.pieces[1].bytes == (size_t)m_cap * 8, "xy rows");
        CHECK(a.pieces[2].bytes == (size_t)(n_seg + 1) * 4, "offsets");
        CHECK(a.pieces[3].bytes == (size_t)n_seg * 72 && a.pieces[4].bytes == (size_t)n_seg * 4, "H / found");
        CHECK(a.pieces[5].bytes == (size_t)m_cap, "staged mask");
      });
    }
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("affine layouts ok\n");
  return 0;
}
