// The scratch layouts of the segmented homography (sift-gpu_amd/csrc/scratch.hpp:
// homog_layout, homog_host_layout) at their smallest and some odd counts,
// without a GPU: each piece starts on a 256-byte boundary, pieces are pairwise
// disjoint and lie inside the measured total, the measuring pass (null base)
// agrees with the pass on a real block, every field is the piece it should be
// and holds what the kernels index: kHomogRound subsets (4 rows each), models
// (9 doubles) and counts per segment, one state per segment, one mask byte per
// pair row.  The block is a heap allocation of exactly the measured size and
// every piece is written end to end, so an address sanitizer build also sees
// any piece that leaves it.
#include "layout_check.hpp"

// pieces first .. first + 4 are the device form's, sized for n_seg segments and m_cap rows
#define PARTS(s, first, n_seg, m_cap)                                                                           \
  do {                                                                                                          \
    const size_t jobs_ = (size_t)(n_seg) * kHomogRound;                                                         \
    AT((s).subsets, (first));                                                                                   \
    AT((s).models, (first) + 1);                                                                                \
    AT((s).counts, (first) + 2);                                                                                \
    AT((s).state, (first) + 3);                                                                                 \
    AT((s).mask, (first) + 4);                                                                                  \
    CHECK(a.pieces[(first)].bytes == jobs_ * 4 * sizeof(int), "subsets: 4 rows per hypothesis");                \
    CHECK(a.pieces[(first) + 1].bytes == jobs_ * 9 * sizeof(double), "models: 9 doubles per hypothesis");       \
    CHECK(a.pieces[(first) + 2].bytes == jobs_ * sizeof(int), "counts: one per hypothesis");                    \
    CHECK(a.pieces[(first) + 3].bytes == (size_t)(n_seg) * sizeof(HomogState), "one state per segment");        \
    CHECK(a.pieces[(first) + 4].bytes == (size_t)(m_cap), "one mask byte per pair row");                        \
  } while (0)

int main() {
  char what[160];
  static_assert(sizeof(HomogState) == 9 * sizeof(double) + 2 * sizeof(int), "HomogState has no padding");
  static_assert(kHomogRound == 64, "one wave solves a round's DLTs");
  for (int n_seg : {1, 3, 63, 300})
    for (int m_cap : {1, 4, 5, 257, 4099}) {
      snprintf(what, sizeof(what), "homog n_seg=%d m_cap=%d", n_seg, m_cap);
      run(what, 5, [&](Carver& a, char* base) {
        const HomogParts s = homog_layout(a, n_seg, m_cap);
        PARTS(s, 0, n_seg, m_cap);
      });
      run(what, 11, [&](Carver& a, char* base) {
        const HomogHost s = homog_host_layout(a, n_seg, m_cap);
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
        PARTS(s.parts, 6, n_seg, m_cap);
      });
    }
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("homography layouts ok\n");
  return 0;
}
