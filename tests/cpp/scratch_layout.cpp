// Every scratch layout of sift-gpu_amd/csrc/scratch.hpp at its smallest and
// degenerate counts, without a GPU: each piece starts on a 256-byte boundary,
// pieces are pairwise disjoint and lie inside the measured total, and the
// measuring pass (null base) agrees with the pass on a real block.  The block
// is a heap allocation of exactly the measured size and every piece is written
// end to end, so an address sanitizer build also sees any piece that leaves it.
#include "layout_check.hpp"

int main() {
  char what[160];
  for (int splits : {1, 3})
    for (int k : {1, 2})
      for (int nt : {0, 1, 5}) {
        snprintf(what, sizeof(what), "knn nq=1 nt=%d k=%d splits=%d", nt, k, splits);
        run(what, 2, [&](Carver& a, char* base) {
          const KnnParts s = knn_layout(a, 1, splits);
          AT(s.dist, 0);
          AT(s.idx, 1);
          CHECK(a.pieces[0].bytes == (size_t)splits * 8 && a.pieces[1].bytes == (size_t)splits * 8, "partials");
        });
        run(what, 6, [&](Carver& a, char* base) {
          const KnnHost s = knn_host_layout(a, 1, nt, k, splits);
          AT(s.query, 0);
          AT(s.train, 1);
          AT(s.idx, 2);
          AT(s.dist, 3);
          AT(s.parts.dist, 4);
          AT(s.parts.idx, 5);
          CHECK(a.pieces[1].bytes == (size_t)(nt ? nt : 1) * 512, "train rows keep one element");
        });
      }
  for (int splits : {1, 4})
    for (int k : {1, 2})
      for (int t_cap : {0, 7})
        for (bool t_off : {false, true})
          for (int n_seg : {1, 3}) {
            snprintf(what, sizeof(what), "seg n_seg=%d q_cap=5 t_cap=%d t_off=%d k=%d splits=%d", n_seg, t_cap, t_off, k,
                     splits);
            run(what, 3, [&](Carver& a, char* base) {
              const SegParts s = seg_layout(a, n_seg, 5, splits);
              AT(s.tile_start, 0);
              AT(s.parts.dist, 1);
              AT(s.parts.idx, 2);
              CHECK(a.pieces[1].bytes == (splits > 1 ? (size_t)splits * 5 * 8 : 0), "partials only above one split");
            });
            run(what, 9, [&](Carver& a, char* base) {
              const SegHost s = seg_host_layout(a, n_seg, 5, t_cap, t_off, k, splits);
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
            });
          }
  for (bool pairs : {false, true})
    for (bool t_off : {false, true})
      for (int m_cap : {0, 6})
        for (int t_cap : {0, 4}) {
          snprintf(what, sizeof(what), "ratio q_cap=3 t_cap=%d m_cap=%d pairs=%d t_off=%d", t_cap, m_cap, pairs, t_off);
          run(what, 1, [&](Carver& a, char* base) { AT(ratio_layout(a, 2), 0); });
          run(what, pairs ? 11 : 7, [&](Carver& a, char* base) {
            const RatioHost s = ratio_host_layout(a, 2, 3, t_cap, m_cap, pairs, t_off, 2);
            int i = 0;
            AT(s.idx, i++);
            AT(s.dist, i++);
            AT(s.q_off, i++);
            if (t_off) AT(s.t_off, i);
            CHECK(t_off || s.t_off == nullptr, "t_off without train offsets");
            ++i;
            AT(s.m_off, i++);
            if (pairs) {
              AT(s.q_kpts, i++);
              AT(s.t_kpts, i++);
            }
            AT(s.matches, i++);
            CHECK(a.pieces[i - 1].bytes == (size_t)(m_cap ? m_cap : 1) * sizeof(sift_match), "records keep one element");
            if (pairs) {
              AT(s.src_xy, i++);
              AT(s.dst_xy, i++);
            }
            CHECK(pairs || (!s.q_kpts && !s.t_kpts && !s.src_xy && !s.dst_xy), "pair buffers without keypoints");
            AT(s.blk_scan, i++);
          });
        }
  for (size_t stride : {(size_t)3, (size_t)300}) {
    snprintf(what, sizeof(what), "bgr 1x1 -> 1x1 stride=%zu", stride);
    run(what, 2, [&](Carver& a, char* base) {
      const BgrHost s = bgr_host_layout(a, 1, stride, 1, 1);
      AT(s.src, 0);
      AT(s.gray, 1);
    });
  }
  if (failures) return printf("%d checks failed\n", failures), 1;
  printf("scratch layouts ok\n");
  return 0;
}
