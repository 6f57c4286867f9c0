// scratch.hpp -- how the matcher, byte-matcher, windowed-matcher, epipolar-matcher, cross-check, front-end, segmented-homography and
// segmented-affine and match-join entry points divide the context's one scratch block (sift_ctx::d_match).  Each
// layout is described once, as a function of a Carver, and run twice: on a null
// base to measure the block, then on the block itself.  The four segmented
// matchers share one host and one cross-match layout, templates over a metric
// tag (L1F32, L1U8, L2SqrU8, L2SqrF32).  Plain host C++ (no HIP
// include), so that tests/cpp/scratch_layout.cpp, match_u8_layout.cpp,
// match_l2_u8_layout.cpp, match_l2_f32_layout.cpp, cross_check_layout.cpp, homography_layout.cpp, match_window_layout.cpp,
// match_epipolar_layout.cpp, affine_layout.cpp and join_layout.cpp check every layout without a GPU.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sift_hip.h"

namespace sift {

// Bump allocator over one block: every piece starts on a 256-byte boundary.
// On a null base it only measures (every pointer it returns is null).
class Carver {
 public:
  struct Piece { size_t off, bytes; };
  static constexpr size_t kAlign = 256;
  static constexpr int kMaxPieces = 24;
  Piece pieces[kMaxPieces] = {};  // what was taken so far, for the layout test
  int n_pieces = 0;

  explicit Carver(void* base) : base_(static_cast<char*>(base)) {}
  template <typename T>
  T* take(size_t count) {
    const size_t at = bytes();
    if (n_pieces < kMaxPieces) pieces[n_pieces++] = Piece{at, count * sizeof(T)};
    end_ = at + count * sizeof(T);
    return base_ ? reinterpret_cast<T*>(base_ + at) : nullptr;
  }
  template <typename T>
  T* take_if(bool keep, size_t count) {  // the place is taken either way; null unless keep
    T* p = take<T>(count);
    return keep ? p : nullptr;
  }
  size_t bytes() const { return (end_ + kAlign - 1) / kAlign * kAlign; }

 private:
  char* base_;
  size_t end_ = 0;
};

// A buffer the kernels index even when its count is 0 keeps one element.
inline size_t at_least_one(int n) { return n > 0 ? (size_t)n : 1; }

constexpr size_t kDescRow = 128;  // floats per descriptor (kDescLen)
struct Float2 { float x, y; };    // layout of HIP's float2 / int2
struct Int2 { int x, y; };

// Every layout below takes its pieces in member order (a braced list is
// evaluated left to right).

// Per-split partial results of one kNN launch.
struct KnnParts { Float2* dist; Int2* idx; };
inline KnnParts knn_parts(Carver& a, size_t n) { return {a.take<Float2>(n), a.take<Int2>(n)}; }

// sift_knn_match_l1_device: the partials of knn_splits() splits.
inline KnnParts knn_layout(Carver& a, int n_query, int splits) { return knn_parts(a, (size_t)splits * n_query); }

// sift_knn_match_l1: staged descriptors and results, then the partials.
struct KnnHost { float *query, *train; int* idx; float* dist; KnnParts parts; };
inline KnnHost knn_host_layout(Carver& a, int n_query, int n_train, int k, int splits) {
  return {a.take<float>((size_t)n_query * kDescRow), a.take<float>(at_least_one(n_train) * kDescRow),
          a.take<int>((size_t)n_query * k), a.take<float>((size_t)n_query * k), knn_layout(a, n_query, splits)};
}

// sift_knn_match_l1_segmented_device: the query-tile table, then the partials
// of knn_seg_splits() splits (none for one split).
struct SegParts { int* tile_start; KnnParts parts; };
inline SegParts seg_layout(Carver& a, int n_segments, int q_cap, int splits) {
  return {a.take<int>((size_t)n_segments + 1), knn_parts(a, splits > 1 ? (size_t)splits * q_cap : 0)};
}

// ---- 8-bit descriptors (match_u8.hip) ----
// A byte row is kDescRow bytes.  The matcher's query tile is 64 x Q rows, but a
// layout depends on it only through the split count the caller passes: the tile
// table has one entry per segment whatever the tile, and the partials one per
// (split, query row).  The partial distances are integers.
struct KnnPartsU8 { Int2* dist; Int2* idx; };

// sift_knn_match_l1_u8_segmented_device: the query-tile table, then the
// partials of knn_u8_seg_splits() splits (none for one split).
struct SegPartsU8 { int* tile_start; KnnPartsU8 parts; };
inline SegPartsU8 seg_u8_layout(Carver& a, int n_segments, int q_cap, int splits) {
  const size_t n = splits > 1 ? (size_t)splits * q_cap : 0;
  return {a.take<int>((size_t)n_segments + 1), {a.take<Int2>(n), a.take<Int2>(n)}};
}

// ---- squared L2 on 8-bit descriptors (match_l2_u8.hip) ----
// sift_knn_match_l2sqr_u8_segmented_device: the query-tile table, one int per
// row for the squared norms of the biased rows -- every query row, every train
// row and kL2PadRows zero entries after them, which a tile at the end of the
// train buffer reads and masks -- then the integer partials of
// knn_l2_u8_seg_splits() splits (none for one split).
constexpr int kL2PadRows = 32;  // common.hpp's kL2NormPad
struct SegPartsL2U8 { int* tile_start; int *q_norm, *t_norm; KnnPartsU8 parts; };
inline SegPartsL2U8 seg_l2_u8_layout(Carver& a, int n_segments, int q_cap, int t_cap, int splits) {
  const size_t n = splits > 1 ? (size_t)splits * q_cap : 0;
  return {a.take<int>((size_t)n_segments + 1), a.take<int>((size_t)q_cap), a.take<int>((size_t)t_cap + kL2PadRows),
          {a.take<Int2>(n), a.take<Int2>(n)}};
}

// ---- squared L2 on float descriptors (match_l2_f32.hip) ----
// sift_knn_match_l2sqr_f32_segmented_device: the query-tile table, one float per
// row for chain(x, x) -- every query row, every train row and kL2F32PadRows
// entries after them, which a step at the end of the train buffer reads and
// masks -- then the float partials of knn_l2_f32_seg_splits() splits (none for
// one split).
constexpr int kL2F32PadRows = 64;  // common.hpp's kL2F32NormPad
struct SegPartsL2F32 { int* tile_start; float *q_norm, *t_norm; KnnParts parts; };
inline SegPartsL2F32 seg_l2_f32_layout(Carver& a, int n_segments, int q_cap, int t_cap, int splits) {
  return {a.take<int>((size_t)n_segments + 1), a.take<float>((size_t)q_cap),
          a.take<float>((size_t)t_cap + kL2F32PadRows), knn_parts(a, splits > 1 ? (size_t)splits * q_cap : 0)};
}

// ---- one description of the four segmented matchers' scratch ----
// What a layout needs of a metric: the element type of a descriptor row and the
// device form's pieces (the L1 forms ignore t_cap).  apps.hip adds the stage,
// the split count and the launcher to each.
struct L1F32 {
  using Row = float; using Seg = SegParts;
  static Seg layout(Carver& a, int n, int q_cap, int, int splits) { return seg_layout(a, n, q_cap, splits); }
};
struct L1U8 {
  using Row = uint8_t; using Seg = SegPartsU8;
  static Seg layout(Carver& a, int n, int q_cap, int, int splits) { return seg_u8_layout(a, n, q_cap, splits); }
};
struct L2SqrU8 {
  using Row = uint8_t; using Seg = SegPartsL2U8;
  static Seg layout(Carver& a, int n, int q_cap, int t_cap, int s) { return seg_l2_u8_layout(a, n, q_cap, t_cap, s); }
};
struct L2SqrF32 {
  using Row = float; using Seg = SegPartsL2F32;
  static Seg layout(Carver& a, int n, int q_cap, int t_cap, int s) { return seg_l2_f32_layout(a, n, q_cap, t_cap, s); }
};

// The host form of a segmented matcher, and the one-segment byte forms
// (sift_knn_match_l1_u8, _l2sqr_u8, _l2sqr_f32: one segment over a shared train set, the
// library writes q_off itself): the staged rows, results and offsets -- t_off
// keeps its place when the caller has no train offsets, and is null then --
// then the device form's pieces.
template <typename M>
struct SegHostOf { typename M::Row *query, *train; int* idx; float* dist; int *q_off, *t_off; typename M::Seg seg; };
template <typename M>
SegHostOf<M> seg_host_layout_of(Carver& a, int n_segments, int q_cap, int t_cap, bool has_t_off, int k, int splits) {
  using Row = typename M::Row;
  return {a.take<Row>((size_t)q_cap * kDescRow), a.take<Row>(at_least_one(t_cap) * kDescRow),
          a.take<int>((size_t)q_cap * k),        a.take<float>((size_t)q_cap * k),
          a.take<int>((size_t)n_segments + 1),   a.take_if<int>(has_t_off, (size_t)n_segments + 1),
          M::layout(a, n_segments, q_cap, t_cap, splits)};
}
using SegHost = SegHostOf<L1F32>;  // the names the layout tests use
using SegHostU8 = SegHostOf<L1U8>;
using SegHostL2U8 = SegHostOf<L2SqrU8>;
using SegHostL2F32 = SegHostOf<L2SqrF32>;
constexpr auto seg_host_layout = seg_host_layout_of<L1F32>;
constexpr auto seg_u8_host_layout = seg_host_layout_of<L1U8>;
constexpr auto seg_l2_u8_host_layout = seg_host_layout_of<L2SqrU8>;
constexpr auto seg_l2_f32_host_layout = seg_host_layout_of<L2SqrF32>;

// sift_descriptors_to_u8: the staged float rows, then the byte rows.
struct QuantHostU8 { float* desc; uint8_t* out; };
inline QuantHostU8 quant_u8_host_layout(Carver& a, int n) {
  return {a.take<float>((size_t)n * kDescRow), a.take<uint8_t>((size_t)n * kDescRow)};
}

// sift_ratio_matches_device: the block scan of ratio_blocks() blocks.
inline int* ratio_layout(Carver& a, int blocks) { return a.take<int>((size_t)blocks + 1); }

// sift_ratio_matches: the staged kNN results and offsets, the keypoints and
// point pairs only when the caller asks for pairs, the records, the block scan.
struct RatioHost {
  int* idx; float* dist; int *q_off, *t_off, *m_off; sift_keypoint *q_kpts, *t_kpts; sift_match* matches;
  float *src_xy, *dst_xy; int* blk_scan;
};
inline RatioHost ratio_host_layout(Carver& a, int n_segments, int q_cap, int t_cap, int m_cap, bool pairs,
                                   bool has_t_off, int blocks) {
  const size_t offs = (size_t)n_segments + 1, m = at_least_one(m_cap);
  return {a.take<int>((size_t)q_cap * 2), a.take<float>((size_t)q_cap * 2), a.take<int>(offs),
          a.take_if<int>(has_t_off, offs), a.take<int>(offs),
          pairs ? a.take<sift_keypoint>((size_t)q_cap) : nullptr,
          pairs ? a.take<sift_keypoint>(at_least_one(t_cap)) : nullptr, a.take<sift_match>(m),
          pairs ? a.take<float>(m * 2) : nullptr, pairs ? a.take<float>(m * 2) : nullptr, ratio_layout(a, blocks)};
}

// ---- cross-check (cross_check.hip) ----
// sift_cross_check_matches_device: the block scan of cross_blocks() blocks.
inline int* cross_layout(Carver& a, int blocks) { return a.take<int>((size_t)blocks + 1); }

// sift_cross_check_matches: the staged forward ([q_cap][fwd_k]) and reverse
// ([t_cap][rev_k]) results and the three offset arrays, the keypoints and point
// pairs only when the caller asks for pairs, the records, the block scan.
struct CrossHost {
  int* idx; float* dist; int* ridx; int *q_off, *t_off, *m_off; sift_keypoint *q_kpts, *t_kpts; sift_match* matches;
  float *src_xy, *dst_xy; int* blk_scan;
};
inline CrossHost cross_host_layout(Carver& a, int n_segments, int q_cap, int fwd_k, int t_cap, int rev_k, int m_cap,
                                   bool pairs, int blocks) {
  const size_t offs = (size_t)n_segments + 1, m = at_least_one(m_cap);
  return {a.take<int>((size_t)q_cap * fwd_k), a.take<float>((size_t)q_cap * fwd_k),
          a.take<int>(at_least_one(t_cap) * rev_k), a.take<int>(offs), a.take<int>(offs), a.take<int>(offs),
          pairs ? a.take<sift_keypoint>((size_t)q_cap) : nullptr,
          pairs ? a.take<sift_keypoint>(at_least_one(t_cap)) : nullptr, a.take<sift_match>(m),
          pairs ? a.take<float>(m * 2) : nullptr, pairs ? a.take<float>(m * 2) : nullptr, cross_layout(a, blocks)};
}

// sift_cross_match_segmented_device: the forward ([q_cap][fwd_k]) and reverse
// ([t_cap][1]) tables -- rdist only takes the distances the reverse pass writes,
// nothing reads it -- and the stage's block scan, then the scratch of the
// forward and of the reverse matcher pass, each that matcher's own device
// layout (the reverse pass has the capacities exchanged).  The whole block is
// measured and grown before the first enqueue, so neither pass can move a table
// under a kernel that is already in the stream.  The two passes' pieces are not
// aliased (15 pieces at most, the squared-L2 form).
struct CrossTables { int* idx; float* dist; int* ridx; float* rdist; int* blk_scan; };
inline CrossTables cross_tables(Carver& a, int q_cap, int fwd_k, int t_cap, int blocks) {
  return {a.take<int>((size_t)q_cap * fwd_k), a.take<float>((size_t)q_cap * fwd_k), a.take<int>(at_least_one(t_cap)),
          a.take<float>(at_least_one(t_cap)), cross_layout(a, blocks)};
}
template <typename Parts>
struct CrossMatch { CrossTables tab; Parts fwd, rev; };
template <typename M>
CrossMatch<typename M::Seg> cross_match_layout_of(Carver& a, int n_segments, int q_cap, int t_cap, int fwd_k,
                                                  int fwd_splits, int rev_splits, int blocks) {
  return {cross_tables(a, q_cap, fwd_k, t_cap, blocks), M::layout(a, n_segments, q_cap, t_cap, fwd_splits),
          M::layout(a, n_segments, t_cap, q_cap, rev_splits)};
}
constexpr auto cross_match_layout = cross_match_layout_of<L1F32>;
constexpr auto cross_match_u8_layout = cross_match_layout_of<L1U8>;
constexpr auto cross_match_l2_u8_layout = cross_match_layout_of<L2SqrU8>;

// ---- spatially gated matching (match_window.hip) ----
// The search grid of sift_knn_match_window_segmented_device, from host
// arguments only: square cells of side max(radius, 1 px), grown until one grid
// has at most window_cell_cap() cells -- kWindowMaxCells, and no more than four
// per train row of an even share of the buffer (finer cells than that hold
// nothing).  radius = +inf is one cell.  The extent rows x cols is a hint: the
// kernels clamp every point to the border cells, and no result depends on the
// grid's shape.
constexpr int kWindowMaxCells = 4096;
struct WindowGrid { int nx, ny; float inv_cell; };
inline int window_cell_cap(int t_cap, int n_grids) {
  const long long per = ((long long)t_cap + n_grids - 1) / n_grids * 4;
  return per < 1 ? 1 : (per > kWindowMaxCells ? kWindowMaxCells : (int)per);
}
inline WindowGrid window_grid(float radius, int rows, int cols, int t_cap, int n_grids) {
  const double cap = window_cell_cap(t_cap, n_grids);
  double cell = radius > 1.f ? (double)radius : 1.;
  if (cell > 2e9) return {1, 1, 0.f};  // wider than any extent, +inf included
  for (;; cell *= 1.125) {
    const double nx = ceil(cols / cell), ny = ceil(rows / cell);
    if (nx * ny <= cap) return {(int)nx, (int)ny, (float)(1. / cell)};
  }
}

// sift_knn_match_window_segmented_device: per grid (one per train segment, one
// in all for a shared train set) the scanned cell counts and their total, then
// the local train indices and the positions in cell order, one per train row.
struct WindowParts { int* cell_end; int* cell_rows; Float2* cell_xy; };
inline WindowParts window_layout(Carver& a, int n_grids, int n_cells, int t_cap) {
  return {a.take<int>((size_t)n_grids * ((size_t)n_cells + 1)), a.take<int>(at_least_one(t_cap)),
          a.take<Float2>(at_least_one(t_cap))};
}

// sift_knn_match_window_segmented: the staged rows (row_bytes each: 512 for
// float rows, 128 for byte rows), keypoints, results and offsets -- t_off, H
// and found keep their places when the caller has none, and are null then --
// then the device form's pieces.
struct WindowHost {
  uint8_t *query, *train; sift_keypoint *q_kpts, *t_kpts; int* idx; float* dist; int *q_off, *t_off; double* H;
  int* found; WindowParts win;
};
inline WindowHost window_host_layout(Carver& a, int n_segments, int q_cap, int t_cap, size_t row_bytes, bool has_t_off,
                                     bool has_H, bool has_found, int k, int n_grids, int n_cells) {
  return {a.take<uint8_t>((size_t)q_cap * row_bytes), a.take<uint8_t>(at_least_one(t_cap) * row_bytes),
          a.take<sift_keypoint>((size_t)q_cap), a.take<sift_keypoint>(at_least_one(t_cap)),
          a.take<int>((size_t)q_cap * k), a.take<float>((size_t)q_cap * k), a.take<int>((size_t)n_segments + 1),
          a.take_if<int>(has_t_off, (size_t)n_segments + 1), a.take_if<double>(has_H, (size_t)n_segments * 9),
          a.take_if<int>(has_found, (size_t)n_segments), window_layout(a, n_grids, n_cells, t_cap)};
}

// ---- matching along epipolar lines (match_epipolar.hip) ----
// The search grid of sift_knn_match_epipolar_segmented_device, under
// window_grid's cell cap: square cells of side kEpipolarCellScale x
// max(min(radius, band), 1 px), grown until one grid fits the cap.  The walk
// visits the cells of a strip 2 band wide inside a window 2 radius wide, so the
// narrower of the two sets the useful cell side; the scale is the A/B of
// profiles/match_epipolar_ab.txt.  Both +inf is one cell.  No result depends on
// the grid's shape.
#ifndef SIFT_EPIPOLAR_CELL_SCALE
#define SIFT_EPIPOLAR_CELL_SCALE 1
#endif
constexpr double kEpipolarCellScale = SIFT_EPIPOLAR_CELL_SCALE;
inline WindowGrid epipolar_grid(float radius, double band, int rows, int cols, int t_cap, int n_grids) {
  const double cap = window_cell_cap(t_cap, n_grids);
  double cell = band < (double)radius ? band : (double)radius;
  cell = (cell > 1. ? cell : 1.) * kEpipolarCellScale;
  if (!(cell <= 2e9)) return {1, 1, 0.f};  // wider than any extent, +inf included
  for (;; cell *= 1.125) {
    const double nx = ceil(cols / cell), ny = ceil(rows / cell);
    if (nx * ny <= cap) return {(int)nx, (int)ny, (float)(1. / cell)};
  }
}

// sift_knn_match_epipolar_segmented_device carves window_layout.
// sift_knn_match_epipolar_segmented: the windowed matcher's host layout with F
// ([n_segments][9] doubles) in H's place.
struct EpipolarHost {
  uint8_t *query, *train; sift_keypoint *q_kpts, *t_kpts; int* idx; float* dist; int *q_off, *t_off; double* F;
  int* found; WindowParts win;
};
inline EpipolarHost epipolar_host_layout(Carver& a, int n_segments, int q_cap, int t_cap, size_t row_bytes,
                                         bool has_t_off, bool has_F, bool has_found, int k, int n_grids, int n_cells) {
  return {a.take<uint8_t>((size_t)q_cap * row_bytes), a.take<uint8_t>(at_least_one(t_cap) * row_bytes),
          a.take<sift_keypoint>((size_t)q_cap), a.take<sift_keypoint>(at_least_one(t_cap)),
          a.take<int>((size_t)q_cap * k), a.take<float>((size_t)q_cap * k), a.take<int>((size_t)n_segments + 1),
          a.take_if<int>(has_t_off, (size_t)n_segments + 1), a.take_if<double>(has_F, (size_t)n_segments * 9),
          a.take_if<int>(has_found, (size_t)n_segments), window_layout(a, n_grids, n_cells, t_cap)};
}

// sift_bgr8_to_gray: the strided source rows, then the packed gray image.
struct BgrHost { uint8_t* src; float* gray; };
inline BgrHost bgr_host_layout(Carver& a, int rows, size_t row_stride, int out_rows, int out_cols) {
  return {a.take<uint8_t>((size_t)rows * row_stride), a.take<float>((size_t)out_rows * out_cols)};
}

// sift_upsample2x: the strided source rows (in floats), then the packed doubled image.
struct UpsampleHost { float* src; float* dst; };
inline UpsampleHost upsample_host_layout(Carver& a, int rows, int cols, size_t row_stride) {
  return {a.take<float>((size_t)rows * row_stride), a.take<float>((size_t)4 * rows * cols)};
}

// sift_warp_perspective: the strided source rows (in bytes), the homography, then the packed warped image.
struct WarpHost { uint8_t* src; double* H; uint8_t* dst; };
inline WarpHost warp_host_layout(Carver& a, int rows, size_t row_stride, int out_rows, size_t out_row_bytes) {
  return {a.take<uint8_t>((size_t)rows * row_stride), a.take<double>(9), a.take<uint8_t>((size_t)out_rows * out_row_bytes)};
}

// sift_find_homography_segmented_device (homography_batch.hip): per segment one
// round of kHomogRound hypotheses -- the accepted 4-point subsets, their models
// and inlier counts (-1: no model) -- then the state the RANSAC kernel hands to
// the refinement kernel, and the best hypothesis's inlier mask by pair row.
constexpr int kHomogRound = 64;
struct HomogState { double best[9]; int found, max_good; };
struct HomogParts { int* subsets; double* models; int* counts; HomogState* state; unsigned char* mask; };
inline HomogParts homog_layout(Carver& a, int n_segments, int m_cap) {
  const size_t jobs = (size_t)n_segments * kHomogRound;
  return {a.take<int>(jobs * 4), a.take<double>(jobs * 9), a.take<int>(jobs), a.take<HomogState>((size_t)n_segments),
          a.take<unsigned char>((size_t)m_cap)};
}

// sift_find_homography_segmented: the staged point pairs and offsets, the
// staged results, then the device form's pieces.
struct HomogHost {
  float *src_xy, *dst_xy; int* m_off; double* H; int* found; unsigned char* mask; HomogParts parts;
};
inline HomogHost homog_host_layout(Carver& a, int n_segments, int m_cap) {
  return {a.take<float>((size_t)m_cap * 2), a.take<float>((size_t)m_cap * 2), a.take<int>((size_t)n_segments + 1),
          a.take<double>((size_t)n_segments * 9), a.take<int>((size_t)n_segments),
          a.take<unsigned char>((size_t)m_cap), homog_layout(a, n_segments, m_cap)};
}

// ---- affine / similarity estimation (affine_batch.hip) ----
// sift_estimate_affine_segmented_device: a round is kAffineRound hypotheses, one
// per thread of the segment's workgroup.  A round's subsets and inlier counts
// live in LDS, the hypotheses in registers, and the kernel's tail takes the
// best hypothesis's mask again from its model, so the device form carves
// nothing from the block.
constexpr int kAffineRound = 128;

// sift_estimate_affine_segmented: the staged point pairs and offsets, then the
// staged results.
struct AffineHost { float *src_xy, *dst_xy; int* m_off; double* H; int* found; unsigned char* mask; };
inline AffineHost affine_host_layout(Carver& a, int n_segments, int m_cap) {
  return {a.take<float>((size_t)m_cap * 2), a.take<float>((size_t)m_cap * 2), a.take<int>((size_t)n_segments + 1),
          a.take<double>((size_t)n_segments * 9), a.take<int>((size_t)n_segments),
          a.take<unsigned char>((size_t)m_cap)};
}

// ---- fundamental matrix estimation (fundamental_batch.hip) ----
// sift_find_fundamental_segmented_device: a round is kFundRound hypotheses, one
// normalised 8-point solve per thread of the segment's workgroup.  A round's
// subsets (8 rows each) and inlier counts live in LDS beside the refit's 64 x 45
// terms (33 KB in all), the hypotheses in registers, so the device form
// carves nothing from the block.  256 by the A/B of
// profiles/fundamental_batch_ab.txt (64, 128, 256).
constexpr int kFundRound = 256;

// sift_find_fundamental_segmented stages what sift_estimate_affine_segmented
// stages (pairs, offsets, nine doubles and a flag per segment, the mask):
// affine_host_layout is its layout too.

// ---- relative pose and triangulation (pose_batch.hip) ----
// sift_recover_pose_segmented_device and sift_triangulate_points_segmented_device
// carve nothing: a segment's decomposition and its four counts live in LDS.
// sift_recover_pose_segmented stages the estimate's layout (pairs, offsets, F in
// H, found, the mask read), then the calibrations and the results.
struct PoseHost {
  AffineHost in; double *K_src, *K_dst, *pose, *E; int *pose_found, *n_good; unsigned char* mask_out; double* xyz;
};
inline PoseHost pose_host_layout(Carver& a, int n_segments, int m_cap, int k_per_segment) {
  const size_t ks = k_per_segment ? (size_t)n_segments * 9 : 9;
  return {affine_host_layout(a, n_segments, m_cap), a.take<double>(ks), a.take<double>(ks),
          a.take<double>((size_t)n_segments * 12), a.take<double>((size_t)n_segments * 9),
          a.take<int>((size_t)n_segments), a.take<int>((size_t)n_segments), a.take<unsigned char>((size_t)m_cap),
          a.take<double>((size_t)m_cap * 3)};
}

// ---- absolute pose from 3-D / 2-D rows (pnp_batch.hip) ----
// sift_solve_pnp_segmented_device carves nothing: a round is kPnpRound
// hypotheses, one P3P solve per thread of the segment's workgroup; a round's
// subsets (4 rows each) and inlier counts live in LDS beside the refit's 64 x 28
// terms (20 KB in all), the hypotheses in registers.
#ifndef SIFT_PNP_ROUND
#define SIFT_PNP_ROUND 256
#endif
constexpr int kPnpRound = SIFT_PNP_ROUND;
// sift_solve_pnp_segmented stages the rows read (3-D points, pixels, the row
// mask), the offsets and the calibrations, then the results.
struct PnpHost {
  double* xyz; float* xy; int* m_off; unsigned char* row_mask; double *K, *pose; int *found, *n_inliers;
  unsigned char* mask;
};
inline PnpHost pnp_host_layout(Carver& a, int n_segments, int m_cap, int k_per_segment) {
  return {a.take<double>((size_t)m_cap * 3), a.take<float>((size_t)m_cap * 2), a.take<int>((size_t)n_segments + 1),
          a.take<unsigned char>((size_t)m_cap), a.take<double>(k_per_segment ? (size_t)n_segments * 9 : 9),
          a.take<double>((size_t)n_segments * 12), a.take<int>((size_t)n_segments), a.take<int>((size_t)n_segments),
          a.take<unsigned char>((size_t)m_cap)};
}

// ---- the join of two match tables on a shared keypoint (join.hip) ----
// The stage walks each table in blocks of kJoinRows rows that never span two
// segments, so a block has one segment and one key slice: tile tables like the
// matchers' (entry s = the blocks of the segments before s, entry n_segments =
// all of them), one per table.  join_max_tiles() is the most blocks a table's
// capacity allows when its segments do not overlap, and the size of the grid.
// sift_join_matches_segmented_device: the lookup (one uint64 per key of the
// shared views, all ones = no winner), the two tile tables, then the block scan
// of the B table's join_max_tiles() blocks.
constexpr int kJoinRows = 256;
inline int join_max_tiles(int cap, int n_segments) { return cap / kJoinRows + n_segments; }
struct JoinParts { uint64_t* lookup; int *a_tiles, *b_tiles, *blk_scan; };
inline JoinParts join_layout(Carver& a, int n_segments, int key_cap, int b_cap) {
  const size_t offs = (size_t)n_segments + 1;
  return {a.take<uint64_t>(at_least_one(key_cap)), a.take<int>(offs), a.take<int>(offs),
          a.take<int>((size_t)join_max_tiles(b_cap, n_segments) + 1)};
}

// sift_join_matches_segmented: the staged tables (records, offsets, mask, the
// rows gathered from: 3-D points of A, pixels of B), the key offsets and the
// staged results, then the device form's pieces.  A buffer the caller left out
// keeps its place and is null.
struct JoinHost {
  sift_match* a; int* a_off; unsigned char* a_mask; double* a_xyz;
  sift_match* b; int* b_off; unsigned char* b_mask; float* b_xy; int* key_off;
  double* xyz_out; float* xy_out; int *a_row, *b_row; unsigned char* b_joined; int* j_off; JoinParts parts;
};
struct JoinHostHas { bool a_mask, a_xyz, b_mask, b_xy, xyz_out, xy_out, a_row, b_row, b_joined; };
inline JoinHost join_host_layout(Carver& a, int n_segments, int a_cap, int b_cap, int key_cap, int j_cap,
                                 const JoinHostHas& has) {
  const size_t offs = (size_t)n_segments + 1, na = at_least_one(a_cap), nb = at_least_one(b_cap),
               nj = at_least_one(j_cap);
  return {a.take<sift_match>(na), a.take<int>(offs), a.take_if<unsigned char>(has.a_mask, na),
          a.take_if<double>(has.a_xyz, na * 3), a.take<sift_match>(nb), a.take<int>(offs),
          a.take_if<unsigned char>(has.b_mask, nb), a.take_if<float>(has.b_xy, nb * 2), a.take<int>(offs),
          a.take_if<double>(has.xyz_out, nj * 3), a.take_if<float>(has.xy_out, nj * 2), a.take_if<int>(has.a_row, nj),
          a.take_if<int>(has.b_row, nj), a.take_if<unsigned char>(has.b_joined, nb), a.take<int>(offs),
          join_layout(a, n_segments, key_cap, b_cap)};
}

// ---- lens undistortion (undistort.hip) ----
// The device forms carve nothing.  sift_undistort stages one image, its camera
// (K, the eight coefficients, newK) and the result; sift_undistort_points_segmented
// the rows read and written (xy_stride bytes each), the offsets, the cameras and the flags.
struct UndistortHost { uint8_t* src; double *K, *dist, *newK; uint8_t* dst; };
inline UndistortHost undistort_host_layout(Carver& a, int rows, size_t row_stride, int out_rows, size_t out_row_bytes) {
  return {a.take<uint8_t>((size_t)rows * row_stride), a.take<double>(9), a.take<double>(8), a.take<double>(9),
          a.take<uint8_t>((size_t)out_rows * out_row_bytes)};
}
struct UndistortPtsHost { float *src, *dst; int* m_off; double *K, *dist, *P; int* ok; };
inline UndistortPtsHost undistort_pts_host_layout(Carver& a, int n_segments, int m_cap, size_t stride,
                                                  int k_per_segment) {
  const size_t cams = k_per_segment ? (size_t)n_segments : 1, row_floats = stride / sizeof(float);
  return {a.take<float>((size_t)m_cap * row_floats), a.take<float>((size_t)m_cap * row_floats),
          a.take<int>((size_t)n_segments + 1), a.take<double>(cams * 9), a.take<double>(cams * 8),
          a.take<double>(cams * 9), a.take<int>((size_t)n_segments)};
}

}  // namespace sift
