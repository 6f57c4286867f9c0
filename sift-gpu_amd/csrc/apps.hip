// apps.hip -- the application stages behind the C ABI (include/sift_hip.h):
// the L1 kNN matcher, the byte quantiser, the four segmented matchers (float
// L1, byte L1, byte squared L2, float squared L2), the windowed and the epipolar matcher, the ratio test with
// point pairs, the cross-check stage with its one-call form, the BGR8 front
// end and the doubled image, each in a device and a host form, the one-pair
// homography wrappers, the segmented homography and corner transform, the
// affine / similarity estimate and the fundamental matrix (each one pair set
// and segmented; fundamental.hip, fundamental_batch.hip), and the
// perspective warp of a batch, and the join of two match tables (join.hip, join_rule.hpp).  Host code only; the kernels live in match.hip,
// match_u8.hip, match_l2_u8.hip, match_l2_f32.hip, match_window.hip, match_epipolar.hip, cross_check.hip,
// frontend.hip, upsample.hip, homography_batch.hip, affine_batch.hip and warp.hip (the one-pair
// homography and affine estimate are host code in homography.hip and affine.hip).  The segmented matchers are one path, written once as
// function templates over a metric tag (MatchL1F32, MatchL1U8, MatchL2SqrU8, MatchL2SqrF32);
// their extern "C" entry points only forward.  Every form carves its scratch
// from the context's one block by a layout of scratch.hpp.
#include <cstring>

#include "ctx.hpp"
#include "join_rule.hpp"
#include "scratch.hpp"
#include "undistort_math.hpp"
#include "warp_math.hpp"

using namespace sift;

namespace {

static_assert(kDescRow == kDescLen && sizeof(Float2) == sizeof(float2) && sizeof(Int2) == sizeof(int2) &&
                  kL2PadRows == kL2NormPad && kL2F32PadRows == kL2F32NormPad,
              "scratch.hpp restates these without the HIP headers");
float2* dev(Float2* p) { return reinterpret_cast<float2*>(p); }
int2* dev(Int2* p) { return reinterpret_cast<int2*>(p); }

// Runs layout(Carver&) twice: on a null base to size the scratch block, then
// on the block itself.
template <typename S, typename F>
int carve(sift_ctx* c, S* out, F&& layout) {
  Carver measure(nullptr);
  layout(measure);
  if (int rc = ensure_match(c, measure.bytes())) return rc;
  Carver real(c->d_match.get());
  *out = layout(real);
  return SIFT_OK;
}

bool aligned16(const void* a, const void* b) {
  return !((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15);
}
const char* const kRowsUnaligned = "descriptor rows must be 16-byte aligned";

int clamp_off(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

bool known_metric(int metric) {
  return metric == SIFT_METRIC_L1_F32 || metric == SIFT_METRIC_L1_U8 || metric == SIFT_METRIC_L2SQR_U8;
}
const char* const kBadMetric = "metric must be one of SIFT_METRIC_L1_F32, _L1_U8, _L2SQR_U8";

// Rows [clamp(q_offsets[0]), clamp(q_offsets[n_segments])) of a [q_cap][k]
// result come back: the others are left untouched, as in the device form.
int copy_back_live_rows(sift_ctx* c, const int* q_offsets, int n_segments, int q_cap, int k, int* idx, float* dist,
                        const int* d_idx, const float* d_dist) {
  const int lo = clamp_off(q_offsets[0], q_cap), hi = clamp_off(q_offsets[n_segments], q_cap);
  if (hi > lo) {
    const size_t n = (size_t)(hi - lo) * k, o = (size_t)lo * k;
    HIP_TRY(c, hipMemcpyAsync(idx + o, d_idx + o, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dist + o, d_dist + o, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

// The match offsets come back first; then only the written records, with their
// point pairs when the caller asked for them.
int copy_back_records(sift_ctx* c, int n_segments, int m_cap, bool pairs, int* m_offsets, const int* d_m_off,
                      sift_match* matches, const sift_match* d_matches, float* src_xy, const float* d_src_xy,
                      float* dst_xy, const float* d_dst_xy) {
  const size_t ob = (size_t)(n_segments + 1) * sizeof(int);
  HIP_TRY(c, hipMemcpyAsync(m_offsets, d_m_off, ob, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const size_t n = (size_t)(m_offsets[n_segments] < m_cap ? m_offsets[n_segments] : m_cap);
  if (n) {
    HIP_TRY(c, hipMemcpyAsync(matches, d_matches, n * sizeof(sift_match), hipMemcpyDeviceToHost, c->stream));
    if (pairs) {
      HIP_TRY(c, hipMemcpyAsync(src_xy, d_src_xy, n * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipMemcpyAsync(dst_xy, d_dst_xy, n * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return SIFT_OK;
}

// The keypoints of both sides, for a stage that gathers point pairs.
int upload_kpts(sift_ctx* c, sift_keypoint* d_q, const sift_keypoint* q_kpts, int q_cap, sift_keypoint* d_t,
                const sift_keypoint* t_kpts, int t_cap) {
  HIP_TRY(c, hipMemcpyAsync(d_q, q_kpts, (size_t)q_cap * sizeof(sift_keypoint), hipMemcpyHostToDevice, c->stream));
  if (t_cap)
    HIP_TRY(c, hipMemcpyAsync(d_t, t_kpts, (size_t)t_cap * sizeof(sift_keypoint), hipMemcpyHostToDevice, c->stream));
  return SIFT_OK;
}

// The check_* functions hold the argument checks that the device and the host
// form of an entry point share, in the order they fire; a call with nothing to
// do (no queries, no segments) passes them whatever its buffers.

// ---- BFMatcher(NORM_L1).knnMatch, src/main.cpp:25-27 ----
int check_knn(sift_ctx* c, const void* query, int n_query, const void* train, int n_train, int k, const int* idx,
              const float* dist) {
  if (!c) return SIFT_E_INVALID;
  if (n_query < 0 || n_train < 0) return fail(c, SIFT_E_INVALID, "negative descriptor count");
  if (k != 1 && k != 2) return fail(c, SIFT_E_INVALID, "k must be 1 or 2");
  if (n_query == 0) return SIFT_OK;
  if (!query || !idx || !dist || (n_train > 0 && !train)) return fail(c, SIFT_E_INVALID, "null buffer");
  return SIFT_OK;
}

int knn_device(sift_ctx* c, const float* q, int nq, const float* t, int nt, int k, int splits, int* idx, float* dist,
               KnnParts parts) {
  {
    StageScope s(c, ST_MATCH, 2.0 * kDescLen * nq * (double)nt, 512.0 * (nq + (double)nt));
    launch_knn_l1(c->stream, q, nq, t, nt, k, splits, dev(parts.dist), dev(parts.idx), idx, dist);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// ---- a whole batch: segmented knnMatch, ratio test, point pairs (src/main.cpp:25-52) ----
int check_seg(sift_ctx* c, const void* query, const int* q_offsets, int n_segments, int q_cap, const void* train,
              int t_cap, int k, const int* idx, const float* dist) {
  if (!c) return SIFT_E_INVALID;
  if (n_segments < 0 || q_cap < 0 || t_cap < 0) return fail(c, SIFT_E_INVALID, "negative count");
  if (k != 1 && k != 2) return fail(c, SIFT_E_INVALID, "k must be 1 or 2");
  if (n_segments == 0 || q_cap == 0) return SIFT_OK;
  if (!query || !q_offsets || !idx || !dist || (t_cap > 0 && !train)) return fail(c, SIFT_E_INVALID, "null buffer");
  return SIFT_OK;
}

// ---- the four segmented matchers: one metric description, one path ----
// One segmented call: the buffers are device pointers.
template <typename Row>
struct SegCall {
  const Row* q; const int* qoff; int n_segments, q_cap; const Row* t; const int* toff; int t_cap, k, splits;
  int* idx; float* dist;
};

// A metric: scratch.hpp's row type and device pieces, and here the stage, the
// split count and the launcher (match.hip, match_u8.hip, match_l2_u8.hip,
// match_l2_f32.hip).
struct MatchL1F32 : L1F32 {
  static constexpr int kStage = ST_MATCH_SEG;
  static constexpr auto splits = knn_seg_splits;
  static void launch(hipStream_t st, const SegCall<Row>& A, const Seg& s) {
    launch_knn_l1_seg(st, A.q, A.qoff, A.n_segments, A.q_cap, A.t, A.toff, A.t_cap, A.k, A.splits, s.tile_start,
                      dev(s.parts.dist), dev(s.parts.idx), A.idx, A.dist);
  }
};
struct MatchL1U8 : L1U8 {
  static constexpr int kStage = ST_MATCH_U8;
  static constexpr auto splits = knn_u8_seg_splits;
  static void launch(hipStream_t st, const SegCall<Row>& A, const Seg& s) {
    launch_knn_l1_u8_seg(st, A.q, A.qoff, A.n_segments, A.q_cap, A.t, A.toff, A.t_cap, A.k, A.splits, s.tile_start,
                         dev(s.parts.dist), dev(s.parts.idx), A.idx, A.dist);
  }
};
struct MatchL2SqrU8 : L2SqrU8 {
  static constexpr int kStage = ST_MATCH_L2_U8;
  static constexpr auto splits = knn_l2_u8_seg_splits;
  static void launch(hipStream_t st, const SegCall<Row>& A, const Seg& s) {
    launch_knn_l2sqr_u8_seg(st, A.q, A.qoff, A.n_segments, A.q_cap, A.t, A.toff, A.t_cap, A.k, A.splits, s.tile_start,
                            s.q_norm, s.t_norm, dev(s.parts.dist), dev(s.parts.idx), A.idx, A.dist);
  }
};
struct MatchL2SqrF32 : L2SqrF32 {
  static constexpr int kStage = ST_MATCH_L2_F32;
  static constexpr auto splits = knn_l2_f32_seg_splits;
  static void launch(hipStream_t st, const SegCall<Row>& A, const Seg& s) {
    launch_knn_l2sqr_f32_seg(st, A.q, A.qoff, A.n_segments, A.q_cap, A.t, A.toff, A.t_cap, A.k, A.splits, s.tile_start,
                             s.q_norm, s.t_norm, dev(s.parts.dist), dev(s.parts.idx), A.idx, A.dist);
  }
};

template <typename M>
int knn_seg_device(sift_ctx* c, const SegCall<typename M::Row>& A, const typename M::Seg& s) {
  {
    StageScope sc(c, M::kStage);  // the work depends on offsets only the device knows
    M::launch(c->stream, A, s);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// The _segmented_device entry points.
template <typename M, typename Row = typename M::Row>
int seg_match_device(sift_ctx* c, const Row* d_query, const int* d_q_offsets, int n_segments, int q_cap,
                     const Row* d_train, const int* d_t_offsets, int t_cap, int k, int* d_idx, float* d_dist) {
  int rc = check_seg(c, d_query, d_q_offsets, n_segments, q_cap, d_train, t_cap, k, d_idx, d_dist);
  if (rc || n_segments == 0 || q_cap == 0) return rc;
  if (!aligned16(d_query, d_train)) return fail(c, SIFT_E_INVALID, kRowsUnaligned);
  (void)hipSetDevice(c->device);
  const int splits = M::splits(q_cap, n_segments, t_cap, d_t_offsets != nullptr);
  typename M::Seg S;
  if ((rc = carve(c, &S, [&](Carver& a) { return M::layout(a, n_segments, q_cap, t_cap, splits); }))) return rc;
  return knn_seg_device<M>(
      c, {d_query, d_q_offsets, n_segments, q_cap, d_train, d_t_offsets, t_cap, k, splits, d_idx, d_dist}, S);
}

// The host forms after their checks: carve, upload, launch, the live rows come
// back.  q_offsets null: one segment [0, q_cap) over the shared train set, whose
// two offsets the library writes itself.
template <typename M, typename Row = typename M::Row>
int seg_host(sift_ctx* c, const Row* query, const int* q_offsets, int n_segments, int q_cap, const Row* train,
             const int* t_offsets, int t_cap, int k, int* idx, float* dist) {
  (void)hipSetDevice(c->device);
  const int splits = M::splits(q_cap, n_segments, t_cap, t_offsets != nullptr);
  SegHostOf<M> S;
  int rc = carve(c, &S, [&](Carver& a) {
    return seg_host_layout_of<M>(a, n_segments, q_cap, t_cap, t_offsets != nullptr, k, splits);
  });
  if (rc) return rc;
  const size_t row = kDescLen * sizeof(Row), ob = (size_t)(n_segments + 1) * sizeof(int);
  HIP_TRY(c, hipMemcpyAsync(S.query, query, q_cap * row, hipMemcpyHostToDevice, c->stream));
  if (t_cap) HIP_TRY(c, hipMemcpyAsync(S.train, train, t_cap * row, hipMemcpyHostToDevice, c->stream));
  if (q_offsets)
    HIP_TRY(c, hipMemcpyAsync(S.q_off, q_offsets, ob, hipMemcpyHostToDevice, c->stream));
  else
    launch_set_offsets(c->stream, S.q_off, 0, q_cap);
  if (S.t_off) HIP_TRY(c, hipMemcpyAsync(S.t_off, t_offsets, ob, hipMemcpyHostToDevice, c->stream));
  if ((rc = knn_seg_device<M>(
           c, {S.query, S.q_off, n_segments, q_cap, S.train, S.t_off, t_cap, k, splits, S.idx, S.dist}, S.seg)))
    return rc;
  const int whole[2] = {0, q_cap};
  return copy_back_live_rows(c, q_offsets ? q_offsets : whole, n_segments, q_cap, k, idx, dist, S.idx, S.dist);
}

// The _segmented entry points.
template <typename M, typename Row = typename M::Row>
int seg_match_host(sift_ctx* c, const Row* query, const int* q_offsets, int n_segments, int q_cap, const Row* train,
                   const int* t_offsets, int t_cap, int k, int* idx, float* dist) {
  int rc = check_seg(c, query, q_offsets, n_segments, q_cap, train, t_cap, k, idx, dist);
  if (rc || n_segments == 0 || q_cap == 0) return rc;
  return seg_host<M>(c, query, q_offsets, n_segments, q_cap, train, t_offsets, t_cap, k, idx, dist);
}

// The one-segment entry points (the byte metrics and float squared L2).
template <typename M, typename Row = typename M::Row>
int one_seg_match_host(sift_ctx* c, const Row* query, int n_query, const Row* train, int n_train, int k, int* idx,
                       float* dist) {
  int rc = check_knn(c, query, n_query, train, n_train, k, idx, dist);
  if (rc || n_query == 0) return rc;
  return seg_host<M>(c, query, nullptr, 1, n_query, train, nullptr, n_train, k, idx, dist);
}

// t_cap: the host form's train keypoint count (the device form never reads it: 0).
int check_ratio(sift_ctx* c, const int* idx, const float* dist, const int* q_offsets, int n_segments, int q_cap,
                const sift_keypoint* q_kpts, const sift_keypoint* t_kpts, int t_cap, const sift_match* matches,
                const float* src_xy, const float* dst_xy, int m_cap, const int* m_offsets) {
  if (!c) return SIFT_E_INVALID;
  if (n_segments < 0 || q_cap < 0 || m_cap < 0 || (q_kpts && t_cap < 0))
    return fail(c, SIFT_E_INVALID, "negative count");
  if (n_segments == 0 || q_cap == 0) return SIFT_OK;
  if (!idx || !dist || !q_offsets || !m_offsets || (m_cap > 0 && !matches))
    return fail(c, SIFT_E_INVALID, "null buffer");
  if (q_kpts && (!t_kpts || (m_cap > 0 && (!src_xy || !dst_xy))))
    return fail(c, SIFT_E_INVALID, "point pairs need the train keypoints and both xy buffers");
  return SIFT_OK;
}

int ratio_device(sift_ctx* c, const int* idx, const float* dist, const int* qoff, int n_segments, int q_cap,
                 double ratio, const sift_keypoint* q_kpts, const sift_keypoint* t_kpts, const int* toff,
                 sift_match* matches, float* src_xy, float* dst_xy, int m_cap, int* moff, int* blk_scan) {
  {
    StageScope sc(c, ST_RATIO, 0, 16.0 * q_cap);
    launch_ratio_matches(c->stream, idx, dist, qoff, n_segments, q_cap, ratio, q_kpts, t_kpts, toff, matches,
                         src_xy, dst_xy, m_cap, moff, blk_scan);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// ---- 8-bit descriptors: the quantiser (match_u8.hip) ----
int check_quant(sift_ctx* c, const float* desc, int n, const uint8_t* out) {
  if (!c) return SIFT_E_INVALID;
  if (n < 0) return fail(c, SIFT_E_INVALID, "negative descriptor count");
  if (n == 0) return SIFT_OK;
  if (!desc || !out) return fail(c, SIFT_E_INVALID, "null buffer");
  return SIFT_OK;
}

int quant_device(sift_ctx* c, const float* desc, const int* n_rows, int row_cap, uint8_t* out) {
  {
    StageScope s(c, ST_QUANT_U8, 0, 5.0 * kDescLen * row_cap);
    launch_desc_to_u8(c->stream, desc, n_rows, row_cap, out);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// ---- spatially gated matching: the segmented matcher of a metric inside a search window (match_window.hip) ----
size_t metric_row_bytes(int metric) { return metric == SIFT_METRIC_L1_F32 ? kDescLen * sizeof(float) : kDescLen; }

int check_window(sift_ctx* c, int metric, const void* query, const sift_keypoint* q_kpts, const int* q_offsets,
                 int n_segments, int q_cap, const void* train, const sift_keypoint* t_kpts, int t_cap, float radius,
                 int rows, int cols, int k, const int* idx, const float* dist) {
  if (!c) return SIFT_E_INVALID;
  if (!known_metric(metric)) return fail(c, SIFT_E_INVALID, kBadMetric);
  if (n_segments < 0 || q_cap < 0 || t_cap < 0) return fail(c, SIFT_E_INVALID, "negative count");
  if (k != 1 && k != 2) return fail(c, SIFT_E_INVALID, "k must be 1 or 2");
  if (!(radius >= 0)) return fail(c, SIFT_E_INVALID, "radius must be 0 or positive (+inf: no gate)");
  if (rows < 1 || cols < 1) return fail(c, SIFT_E_INVALID, "rows and cols must be at least 1");
  if (n_segments == 0 || q_cap == 0) return SIFT_OK;
  if (!query || !q_offsets || !idx || !dist || (t_cap > 0 && !train)) return fail(c, SIFT_E_INVALID, "null buffer");
  if (!q_kpts || !t_kpts) return fail(c, SIFT_E_INVALID, "the window needs both keypoint arrays");
  return SIFT_OK;
}

// The caller's buffers (device pointers), the grid and the scratch pieces, as the kernels take them.
int window_device(sift_ctx* c, int metric, const void* q, const sift_keypoint* q_kpts, const int* qoff, int n_segments,
                  int q_cap, const void* t, const sift_keypoint* t_kpts, const int* toff, int t_cap, const double* H,
                  const int* found, float radius, int k, int* idx, float* dist, WindowGrid G, WindowParts P) {
  const WindowArgs A{metric, q, q_kpts, qoff, n_segments, q_cap, t, t_kpts, toff, t_cap, H, found, radius,
                     G.nx, G.ny, G.inv_cell, P.cell_end, P.cell_rows, dev(P.cell_xy), k, idx, dist};
  {
    StageScope sc(c, ST_WINDOW_BIN, 0, 2.0 * (sizeof(sift_keypoint) + 12.0) * A.t_cap);
    HIP_TRY(c, launch_window_bin(c->stream, A));
  }
  {
    StageScope sc(c, ST_MATCH_WINDOW);  // the work depends on offsets and positions only the device knows
    launch_knn_window(c->stream, A);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// ---- matching along epipolar lines: the windowed matcher gated by the band of F as well (match_epipolar.hip) ----
int check_epipolar(sift_ctx* c, int metric, const void* query, const sift_keypoint* q_kpts, const int* q_offsets,
                   int n_segments, int q_cap, const void* train, const sift_keypoint* t_kpts, int t_cap, double band,
                   float radius, int rows, int cols, int k, const int* idx, const float* dist) {
  if (!c) return SIFT_E_INVALID;
  if (!(band >= 0)) return fail(c, SIFT_E_INVALID, "band must be 0 or positive (+inf: no gate)");
  return check_window(c, metric, query, q_kpts, q_offsets, n_segments, q_cap, train, t_kpts, t_cap, radius, rows, cols,
                      k, idx, dist);
}

// As window_device; F in H's place, the limit as the estimate forms its own.
int epipolar_device(sift_ctx* c, int metric, const void* q, const sift_keypoint* q_kpts, const int* qoff,
                    int n_segments, int q_cap, const void* t, const sift_keypoint* t_kpts, const int* toff, int t_cap,
                    const double* F, const int* found, double band, float radius, int k, int* idx, float* dist,
                    WindowGrid G, WindowParts P) {
  const EpipolarArgs A{{metric, q, q_kpts, qoff, n_segments, q_cap, t, t_kpts, toff, t_cap, F, found, radius,
                        G.nx, G.ny, G.inv_cell, P.cell_end, P.cell_rows, dev(P.cell_xy), k, idx, dist},
                       (float)(band * band)};
  {
    StageScope sc(c, ST_WINDOW_BIN, 0, 2.0 * (sizeof(sift_keypoint) + 12.0) * A.W.t_cap);
    HIP_TRY(c, launch_window_bin(c->stream, A.W));
  }
  {
    StageScope sc(c, ST_MATCH_EPIPOLAR);  // the work depends on offsets, positions and models only the device knows
    launch_knn_epipolar(c->stream, A);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// ---- cross-check: the join of a forward and a reverse matcher result (cross_check.hip) ----
// The checks of the train offsets and the outputs, and of the ratio: shared with the one-call form.
int check_cross_out(sift_ctx* c, const int* t_offsets, const sift_keypoint* q_kpts, const sift_keypoint* t_kpts,
                    const sift_match* matches, const float* src_xy, const float* dst_xy, int m_cap,
                    const int* m_offsets) {
  if (!t_offsets)
    return fail(c, SIFT_E_INVALID, "cross-check needs train offsets: a shared train set has no reverse result");
  if (!m_offsets || (m_cap > 0 && !matches)) return fail(c, SIFT_E_INVALID, "null buffer");
  if (q_kpts && (!t_kpts || (m_cap > 0 && (!src_xy || !dst_xy))))
    return fail(c, SIFT_E_INVALID, "point pairs need the train keypoints and both xy buffers");
  return SIFT_OK;
}

int check_cross_ratio(sift_ctx* c, double ratio, int fwd_k) {
  if (!(ratio >= 0)) return fail(c, SIFT_E_INVALID, "ratio must be 0 (cross-check only) or positive");
  if (ratio > 0 && fwd_k != 2) return fail(c, SIFT_E_INVALID, "the ratio test needs the k = 2 forward result");
  return SIFT_OK;
}

int check_cross(sift_ctx* c, const int* idx, const float* dist, int fwd_k, const int* q_offsets, int n_segments,
                int q_cap, const int* ridx, int rev_k, const int* t_offsets, int t_cap, double ratio,
                const sift_keypoint* q_kpts, const sift_keypoint* t_kpts, const sift_match* matches,
                const float* src_xy, const float* dst_xy, int m_cap, const int* m_offsets) {
  if (!c) return SIFT_E_INVALID;
  if (n_segments < 0 || q_cap < 0 || t_cap < 0 || m_cap < 0) return fail(c, SIFT_E_INVALID, "negative count");
  if ((fwd_k != 1 && fwd_k != 2) || (rev_k != 1 && rev_k != 2))
    return fail(c, SIFT_E_INVALID, "fwd_k and rev_k must be 1 or 2");
  if (int rc = check_cross_ratio(c, ratio, fwd_k)) return rc;
  if (n_segments == 0 || q_cap == 0) return SIFT_OK;
  if (!idx || !dist || !q_offsets || (t_cap > 0 && !ridx)) return fail(c, SIFT_E_INVALID, "null buffer");
  return check_cross_out(c, t_offsets, q_kpts, t_kpts, matches, src_xy, dst_xy, m_cap, m_offsets);
}

int cross_device(sift_ctx* c, const int* idx, const float* dist, int fwd_k, const int* qoff, int n_segments, int q_cap,
                 const int* ridx, int rev_k, const int* toff, int t_cap, double ratio, const sift_keypoint* q_kpts,
                 const sift_keypoint* t_kpts, sift_match* matches, float* src_xy, float* dst_xy, int m_cap, int* moff,
                 int* blk_scan) {
  {
    StageScope sc(c, ST_CROSS, 0, (8.0 * fwd_k + 4.0) * q_cap);
    launch_cross_check(c->stream, idx, dist, fwd_k, qoff, n_segments, q_cap, ridx, rev_k, toff, t_cap, ratio, q_kpts,
                       t_kpts, matches, src_xy, dst_xy, m_cap, moff, blk_scan);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// The forward (k = fwd_k) and the reverse (k = 1, the sides exchanged) pass of
// one metric into the tables of its CrossMatch layout, carved here and handed
// back in T.  A batch without train rows has no reverse pass (and no neighbour
// to look up in its table).
struct CrossArgs {
  const void *query, *train;
  const int *q_off, *t_off;
  int n_segments, q_cap, t_cap, fwd_k, fwd_splits, rev_splits;
};

template <typename M>
int cross_passes(sift_ctx* c, CrossArgs A, int blocks, CrossTables* T) {
  using Row = typename M::Row;
  const Row *q = static_cast<const Row*>(A.query), *t = static_cast<const Row*>(A.train);
  A.fwd_splits = M::splits(A.q_cap, A.n_segments, A.t_cap, true);
  A.rev_splits = M::splits(A.t_cap, A.n_segments, A.q_cap, true);
  CrossMatch<typename M::Seg> S;
  int rc = carve(c, &S, [&](Carver& a) {
    return cross_match_layout_of<M>(a, A.n_segments, A.q_cap, A.t_cap, A.fwd_k, A.fwd_splits, A.rev_splits, blocks);
  });
  if (rc) return rc;
  *T = S.tab;
  if ((rc = knn_seg_device<M>(c, {q, A.q_off, A.n_segments, A.q_cap, t, A.t_off, A.t_cap, A.fwd_k, A.fwd_splits,
                                  S.tab.idx, S.tab.dist}, S.fwd)))
    return rc;
  if (A.t_cap == 0) return SIFT_OK;
  return knn_seg_device<M>(
      c, {t, A.t_off, A.n_segments, A.t_cap, q, A.q_off, A.q_cap, 1, A.rev_splits, S.tab.ridx, S.tab.rdist}, S.rev);
}

// ---- a whole batch: findHomography(RANSAC) per segment of the ratio stage's pairs (src/main.cpp:54-55) ----
int check_homog(sift_ctx* c, const float* src_xy, const float* dst_xy, const int* m_offsets, int n_segments,
                int m_cap, const double* H, const int* found) {
  if (!c) return SIFT_E_INVALID;
  if (n_segments < 0 || m_cap < 0) return fail(c, SIFT_E_INVALID, "negative count");
  if (n_segments == 0 || m_cap == 0) return SIFT_OK;
  if (!src_xy || !dst_xy || !m_offsets || !H || !found) return fail(c, SIFT_E_INVALID, "null buffer");
  return SIFT_OK;
}

int homog_device(sift_ctx* c, const float* src_xy, const float* dst_xy, const int* moff, int n_segments, int m_cap,
                 double thr, int max_iters, double confidence, double* H, int* found, unsigned char* mask_out,
                 HomogParts P) {
  {
    StageScope sc(c, ST_HOMOG_SEG);  // the work depends on offsets and points only the device knows
    launch_homography_seg(c->stream, src_xy, dst_xy, moff, n_segments, m_cap, thr, max_iters, confidence, P.subsets,
                          P.models, P.counts, P.state, P.mask, H, found, mask_out);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// ---- a whole batch: estimateAffine2D / estimateAffinePartial2D per segment of the same pairs ----
int check_affine(sift_ctx* c, const float* src_xy, const float* dst_xy, const int* m_offsets, int n_segments,
                 int m_cap, int model, const double* H, const int* found) {
  if (!c) return SIFT_E_INVALID;
  if (model != SIFT_MODEL_AFFINE && model != SIFT_MODEL_SIMILARITY) return fail(c, SIFT_E_INVALID, "unknown model");
  return check_homog(c, src_xy, dst_xy, m_offsets, n_segments, m_cap, H, found);
}

int affine_device(sift_ctx* c, const float* src_xy, const float* dst_xy, const int* moff, int n_segments, int m_cap,
                  int model, double thr, int max_iters, double confidence, double* H, int* found,
                  unsigned char* mask_out) {
  {
    StageScope sc(c, ST_AFFINE_SEG);  // the work depends on offsets and points only the device knows
    launch_affine_seg(c->stream, src_xy, dst_xy, moff, n_segments, m_cap, model, thr, max_iters, confidence, H, found,
                      mask_out);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// ---- a whole batch: findFundamentalMat(FM_RANSAC) per segment of the same pairs ----
int fundamental_device(sift_ctx* c, const float* src_xy, const float* dst_xy, const int* moff, int n_segments,
                       int m_cap, double thr, int max_iters, double confidence, double* F, int* found,
                       unsigned char* mask_out) {
  {
    StageScope sc(c, ST_FUND_SEG);  // the work depends on offsets and points only the device knows
    launch_fundamental_seg(c->stream, src_xy, dst_xy, moff, n_segments, m_cap, thr, max_iters, confidence, F, found,
                           mask_out);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// ---- a whole batch: recoverPose per segment of the same pairs, and triangulatePoints ----
int check_pose(sift_ctx* c, const float* src_xy, const float* dst_xy, const int* m_offsets, int n_segments, int m_cap,
               const double* F, const int* found, const double* K_src, const double* K_dst, int k_per_segment,
               const double* pose, const int* pose_found, const int* n_good) {
  if (!c) return SIFT_E_INVALID;
  if (n_segments < 0 || m_cap < 0) return fail(c, SIFT_E_INVALID, "negative count");
  if (k_per_segment != 0 && k_per_segment != 1) return fail(c, SIFT_E_INVALID, "k_per_segment must be 0 or 1");
  if (n_segments == 0 || m_cap == 0) return SIFT_OK;
  if (!src_xy || !dst_xy || !m_offsets || !F || !found || !K_src || !K_dst || !pose || !pose_found || !n_good)
    return fail(c, SIFT_E_INVALID, "null buffer");
  return SIFT_OK;
}

int pose_device(sift_ctx* c, const float* src_xy, const float* dst_xy, const int* moff, int n_segments, int m_cap,
                const double* F, const int* found, const double* K_src, const double* K_dst, int k_per_segment,
                const unsigned char* mask_in, double distance_thresh, double* pose, double* E, int* pose_found,
                int* n_good, unsigned char* mask_out, double* xyz) {
  {
    StageScope sc(c, ST_POSE_SEG);  // the work depends on offsets and points only the device knows
    launch_recover_pose_seg(c->stream, src_xy, dst_xy, moff, n_segments, m_cap, F, found, K_src, K_dst, k_per_segment,
                            mask_in, distance_thresh, pose, E, pose_found, n_good, mask_out, xyz);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// ---- a whole batch: solvePnPRansac per segment of 3-D / 2-D rows ----
int check_pnp(sift_ctx* c, const double* xyz, const float* xy, const int* m_offsets, int n_segments, int m_cap,
              const double* K, int k_per_segment, const double* pose, const int* found, const int* n_inliers) {
  if (!c) return SIFT_E_INVALID;
  if (n_segments < 0 || m_cap < 0) return fail(c, SIFT_E_INVALID, "negative count");
  if (k_per_segment != 0 && k_per_segment != 1) return fail(c, SIFT_E_INVALID, "k_per_segment must be 0 or 1");
  if (n_segments == 0 || m_cap == 0) return SIFT_OK;
  if (!xyz || !xy || !m_offsets || !K || !pose || !found || !n_inliers) return fail(c, SIFT_E_INVALID, "null buffer");
  return SIFT_OK;
}

int pnp_device(sift_ctx* c, const double* xyz, const float* xy, const int* moff, int n_segments, int m_cap,
               const unsigned char* row_mask, const double* K, int k_per_segment, double thr, int max_iters,
               double confidence, double* pose, int* found, int* n_inliers, unsigned char* mask_out) {
  {
    StageScope sc(c, ST_PNP_SEG);  // the work depends on offsets and rows only the device knows
    launch_pnp_seg(c->stream, xyz, xy, moff, n_segments, m_cap, row_mask, K, k_per_segment, thr, max_iters, confidence,
                   pose, found, n_inliers, mask_out);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// ---- a whole batch: the join of two record tables on a shared keypoint (join.hip) ----
bool join_side_ok(int side) { return side == SIFT_JOIN_QUERY || side == SIFT_JOIN_TRAIN; }

// One call's buffers, device or host pointers alike.
struct JoinCall {
  const sift_match* a; const int* a_off; int a_cap, a_side; const unsigned char* a_mask; const double* a_xyz;
  const sift_match* b; const int* b_off; int b_cap, b_side; const unsigned char* b_mask; const float* b_xy;
  const int* key_off; int key_cap, n_segments;
  double* xyz_out; float* xy_out; int *a_row, *b_row; unsigned char* b_joined; int j_cap; int* j_off;
};

int check_join(sift_ctx* c, const JoinCall& J) {
  if (!c) return SIFT_E_INVALID;
  if (J.n_segments < 0 || J.a_cap < 0 || J.b_cap < 0 || J.key_cap < 0 || J.j_cap < 0)
    return fail(c, SIFT_E_INVALID, "negative count");
  if (!join_side_ok(J.a_side) || !join_side_ok(J.b_side))
    return fail(c, SIFT_E_INVALID, "a key side must be SIFT_JOIN_QUERY or SIFT_JOIN_TRAIN");
  if (J.n_segments == 0) return SIFT_OK;
  if (!J.a_off || !J.b_off || !J.key_off || !J.j_off || (J.a_cap > 0 && !J.a) || (J.b_cap > 0 && !J.b))
    return fail(c, SIFT_E_INVALID, "null buffer");
  if ((J.xyz_out && !J.a_xyz) || (J.xy_out && !J.b_xy))
    return fail(c, SIFT_E_INVALID, "null buffer: xyz_out needs a_xyz, xy_out needs b_xy");
  return SIFT_OK;
}

int join_device(sift_ctx* c, const JoinCall& J, const JoinParts& P) {
  {
    StageScope sc(c, ST_JOIN);  // the work depends on offsets and keys only the device knows
    launch_join_matches(c->stream, J.a, J.a_off, J.a_cap, J.a_side, J.a_mask, J.a_xyz, J.b, J.b_off, J.b_cap, J.b_side,
                        J.b_mask, J.b_xy, J.key_off, J.key_cap, J.n_segments, J.xyz_out, J.xy_out, J.a_row, J.b_row,
                        J.b_joined, J.j_cap, J.j_off, reinterpret_cast<unsigned long long*>(P.lookup), P.a_tiles,
                        P.b_tiles, P.blk_scan);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// ---- readImage front end, src/main.cpp:79-87 ----
int check_bgr(sift_ctx* c, const void* bgr, int batch, int rows, int cols, int out_rows, int out_cols,
              const void* gray) {
  if (!c) return SIFT_E_INVALID;
  if (!bgr || !gray) return fail(c, SIFT_E_INVALID, "null buffer");
  if (batch < 1 || rows < 1 || cols < 1 || out_rows < 1 || out_cols < 1)
    return fail(c, SIFT_E_INVALID, "empty image");
  return SIFT_OK;
}

// ---- warpPerspective of a batch (warp.hip, warp_math.hpp) ----
// The checks the device and the host form share; bpp: bytes per pixel.
int check_warp(sift_ctx* c, int pixel, int channels, const void* src, int rows, int cols, const double* H,
               unsigned flags, const void* dst, int out_rows, int out_cols, size_t* bpp) {
  if (!c) return SIFT_E_INVALID;
  if (!(pixel == SIFT_PIXEL_F32 && channels == 1) && !(pixel == SIFT_PIXEL_U8 && (channels == 1 || channels == 3)))
    return fail(c, SIFT_E_INVALID, "pixel / channels must be F32 x 1, U8 x 1 or U8 x 3");
  if (flags & ~SIFT_WARP_INVERSE_MAP) return fail(c, SIFT_E_INVALID, "unknown warp flag");
  if (!src || !H || !dst) return fail(c, SIFT_E_INVALID, "null buffer");
  if (rows < 1 || cols < 1 || out_rows < 1 || out_cols < 1) return fail(c, SIFT_E_INVALID, "empty image");
  if (rows > (1 << 30) || cols > (1 << 30) || out_rows > (1 << 30) || out_cols > (1 << 30))
    return fail(c, SIFT_E_SIZE, "a dimension exceeds 2^30");
  *bpp = pixel == SIFT_PIXEL_F32 ? sizeof(float) : (size_t)channels;
  return SIFT_OK;
}

// ---- undistort / undistortPoints of a batch (undistort.hip, undistort_math.hpp) ----
// The checks the device and the host form of the image call share, in the warp call's order.
int check_undistort(sift_ctx* c, int pixel, int channels, const void* src, int rows, int cols, const double* K,
                    const double* dist, int k_per_segment, const void* dst, int out_rows, int out_cols, size_t* bpp) {
  if (!c) return SIFT_E_INVALID;
  if (!(pixel == SIFT_PIXEL_F32 && channels == 1) && !(pixel == SIFT_PIXEL_U8 && (channels == 1 || channels == 3)))
    return fail(c, SIFT_E_INVALID, "pixel / channels must be F32 x 1, U8 x 1 or U8 x 3");
  if (k_per_segment != 0 && k_per_segment != 1) return fail(c, SIFT_E_INVALID, "k_per_segment must be 0 or 1");
  if (!src || !K || !dist || !dst) return fail(c, SIFT_E_INVALID, "null buffer");
  if (rows < 1 || cols < 1 || out_rows < 1 || out_cols < 1) return fail(c, SIFT_E_INVALID, "empty image");
  if (rows > (1 << 30) || cols > (1 << 30) || out_rows > (1 << 30) || out_cols > (1 << 30))
    return fail(c, SIFT_E_SIZE, "a dimension exceeds 2^30");
  *bpp = pixel == SIFT_PIXEL_F32 ? sizeof(float) : (size_t)channels;
  return SIFT_OK;
}

// The checks the two segmented forms of the point call share; m_cap == 0 still reports the flags.
int check_undistort_points(sift_ctx* c, const void* src, const void* dst, size_t stride, const int* m_offsets,
                           int n_segments, int m_cap, const double* K, const double* dist, int k_per_segment,
                           int iters, const int* ok) {
  if (!c) return SIFT_E_INVALID;
  if (n_segments < 0 || m_cap < 0) return fail(c, SIFT_E_INVALID, "negative count");
  if (k_per_segment != 0 && k_per_segment != 1) return fail(c, SIFT_E_INVALID, "k_per_segment must be 0 or 1");
  if (!umath::iters_ok(iters)) return fail(c, SIFT_E_INVALID, "iters must be 0 .. 100");
  if (!umath::stride_ok(stride)) return fail(c, SIFT_E_INVALID, "xy_stride_bytes must be a multiple of 4, at least 8");
  if (n_segments == 0) return SIFT_OK;
  if (!m_offsets || !K || !dist || !ok || (m_cap > 0 && (!src || !dst))) return fail(c, SIFT_E_INVALID, "null buffer");
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % sizeof(float))
    return fail(c, SIFT_E_INVALID, "point rows must be 4-byte aligned");
  return SIFT_OK;
}

}  // namespace

extern "C" {

int sift_knn_match_l1_device(sift_ctx* c, const float* d_query, int n_query, const float* d_train, int n_train,
                             int k, int* d_idx, float* d_dist) {
  int rc = check_knn(c, d_query, n_query, d_train, n_train, k, d_idx, d_dist);
  if (rc || n_query == 0) return rc;
  if (!aligned16(d_query, d_train)) return fail(c, SIFT_E_INVALID, kRowsUnaligned);
  (void)hipSetDevice(c->device);
  const int splits = knn_splits(n_query, n_train);
  KnnParts parts;
  if ((rc = carve(c, &parts, [&](Carver& a) { return knn_layout(a, n_query, splits); }))) return rc;
  return knn_device(c, d_query, n_query, d_train, n_train, k, splits, d_idx, d_dist, parts);
}

int sift_knn_match_l1(sift_ctx* c, const float* query, int n_query, const float* train, int n_train, int k,
                      int* idx, float* dist) {
  int rc = check_knn(c, query, n_query, train, n_train, k, idx, dist);
  if (rc || n_query == 0) return rc;
  (void)hipSetDevice(c->device);
  const int splits = knn_splits(n_query, n_train);
  KnnHost S;
  if ((rc = carve(c, &S, [&](Carver& a) { return knn_host_layout(a, n_query, n_train, k, splits); }))) return rc;
  const size_t row = kDescLen * sizeof(float);
  HIP_TRY(c, hipMemcpyAsync(S.query, query, n_query * row, hipMemcpyHostToDevice, c->stream));
  if (n_train) HIP_TRY(c, hipMemcpyAsync(S.train, train, n_train * row, hipMemcpyHostToDevice, c->stream));
  if ((rc = knn_device(c, S.query, n_query, S.train, n_train, k, splits, S.idx, S.dist, S.parts))) return rc;
  HIP_TRY(c, hipMemcpyAsync(idx, S.idx, (size_t)n_query * k * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(dist, S.dist, (size_t)n_query * k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

int sift_knn_match_l1_segmented_device(sift_ctx* c, const float* d_query, const int* d_q_offsets, int n_segments,
                                       int q_cap, const float* d_train, const int* d_t_offsets, int t_cap, int k,
                                       int* d_idx, float* d_dist) {
  return seg_match_device<MatchL1F32>(c, d_query, d_q_offsets, n_segments, q_cap, d_train, d_t_offsets, t_cap, k, d_idx,
                                      d_dist);
}

int sift_knn_match_l1_segmented(sift_ctx* c, const float* query, const int* q_offsets, int n_segments, int q_cap,
                                const float* train, const int* t_offsets, int t_cap, int k, int* idx, float* dist) {
  return seg_match_host<MatchL1F32>(c, query, q_offsets, n_segments, q_cap, train, t_offsets, t_cap, k, idx, dist);
}

int sift_descriptors_to_u8_device(sift_ctx* c, const float* d_desc, const int* d_n_rows, int row_cap,
                                  uint8_t* d_out) {
  int rc = check_quant(c, d_desc, row_cap, d_out);
  if (rc || row_cap == 0) return rc;
  if (!aligned16(d_desc, d_out)) return fail(c, SIFT_E_INVALID, kRowsUnaligned);
  (void)hipSetDevice(c->device);
  return quant_device(c, d_desc, d_n_rows, row_cap, d_out);
}

int sift_descriptors_to_u8(sift_ctx* c, const float* desc, int n, uint8_t* out) {
  int rc = check_quant(c, desc, n, out);
  if (rc || n == 0) return rc;
  (void)hipSetDevice(c->device);
  QuantHostU8 S;
  if ((rc = carve(c, &S, [&](Carver& a) { return quant_u8_host_layout(a, n); }))) return rc;
  HIP_TRY(c, hipMemcpyAsync(S.desc, desc, (size_t)n * kDescLen * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if ((rc = quant_device(c, S.desc, nullptr, n, S.out))) return rc;
  HIP_TRY(c, hipMemcpyAsync(out, S.out, (size_t)n * kDescLen, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

int sift_knn_match_l1_u8_segmented_device(sift_ctx* c, const uint8_t* d_query, const int* d_q_offsets,
                                          int n_segments, int q_cap, const uint8_t* d_train,
                                          const int* d_t_offsets, int t_cap, int k, int* d_idx, float* d_dist) {
  return seg_match_device<MatchL1U8>(c, d_query, d_q_offsets, n_segments, q_cap, d_train, d_t_offsets, t_cap, k, d_idx,
                                     d_dist);
}

int sift_knn_match_l1_u8_segmented(sift_ctx* c, const uint8_t* query, const int* q_offsets, int n_segments,
                                   int q_cap, const uint8_t* train, const int* t_offsets, int t_cap, int k,
                                   int* idx, float* dist) {
  return seg_match_host<MatchL1U8>(c, query, q_offsets, n_segments, q_cap, train, t_offsets, t_cap, k, idx, dist);
}

// One segment [0, n_query) over the shared train set; the library writes the two offsets itself.
int sift_knn_match_l1_u8(sift_ctx* c, const uint8_t* query, int n_query, const uint8_t* train, int n_train, int k,
                         int* idx, float* dist) {
  return one_seg_match_host<MatchL1U8>(c, query, n_query, train, n_train, k, idx, dist);
}

int sift_knn_match_l2sqr_u8_segmented_device(sift_ctx* c, const uint8_t* d_query, const int* d_q_offsets,
                                             int n_segments, int q_cap, const uint8_t* d_train,
                                             const int* d_t_offsets, int t_cap, int k, int* d_idx, float* d_dist) {
  return seg_match_device<MatchL2SqrU8>(c, d_query, d_q_offsets, n_segments, q_cap, d_train, d_t_offsets, t_cap, k,
                                        d_idx, d_dist);
}

int sift_knn_match_l2sqr_u8_segmented(sift_ctx* c, const uint8_t* query, const int* q_offsets, int n_segments,
                                      int q_cap, const uint8_t* train, const int* t_offsets, int t_cap, int k,
                                      int* idx, float* dist) {
  return seg_match_host<MatchL2SqrU8>(c, query, q_offsets, n_segments, q_cap, train, t_offsets, t_cap, k, idx, dist);
}

// One segment [0, n_query) over the shared train set; the library writes the two offsets itself.
int sift_knn_match_l2sqr_u8(sift_ctx* c, const uint8_t* query, int n_query, const uint8_t* train, int n_train, int k,
                            int* idx, float* dist) {
  return one_seg_match_host<MatchL2SqrU8>(c, query, n_query, train, n_train, k, idx, dist);
}

int sift_knn_match_l2sqr_f32_segmented_device(sift_ctx* c, const float* d_query, const int* d_q_offsets,
                                              int n_segments, int q_cap, const float* d_train,
                                              const int* d_t_offsets, int t_cap, int k, int* d_idx, float* d_dist) {
  return seg_match_device<MatchL2SqrF32>(c, d_query, d_q_offsets, n_segments, q_cap, d_train, d_t_offsets, t_cap, k,
                                         d_idx, d_dist);
}

int sift_knn_match_l2sqr_f32_segmented(sift_ctx* c, const float* query, const int* q_offsets, int n_segments,
                                       int q_cap, const float* train, const int* t_offsets, int t_cap, int k,
                                       int* idx, float* dist) {
  return seg_match_host<MatchL2SqrF32>(c, query, q_offsets, n_segments, q_cap, train, t_offsets, t_cap, k, idx, dist);
}

// One segment [0, n_query) over the shared train set; the library writes the two offsets itself.
int sift_knn_match_l2sqr_f32(sift_ctx* c, const float* query, int n_query, const float* train, int n_train, int k,
                             int* idx, float* dist) {
  return one_seg_match_host<MatchL2SqrF32>(c, query, n_query, train, n_train, k, idx, dist);
}

int sift_ratio_matches_device(sift_ctx* c, const int* d_idx, const float* d_dist, const int* d_q_offsets,
                              int n_segments, int q_cap, double ratio, const sift_keypoint* d_q_kpts,
                              const sift_keypoint* d_t_kpts, const int* d_t_offsets, sift_match* d_matches,
                              float* d_src_xy, float* d_dst_xy, int m_cap, int* d_m_offsets) {
  int rc = check_ratio(c, d_idx, d_dist, d_q_offsets, n_segments, q_cap, d_q_kpts, d_t_kpts, 0, d_matches, d_src_xy,
                       d_dst_xy, m_cap, d_m_offsets);
  if (rc || n_segments == 0 || q_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  int* blk_scan = nullptr;
  if ((rc = carve(c, &blk_scan, [&](Carver& a) { return ratio_layout(a, ratio_blocks(q_cap)); }))) return rc;
  return ratio_device(c, d_idx, d_dist, d_q_offsets, n_segments, q_cap, ratio, d_q_kpts, d_t_kpts, d_t_offsets,
                      d_matches, d_src_xy, d_dst_xy, m_cap, d_m_offsets, blk_scan);
}

int sift_ratio_matches(sift_ctx* c, const int* idx, const float* dist, const int* q_offsets, int n_segments,
                       int q_cap, double ratio, const sift_keypoint* q_kpts, const sift_keypoint* t_kpts, int t_cap,
                       const int* t_offsets, sift_match* matches, float* src_xy, float* dst_xy, int m_cap,
                       int* m_offsets) {
  int rc = check_ratio(c, idx, dist, q_offsets, n_segments, q_cap, q_kpts, t_kpts, t_cap, matches, src_xy, dst_xy,
                       m_cap, m_offsets);
  if (rc || n_segments == 0 || q_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  RatioHost S;
  if ((rc = carve(c, &S, [&](Carver& a) {
         return ratio_host_layout(a, n_segments, q_cap, t_cap, m_cap, q_kpts != nullptr, t_offsets != nullptr,
                                  ratio_blocks(q_cap));
       })))
    return rc;
  const size_t ob = (size_t)(n_segments + 1) * sizeof(int);
  HIP_TRY(c, hipMemcpyAsync(S.idx, idx, (size_t)q_cap * 2 * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.dist, dist, (size_t)q_cap * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.q_off, q_offsets, ob, hipMemcpyHostToDevice, c->stream));
  if (S.t_off) HIP_TRY(c, hipMemcpyAsync(S.t_off, t_offsets, ob, hipMemcpyHostToDevice, c->stream));
  if (q_kpts && (rc = upload_kpts(c, S.q_kpts, q_kpts, q_cap, S.t_kpts, t_kpts, t_cap))) return rc;
  if ((rc = ratio_device(c, S.idx, S.dist, S.q_off, n_segments, q_cap, ratio, S.q_kpts, S.t_kpts, S.t_off, S.matches,
                         S.src_xy, S.dst_xy, m_cap, S.m_off, S.blk_scan)))
    return rc;
  return copy_back_records(c, n_segments, m_cap, q_kpts != nullptr, m_offsets, S.m_off, matches, S.matches, src_xy,
                           S.src_xy, dst_xy, S.dst_xy);
}

int sift_cross_check_matches_device(sift_ctx* c, const int* d_idx, const float* d_dist, int fwd_k,
                                    const int* d_q_offsets, int n_segments, int q_cap, const int* d_ridx, int rev_k,
                                    const int* d_t_offsets, int t_cap, double ratio, const sift_keypoint* d_q_kpts,
                                    const sift_keypoint* d_t_kpts, sift_match* d_matches, float* d_src_xy,
                                    float* d_dst_xy, int m_cap, int* d_m_offsets) {
  int rc = check_cross(c, d_idx, d_dist, fwd_k, d_q_offsets, n_segments, q_cap, d_ridx, rev_k, d_t_offsets, t_cap,
                       ratio, d_q_kpts, d_t_kpts, d_matches, d_src_xy, d_dst_xy, m_cap, d_m_offsets);
  if (rc || n_segments == 0 || q_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  int* blk_scan = nullptr;
  if ((rc = carve(c, &blk_scan, [&](Carver& a) { return cross_layout(a, cross_blocks(q_cap)); }))) return rc;
  return cross_device(c, d_idx, d_dist, fwd_k, d_q_offsets, n_segments, q_cap, d_ridx, rev_k, d_t_offsets, t_cap,
                      ratio, d_q_kpts, d_t_kpts, d_matches, d_src_xy, d_dst_xy, m_cap, d_m_offsets, blk_scan);
}

int sift_cross_check_matches(sift_ctx* c, const int* idx, const float* dist, int fwd_k, const int* q_offsets,
                             int n_segments, int q_cap, const int* ridx, int rev_k, const int* t_offsets, int t_cap,
                             double ratio, const sift_keypoint* q_kpts, const sift_keypoint* t_kpts,
                             sift_match* matches, float* src_xy, float* dst_xy, int m_cap, int* m_offsets) {
  int rc = check_cross(c, idx, dist, fwd_k, q_offsets, n_segments, q_cap, ridx, rev_k, t_offsets, t_cap, ratio, q_kpts,
                       t_kpts, matches, src_xy, dst_xy, m_cap, m_offsets);
  if (rc || n_segments == 0 || q_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  CrossHost S;
  if ((rc = carve(c, &S, [&](Carver& a) {
         return cross_host_layout(a, n_segments, q_cap, fwd_k, t_cap, rev_k, m_cap, q_kpts != nullptr,
                                  cross_blocks(q_cap));
       })))
    return rc;
  const size_t ob = (size_t)(n_segments + 1) * sizeof(int);
  HIP_TRY(c, hipMemcpyAsync(S.idx, idx, (size_t)q_cap * fwd_k * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.dist, dist, (size_t)q_cap * fwd_k * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if (t_cap)
    HIP_TRY(c, hipMemcpyAsync(S.ridx, ridx, (size_t)t_cap * rev_k * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.q_off, q_offsets, ob, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.t_off, t_offsets, ob, hipMemcpyHostToDevice, c->stream));
  if (q_kpts && (rc = upload_kpts(c, S.q_kpts, q_kpts, q_cap, S.t_kpts, t_kpts, t_cap))) return rc;
  if ((rc = cross_device(c, S.idx, S.dist, fwd_k, S.q_off, n_segments, q_cap, S.ridx, rev_k, S.t_off, t_cap, ratio,
                         S.q_kpts, S.t_kpts, S.matches, S.src_xy, S.dst_xy, m_cap, S.m_off, S.blk_scan)))
    return rc;
  return copy_back_records(c, n_segments, m_cap, q_kpts != nullptr, m_offsets, S.m_off, matches, S.matches, src_xy,
                           S.src_xy, dst_xy, S.dst_xy);
}

int sift_cross_match_segmented_device(sift_ctx* c, int metric, const void* d_query, const int* d_q_offsets,
                                      int n_segments, int q_cap, const void* d_train, const int* d_t_offsets,
                                      int t_cap, double ratio, const sift_keypoint* d_q_kpts,
                                      const sift_keypoint* d_t_kpts, sift_match* d_matches, float* d_src_xy,
                                      float* d_dst_xy, int m_cap, int* d_m_offsets) {
  if (!c) return SIFT_E_INVALID;
  if (!known_metric(metric)) return fail(c, SIFT_E_INVALID, kBadMetric);
  if (n_segments < 0 || q_cap < 0 || t_cap < 0 || m_cap < 0) return fail(c, SIFT_E_INVALID, "negative count");
  const int fwd_k = ratio > 0 ? 2 : 1;
  int rc = check_cross_ratio(c, ratio, fwd_k);
  if (rc || n_segments == 0 || q_cap == 0) return rc;
  if (!d_query || !d_q_offsets || (t_cap > 0 && !d_train)) return fail(c, SIFT_E_INVALID, "null buffer");
  if ((rc = check_cross_out(c, d_t_offsets, d_q_kpts, d_t_kpts, d_matches, d_src_xy, d_dst_xy, m_cap, d_m_offsets)))
    return rc;
  if (!aligned16(d_query, d_train)) return fail(c, SIFT_E_INVALID, kRowsUnaligned);
  (void)hipSetDevice(c->device);
  // Every piece of both passes and of the stage is carved before the first
  // enqueue: the block cannot grow (and move the tables) between the launches.
  const CrossArgs A{d_query, d_train, d_q_offsets, d_t_offsets, n_segments, q_cap, t_cap, fwd_k, 1, 1};
  const int blocks = cross_blocks(q_cap);
  CrossTables T;
  rc = metric == SIFT_METRIC_L1_F32  ? cross_passes<MatchL1F32>(c, A, blocks, &T)
       : metric == SIFT_METRIC_L1_U8 ? cross_passes<MatchL1U8>(c, A, blocks, &T)
                                     : cross_passes<MatchL2SqrU8>(c, A, blocks, &T);
  if (rc) return rc;
  return cross_device(c, T.idx, T.dist, fwd_k, d_q_offsets, n_segments, q_cap, T.ridx, 1, d_t_offsets, t_cap, ratio,
                      d_q_kpts, d_t_kpts, d_matches, d_src_xy, d_dst_xy, m_cap, d_m_offsets, T.blk_scan);
}

int sift_knn_match_window_segmented_device(sift_ctx* c, int metric, const void* d_query,
                                           const sift_keypoint* d_q_kpts, const int* d_q_offsets, int n_segments,
                                           int q_cap, const void* d_train, const sift_keypoint* d_t_kpts,
                                           const int* d_t_offsets, int t_cap, const double* d_H, const int* d_found,
                                           float radius, int rows, int cols, int k, int* d_idx, float* d_dist) {
  int rc = check_window(c, metric, d_query, d_q_kpts, d_q_offsets, n_segments, q_cap, d_train, d_t_kpts, t_cap,
                        radius, rows, cols, k, d_idx, d_dist);
  if (rc || n_segments == 0 || q_cap == 0) return rc;
  if (!aligned16(d_query, d_train)) return fail(c, SIFT_E_INVALID, kRowsUnaligned);
  (void)hipSetDevice(c->device);
  const int n_grids = d_t_offsets ? n_segments : 1;
  const WindowGrid G = window_grid(radius, rows, cols, t_cap, n_grids);
  WindowParts P;
  if ((rc = carve(c, &P, [&](Carver& a) { return window_layout(a, n_grids, G.nx * G.ny, t_cap); }))) return rc;
  return window_device(c, metric, d_query, d_q_kpts, d_q_offsets, n_segments, q_cap, d_train, d_t_kpts, d_t_offsets,
                       t_cap, d_H, d_found, radius, k, d_idx, d_dist, G, P);
}

int sift_knn_match_window_segmented(sift_ctx* c, int metric, const void* query, const sift_keypoint* q_kpts,
                                    const int* q_offsets, int n_segments, int q_cap, const void* train,
                                    const sift_keypoint* t_kpts, const int* t_offsets, int t_cap, const double* H,
                                    const int* found, float radius, int rows, int cols, int k, int* idx,
                                    float* dist) {
  int rc = check_window(c, metric, query, q_kpts, q_offsets, n_segments, q_cap, train, t_kpts, t_cap, radius, rows,
                        cols, k, idx, dist);
  if (rc || n_segments == 0 || q_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  const int n_grids = t_offsets ? n_segments : 1;
  const WindowGrid G = window_grid(radius, rows, cols, t_cap, n_grids);
  const size_t row = metric_row_bytes(metric);
  WindowHost S;
  if ((rc = carve(c, &S, [&](Carver& a) {
         return window_host_layout(a, n_segments, q_cap, t_cap, row, t_offsets != nullptr, H != nullptr,
                                   found != nullptr, k, n_grids, G.nx * G.ny);
       })))
    return rc;
  const size_t ob = (size_t)(n_segments + 1) * sizeof(int);
  HIP_TRY(c, hipMemcpyAsync(S.query, query, q_cap * row, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.q_kpts, q_kpts, (size_t)q_cap * sizeof(sift_keypoint), hipMemcpyHostToDevice,
                            c->stream));
  if (t_cap) {
    HIP_TRY(c, hipMemcpyAsync(S.train, train, t_cap * row, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(S.t_kpts, t_kpts, (size_t)t_cap * sizeof(sift_keypoint), hipMemcpyHostToDevice,
                              c->stream));
  }
  HIP_TRY(c, hipMemcpyAsync(S.q_off, q_offsets, ob, hipMemcpyHostToDevice, c->stream));
  if (S.t_off) HIP_TRY(c, hipMemcpyAsync(S.t_off, t_offsets, ob, hipMemcpyHostToDevice, c->stream));
  if (S.H)
    HIP_TRY(c, hipMemcpyAsync(S.H, H, (size_t)n_segments * 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (S.found)
    HIP_TRY(c, hipMemcpyAsync(S.found, found, (size_t)n_segments * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if ((rc = window_device(c, metric, S.query, S.q_kpts, S.q_off, n_segments, q_cap, S.train, S.t_kpts, S.t_off, t_cap,
                          S.H, S.found, radius, k, S.idx, S.dist, G, S.win)))
    return rc;
  return copy_back_live_rows(c, q_offsets, n_segments, q_cap, k, idx, dist, S.idx, S.dist);
}

int sift_knn_match_epipolar_segmented_device(sift_ctx* c, int metric, const void* d_query,
                                             const sift_keypoint* d_q_kpts, const int* d_q_offsets, int n_segments,
                                             int q_cap, const void* d_train, const sift_keypoint* d_t_kpts,
                                             const int* d_t_offsets, int t_cap, const double* d_F, const int* d_found,
                                             double band, float radius, int rows, int cols, int k, int* d_idx,
                                             float* d_dist) {
  int rc = check_epipolar(c, metric, d_query, d_q_kpts, d_q_offsets, n_segments, q_cap, d_train, d_t_kpts, t_cap, band,
                          radius, rows, cols, k, d_idx, d_dist);
  if (rc || n_segments == 0 || q_cap == 0) return rc;
  if (!aligned16(d_query, d_train)) return fail(c, SIFT_E_INVALID, kRowsUnaligned);
  (void)hipSetDevice(c->device);
  const int n_grids = d_t_offsets ? n_segments : 1;
  const WindowGrid G = epipolar_grid(radius, d_F ? band : INFINITY, rows, cols, t_cap, n_grids);
  WindowParts P;
  if ((rc = carve(c, &P, [&](Carver& a) { return window_layout(a, n_grids, G.nx * G.ny, t_cap); }))) return rc;
  return epipolar_device(c, metric, d_query, d_q_kpts, d_q_offsets, n_segments, q_cap, d_train, d_t_kpts, d_t_offsets,
                         t_cap, d_F, d_found, band, radius, k, d_idx, d_dist, G, P);
}

int sift_knn_match_epipolar_segmented(sift_ctx* c, int metric, const void* query, const sift_keypoint* q_kpts,
                                      const int* q_offsets, int n_segments, int q_cap, const void* train,
                                      const sift_keypoint* t_kpts, const int* t_offsets, int t_cap, const double* F,
                                      const int* found, double band, float radius, int rows, int cols, int k, int* idx,
                                      float* dist) {
  int rc = check_epipolar(c, metric, query, q_kpts, q_offsets, n_segments, q_cap, train, t_kpts, t_cap, band, radius,
                          rows, cols, k, idx, dist);
  if (rc || n_segments == 0 || q_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  const int n_grids = t_offsets ? n_segments : 1;
  const WindowGrid G = epipolar_grid(radius, F ? band : INFINITY, rows, cols, t_cap, n_grids);
  const size_t row = metric_row_bytes(metric);
  EpipolarHost S;
  if ((rc = carve(c, &S, [&](Carver& a) {
         return epipolar_host_layout(a, n_segments, q_cap, t_cap, row, t_offsets != nullptr, F != nullptr,
                                     found != nullptr, k, n_grids, G.nx * G.ny);
       })))
    return rc;
  const size_t ob = (size_t)(n_segments + 1) * sizeof(int);
  HIP_TRY(c, hipMemcpyAsync(S.query, query, q_cap * row, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.q_kpts, q_kpts, (size_t)q_cap * sizeof(sift_keypoint), hipMemcpyHostToDevice,
                            c->stream));
  if (t_cap) {
    HIP_TRY(c, hipMemcpyAsync(S.train, train, t_cap * row, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(S.t_kpts, t_kpts, (size_t)t_cap * sizeof(sift_keypoint), hipMemcpyHostToDevice,
                              c->stream));
  }
  HIP_TRY(c, hipMemcpyAsync(S.q_off, q_offsets, ob, hipMemcpyHostToDevice, c->stream));
  if (S.t_off) HIP_TRY(c, hipMemcpyAsync(S.t_off, t_offsets, ob, hipMemcpyHostToDevice, c->stream));
  if (S.F)
    HIP_TRY(c, hipMemcpyAsync(S.F, F, (size_t)n_segments * 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (S.found)
    HIP_TRY(c, hipMemcpyAsync(S.found, found, (size_t)n_segments * sizeof(int), hipMemcpyHostToDevice, c->stream));
  if ((rc = epipolar_device(c, metric, S.query, S.q_kpts, S.q_off, n_segments, q_cap, S.train, S.t_kpts, S.t_off,
                            t_cap, S.F, S.found, band, radius, k, S.idx, S.dist, G, S.win)))
    return rc;
  return copy_back_live_rows(c, q_offsets, n_segments, q_cap, k, idx, dist, S.idx, S.dist);
}

int sift_bgr8_to_gray_device(sift_ctx* c, const uint8_t* d_bgr, int batch, int rows, int cols, size_t row_stride,
                             size_t img_stride, int out_rows, int out_cols, float* d_gray, size_t out_row_stride,
                             size_t out_img_stride) {
  if (int rc = check_bgr(c, d_bgr, batch, rows, cols, out_rows, out_cols, d_gray)) return rc;
  if (row_stride < (size_t)cols * 3 || (batch > 1 && img_stride < row_stride * rows))
    return fail(c, SIFT_E_INVALID, "source strides too small");
  if (out_row_stride % sizeof(float) || out_img_stride % sizeof(float) ||
      out_row_stride < (size_t)out_cols * sizeof(float) ||
      (batch > 1 && out_img_stride < out_row_stride * out_rows))
    return fail(c, SIFT_E_INVALID, "output strides");
  (void)hipSetDevice(c->device);
  {
    StageScope s(c, ST_UPLOAD, 0, (3.0 * rows * cols + 4.0 * out_rows * out_cols) * batch);
    launch_bgr8_gray(c->stream, d_bgr, (long long)row_stride, (long long)img_stride, rows, cols, d_gray,
                     (long long)(out_row_stride / sizeof(float)), (long long)(out_img_stride / sizeof(float)),
                     out_rows, out_cols, batch);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

int sift_bgr8_to_gray(sift_ctx* c, const uint8_t* bgr, int rows, int cols, size_t row_stride, int out_rows,
                      int out_cols, float* gray) {
  int rc = check_bgr(c, bgr, 1, rows, cols, out_rows, out_cols, gray);
  if (rc) return rc;
  if (row_stride < (size_t)cols * 3) return fail(c, SIFT_E_INVALID, "row stride too small");
  (void)hipSetDevice(c->device);
  BgrHost S;  // the matcher's scratch doubles as staging here
  if ((rc = carve(c, &S, [&](Carver& a) { return bgr_host_layout(a, rows, row_stride, out_rows, out_cols); })))
    return rc;
  // a strided view (an ROI) owns no padding after its last row: copy only what the image owns
  const size_t owned = (size_t)(rows - 1) * row_stride + (size_t)cols * 3;
  HIP_TRY(c, hipMemcpyAsync(S.src, bgr, owned, hipMemcpyHostToDevice, c->stream));
  if ((rc = sift_bgr8_to_gray_device(c, S.src, 1, rows, cols, row_stride, 0, out_rows, out_cols, S.gray,
                                     (size_t)out_cols * sizeof(float), 0)))
    return rc;
  HIP_TRY(c, hipMemcpyAsync(gray, S.gray, (size_t)out_rows * out_cols * sizeof(float), hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

// ---- the doubled image (upsample.hip): cv::resize to twice the size, INTER_LINEAR on CV_32F ----
int sift_upsample2x_device(sift_ctx* c, const float* d_src, int batch, int rows, int cols, size_t row_stride,
                           size_t img_stride, float* d_dst, size_t out_row_stride, size_t out_img_stride) {
  if (!c) return SIFT_E_INVALID;
  if (!d_src || !d_dst) return fail(c, SIFT_E_INVALID, "null buffer");
  if (batch < 1 || rows < 1 || cols < 1) return fail(c, SIFT_E_INVALID, "empty image");
  if (rows > (1 << 30) || cols > (1 << 30)) return fail(c, SIFT_E_SIZE, "the doubled dimensions exceed an int");
  if (row_stride < (size_t)cols || (batch > 1 && img_stride < row_stride * rows))
    return fail(c, SIFT_E_INVALID, "source strides too small");
  if (out_row_stride < (size_t)cols * 2 || (batch > 1 && out_img_stride < out_row_stride * rows * 2))
    return fail(c, SIFT_E_INVALID, "output strides too small");
  (void)hipSetDevice(c->device);
  {
    StageScope s(c, ST_UPSAMPLE, 0, 20.0 * rows * cols * batch);
    launch_upsample2x(c->stream, d_src, (long long)row_stride, (long long)img_stride, rows, cols, d_dst,
                      (long long)out_row_stride, (long long)out_img_stride, batch);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

int sift_upsample2x(sift_ctx* c, const float* src, int rows, int cols, size_t row_stride_bytes, float* dst) {
  if (!c) return SIFT_E_INVALID;
  if (!src || !dst) return fail(c, SIFT_E_INVALID, "null buffer");
  if (rows < 1 || cols < 1) return fail(c, SIFT_E_INVALID, "empty image");
  if (rows > (1 << 30) || cols > (1 << 30)) return fail(c, SIFT_E_SIZE, "the doubled dimensions exceed an int");
  if (row_stride_bytes == 0) row_stride_bytes = (size_t)cols * sizeof(float);
  if (row_stride_bytes % sizeof(float) || row_stride_bytes < (size_t)cols * sizeof(float))
    return fail(c, SIFT_E_INVALID, "row stride must be a multiple of 4 bytes and at least cols * 4");
  (void)hipSetDevice(c->device);
  const size_t stride = row_stride_bytes / sizeof(float);
  UpsampleHost S;  // the matcher's scratch doubles as staging here
  int rc = carve(c, &S, [&](Carver& a) { return upsample_host_layout(a, rows, cols, stride); });
  if (rc) return rc;
  // a strided view (an ROI) owns no padding after its last row: copy only what the image owns
  const size_t owned = ((size_t)(rows - 1) * stride + (size_t)cols) * sizeof(float);
  HIP_TRY(c, hipMemcpyAsync(S.src, src, owned, hipMemcpyHostToDevice, c->stream));
  if ((rc = sift_upsample2x_device(c, S.src, 1, rows, cols, stride, 0, S.dst, (size_t)cols * 2, 0))) return rc;
  HIP_TRY(c, hipMemcpyAsync(dst, S.dst, (size_t)4 * rows * cols * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

// ---- findHomography(RANSAC) + perspectiveTransform, src/main.cpp:54-62 ----
int sift_find_homography(const float* src_xy, const float* dst_xy, int n, double ransac_thresh, int max_iters,
                         double confidence, double* H, unsigned char* inlier_mask) {
  if (!src_xy || !dst_xy || !H || n < 0) return SIFT_E_INVALID;
  if (!find_homography_ransac(src_xy, dst_xy, n, ransac_thresh, max_iters, confidence, H, inlier_mask)) {
    for (int i = 0; i < 9; ++i) H[i] = 0;  // OpenCV returns an empty Mat
    return SIFT_E_INVALID;
  }
  return SIFT_OK;
}

int sift_perspective_transform(const double* H, const float* xy, int n, float* out_xy) {
  if (!H || n < 0 || (n > 0 && (!xy || !out_xy))) return SIFT_E_INVALID;
  perspective_transform(H, xy, n, out_xy);
  return SIFT_OK;
}

// ---- the same for every segment of the ratio stage's point pairs, in stream order ----
int sift_find_homography_segmented_device(sift_ctx* c, const float* d_src_xy, const float* d_dst_xy,
                                          const int* d_m_offsets, int n_segments, int m_cap, double ransac_thresh,
                                          int max_iters, double confidence, double* d_H, int* d_found,
                                          unsigned char* d_inlier_mask) {
  int rc = check_homog(c, d_src_xy, d_dst_xy, d_m_offsets, n_segments, m_cap, d_H, d_found);
  if (rc || n_segments == 0 || m_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  HomogParts P;
  if ((rc = carve(c, &P, [&](Carver& a) { return homog_layout(a, n_segments, m_cap); }))) return rc;
  return homog_device(c, d_src_xy, d_dst_xy, d_m_offsets, n_segments, m_cap, ransac_thresh, max_iters, confidence,
                      d_H, d_found, d_inlier_mask, P);
}

int sift_find_homography_segmented(sift_ctx* c, const float* src_xy, const float* dst_xy, const int* m_offsets,
                                   int n_segments, int m_cap, double ransac_thresh, int max_iters, double confidence,
                                   double* H, int* found, unsigned char* inlier_mask) {
  int rc = check_homog(c, src_xy, dst_xy, m_offsets, n_segments, m_cap, H, found);
  if (rc || n_segments == 0 || m_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  HomogHost S;
  if ((rc = carve(c, &S, [&](Carver& a) { return homog_host_layout(a, n_segments, m_cap); }))) return rc;
  const size_t xyb = (size_t)m_cap * 2 * sizeof(float), ob = (size_t)(n_segments + 1) * sizeof(int);
  HIP_TRY(c, hipMemcpyAsync(S.src_xy, src_xy, xyb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.dst_xy, dst_xy, xyb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.m_off, m_offsets, ob, hipMemcpyHostToDevice, c->stream));
  if ((rc = homog_device(c, S.src_xy, S.dst_xy, S.m_off, n_segments, m_cap, ransac_thresh, max_iters, confidence, S.H,
                         S.found, inlier_mask ? S.mask : nullptr, S.parts)))
    return rc;
  HIP_TRY(c, hipMemcpyAsync(H, S.H, (size_t)n_segments * 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(found, S.found, (size_t)n_segments * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  // only the segments' mask bytes come back: the others are left untouched, as in the device form
  const int lo = clamp_off(m_offsets[0], m_cap), hi = clamp_off(m_offsets[n_segments], m_cap);
  if (inlier_mask && hi > lo)
    HIP_TRY(c, hipMemcpyAsync(inlier_mask + lo, S.mask + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

// ---- estimateAffine2D / estimateAffinePartial2D: one pair set on the host, a batch on the device ----
int sift_estimate_affine(const float* src_xy, const float* dst_xy, int n, int model, double ransac_thresh,
                         int max_iters, double confidence, double* A, unsigned char* inlier_mask) {
  if (!src_xy || !dst_xy || !A || n < 0) return SIFT_E_INVALID;
  if (!estimate_affine_ransac(src_xy, dst_xy, n, model, ransac_thresh, max_iters, confidence, A, inlier_mask)) {
    for (int i = 0; i < 6; ++i) A[i] = 0;  // OpenCV returns an empty Mat
    if (inlier_mask) memset(inlier_mask, 0, (size_t)n);
    return SIFT_E_INVALID;
  }
  return SIFT_OK;
}

int sift_estimate_affine_segmented_device(sift_ctx* c, const float* d_src_xy, const float* d_dst_xy,
                                          const int* d_m_offsets, int n_segments, int m_cap, int model,
                                          double ransac_thresh, int max_iters, double confidence, double* d_H,
                                          int* d_found, unsigned char* d_inlier_mask) {
  int rc = check_affine(c, d_src_xy, d_dst_xy, d_m_offsets, n_segments, m_cap, model, d_H, d_found);
  if (rc || n_segments == 0 || m_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  return affine_device(c, d_src_xy, d_dst_xy, d_m_offsets, n_segments, m_cap, model, ransac_thresh, max_iters,
                       confidence, d_H, d_found, d_inlier_mask);
}

int sift_estimate_affine_segmented(sift_ctx* c, const float* src_xy, const float* dst_xy, const int* m_offsets,
                                   int n_segments, int m_cap, int model, double ransac_thresh, int max_iters,
                                   double confidence, double* H, int* found, unsigned char* inlier_mask) {
  int rc = check_affine(c, src_xy, dst_xy, m_offsets, n_segments, m_cap, model, H, found);
  if (rc || n_segments == 0 || m_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  AffineHost S;
  if ((rc = carve(c, &S, [&](Carver& a) { return affine_host_layout(a, n_segments, m_cap); }))) return rc;
  const size_t xyb = (size_t)m_cap * 2 * sizeof(float), ob = (size_t)(n_segments + 1) * sizeof(int);
  HIP_TRY(c, hipMemcpyAsync(S.src_xy, src_xy, xyb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.dst_xy, dst_xy, xyb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.m_off, m_offsets, ob, hipMemcpyHostToDevice, c->stream));
  if ((rc = affine_device(c, S.src_xy, S.dst_xy, S.m_off, n_segments, m_cap, model, ransac_thresh, max_iters,
                          confidence, S.H, S.found, inlier_mask ? S.mask : nullptr)))
    return rc;
  HIP_TRY(c, hipMemcpyAsync(H, S.H, (size_t)n_segments * 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(found, S.found, (size_t)n_segments * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  // only the segments' mask bytes come back: the others are left untouched, as in the device form
  const int lo = clamp_off(m_offsets[0], m_cap), hi = clamp_off(m_offsets[n_segments], m_cap);
  if (inlier_mask && hi > lo)
    HIP_TRY(c, hipMemcpyAsync(inlier_mask + lo, S.mask + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

// ---- findFundamentalMat(FM_RANSAC): one pair set on the host, a batch on the device ----
int sift_find_fundamental(const float* src_xy, const float* dst_xy, int n, double ransac_thresh, int max_iters,
                          double confidence, double* F, unsigned char* inlier_mask) {
  if (!src_xy || !dst_xy || !F || n < 0) return SIFT_E_INVALID;
  if (!find_fundamental_ransac(src_xy, dst_xy, n, ransac_thresh, max_iters, confidence, F, inlier_mask)) {
    for (int i = 0; i < 9; ++i) F[i] = 0;  // OpenCV returns an empty Mat
    if (inlier_mask) memset(inlier_mask, 0, (size_t)n);
    return SIFT_E_INVALID;
  }
  return SIFT_OK;
}

int sift_find_fundamental_segmented_device(sift_ctx* c, const float* d_src_xy, const float* d_dst_xy,
                                           const int* d_m_offsets, int n_segments, int m_cap, double ransac_thresh,
                                           int max_iters, double confidence, double* d_F, int* d_found,
                                           unsigned char* d_inlier_mask) {
  int rc = check_homog(c, d_src_xy, d_dst_xy, d_m_offsets, n_segments, m_cap, d_F, d_found);
  if (rc || n_segments == 0 || m_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  return fundamental_device(c, d_src_xy, d_dst_xy, d_m_offsets, n_segments, m_cap, ransac_thresh, max_iters,
                            confidence, d_F, d_found, d_inlier_mask);
}

int sift_find_fundamental_segmented(sift_ctx* c, const float* src_xy, const float* dst_xy, const int* m_offsets,
                                    int n_segments, int m_cap, double ransac_thresh, int max_iters, double confidence,
                                    double* F, int* found, unsigned char* inlier_mask) {
  int rc = check_homog(c, src_xy, dst_xy, m_offsets, n_segments, m_cap, F, found);
  if (rc || n_segments == 0 || m_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  AffineHost S;  // the same staging as the affine estimate's (scratch.hpp)
  if ((rc = carve(c, &S, [&](Carver& a) { return affine_host_layout(a, n_segments, m_cap); }))) return rc;
  const size_t xyb = (size_t)m_cap * 2 * sizeof(float), ob = (size_t)(n_segments + 1) * sizeof(int);
  HIP_TRY(c, hipMemcpyAsync(S.src_xy, src_xy, xyb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.dst_xy, dst_xy, xyb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.m_off, m_offsets, ob, hipMemcpyHostToDevice, c->stream));
  if ((rc = fundamental_device(c, S.src_xy, S.dst_xy, S.m_off, n_segments, m_cap, ransac_thresh, max_iters,
                               confidence, S.H, S.found, inlier_mask ? S.mask : nullptr)))
    return rc;
  HIP_TRY(c, hipMemcpyAsync(F, S.H, (size_t)n_segments * 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(found, S.found, (size_t)n_segments * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  // only the segments' mask bytes come back: the others are left untouched, as in the device form
  const int lo = clamp_off(m_offsets[0], m_cap), hi = clamp_off(m_offsets[n_segments], m_cap);
  if (inlier_mask && hi > lo)
    HIP_TRY(c, hipMemcpyAsync(inlier_mask + lo, S.mask + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

// ---- recoverPose / triangulatePoints: one pair set on the host, a batch on the device ----
int sift_recover_pose(const double* F, const double* K_src, const double* K_dst, const float* src_xy,
                      const float* dst_xy, int n, const unsigned char* mask_in, double distance_thresh, double* pose,
                      double* E, unsigned char* mask_out, double* xyz, int* n_good) {
  if (!F || !K_src || !K_dst || !pose || !n_good || n < 0 || (n > 0 && (!src_xy || !dst_xy)))
    return SIFT_E_INVALID;
  // none: recover_pose has zeroed every output
  return recover_pose(F, K_src, K_dst, src_xy, dst_xy, n, mask_in, distance_thresh, pose, E, mask_out, xyz, n_good)
             ? SIFT_OK
             : SIFT_E_INVALID;
}

int sift_recover_pose_segmented_device(sift_ctx* c, const float* d_src_xy, const float* d_dst_xy,
                                       const int* d_m_offsets, int n_segments, int m_cap, const double* d_F,
                                       const int* d_found, const double* d_K_src, const double* d_K_dst,
                                       int k_per_segment, const unsigned char* d_mask_in, double distance_thresh,
                                       double* d_pose, double* d_E, int* d_pose_found, int* d_n_good,
                                       unsigned char* d_mask_out, double* d_xyz) {
  int rc = check_pose(c, d_src_xy, d_dst_xy, d_m_offsets, n_segments, m_cap, d_F, d_found, d_K_src, d_K_dst,
                      k_per_segment, d_pose, d_pose_found, d_n_good);
  if (rc || n_segments == 0 || m_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  return pose_device(c, d_src_xy, d_dst_xy, d_m_offsets, n_segments, m_cap, d_F, d_found, d_K_src, d_K_dst,
                     k_per_segment, d_mask_in, distance_thresh, d_pose, d_E, d_pose_found, d_n_good, d_mask_out,
                     d_xyz);
}

int sift_recover_pose_segmented(sift_ctx* c, const float* src_xy, const float* dst_xy, const int* m_offsets,
                                int n_segments, int m_cap, const double* F, const int* found, const double* K_src,
                                const double* K_dst, int k_per_segment, const unsigned char* mask_in,
                                double distance_thresh, double* pose, double* E, int* pose_found, int* n_good,
                                unsigned char* mask_out, double* xyz) {
  int rc = check_pose(c, src_xy, dst_xy, m_offsets, n_segments, m_cap, F, found, K_src, K_dst, k_per_segment, pose,
                      pose_found, n_good);
  if (rc || n_segments == 0 || m_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  PoseHost S;
  if ((rc = carve(c, &S, [&](Carver& a) { return pose_host_layout(a, n_segments, m_cap, k_per_segment); }))) return rc;
  const size_t xyb = (size_t)m_cap * 2 * sizeof(float), ob = (size_t)(n_segments + 1) * sizeof(int);
  const size_t kb = (k_per_segment ? (size_t)n_segments : 1) * 9 * sizeof(double);
  const int lo = clamp_off(m_offsets[0], m_cap), hi = clamp_off(m_offsets[n_segments], m_cap);
  HIP_TRY(c, hipMemcpyAsync(S.in.src_xy, src_xy, xyb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.in.dst_xy, dst_xy, xyb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.in.m_off, m_offsets, ob, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.in.H, F, (size_t)n_segments * 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.in.found, found, (size_t)n_segments * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.K_src, K_src, kb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.K_dst, K_dst, kb, hipMemcpyHostToDevice, c->stream));
  if (mask_in) HIP_TRY(c, hipMemcpyAsync(S.in.mask, mask_in, (size_t)m_cap, hipMemcpyHostToDevice, c->stream));
  // rows of [lo, hi) that no segment owns (offsets that skip rows) go out and come back as they are
  if (mask_out && hi > lo)
    HIP_TRY(c, hipMemcpyAsync(S.mask_out + lo, mask_out + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, c->stream));
  if (xyz && hi > lo)
    HIP_TRY(c, hipMemcpyAsync(S.xyz + (size_t)lo * 3, xyz + (size_t)lo * 3, (size_t)(hi - lo) * 3 * sizeof(double),
                              hipMemcpyHostToDevice, c->stream));
  if ((rc = pose_device(c, S.in.src_xy, S.in.dst_xy, S.in.m_off, n_segments, m_cap, S.in.H, S.in.found, S.K_src,
                        S.K_dst, k_per_segment, mask_in ? S.in.mask : nullptr, distance_thresh, S.pose,
                        E ? S.E : nullptr, S.pose_found, S.n_good, mask_out ? S.mask_out : nullptr,
                        xyz ? S.xyz : nullptr)))
    return rc;
  HIP_TRY(c, hipMemcpyAsync(pose, S.pose, (size_t)n_segments * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (E) HIP_TRY(c, hipMemcpyAsync(E, S.E, (size_t)n_segments * 9 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(pose_found, S.pose_found, (size_t)n_segments * sizeof(int), hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipMemcpyAsync(n_good, S.n_good, (size_t)n_segments * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  // only the segments' rows come back: the others are left untouched, as in the device form
  if (mask_out && hi > lo)
    HIP_TRY(c, hipMemcpyAsync(mask_out + lo, S.mask_out + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, c->stream));
  if (xyz && hi > lo)
    HIP_TRY(c, hipMemcpyAsync(xyz + (size_t)lo * 3, S.xyz + (size_t)lo * 3, (size_t)(hi - lo) * 3 * sizeof(double),
                              hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

int sift_triangulate_points(const double* P_src, const double* P_dst, const float* src_xy, const float* dst_xy, int n,
                            double* xyzw) {
  if (!P_src || !P_dst || n < 0 || (n > 0 && (!src_xy || !dst_xy || !xyzw))) return SIFT_E_INVALID;
  triangulate_points(P_src, P_dst, src_xy, dst_xy, n, xyzw);
  return SIFT_OK;
}

int sift_triangulate_points_segmented_device(sift_ctx* c, const float* d_src_xy, const float* d_dst_xy,
                                             const int* d_m_offsets, int n_segments, int m_cap, const double* d_P_src,
                                             const double* d_P_dst, double* d_xyzw) {
  if (!c) return SIFT_E_INVALID;
  if (n_segments < 0 || m_cap < 0) return fail(c, SIFT_E_INVALID, "negative count");
  if (n_segments == 0 || m_cap == 0) return SIFT_OK;
  if (!d_src_xy || !d_dst_xy || !d_m_offsets || !d_P_src || !d_P_dst || !d_xyzw)
    return fail(c, SIFT_E_INVALID, "null buffer");
  (void)hipSetDevice(c->device);
  {
    StageScope sc(c, ST_TRI_SEG);  // the work depends on offsets only the device knows
    launch_triangulate_seg(c->stream, d_src_xy, d_dst_xy, d_m_offsets, n_segments, m_cap, d_P_src, d_P_dst, d_xyzw);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// ---- solveP3P / solvePnPRansac: one row set on the host, a batch on the device ----
int sift_solve_p3p(const double* xyz, const float* xy, const double* K, double* poses, int* n_solutions) {
  if (!xyz || !xy || !K || !poses || !n_solutions) return SIFT_E_INVALID;
  *n_solutions = solve_p3p(xyz, xy, K, poses);
  return SIFT_OK;
}

int sift_solve_pnp(const double* xyz, const float* xy, int n, const unsigned char* row_mask, const double* K,
                   double reproj_thresh, int max_iters, double confidence, double* pose, unsigned char* inlier_mask,
                   int* n_inliers) {
  if (!K || !pose || !n_inliers || n < 0 || (n > 0 && (!xyz || !xy))) return SIFT_E_INVALID;
  // none: solve_pnp_ransac has zeroed every output
  return solve_pnp_ransac(xyz, xy, n, row_mask, K, reproj_thresh, max_iters, confidence, pose, inlier_mask, n_inliers)
             ? SIFT_OK
             : SIFT_E_INVALID;
}

int sift_solve_pnp_segmented_device(sift_ctx* c, const double* d_xyz, const float* d_xy, const int* d_m_offsets,
                                    int n_segments, int m_cap, const unsigned char* d_row_mask, const double* d_K,
                                    int k_per_segment, double reproj_thresh, int max_iters, double confidence,
                                    double* d_pose, int* d_found, int* d_n_inliers, unsigned char* d_inlier_mask) {
  int rc = check_pnp(c, d_xyz, d_xy, d_m_offsets, n_segments, m_cap, d_K, k_per_segment, d_pose, d_found, d_n_inliers);
  if (rc || n_segments == 0 || m_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  return pnp_device(c, d_xyz, d_xy, d_m_offsets, n_segments, m_cap, d_row_mask, d_K, k_per_segment, reproj_thresh,
                    max_iters, confidence, d_pose, d_found, d_n_inliers, d_inlier_mask);
}

int sift_solve_pnp_segmented(sift_ctx* c, const double* xyz, const float* xy, const int* m_offsets, int n_segments,
                             int m_cap, const unsigned char* row_mask, const double* K, int k_per_segment,
                             double reproj_thresh, int max_iters, double confidence, double* pose, int* found,
                             int* n_inliers, unsigned char* inlier_mask) {
  int rc = check_pnp(c, xyz, xy, m_offsets, n_segments, m_cap, K, k_per_segment, pose, found, n_inliers);
  if (rc || n_segments == 0 || m_cap == 0) return rc;
  (void)hipSetDevice(c->device);
  PnpHost S;
  if ((rc = carve(c, &S, [&](Carver& a) { return pnp_host_layout(a, n_segments, m_cap, k_per_segment); }))) return rc;
  const size_t ob = (size_t)(n_segments + 1) * sizeof(int);
  const size_t kb = (k_per_segment ? (size_t)n_segments : 1) * 9 * sizeof(double);
  int lo = m_cap, hi = 0;  // the span the segments' rows lie in, backwards and overlapping ones included
  for (int b = 0; b <= n_segments; ++b) {
    const int v = clamp_off(m_offsets[b], m_cap);
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  HIP_TRY(c, hipMemcpyAsync(S.xyz, xyz, (size_t)m_cap * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.xy, xy, (size_t)m_cap * 2 * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.m_off, m_offsets, ob, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.K, K, kb, hipMemcpyHostToDevice, c->stream));
  if (row_mask) HIP_TRY(c, hipMemcpyAsync(S.row_mask, row_mask, (size_t)m_cap, hipMemcpyHostToDevice, c->stream));
  // bytes of [lo, hi) that no segment owns (offsets that skip rows) go out and come back as they are
  if (inlier_mask && hi > lo)
    HIP_TRY(c, hipMemcpyAsync(S.mask + lo, inlier_mask + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, c->stream));
  if ((rc = pnp_device(c, S.xyz, S.xy, S.m_off, n_segments, m_cap, row_mask ? S.row_mask : nullptr, S.K, k_per_segment,
                       reproj_thresh, max_iters, confidence, S.pose, S.found, S.n_inliers,
                       inlier_mask ? S.mask : nullptr)))
    return rc;
  HIP_TRY(c, hipMemcpyAsync(pose, S.pose, (size_t)n_segments * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(found, S.found, (size_t)n_segments * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(n_inliers, S.n_inliers, (size_t)n_segments * sizeof(int), hipMemcpyDeviceToHost,
                            c->stream));
  // only the segments' mask bytes come back: the others are left untouched, as in the device form
  if (inlier_mask && hi > lo)
    HIP_TRY(c, hipMemcpyAsync(inlier_mask + lo, S.mask + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

// ---- the join of two record tables: one segment on the host, a batch on the device ----
int sift_join_matches(const sift_match* a, int na, int a_key_side, const unsigned char* a_mask, const double* a_xyz,
                      const sift_match* b, int nb, int b_key_side, const unsigned char* b_mask, const float* b_xy,
                      int n_keys, double* xyz_out, float* xy_out, int* a_row, int* b_row, unsigned char* b_joined) {
  if (na < 0 || nb < 0 || n_keys < 0 || !join_side_ok(a_key_side) || !join_side_ok(b_key_side) || (na > 0 && !a) ||
      (nb > 0 && !b) || (xyz_out && !a_xyz) || (xy_out && !b_xy))
    return SIFT_E_INVALID;
  return join_matches(a, na, a_key_side, a_mask, a_xyz, b, nb, b_key_side, b_mask, b_xy, n_keys, xyz_out, xy_out,
                      a_row, b_row, b_joined);
}

int sift_join_matches_segmented_device(sift_ctx* c, const sift_match* d_a, const int* d_a_offsets, int a_cap,
                                       int a_key_side, const unsigned char* d_a_mask, const double* d_a_xyz,
                                       const sift_match* d_b, const int* d_b_offsets, int b_cap, int b_key_side,
                                       const unsigned char* d_b_mask, const float* d_b_xy, const int* d_key_offsets,
                                       int key_cap, int n_segments, double* d_xyz_out, float* d_xy_out, int* d_a_row,
                                       int* d_b_row, unsigned char* d_b_joined, int j_cap, int* d_j_offsets) {
  const JoinCall J{d_a, d_a_offsets, a_cap, a_key_side, d_a_mask, d_a_xyz, d_b, d_b_offsets, b_cap, b_key_side, d_b_mask,
                   d_b_xy, d_key_offsets, key_cap, n_segments, d_xyz_out, d_xy_out, d_a_row, d_b_row, d_b_joined, j_cap,
                   d_j_offsets};
  int rc = check_join(c, J);
  if (rc || n_segments == 0) return rc;
  if (!aligned16(d_a, d_b)) return fail(c, SIFT_E_INVALID, "record tables must be 16-byte aligned");
  (void)hipSetDevice(c->device);
  if (b_cap == 0) {  // no B rows: nothing joins, and no byte of d_b_joined belongs to a segment
    HIP_TRY(c, hipMemsetAsync(d_j_offsets, 0, (size_t)(n_segments + 1) * sizeof(int), c->stream));
    return SIFT_OK;
  }
  JoinParts P;
  if ((rc = carve(c, &P, [&](Carver& s) { return join_layout(s, n_segments, key_cap, b_cap); }))) return rc;
  return join_device(c, J, P);
}

int sift_join_matches_segmented(sift_ctx* c, const sift_match* a, const int* a_offsets, int a_cap, int a_key_side,
                                const unsigned char* a_mask, const double* a_xyz, const sift_match* b,
                                const int* b_offsets, int b_cap, int b_key_side, const unsigned char* b_mask,
                                const float* b_xy, const int* key_offsets, int key_cap, int n_segments,
                                double* xyz_out, float* xy_out, int* a_row, int* b_row, unsigned char* b_joined,
                                int j_cap, int* j_offsets) {
  const JoinCall H{a, a_offsets, a_cap, a_key_side, a_mask, a_xyz, b, b_offsets, b_cap, b_key_side, b_mask, b_xy,
                   key_offsets, key_cap, n_segments, xyz_out, xy_out, a_row, b_row, b_joined, j_cap, j_offsets};
  int rc = check_join(c, H);
  if (rc || n_segments == 0) return rc;
  const size_t ob = (size_t)(n_segments + 1) * sizeof(int);
  if (b_cap == 0) {
    memset(j_offsets, 0, ob);
    return SIFT_OK;
  }
  (void)hipSetDevice(c->device);
  JoinHost S;
  const JoinHostHas has{a_mask != nullptr, a_xyz != nullptr, b_mask != nullptr, b_xy != nullptr, xyz_out != nullptr,
                        xy_out != nullptr, a_row != nullptr, b_row != nullptr, b_joined != nullptr};
  if ((rc = carve(c, &S, [&](Carver& s) { return join_host_layout(s, n_segments, a_cap, b_cap, key_cap, j_cap, has); })))
    return rc;
  int lo = b_cap, hi = 0;  // the span the segments' B rows lie in, backwards and overlapping ones included
  for (int s = 0; s <= n_segments; ++s) {
    const int v = clamp_off(b_offsets[s], b_cap);
    lo = v < lo ? v : lo;
    hi = v > hi ? v : hi;
  }
  const hipStream_t st = c->stream;
  if (a_cap) HIP_TRY(c, hipMemcpyAsync(S.a, a, (size_t)a_cap * sizeof(sift_match), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(S.a_off, a_offsets, ob, hipMemcpyHostToDevice, st));
  if (a_mask && a_cap) HIP_TRY(c, hipMemcpyAsync(S.a_mask, a_mask, (size_t)a_cap, hipMemcpyHostToDevice, st));
  if (a_xyz && a_cap)
    HIP_TRY(c, hipMemcpyAsync(S.a_xyz, a_xyz, (size_t)a_cap * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(S.b, b, (size_t)b_cap * sizeof(sift_match), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(S.b_off, b_offsets, ob, hipMemcpyHostToDevice, st));
  if (b_mask) HIP_TRY(c, hipMemcpyAsync(S.b_mask, b_mask, (size_t)b_cap, hipMemcpyHostToDevice, st));
  if (b_xy) HIP_TRY(c, hipMemcpyAsync(S.b_xy, b_xy, (size_t)b_cap * 2 * sizeof(float), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(S.key_off, key_offsets, ob, hipMemcpyHostToDevice, st));
  // bytes of [lo, hi) that no segment owns (offsets that skip rows) go out and come back as they are
  if (b_joined && hi > lo)
    HIP_TRY(c, hipMemcpyAsync(S.b_joined + lo, b_joined + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, st));
  const JoinCall D{S.a, S.a_off, a_cap, a_key_side, S.a_mask, S.a_xyz, S.b, S.b_off, b_cap, b_key_side, S.b_mask, S.b_xy,
                   S.key_off, key_cap, n_segments, S.xyz_out, S.xy_out, S.a_row, S.b_row, S.b_joined, j_cap, S.j_off};
  if ((rc = join_device(c, D, S.parts))) return rc;
  // the offsets come back first; then only the written rows
  HIP_TRY(c, hipMemcpyAsync(j_offsets, S.j_off, ob, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const size_t n = (size_t)(j_offsets[n_segments] < j_cap ? j_offsets[n_segments] : j_cap);
  if (n) {
    if (xyz_out) HIP_TRY(c, hipMemcpyAsync(xyz_out, S.xyz_out, n * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (xy_out) HIP_TRY(c, hipMemcpyAsync(xy_out, S.xy_out, n * 2 * sizeof(float), hipMemcpyDeviceToHost, st));
    if (a_row) HIP_TRY(c, hipMemcpyAsync(a_row, S.a_row, n * sizeof(int), hipMemcpyDeviceToHost, st));
    if (b_row) HIP_TRY(c, hipMemcpyAsync(b_row, S.b_row, n * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  if (b_joined && hi > lo)
    HIP_TRY(c, hipMemcpyAsync(b_joined + lo, S.b_joined + lo, (size_t)(hi - lo), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return SIFT_OK;
}

int sift_perspective_transform_segmented_device(sift_ctx* c, const double* d_H, const int* d_found, int n_segments,
                                                const float* d_xy, int n_pts, float* d_out_xy) {
  if (!c) return SIFT_E_INVALID;
  if (n_segments < 0 || n_pts < 0) return fail(c, SIFT_E_INVALID, "negative count");
  if (n_segments == 0 || n_pts == 0) return SIFT_OK;
  if (!d_H || !d_found || !d_xy || !d_out_xy) return fail(c, SIFT_E_INVALID, "null buffer");
  (void)hipSetDevice(c->device);
  {
    StageScope sc(c, ST_HOMOG_SEG, 0, 8.0 * n_pts * (n_segments + 1.0) + 76.0 * n_segments);
    launch_perspective_seg(c->stream, d_H, d_found, n_segments, d_xy, n_pts, d_out_xy);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

// ---- warpPerspective of every image of a batch by its own homography (warp.hip) ----
int sift_warp_perspective_segmented_device(sift_ctx* c, int pixel, int channels, const void* d_src, int rows, int cols,
                                           size_t row_stride, size_t img_stride, const double* d_H,
                                           const int* d_found, int n_segments, unsigned flags, void* d_dst,
                                           int out_rows, int out_cols, size_t out_row_stride,
                                           size_t out_img_stride) {
  if (!c) return SIFT_E_INVALID;
  if (n_segments < 0) return fail(c, SIFT_E_INVALID, "negative count");
  if (n_segments == 0) return SIFT_OK;
  size_t bpp = 0;
  if (int rc = check_warp(c, pixel, channels, d_src, rows, cols, d_H, flags, d_dst, out_rows, out_cols, &bpp))
    return rc;
  if (row_stride == 0) row_stride = (size_t)cols * bpp;
  if (out_row_stride == 0) out_row_stride = (size_t)out_cols * bpp;
  if (out_img_stride == 0) out_img_stride = out_row_stride * out_rows;
  if (row_stride < (size_t)cols * bpp || (img_stride != 0 && n_segments > 1 && img_stride < row_stride * rows))
    return fail(c, SIFT_E_INVALID, "source strides too small");
  if (out_row_stride < (size_t)out_cols * bpp || (n_segments > 1 && out_img_stride < out_row_stride * out_rows))
    return fail(c, SIFT_E_INVALID, "output strides too small");
  if (pixel == SIFT_PIXEL_F32 &&
      ((row_stride | img_stride | out_row_stride | out_img_stride) % sizeof(float) ||
       ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) % sizeof(float))))
    return fail(c, SIFT_E_INVALID, "float buffers and strides must be multiples of 4 bytes");
  (void)hipSetDevice(c->device);
  {
    StageScope s(c, ST_WARP, 0, 2.0 * bpp * out_rows * (double)out_cols * n_segments);
    launch_warp_perspective(c->stream, pixel == SIFT_PIXEL_U8, channels, d_src, (long long)row_stride,
                            (long long)img_stride, rows, cols, d_H, d_found, n_segments,
                            (flags & SIFT_WARP_INVERSE_MAP) != 0, d_dst, (long long)out_row_stride,
                            (long long)out_img_stride, out_rows, out_cols);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

int sift_warp_perspective(sift_ctx* c, int pixel, int channels, const void* src, int rows, int cols, size_t row_stride,
                          const double* H, unsigned flags, void* dst, int out_rows, int out_cols) {
  size_t bpp = 0;
  int rc = check_warp(c, pixel, channels, src, rows, cols, H, flags, dst, out_rows, out_cols, &bpp);
  if (rc) return rc;
  if (row_stride == 0) row_stride = (size_t)cols * bpp;
  if (row_stride < (size_t)cols * bpp || (pixel == SIFT_PIXEL_F32 && row_stride % sizeof(float)))
    return fail(c, SIFT_E_INVALID, "row stride too small for its row, or a float stride not a multiple of 4 bytes");
  const size_t out_row = (size_t)out_cols * bpp, out_bytes = out_row * out_rows;
  double M[9];
  if (!wmath::warp_matrix(H, (flags & SIFT_WARP_INVERSE_MAP) != 0, M)) {  // the kernel's own rule: nothing to run
    memset(dst, 0, out_bytes);
    return fail(c, SIFT_E_INVALID, "the homography warps to nothing (singular or non-finite)");
  }
  (void)hipSetDevice(c->device);
  WarpHost S;  // the matcher's scratch doubles as staging here
  if ((rc = carve(c, &S, [&](Carver& a) { return warp_host_layout(a, rows, row_stride, out_rows, out_row); })))
    return rc;
  // a strided view (an ROI) owns no padding after its last row: copy only what the image owns
  const size_t owned = (size_t)(rows - 1) * row_stride + (size_t)cols * bpp;
  HIP_TRY(c, hipMemcpyAsync(S.src, src, owned, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.H, H, 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = sift_warp_perspective_segmented_device(c, pixel, channels, S.src, rows, cols, row_stride, 0, S.H, nullptr,
                                                   1, flags, S.dst, out_rows, out_cols, out_row, 0)))
    return rc;
  HIP_TRY(c, hipMemcpyAsync(dst, S.dst, out_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

// ---- undistort of every image of a batch through one camera or its own (undistort.hip) ----
int sift_undistort_batch_device(sift_ctx* c, int pixel, int channels, const void* d_src, int rows, int cols,
                                size_t row_stride, size_t img_stride, const double* d_K, const double* d_dist,
                                const double* d_newK, int k_per_segment, int n, void* d_dst, int out_rows,
                                int out_cols, size_t out_row_stride, size_t out_img_stride) {
  if (!c) return SIFT_E_INVALID;
  if (n < 0) return fail(c, SIFT_E_INVALID, "negative count");
  if (n == 0) return SIFT_OK;
  size_t bpp = 0;
  if (int rc = check_undistort(c, pixel, channels, d_src, rows, cols, d_K, d_dist, k_per_segment, d_dst, out_rows,
                               out_cols, &bpp))
    return rc;
  if (row_stride == 0) row_stride = (size_t)cols * bpp;
  if (out_row_stride == 0) out_row_stride = (size_t)out_cols * bpp;
  if (out_img_stride == 0) out_img_stride = out_row_stride * out_rows;
  if (row_stride < (size_t)cols * bpp || (img_stride != 0 && n > 1 && img_stride < row_stride * rows))
    return fail(c, SIFT_E_INVALID, "source strides too small");
  if (out_row_stride < (size_t)out_cols * bpp || (n > 1 && out_img_stride < out_row_stride * out_rows))
    return fail(c, SIFT_E_INVALID, "output strides too small");
  if (pixel == SIFT_PIXEL_F32 &&
      ((row_stride | img_stride | out_row_stride | out_img_stride) % sizeof(float) ||
       ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst)) % sizeof(float))))
    return fail(c, SIFT_E_INVALID, "float buffers and strides must be multiples of 4 bytes");
  (void)hipSetDevice(c->device);
  {
    StageScope s(c, ST_UNDISTORT, 0, 2.0 * bpp * out_rows * (double)out_cols * n);
    launch_undistort(c->stream, pixel == SIFT_PIXEL_U8, channels, d_src, (long long)row_stride, (long long)img_stride,
                     rows, cols, d_K, d_dist, d_newK, k_per_segment, n, d_dst, (long long)out_row_stride,
                     (long long)out_img_stride, out_rows, out_cols);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

int sift_undistort(sift_ctx* c, int pixel, int channels, const void* src, int rows, int cols, size_t row_stride,
                   const double* K, const double* dist, const double* newK, void* dst, int out_rows, int out_cols) {
  size_t bpp = 0;
  int rc = check_undistort(c, pixel, channels, src, rows, cols, K, dist, 0, dst, out_rows, out_cols, &bpp);
  if (rc) return rc;
  if (row_stride == 0) row_stride = (size_t)cols * bpp;
  if (row_stride < (size_t)cols * bpp || (pixel == SIFT_PIXEL_F32 && row_stride % sizeof(float)))
    return fail(c, SIFT_E_INVALID, "row stride too small for its row, or a float stride not a multiple of 4 bytes");
  const size_t out_row = (size_t)out_cols * bpp, out_bytes = out_row * out_rows;
  umath::ImageCam cam;
  if (!umath::image_camera(K, dist, newK, cam)) {  // the kernel's own rule: nothing to run
    memset(dst, 0, out_bytes);
    return fail(c, SIFT_E_INVALID, "the camera undistorts to nothing (singular or non-finite)");
  }
  (void)hipSetDevice(c->device);
  UndistortHost S;  // the matcher's scratch doubles as staging here
  if ((rc = carve(c, &S, [&](Carver& a) { return undistort_host_layout(a, rows, row_stride, out_rows, out_row); })))
    return rc;
  // a strided view (an ROI) owns no padding after its last row: copy only what the image owns
  const size_t owned = (size_t)(rows - 1) * row_stride + (size_t)cols * bpp;
  HIP_TRY(c, hipMemcpyAsync(S.src, src, owned, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.K, K, 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.dist, dist, 8 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (newK) HIP_TRY(c, hipMemcpyAsync(S.newK, newK, 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = sift_undistort_batch_device(c, pixel, channels, S.src, rows, cols, row_stride, 0, S.K, S.dist,
                                        newK ? S.newK : nullptr, 0, 1, S.dst, out_rows, out_cols, out_row, 0)))
    return rc;
  HIP_TRY(c, hipMemcpyAsync(dst, S.dst, out_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

// ---- undistortPoints: one camera on the host, every segment of a batch on the device ----
int sift_undistort_points(const double* K, const double* dist, const double* P, int iters, const void* src, void* dst,
                          size_t xy_stride_bytes, int n) {
  if (!K || !dist || n < 0 || (n > 0 && (!src || !dst)) || !umath::iters_ok(iters) ||
      !umath::stride_ok(xy_stride_bytes))
    return SIFT_E_INVALID;
  // a camera with no rule: undistort_points has zeroed the rows
  return undistort_points(K, dist, P, iters, src, dst, xy_stride_bytes, n) ? SIFT_OK : SIFT_E_INVALID;
}

int sift_undistort_points_segmented_device(sift_ctx* c, const void* d_src, void* d_dst, size_t xy_stride_bytes,
                                           const int* d_m_offsets, int n_segments, int m_cap, const double* d_K,
                                           const double* d_dist, const double* d_P, int k_per_segment, int iters,
                                           int* d_ok) {
  int rc = check_undistort_points(c, d_src, d_dst, xy_stride_bytes, d_m_offsets, n_segments, m_cap, d_K, d_dist,
                                  k_per_segment, iters, d_ok);
  if (rc || n_segments == 0) return rc;
  (void)hipSetDevice(c->device);
  {
    StageScope sc(c, ST_UNDISTORT);  // the work depends on offsets only the device knows
    launch_undistort_points_seg(c->stream, d_src, d_dst, (long long)xy_stride_bytes, d_m_offsets, n_segments, m_cap,
                                d_K, d_dist, d_P, k_per_segment, iters, d_ok);
  }
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

int sift_undistort_points_segmented(sift_ctx* c, const void* src, void* dst, size_t xy_stride_bytes,
                                    const int* m_offsets, int n_segments, int m_cap, const double* K,
                                    const double* dist, const double* P, int k_per_segment, int iters, int* ok) {
  int rc = check_undistort_points(c, src, dst, xy_stride_bytes, m_offsets, n_segments, m_cap, K, dist, k_per_segment,
                                  iters, ok);
  if (rc || n_segments == 0) return rc;
  (void)hipSetDevice(c->device);
  UndistortPtsHost S;
  if ((rc = carve(c, &S, [&](Carver& a) {
         return undistort_pts_host_layout(a, n_segments, m_cap, xy_stride_bytes, k_per_segment);
       })))
    return rc;
  // the rows any segment can own: segments may run backwards, so every offset bounds them
  int lo = m_cap, hi = 0;
  for (int b = 0; b <= n_segments; ++b) {
    const int o = clamp_off(m_offsets[b], m_cap);
    lo = o < lo ? o : lo;
    hi = o > hi ? o : hi;
  }
  const size_t cams = k_per_segment ? (size_t)n_segments : 1;
  const size_t at = (size_t)lo * xy_stride_bytes, nb = hi > lo ? (size_t)(hi - lo) * xy_stride_bytes : 0;
  const bool in_place = src == dst;
  char* d_dst = reinterpret_cast<char*>(S.dst);
  char* d_src = in_place ? d_dst : reinterpret_cast<char*>(S.src);
  if (nb) {
    // the bytes of a row that are not its (x, y) go out and come back as they are
    HIP_TRY(c, hipMemcpyAsync(d_dst + at, static_cast<const char*>(dst) + at, nb, hipMemcpyHostToDevice, c->stream));
    if (!in_place)
      HIP_TRY(c, hipMemcpyAsync(d_src + at, static_cast<const char*>(src) + at, nb, hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(c, hipMemcpyAsync(S.m_off, m_offsets, (size_t)(n_segments + 1) * sizeof(int), hipMemcpyHostToDevice,
                            c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.K, K, cams * 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(S.dist, dist, cams * 8 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (P) HIP_TRY(c, hipMemcpyAsync(S.P, P, cams * 9 * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if ((rc = sift_undistort_points_segmented_device(c, d_src, d_dst, xy_stride_bytes, S.m_off, n_segments, m_cap, S.K,
                                                   S.dist, P ? S.P : nullptr, k_per_segment, iters, S.ok)))
    return rc;
  if (nb) HIP_TRY(c, hipMemcpyAsync(static_cast<char*>(dst) + at, d_dst + at, nb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(ok, S.ok, (size_t)n_segments * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

}  // extern "C"
