// ctx.hpp -- internal to the C-ABI host layer (ctx.hip, pipeline.hip,
// apps.hip): the context struct, the owners of its allocations, the error and
// profiling helpers, and the declarations those files share.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "common.hpp"

namespace sift {

// Move-only owner of one device (kPinned: pinned host) allocation: a pointer and an
// element count.  grow(n) frees and reallocates only when n exceeds the count
// (the contents are not kept); the destructor frees.
template <typename T, bool kPinned = false>
class Buf {
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  Buf& operator=(Buf&& o) noexcept {
    std::swap(p_, o.p_);
    std::swap(n_, o.n_);
    return *this;
  }
  ~Buf() { reset(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  size_t count() const { return n_; }
  hipError_t grow(size_t n) {
    if (p_ && n <= n_) return hipSuccess;
    reset();
    void* p = nullptr;
    const size_t bytes = sizeof(T) * (n ? n : 1);
    const hipError_t e = kPinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(p);
    n_ = n;
    return hipSuccess;
  }
  void reset() {
    if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr;
    n_ = 0;
  }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// Profiling stages and the names sift_get_stage_stats reports, from one table.
#define SIFT_STAGES(X)                                                                                  \
  X(ST_BLUR_BASE, "blur_base") X(ST_BLUR_OCT, "blur_octave") X(ST_DECIMATE, "decimate") X(ST_DOG, "dog") \
  X(ST_EXTREMA, "extrema") X(ST_REFINE, "refine_orient") X(ST_EMIT, "emit") X(ST_DESC, "descriptor")      \
  X(ST_UPLOAD, "upload") X(ST_DOWNLOAD, "download") X(ST_BLUR1D, "blur_1d") X(ST_PYR_FAST, "pyramid_fast") \
  X(ST_MATCH, "match") X(ST_BLUR_SYM, "blur_octave_sym") X(ST_MATCH_SEG, "match_segmented")               \
  X(ST_RATIO, "ratio_matches") X(ST_HOMOG_SEG, "homography_segmented")                                  \
  X(ST_QUANT_U8, "descriptors_to_u8") X(ST_MATCH_U8, "match_u8_segmented")                               \
  X(ST_MATCH_L2_U8, "match_l2sqr_u8_segmented") X(ST_SELECT, "select_best")                               \
  X(ST_CROSS, "cross_check_matches") X(ST_DETMASK, "detect_mask") X(ST_GRAD, "gradient")                \
  X(ST_COMPUTE_PREP, "compute_prep") X(ST_WINDOW_BIN, "match_window_bin")                              \
  X(ST_MATCH_WINDOW, "match_window_segmented") X(ST_UPSAMPLE, "upsample2x")                \
  X(ST_WARP, "warp") X(ST_AFFINE_SEG, "affine_segmented")                                  \
  X(ST_MATCH_L2_F32, "match_l2sqr_f32_segmented") X(ST_FUND_SEG, "fundamental_segmented") \
  X(ST_MATCH_EPIPOLAR, "match_epipolar") X(ST_POSE_SEG, "recover_pose_segmented")          \
  X(ST_TRI_SEG, "triangulate_segmented") X(ST_UNDISTORT, "undistort") X(ST_PNP_SEG, "pnp_segmented") \
  X(ST_JOIN, "join_matches")
enum Stage {
#define X(id, name) id,
  SIFT_STAGES(X)
#undef X
  ST_N
};

struct StageRec {
  int stage;
  hipEvent_t a, b;
  double flops, bytes;
};

}  // namespace sift

struct sift_ctx {
  int device = 0;
  unsigned flags = 0;
  int n_oct = 5;
  int max_rows = 0, max_cols = 0, max_batch = 0, max_oct = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  // workspace
  sift::Buf<float> d_in;
  long long in_pitch = 0, in_img = 0;
  sift::Buf<float> d_gpyr, d_dog, d_tmp;
  sift::Buf<float2> d_grad;       // per-pixel (magnitude, orientation), gpyr layout
  long long gpyr_elems = 0, dog_elems = 0;
  sift::Buf<float> d_coef;        // base (w=4) then the 4 octave scales
  sift::Buf<float> d_coef_gen;    // per-call coefficients (Gaussian_Blur / _1D)
  bool fast_ok = false;           // SIFT_FLAG_FAST: pyramid_pc.hip's compiled-in taps equal the host's
  // test hooks (SIFT_HIP_TEST_HOOKS, a comma list read at context creation; tests only):
  bool poison_pad = false;        // "poison_pad": NaN into every plane's pitch padding after the pyramid
  bool stall_once = false;        // "pc_stall_once": the next pyr_pc_kernel launch gets an expired wait bound
  // exact blur: launches with fewer 8-pixel tile workgroups than this use the
  // 2-output-per-lane tiles (blur_small_kernel); SIFT_HIP_SMALL_MAX overrides
  long long small_max = 2048;
  int wsz[4] = {0, 0, 0, 0};
  int w_base = 0;
  bool sym_blur = false;          // symmetric scatter blur (blur.hip) for the base and octave scales
  int sym_min = 256;              // ... for launches of >= sym_min 64-column strips x images
  int sym_rows = 0;               //     of >= sym_rows rows (A/B knob, SIFT_HIP_SYM_ROWS_MIN)
  // SIFT_NCL on a batch, exact mode: octaves on the scatter blur skip plane 4
  // and detection evaluates it point by point (SIFT_HIP_DENSE_G4=1: off, A/B)
  bool sparse_g4 = false;
  int g4_grid = 0;                // SIFT_HIP_G4_GRID (tests): 8 or 16 blocks for the plane-4 fill and rounds; 0 = resident
  size_t coef_base_off = 0, coef_oct_off = 0;
  sift::Buf<sift::MathConsts> d_mc;
  // detection workspace: the owners, and the raw-pointer view of them that the
  // launchers take (D is refilled by alloc_candidates, the one place these grow)
  sift::Buf<unsigned> mask;
  sift::Buf<int> blk_counts, cand_total, img_cand_off, kp_scan, kp_total, npeaks, scan_tmp, scan_tiles;
  sift::Buf<sift::Cand> cands;
  sift::Buf<sift::CandOut> couts;
  sift::Buf<float> g4patch;       // sparse flow (SparseG4, common.hpp): 9 floats per candidate slot
  sift::Buf<int> rstate;          //   and the slot's waiting state
  sift::Buf<int> g4wait, g4stat;  //   the waiting list and the call's counters (sift_g4_fill_stats)
  // SIFT_NCL's per-image keypoint budget (sift_set_max_features; 0 = all) and
  // its select (select.hip): contexts with more candidate slots per image than
  // select_block_max run the multi-workgroup form (SIFT_HIP_SELECT_BLOCK_MAX
  // overrides; tests), whose histograms are sel_hist
  int max_features = 0;
  long long select_block_max = 65536;
  sift::Buf<int> sel_hist;
  // the detection mask of sift_detect_compute_masked (detmask.hip), uploaded
  // packed (rows cols bytes apart): max_rows x max_cols bytes, allocated by the
  // first masked host call and never moved, so captured sequences may name it
  sift::Buf<unsigned char> d_detmask;
  // sift_set_upsample (upsample.hip): with it on, SIFT_NCL and sift_compute[_batch]
  // double each image into d_up -- laid out like d_in (in_pitch, in_img; the
  // pitch check_fast is asked about), max_batch images, allocated by the first
  // upsampled call and never moved, so captured sequences may name it
  bool upsample = false;
  sift::Buf<float> d_up;
  sift::DetectBufs D{};
  int blk_cap = 0;
  sift::Buf<int> d_img_off;       // [max_batch+1] for the host entry points
  sift::Buf<sift_keypoint> d_kpts;
  sift::Buf<float> d_desc;
  int kp_cap = 0;
  sift::Buf<int> d_perm;          // descriptor lane-balance ranking scratch (desc_rank_kernel)
  int last_n = -1;                // keypoints held from the last host call
  bool last_has_desc = false;
  sift::Buf<int> d_err;           // sticky error words [assert, workspace, kp capacity] (common.hpp)
  sift::Buf<int> d_stat;          // status_kernel output: {candidates, keypoints, error word, 0}
  sift::Buf<int, true> h_stat;    // pinned copy of d_stat, written at the end of every compute call
  sift::Buf<char> d_match;        // knn-match scratch in bytes (grown on demand, carved by scratch.hpp)
  // hipGraph cache of compute sequences (one per argument set; SIFT_FLAG_NO_GRAPH,
  // _PROFILE and _VERBOSE run the launches directly)
  struct GraphEntry {
    std::vector<char> key;   // everything that shapes the sequence (dims, batch, flags, ...)
    std::vector<char> ptrs;  // the caller's buffers baked into the kernel arguments
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
  };
  std::vector<GraphEntry> graphs;
  long long graph_captures = 0, graph_updates = 0, graph_instantiations = 0;  // sift_graph_stats
  // profiling
  std::vector<sift::StageRec> recs;
  std::vector<hipEvent_t> pool;
  double acc_ms[sift::ST_N] = {0}, acc_flops[sift::ST_N] = {0}, acc_bytes[sift::ST_N] = {0};
  int acc_n[sift::ST_N] = {0};
};

namespace sift {

inline int fail(sift_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

inline int hip_fail(sift_ctx* c, hipError_t e, const char* what) {
  return fail(c, SIFT_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(ctx, expr)                                         \
  do {                                                             \
    hipError_t e_ = (expr);                                        \
    if (e_ != hipSuccess) return sift::hip_fail((ctx), e_, #expr); \
  } while (0)

hipEvent_t get_event(sift_ctx* c);

struct StageScope {
  sift_ctx* c;
  int stage;
  double flops, bytes;
  hipEvent_t a = nullptr;
  StageScope(sift_ctx* c_, int st, double f = 0, double b = 0) : c(c_), stage(st), flops(f), bytes(b) {
    if (c->flags & SIFT_FLAG_PROFILE) {
      a = get_event(c);
      (void)hipEventRecord(a, c->stream);
    }
  }
  ~StageScope() {
    if (a) {
      hipEvent_t b = get_event(c);
      (void)hipEventRecord(b, c->stream);
      c->recs.push_back(StageRec{stage, a, b, flops, bytes});
    }
  }
};

// ---- ctx.hip ----------------------------------------------------------------
// The reference's octave sizes: Size(src.cols/2, src.rows/2), src/sift.cpp:254.
inline void halve(int& rows, int& cols) {
  rows /= 2;
  cols /= 2;
}
int check_dims(sift_ctx* c, int rows, int cols, int n_oct, int batch);
// Prologue of the entry points that take an image or pyramid size: null
// context, the caller's buffers (bufs_ok, else null_msg), the dimensions, then
// the context's device is made current.
int enter(sift_ctx* c, bool bufs_ok, const char* null_msg, int rows, int cols, int n_oct, int batch);
int check_fast(sift_ctx* c, const Layout& L, long long src_row_stride);
// Buffer growth.  The keypoint, ranking and candidate buffers are named by
// captured sequences, so growing one drops the graph cache first.
int ensure_coef_gen(sift_ctx* c, size_t n);
int ensure_kp(sift_ctx* c, int need);
int ensure_perm(sift_ctx* c, int need);
int ensure_match(sift_ctx* c, size_t bytes);
int alloc_candidates(sift_ctx* c, int cap);
void enqueue_status(sift_ctx* c, bool check_cand, const int* img_off, int batch, int kp_cap);
int take_status(sift_ctx* c, bool sticky, int mask, bool kp_internal = false);
constexpr int kAllErr = kErrAssert | kErrWorkspace | kErrKpCapacity | kErrStall;

}  // namespace sift
