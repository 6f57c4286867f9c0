// pipeline.hip -- the SIFT pipeline behind the C ABI (include/sift_hip.h) on
// the context's one HIP stream: SIFT_NCL for a device batch and from host
// memory, the six sub-module entry points, and the test helpers.  Host code
// and one test kernel; the kernels live in blur.hip, pyramid_pc.hip, the
// detection stages (extrema.hip, scan.hip, refine.hip, orient.hip, emit.hip)
// and descriptor.hip.
#include <limits.h>
#include <math.h>
#include <stdio.h>

#include <algorithm>

#include "graph.hpp"

using namespace sift;

namespace {

double plane_px(const Layout& L, int o) { return (double)L.oct[o].rows * L.oct[o].cols; }

bool use_sym_blur(const sift_ctx* c, int rows, int cols, int batch) {
  return c->sym_blur && rows >= c->sym_rows && (long long)((cols + 63) / 64) * batch >= c->sym_min;
}

// The sparse flow (SparseG4, common.hpp) of a SIFT_NCL batch: the octaves the
// scatter blur takes, in exact mode; 0 for every other call.
unsigned sparse_octaves(const sift_ctx* c, const Layout& L, int batch) {
  if (!c->sparse_g4 || (c->flags & SIFT_FLAG_FAST)) return 0;
  unsigned m = 0;
  for (int o = 0; o < L.n_oct; ++o)
    if (use_sym_blur(c, L.oct[o].rows, L.oct[o].cols, batch)) m |= 1u << o;
  return m;
}

const float* coef4_table(const sift_ctx* c) {
  size_t at = c->coef_oct_off;
  for (int q = 0; q < 3; ++q) at += (size_t)(2 * c->wsz[q] + 1) * (2 * c->wsz[q] + 1);
  return c->d_coef + at;
}

// Taps per output pixel of the octave blurs (the first n of the four scales):
// 1-D (row or column pass of the separable form) or 2-D.
double octave_taps(const sift_ctx* c, bool two_d, int n = 4) {
  double taps = 0;
  for (int q = 0; q < n; ++q) taps += two_d ? (double)(2 * c->wsz[q] + 1) * (2 * c->wsz[q] + 1) : 2 * c->wsz[q] + 1;
  return taps;
}

// sift_set_upsample: SIFT_NCL and sift_compute[_batch] run on the doubled image.
// run_dim is the dimension the entry points check against the context's limits
// (one that cannot be doubled in an int is above every limit; a non-positive
// one is passed through for check_dims to refuse).
int run_dim(const sift_ctx* c, int v) { return !c->upsample || v <= 0 ? v : v > (1 << 30) ? INT_MAX : 2 * v; }

// The doubled images' buffer, laid out like d_in; allocated once, never moved.
int ensure_up(sift_ctx* c) {
  if (!c->d_up.get() && c->d_up.grow((size_t)c->in_img * c->max_batch) != hipSuccess)
    return fail(c, SIFT_E_NOMEM, "upsampled image buffer");
  return SIFT_OK;
}

// Doubles the batch's images into d_up (upsample.hip) and returns that plane.
Plane enqueue_upsample(sift_ctx* c, Plane src, int batch, int rows, int cols) {
  StageScope s(c, ST_UPSAMPLE, 0, 20.0 * rows * cols * batch);
  launch_upsample2x(c->stream, src.p, src.pitch, src.img_stride, rows, cols, c->d_up, c->in_pitch, c->in_img, batch);
  return Plane{c->d_up, c->in_pitch, c->in_img};
}

void enqueue_decimate(sift_ctx* c, const Layout& L, int o, int batch) {
  StageScope s(c, ST_DECIMATE, 0, 8.0 * plane_px(L, o) * batch);
  launch_decimate(c->stream, L, o, c->d_gpyr, batch);
}

void enqueue_dog(sift_ctx* c, const Layout& L, int o, int batch) {
  StageScope s(c, ST_DOG, 4.0 * plane_px(L, o) * batch, 36.0 * plane_px(L, o) * batch);
  launch_dog(c->stream, L, o, c->d_gpyr, c->d_dog, batch);
}

// Test switch for the pitch-padding invariant (common.hpp, kPitchAlign):
// overwrite columns [cols, pitch) of every Gaussian plane of the batch with a
// NaN once the pyramid is built, so a later kernel that read them would change
// its output (tests/test_gpu_fast.py::test_pitch_padding_is_never_read).
struct PadArgs {
  float* gpyr;
  long long g_img;
  int n_planes;
  long long off[kMaxOctaves * kScales];
  int rows[kMaxOctaves * kScales], cols[kMaxOctaves * kScales], pitch[kMaxOctaves * kScales];
};
__global__ __launch_bounds__(64) void poison_pad_kernel(PadArgs A) {
  int r = blockIdx.x, p = 0;
  while (p < A.n_planes && r >= A.rows[p]) r -= A.rows[p++];
  if (p >= A.n_planes) return;
  const int x = A.cols[p] + (int)threadIdx.x;
  if (x < A.pitch[p])
    A.gpyr[(long long)blockIdx.y * A.g_img + A.off[p] + (long long)r * A.pitch[p] + x] = __builtin_nanf("");
}
void enqueue_poison_pad(sift_ctx* c, const Layout& L, int batch) {
  PadArgs A{};
  A.gpyr = c->d_gpyr;
  A.g_img = L.g_img;
  int total = 0;
  for (int o = 0; o < L.n_oct; ++o)
    for (int s = 0; s < kScales; ++s) {
      const int p = A.n_planes++;
      A.off[p] = L.oct[o].g_off[s];
      A.rows[p] = L.oct[o].rows;
      A.cols[p] = L.oct[o].cols;
      A.pitch[p] = L.oct[o].pitch;
      total += L.oct[o].rows;
    }
  static_assert(kPitchAlign <= 64, "one lane per padding column");
  hipLaunchKernelGGL(poison_pad_kernel, dim3(total, batch), dim3(64), 0, c->stream, A);
}

// Gaussian pyramid (src/sift.cpp:229-263) + DoG (:265-283) for a batch whose
// input planes are described by src.  Async on c->stream.
void enqueue_pyramid(sift_ctx* c, const Layout& L, Plane src, int batch, bool with_dog, unsigned sparse = 0) {
  hipStream_t st = c->stream;
  if (c->flags & SIFT_FLAG_FAST) {
    // separable pyramid: 24 algorithmic bytes per pixel (1 read + 5 plane
    // writes); 2 x (row + column taps) flops per pixel
    for (int o = 0; o < L.n_oct; ++o) {
      const double px = plane_px(L, o) * batch;
      const double taps = 2.0 * octave_taps(c, false) + (o == 0 ? 2.0 * (2 * c->w_base + 1) : 0.0);
      // pyramid_pc.hip: octave o-1's launch wrote plane 0 of octave o when
      // it is an exact half; otherwise decimate first (plane 0
      // is one of the five plane writes, the decimation's read is not
      // algorithmic, so it is outside the pyramid stage's bytes)
      if (o > 0 && !pyramid_fuses_decimation(L, o)) enqueue_decimate(c, L, o, batch);
      StageScope s(c, ST_PYR_FAST, 2.0 * taps * px, 24.0 * px);
      launch_pyramid_pc(st, L, o, c->d_gpyr, src, batch, c->d_err + 3, c->stall_once);
      c->stall_once = false;
    }
    if (c->poison_pad) enqueue_poison_pad(c, L, batch);
    if (with_dog)
      for (int o = 0; o < L.n_oct; ++o) enqueue_dog(c, L, o, batch);
    return;
  }
  {
    const double px = plane_px(L, 0) * batch;
    const int k = 2 * c->w_base + 1;
    StageScope s(c, ST_BLUR_BASE, 2.0 * k * k * px, 8.0 * px);
    if (use_sym_blur(c, L.oct[0].rows, L.oct[0].cols, batch))
      launch_blur_base_sym(st, src, c->d_gpyr + L.oct[0].g_off[0], L.oct[0].pitch, L.g_img, L.rows, L.cols, batch);
    else
      launch_blur_plane(st, c->w_base, c->d_coef + c->coef_base_off, src, c->d_gpyr + L.oct[0].g_off[0],
                        L.oct[0].pitch, L.g_img, L.rows, L.cols, batch);
  }
  // Every octave blur also writes the next octave's plane 0 when it is an
  // exact half of plane 2 (no decimation launch; the launches of one image are
  // latency-bound, and the batch's decimation was a full extra read of plane 2).
  bool fused = false;  // this octave's plane 0 came out of the previous launch
  for (int o = 0; o < L.n_oct; ++o) {
    const double px = plane_px(L, o) * batch;
    if (o > 0 && !fused) enqueue_decimate(c, L, o, batch);
    {
      const bool sym = use_sym_blur(c, L.oct[o].rows, L.oct[o].cols, batch);
      const bool fuse = o + 1 < L.n_oct && blur_fuses_decimation(L, o + 1);
      // sparse: three planes written (1 read + 3 writes), no w = 18 taps
      const bool no4 = sym && ((sparse >> o) & 1u);
      StageScope s(c, sym ? ST_BLUR_SYM : ST_BLUR_OCT, 2.0 * octave_taps(c, true, no4 ? 3 : 4) * px,
                   (no4 ? 16.0 : 20.0) * px);
      if (sym)
        launch_blur_octave_sym(st, L, o, c->d_gpyr, batch, fuse, no4);
      else if (blur_octave_tiles(L, o, batch) < c->small_max)
        launch_blur_octave_small(st, L, o, c->d_gpyr, c->d_coef + c->coef_oct_off, c->wsz, batch, fuse);
      else
        launch_blur_octave(st, L, o, c->d_gpyr, c->d_coef + c->coef_oct_off, c->wsz, batch, fuse);
      fused = fuse;
    }
    if (with_dog) enqueue_dog(c, L, o, batch);
  }
  if (c->poison_pad) enqueue_poison_pad(c, L, batch);
}

// dog_from_gpyr: the fused extrema pass forms the DoG values from the Gaussian
// pyramid and refinement re-forms the few it needs, so no DoG plane is written
// (SIFT_NCL never returns them); otherwise the DoG planes are already resident
// (sift_find_scale_space_extrema uploads both pyramids).
// max_features > 0 (SIFT_NCL only): each image keeps its best that many
// keypoints by response, ties at the cut included (select.hip), before the
// scan -- so the offsets, the emitted list and the descriptor work are the
// kept keypoints'.
// dm.bytes != nullptr (the *_masked calls only): after the budget, as OpenCV
// orders retainBest and runByPixelsMask, every keypoint on a zero byte of the
// image's detection mask is dropped as well (detmask.hip).
// half (sift_set_upsample; L is the doubled image's): keypoints are emitted in
// the original image's frame, and the mask, which is that image's size, is
// read at those coordinates.
void enqueue_detect(sift_ctx* c, const Layout& L, int batch, sift_keypoint* kpts, int kp_cap,
                    int* img_off, bool dog_from_gpyr, unsigned sparse = 0, int max_features = 0,
                    const DetMask& dm = DetMask{}, bool half = false) {
  hipStream_t st = c->stream;
  {
    StageScope s(c, ST_EXTREMA);
    launch_extrema(st, L, c->d_gpyr, c->d_dog, dog_from_gpyr, c->d_grad, c->d_mc, batch, c->D, sparse);
  }
  {
    StageScope s(c, ST_REFINE);
    // (the sparse flow's fill and step rounds are part of this stage)
    launch_refine_orient(st, L, c->d_gpyr, c->d_grad, dog_from_gpyr ? nullptr : c->d_dog.get(), c->d_mc, c->D, batch,
                         SparseG4{sparse, coef4_table(c), c->g4_grid});
  }
  if (max_features > 0) {
    StageScope s(c, ST_SELECT);
    launch_select_best(st, c->D, batch, max_features, c->D.cand_cap / c->max_batch > c->select_block_max);
  }
  if (dm.bytes) {
    StageScope s(c, ST_DETMASK);
    launch_detmask(st, c->D, batch, dm, half ? L.rows / 2 : L.rows, half ? L.cols / 2 : L.cols,
                   c->D.cand_cap / c->max_batch > c->select_block_max, half);
  }
  {
    StageScope s(c, ST_EMIT);
    launch_emit(st, c->D, batch, kpts, kp_cap, img_off, half);
  }
}

void enqueue_desc(sift_ctx* c, const Layout& L, const sift_keypoint* kpts, const int* img_off,
                  int batch, int kp_cap, float* desc, int first_octave, bool detected) {
  StageScope s(c, ST_DESC);
  launch_descriptors(c->stream, L, c->d_grad, c->d_mc, kpts, img_off, batch, std::min(kp_cap, (int)c->d_perm.count()),
                     desc, first_octave, c->d_err, detected, c->d_perm);
}

int upload_image(sift_ctx* c, const float* img, int rows, int cols, size_t row_stride_bytes) {
  StageScope s(c, ST_UPLOAD, 0, 4.0 * rows * cols);
  HIP_TRY(c, hipMemcpy2DAsync(c->d_in, c->in_pitch * sizeof(float), img, row_stride_bytes,
                              (size_t)cols * sizeof(float), rows, hipMemcpyHostToDevice, c->stream));
  return SIFT_OK;
}

// packed host pyramid <-> pitched device pyramid (image 0)
int copy_pyramid(sift_ctx* c, const Layout& L, float* dev, const float* host_in, float* host_out,
                 int per) {
  size_t off = 0;
  for (int o = 0; o < L.n_oct; ++o) {
    const Octave& O = L.oct[o];
    for (int s = 0; s < per; ++s) {
      float* d = dev + (per == kScales ? O.g_off[s] : O.d_off[s]);
      const size_t w = (size_t)O.cols * sizeof(float);
      if (host_in)
        HIP_TRY(c, hipMemcpy2DAsync(d, O.pitch * sizeof(float), host_in + off, w, w, O.rows,
                                    hipMemcpyHostToDevice, c->stream));
      if (host_out)
        HIP_TRY(c, hipMemcpy2DAsync(host_out + off, w, d, O.pitch * sizeof(float), w, O.rows,
                                    hipMemcpyDeviceToHost, c->stream));
      off += (size_t)O.rows * O.cols;
    }
  }
  return SIFT_OK;
}

void verbose_phase(sift_ctx* c, const char* what, hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  (void)hipEventSynchronize(b);
  (void)hipEventElapsedTime(&ms, a, b);
  printf("%s: %g\n", what, (double)ms);
}

// The whole SIFT_NCL device sequence for a batch (pyramid -> detect ->
// descriptors -> status block), replayed from the context's hipGraph cache;
// SIFT_FLAG_VERBOSE launches it directly with an event between the phases
// and prints the reference's three timing lines.
int enqueue_ncl(sift_ctx* c, const float* d_imgs, int batch, int rows, int cols, size_t row_stride,
                size_t img_stride, sift_keypoint* d_kpts, float* d_desc, int kp_cap, int* d_img_offsets,
                const DetMask& dm = DetMask{}) {
  // sift_set_upsample: the same sequence on the doubled images (rows, cols stay
  // the caller's, which is what the mask and the key are about)
  const bool up = c->upsample;
  const Layout L = make_layout(up ? 2 * rows : rows, up ? 2 * cols : cols, c->n_oct);
  const Plane in{d_imgs, (long long)row_stride, (long long)img_stride};
  if (up)
    if (int rc = ensure_up(c)) return rc;
  if (int rc = check_fast(c, L, up ? c->in_pitch : (long long)row_stride)) return rc;
  // detection yields at most kMaxPeaks keypoints per candidate slot, so the
  // ranking scratch never needs more than that, whatever kp_cap the caller gives
  if (int rc = ensure_perm(c, (int)std::min<long long>(kp_cap, (long long)kMaxPeaks * c->D.cand_cap))) return rc;
  const unsigned sparse = sparse_octaves(c, L, batch);
  const bool verbose = c->flags & SIFT_FLAG_VERBOSE;
  hipEvent_t v[4] = {nullptr, nullptr, nullptr, nullptr};
  auto mark = [&](int i) {
    if (!verbose) return;
    v[i] = get_event(c);
    (void)hipEventRecord(v[i], c->stream);
  };
  auto body = [&]() {
    mark(0);
    const Plane src = up ? enqueue_upsample(c, in, batch, rows, cols) : in;
    enqueue_pyramid(c, L, src, batch, false, sparse);
    mark(1);
    enqueue_detect(c, L, batch, d_kpts, kp_cap, d_img_offsets, true, sparse, c->max_features, dm, up);
    mark(2);
    // the doubled pyramid's first octave is -1: unpackOctave maps the emitted rows back onto it
    enqueue_desc(c, L, d_kpts, d_img_offsets, batch, kp_cap, d_desc, up ? -1 : 0, true);
    mark(3);
    enqueue_status(c, true, d_img_offsets, batch, kp_cap);
  };
  if (verbose) {
    body();
    verbose_phase(c, "pyramid construction time", v[0], v[1]);
    verbose_phase(c, "keypoint localization time", v[1], v[2]);
    verbose_phase(c, "descriptor extraction time", v[2], v[3]);
    c->pool.insert(c->pool.end(), v, v + 4);
    HIP_TRY(c, hipGetLastError());
    return SIFT_OK;
  }
  std::vector<char> key, ptrs;
  // sequence id 1, then everything that shapes the sequence; stall_once is the
  // test hook: a captured poll bound must not be replayed
  key_put(key, 1, batch, rows, cols, row_stride, img_stride, kp_cap, c->n_oct, c->flags, c->stall_once, sparse,
          c->max_features, dm.bytes != nullptr, dm.row_stride, dm.img_stride, up);
  key_put(ptrs, d_imgs, dm.bytes, d_kpts, d_desc, d_img_offsets);
  return run_graphed(c, key, ptrs, body);
}

// The ranking scratch as sift_compute_batch carves it: the two row lists of
// kp_cap ints, then their two counts.
constexpr int kMaxComputeRows = 1 << 30;
int compute_perm_ints(int kp_cap) { return 2 * kp_cap + 2; }

// The device sequence of sift_compute_batch (Feature2D::compute for a batch):
// pyramid -> gradient planes of scales 0..max_layer -> row prep -> the two
// descriptor launches -> status block.  No detection, no host value; replayed
// from the graph cache under sequence id 2.  With max_layer <= 3 the octaves
// on the scatter blur leave plane 4 out (exact mode; the other blur forms
// compute their scales together).
int enqueue_compute(sift_ctx* c, const float* d_imgs, int batch, int rows, int cols, size_t row_stride,
                    size_t img_stride, const sift_keypoint* d_kpts, const int* d_kp_offsets, int kp_cap, int max_layer,
                    float* d_desc) {
  // sift_set_upsample: the doubled images' pyramid, whose first octave is -1;
  // the rows stay in the original image's frame (unpackOctave scales them)
  const bool up = c->upsample;
  const Layout L = make_layout(up ? 2 * rows : rows, up ? 2 * cols : cols, c->n_oct);
  const Plane in{d_imgs, (long long)row_stride, (long long)img_stride};
  const int first_octave = up ? -1 : 0;
  if (up)
    if (int rc = ensure_up(c)) return rc;
  if (int rc = check_fast(c, L, up ? c->in_pitch : (long long)row_stride)) return rc;
  if (int rc = ensure_perm(c, compute_perm_ints(kp_cap))) return rc;
  unsigned skip4 = 0;
  if (max_layer < kScales - 1 && !(c->flags & SIFT_FLAG_FAST))
    for (int o = 0; o < L.n_oct; ++o)
      if (use_sym_blur(c, L.oct[o].rows, L.oct[o].cols, batch)) skip4 |= 1u << o;
  const DescLists lists{c->d_perm, c->d_perm + kp_cap, c->d_perm + 2 * (size_t)kp_cap};
  auto body = [&]() {
    const Plane src = up ? enqueue_upsample(c, in, batch, rows, cols) : in;
    enqueue_pyramid(c, L, src, batch, false, skip4);
    {
      StageScope s(c, ST_GRAD, 0, 12.0 * (max_layer + 1) * (double)L.g_img / kScales * batch);
      launch_grad(c->stream, L, c->d_gpyr, c->d_grad, batch, 0, max_layer, c->d_mc);
    }
    {
      StageScope s(c, ST_COMPUTE_PREP, 0, 36.0 * kp_cap);
      launch_compute_prep(c->stream, L, d_kpts, d_kp_offsets, batch, kp_cap, max_layer, d_desc, c->d_err, lists,
                          first_octave);
    }
    {
      StageScope s(c, ST_DESC);
      launch_descriptors_listed(c->stream, L, c->d_grad, c->d_mc, d_kpts, d_kp_offsets, batch, kp_cap, d_desc,
                                c->d_err, lists, first_octave);
    }
    enqueue_status(c, false, nullptr, batch, kp_cap);  // no detection ran: assertion (and stall) bits only
  };
  std::vector<char> key, ptrs;
  key_put(key, 2, batch, rows, cols, row_stride, img_stride, kp_cap, c->n_oct, c->flags, c->stall_once, max_layer, up);
  key_put(ptrs, d_imgs, d_kpts, d_kp_offsets, d_desc);
  return run_graphed(c, key, ptrs, body);
}

// Tail of the host detection calls.  upload() stages the input once; enqueue()
// queues the device sequence, which ends in the status block.  ONE stream
// synchronisation brings the keypoint count with it, then exactly n results
// are copied.  The internal keypoint buffer is sized at creation for 2
// keypoints per candidate slot; a larger count (more than 2 orientation peaks
// per extremum on average) grows it and runs the sequence again.
template <typename Upload, typename Enqueue>
int host_detect(sift_ctx* c, bool has_desc, sift_keypoint* kpts, float* desc, int cap, int* n_out, Upload&& upload,
                Enqueue&& enqueue) {
  c->last_n = -1;
  *n_out = -1;
  if (int rc = upload()) return rc;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (int rc = enqueue()) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (int rc = take_status(c, false, kAllErr, true)) return rc;
    const int n = c->h_stat[1];
    if (n > c->kp_cap) {  // grow the internal buffer and run again
      if (int rc = ensure_kp(c, n)) return rc;
      continue;
    }
    *n_out = n;
    c->last_n = n;
    c->last_has_desc = has_desc;
    if (n > cap || (n > 0 && (!kpts || (has_desc && !desc))))
      return fail(c, SIFT_E_CAPACITY, "keypoint capacity " + std::to_string(cap) +
                                          " < required " + std::to_string(n));
    if (n > 0 && !has_desc)  // keypoints alone: a blocking copy, no download stage
      HIP_TRY(c, hipMemcpy(kpts, c->d_kpts, sizeof(sift_keypoint) * n, hipMemcpyDeviceToHost));
    else if (n > 0) {
      StageScope s(c, ST_DOWNLOAD, 0, (28.0 + 512.0) * n);
      HIP_TRY(c, hipMemcpyAsync(kpts, c->d_kpts, sizeof(sift_keypoint) * n, hipMemcpyDeviceToHost,
                                c->stream));
      HIP_TRY(c, hipMemcpyAsync(desc, c->d_desc, sizeof(float) * kDescLen * n,
                                hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return SIFT_OK;
  }
  return fail(c, SIFT_E_CAPACITY, "keypoint buffer growth failed");
}

// Gaussian_Blur (the 2-D table of getGaussianKernel) and Gaussian_Blur_1D
// (getGaussianKernel1D(double sigma), src/sift.cpp:157-168, as a row and a
// column pass) differ in their coefficients, launcher, result plane and stage.
int host_blur(sift_ctx* c, const float* src, int rows, int cols, double sigma, float* dst, bool one_d) {
  if (int rc = enter(c, src && dst, "null buffer", rows, cols, 1, 1)) return rc;
  if (!(sigma > 0) || sigma > 100) return fail(c, SIFT_E_INVALID, "sigma out of range");
  const int w = one_d ? (int)floor(3 * sigma) : gaussian_kernel_host((float)sigma, nullptr) / 2, ks = 2 * w + 1;
  std::vector<float> k(one_d ? ks : (size_t)ks * ks);
  if (one_d)
    for (int i = -w; i <= w; ++i)
      k[i + w] = (float)(1. / sqrt(2 * kRefPi * sigma * sigma) *
                         exp(-((double)i * i) * 1. / (2 * sigma * sigma)));
  else
    gaussian_kernel_host((float)sigma, k.data());
  if (int rc = ensure_coef_gen(c, k.size())) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->d_coef_gen, k.data(), k.size() * sizeof(float), hipMemcpyHostToDevice,
                            c->stream));
  if (int rc = upload_image(c, src, rows, cols, (size_t)cols * sizeof(float))) return rc;
  const Plane in{c->d_in, c->in_pitch, c->in_img};
  const float* out = one_d ? c->d_gpyr : c->d_tmp;  // d_gpyr: scratch (>= one max-size plane)
  if (one_d) {
    StageScope s(c, ST_BLUR1D, 4.0 * (2 * w) * rows * cols, 16.0 * rows * cols);
    launch_blur_1d(c->stream, w, c->d_coef_gen, in, c->d_tmp, c->d_gpyr, c->in_pitch, c->in_img, rows, cols, 1);
  } else {
    StageScope s(c, ST_BLUR_BASE, 2.0 * ks * ks * rows * cols, 8.0 * rows * cols);
    launch_blur_plane(c->stream, w, c->d_coef_gen, in, c->d_tmp, c->in_pitch, c->in_img, rows, cols, 1);
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpy2DAsync(dst, (size_t)cols * sizeof(float), out, c->in_pitch * sizeof(float),
                              (size_t)cols * sizeof(float), rows, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

}  // namespace

extern "C" {

int sift_synth_images(sift_ctx* c, float* d_out, int batch, int rows, int cols, size_t row_stride,
                      size_t img_stride, int seed_base) {
  if (!c || !d_out || batch < 1 || rows < 1 || cols < 1 || row_stride < (size_t)cols)
    return fail(c, SIFT_E_INVALID, "bad synth arguments");
  (void)hipSetDevice(c->device);
  launch_synth(c->stream, d_out, batch, rows, cols, (long long)row_stride, (long long)img_stride,
               seed_base);
  HIP_TRY(c, hipGetLastError());
  return SIFT_OK;
}

int sift_copy_results(sift_ctx* c, sift_keypoint* kpts, float* desc, int cap, int* n_out) {
  if (!c) return SIFT_E_INVALID;
  if (!n_out) return fail(c, SIFT_E_INVALID, "null n_out");
  if (c->last_n < 0) return fail(c, SIFT_E_INVALID, "no results held: run a host detect call first");
  const int n = c->last_n;
  *n_out = n;
  if (n > cap) return fail(c, SIFT_E_CAPACITY, "keypoint capacity " + std::to_string(cap) +
                                                   " < required " + std::to_string(n));
  if (n == 0) return SIFT_OK;
  if (!kpts || (desc && !c->last_has_desc)) return fail(c, SIFT_E_INVALID, "nothing to copy into");
  (void)hipSetDevice(c->device);
  {
    StageScope s(c, ST_DOWNLOAD, 0, (28.0 + (desc ? 512.0 : 0.0)) * n);
    HIP_TRY(c, hipMemcpyAsync(kpts, c->d_kpts, sizeof(sift_keypoint) * n, hipMemcpyDeviceToHost, c->stream));
    if (desc)
      HIP_TRY(c, hipMemcpyAsync(desc, c->d_desc, sizeof(float) * kDescLen * n, hipMemcpyDeviceToHost,
                                c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

int sift_detect_compute_batch_masked(sift_ctx* c, const float* d_imgs, int batch, int rows, int cols,
                                     size_t row_stride, size_t img_stride, const uint8_t* d_masks,
                                     size_t mask_row_stride, size_t mask_img_stride, sift_keypoint* d_kpts,
                                     float* d_desc, int kp_cap, int* d_img_offsets) {
  if (!c) return SIFT_E_INVALID;
  int rc = check_dims(c, run_dim(c, rows), run_dim(c, cols), c->n_oct, batch);
  if (rc) return rc;
  if (!d_imgs || !d_kpts || !d_desc || !d_img_offsets || kp_cap < 0 || row_stride < (size_t)cols)
    return fail(c, SIFT_E_INVALID, "null buffer or bad stride");
  if (d_masks && mask_row_stride < (size_t)cols) return fail(c, SIFT_E_INVALID, "mask_row_stride < cols");
  (void)hipSetDevice(c->device);
  c->last_n = -1;
  // without a mask its strides shape nothing: one cached sequence whatever they are
  const DetMask dm = d_masks ? DetMask{d_masks, (long long)mask_row_stride, (long long)mask_img_stride} : DetMask{};
  return enqueue_ncl(c, d_imgs, batch, rows, cols, row_stride, img_stride, d_kpts, d_desc, kp_cap,
                     d_img_offsets, dm);
}

int sift_detect_compute_batch(sift_ctx* c, const float* d_imgs, int batch, int rows, int cols,
                              size_t row_stride, size_t img_stride, sift_keypoint* d_kpts,
                              float* d_desc, int kp_cap, int* d_img_offsets) {
  return sift_detect_compute_batch_masked(c, d_imgs, batch, rows, cols, row_stride, img_stride, nullptr, 0, 0, d_kpts,
                                          d_desc, kp_cap, d_img_offsets);
}

// SIFT_NCL from host memory: upload -> the graphed device sequence -> the
// host-detection tail above.
// With a mask: it is uploaded once, packed, into the context's own buffer
// beside the image; the grow-and-run-again path of host_detect enqueues the
// sequence again on that uploaded copy.
int sift_detect_compute_masked(sift_ctx* c, const float* img, int rows, int cols, size_t row_stride_bytes,
                               const uint8_t* mask, size_t mask_row_stride_bytes, sift_keypoint* kpts, float* desc,
                               int cap, int* n_out) {
  if (!c) return SIFT_E_INVALID;
  if (!img || !n_out) return fail(c, SIFT_E_INVALID, "null image or n_out");
  if (row_stride_bytes == 0) row_stride_bytes = (size_t)cols * sizeof(float);
  if (mask_row_stride_bytes == 0) mask_row_stride_bytes = (size_t)(cols > 0 ? cols : 0);
  if (int rc = check_dims(c, run_dim(c, rows), run_dim(c, cols), c->n_oct, 1)) return rc;
  if (mask && mask_row_stride_bytes < (size_t)cols) return fail(c, SIFT_E_INVALID, "mask_row_stride_bytes < cols");
  (void)hipSetDevice(c->device);
  if (mask && !c->d_detmask.get() &&
      c->d_detmask.grow((size_t)c->max_rows * c->max_cols) != hipSuccess)
    return fail(c, SIFT_E_NOMEM, "detection mask buffer");
  const DetMask dm = mask ? DetMask{c->d_detmask, cols, 0} : DetMask{};
  return host_detect(
      c, true, kpts, desc, cap, n_out,
      [&]() -> int {
        if (int rc = upload_image(c, img, rows, cols, row_stride_bytes)) return rc;
        if (mask) {
          StageScope s(c, ST_UPLOAD, 0, 1.0 * rows * cols);
          HIP_TRY(c, hipMemcpy2DAsync(c->d_detmask, (size_t)cols, mask, mask_row_stride_bytes, (size_t)cols, rows,
                                      hipMemcpyHostToDevice, c->stream));
        }
        return SIFT_OK;
      },
      [&] {
        return enqueue_ncl(c, c->d_in, 1, rows, cols, c->in_pitch, c->in_img, c->d_kpts, c->d_desc, c->kp_cap,
                           c->d_img_off, dm);
      });
}

int sift_detect_compute(sift_ctx* c, const float* img, int rows, int cols, size_t row_stride_bytes,
                        sift_keypoint* kpts, float* desc, int cap, int* n_out) {
  return sift_detect_compute_masked(c, img, rows, cols, row_stride_bytes, nullptr, 0, kpts, desc, cap, n_out);
}

int sift_compute_batch(sift_ctx* c, const float* d_imgs, int batch, int rows, int cols, size_t row_stride,
                       size_t img_stride, const sift_keypoint* d_kpts, const int* d_kp_offsets, int kp_cap,
                       int max_layer, float* d_desc) {
  if (!c) return SIFT_E_INVALID;
  if (max_layer < 0 || max_layer > kScales - 1) return fail(c, SIFT_E_INVALID, "max_layer must be 0 .. 4");
  if (batch < 0 || kp_cap < 0) return fail(c, SIFT_E_INVALID, "negative batch or kp_cap");
  if (batch == 0 || kp_cap == 0) return SIFT_OK;  // no row to describe
  if (!d_imgs || !d_kpts || !d_kp_offsets || !d_desc || row_stride < (size_t)(cols > 0 ? cols : 0))
    return fail(c, SIFT_E_INVALID, "null buffer or bad stride");
  if (int rc = check_dims(c, run_dim(c, rows), run_dim(c, cols), c->n_oct, batch)) return rc;
  if (kp_cap > kMaxComputeRows) return fail(c, SIFT_E_SIZE, "kp_cap above 2^30 rows");
  (void)hipSetDevice(c->device);
  c->last_n = -1;
  return enqueue_compute(c, d_imgs, batch, rows, cols, row_stride, img_stride, d_kpts, d_kp_offsets, kp_cap, max_layer,
                         d_desc);
}

// Feature2D::compute from host memory: upload -> the graphed device sequence
// with batch 1 on the context's own keypoint and descriptor buffers -> one
// synchronisation -> n rows back.  The capacity named to the sequence is the
// internal buffer's, so calls with other counts replay one captured sequence.
int sift_compute(sift_ctx* c, const float* img, int rows, int cols, size_t row_stride_bytes, const sift_keypoint* kpts,
                 int n, int max_layer, float* desc) {
  if (!c) return SIFT_E_INVALID;
  if (max_layer < 0 || max_layer > kScales - 1) return fail(c, SIFT_E_INVALID, "max_layer must be 0 .. 4");
  if (n < 0) return fail(c, SIFT_E_INVALID, "negative keypoint count");
  if (n == 0) return SIFT_OK;
  if (!img || !kpts || !desc) return fail(c, SIFT_E_INVALID, "null buffer");
  if (row_stride_bytes == 0) row_stride_bytes = (size_t)(cols > 0 ? cols : 0) * sizeof(float);
  if (int rc = check_dims(c, run_dim(c, rows), run_dim(c, cols), c->n_oct, 1)) return rc;
  if (n > kMaxComputeRows) return fail(c, SIFT_E_SIZE, "more than 2^30 keypoints");
  (void)hipSetDevice(c->device);
  if (int rc = ensure_kp(c, n)) return rc;
  c->last_n = -1;  // the internal keypoint buffer is reused below
  if (int rc = upload_image(c, img, rows, cols, row_stride_bytes)) return rc;
  const int off[2] = {0, n};
  HIP_TRY(c, hipMemcpyAsync(c->d_img_off, off, sizeof(off), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->d_kpts, kpts, sizeof(sift_keypoint) * n, hipMemcpyHostToDevice, c->stream));
  if (int rc = enqueue_compute(c, c->d_in, 1, rows, cols, c->in_pitch, c->in_img, c->d_kpts, c->d_img_off,
                               std::min(c->kp_cap, kMaxComputeRows), max_layer, c->d_desc))
    return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // the rows are copied whatever the status says: an invalid row holds zeros
  const int rc = take_status(c, false, kErrAssert | kErrStall);
  HIP_TRY(c, hipMemcpy(desc, c->d_desc, sizeof(float) * kDescLen * n, hipMemcpyDeviceToHost));
  return rc;
}

int sift_gaussian_blur(sift_ctx* c, const float* src, int rows, int cols, double sigma, float* dst) {
  return host_blur(c, src, rows, cols, sigma, dst, false);
}

int sift_gaussian_blur_1d(sift_ctx* c, const float* src, int rows, int cols, double sigma, float* dst) {
  return host_blur(c, src, rows, cols, sigma, dst, true);
}

int sift_build_gaussian_pyramid(sift_ctx* c, const float* img, int rows, int cols, int n_octaves,
                                float* gpyr) {
  int rc = enter(c, img && gpyr, "null buffer", rows, cols, n_octaves, 1);
  if (rc) return rc;
  const Layout L = make_layout(rows, cols, n_octaves);
  if ((rc = check_fast(c, L, c->in_pitch))) return rc;
  if ((rc = upload_image(c, img, rows, cols, (size_t)cols * sizeof(float)))) return rc;
  enqueue_pyramid(c, L, Plane{c->d_in, c->in_pitch, c->in_img}, 1, false);
  // SIFT_FLAG_FAST: an expired in-kernel wait of pyr_pc_kernel (err[3]) means
  // the planes are invalid -- reported by this call, and consumed so that it
  // cannot surface in a later one
  enqueue_status(c, false, nullptr, 1, c->kp_cap);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if ((rc = take_status(c, false, kErrStall))) return rc;
  if ((rc = copy_pyramid(c, L, c->d_gpyr, nullptr, gpyr, kScales))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

int sift_build_dog_pyramid(sift_ctx* c, const float* gpyr, int rows, int cols, int n_octaves,
                           float* dog) {
  int rc = enter(c, gpyr && dog, "null buffer", rows, cols, n_octaves, 1);
  if (rc) return rc;
  const Layout L = make_layout(rows, cols, n_octaves);
  if ((rc = copy_pyramid(c, L, c->d_gpyr, gpyr, nullptr, kScales))) return rc;
  for (int o = 0; o < L.n_oct; ++o) enqueue_dog(c, L, o, 1);
  HIP_TRY(c, hipGetLastError());
  if ((rc = copy_pyramid(c, L, c->d_dog, nullptr, dog, kDogPer))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SIFT_OK;
}

int sift_find_scale_space_extrema(sift_ctx* c, const float* gpyr, const float* dog, int rows,
                                  int cols, int n_octaves, sift_keypoint* kpts, int cap, int* n_out) {
  if (int rc = enter(c, gpyr && dog && n_out, "null buffer", rows, cols, n_octaves, 1)) return rc;
  const Layout L = make_layout(rows, cols, n_octaves);
  return host_detect(
      c, false, kpts, nullptr, cap, n_out,
      [&] {
        const int rc = copy_pyramid(c, L, c->d_gpyr, gpyr, nullptr, kScales);
        return rc ? rc : copy_pyramid(c, L, c->d_dog, dog, nullptr, kDogPer);
      },
      [&]() -> int {
        enqueue_detect(c, L, 1, c->d_kpts, c->kp_cap, c->d_img_off, false);
        enqueue_status(c, true, c->d_img_off, 1, c->kp_cap);
        HIP_TRY(c, hipGetLastError());
        return SIFT_OK;
      });
}

int sift_calc_descriptors(sift_ctx* c, const float* gpyr, int rows, int cols, int n_octaves,
                          const sift_keypoint* kpts, int n, float* desc, int first_octave) {
  int rc = enter(c, gpyr && (n <= 0 || (kpts && desc)) && n >= 0, "null buffer", rows, cols, n_octaves, 1);
  if (rc || n == 0) return rc;
  const Layout L = make_layout(rows, cols, n_octaves);
  if ((rc = ensure_kp(c, n))) return rc;
  c->last_n = -1;  // the internal keypoint buffer is reused below
  if ((rc = copy_pyramid(c, L, c->d_gpyr, gpyr, nullptr, kScales))) return rc;
  const int off[2] = {0, n};
  HIP_TRY(c, hipMemcpyAsync(c->d_img_off, off, sizeof(off), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->d_kpts, kpts, sizeof(sift_keypoint) * n, hipMemcpyHostToDevice,
                            c->stream));
  // keypoints may name any scale 0..4 (CV_Assert at src/sift.cpp:744): gradients of all five
  launch_grad(c->stream, L, c->d_gpyr, c->d_grad, 1, 0, kScales - 1, c->d_mc);
  if ((rc = ensure_perm(c, c->kp_cap))) return rc;
  enqueue_desc(c, L, c->d_kpts, c->d_img_off, 1, c->kp_cap, c->d_desc, first_octave, false);
  enqueue_status(c, false, nullptr, 1, c->kp_cap);  // no detection ran: assertion bit only
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if ((rc = take_status(c, false, kErrAssert))) return rc;
  HIP_TRY(c, hipMemcpy(desc, c->d_desc, sizeof(float) * kDescLen * n, hipMemcpyDeviceToHost));
  return SIFT_OK;
}

int sift_selftest_g4_points(sift_ctx* c, const float* plane, int rows, int cols, const int* rc, int n, float* out) {
  if (int r = enter(c, plane && (n <= 0 || (rc && out)) && n >= 0, "null buffer", rows, cols, 1, 1)) return r;
  if (n == 0) return SIFT_OK;
  const Layout L = make_layout(rows, cols, 1);
  std::vector<Cand> pts((size_t)n);
  for (int i = 0; i < n; ++i) {
    if (abs(rc[2 * i]) >= (1 << 20) || abs(rc[2 * i + 1]) >= (1 << 20)) return fail(c, SIFT_E_INVALID, "point out of range");
    pts[i] = Cand{0, kLayers << 8, rc[2 * i], rc[2 * i + 1]};
  }
  Buf<Cand> dpts;  // freed on every way out
  Buf<float> dout;
  HIP_TRY(c, dpts.grow((size_t)n));
  HIP_TRY(c, dout.grow((size_t)n * 9));
  // blocking copies and a synchronisation before every way out: the points
  // and the two device buffers are locals the stream must not outlive
  const size_t w = (size_t)cols * sizeof(float);
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // earlier work may still use d_gpyr
  HIP_TRY(c, hipMemcpy2D(c->d_gpyr + L.oct[0].g_off[0], L.oct[0].pitch * sizeof(float), plane, w, w, rows,
                         hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(dpts, pts.data(), sizeof(Cand) * n, hipMemcpyHostToDevice));
  launch_g4_points(c->stream, L, c->d_gpyr, coef4_table(c), dpts, n, dout, c->g4_grid);
  const hipError_t le = hipGetLastError(), se = hipStreamSynchronize(c->stream);
  HIP_TRY(c, le);
  HIP_TRY(c, se);
  HIP_TRY(c, hipMemcpy(out, dout, sizeof(float) * 9 * n, hipMemcpyDeviceToHost));
  return SIFT_OK;
}

int sift_g4_fill_stats(sift_ctx* c, int* first_slots, int* waiting, int* max_fills) {
  if (!c || !first_slots || !waiting || !max_fills) return SIFT_E_INVALID;
  (void)hipSetDevice(c->device);
  int v[kG4Stats] = {};
  if (c->g4stat.get()) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(v, c->g4stat, sizeof(v), hipMemcpyDeviceToHost));
  }
  *first_slots = v[kG4StatFirst];
  *waiting = v[kG4StatWait];
  // a slot that never waited took its first fill only; the rounds count the others
  *max_fills = std::max(v[kG4StatFills], v[kG4StatFirst] > 0 ? 1 : 0);
  return SIFT_OK;
}

int sift_selftest_math(sift_ctx* c, int op, const float* a, const float* b, float* out, int n) {
  if (!c) return SIFT_E_INVALID;
  if (!a || !out || n < 0 || op < 0 || op > 9 || ((op == 1 || op == 2 || op >= 8) && !b))
    return fail(c, SIFT_E_INVALID, "bad selftest arguments");
  if (n == 0) return SIFT_OK;
  (void)hipSetDevice(c->device);
  Buf<float> da, db, dout;  // freed on every way out
  HIP_TRY(c, da.grow((size_t)n));
  HIP_TRY(c, db.grow((size_t)n));
  HIP_TRY(c, dout.grow((size_t)n));
  hipError_t e = hipMemcpy(da, a, sizeof(float) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess && b) e = hipMemcpy(db, b, sizeof(float) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    if (op >= 8)
      launch_update_num_iters_selftest(c->stream, op == 8 ? 0.995 : 0.5, da, db, dout, n);
    else
      launch_math_selftest(c->stream, op, da, db, dout, n, c->d_mc);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(out, dout, sizeof(float) * n, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(c, e, "sift_selftest_math");
  return SIFT_OK;
}

}  // extern "C"
