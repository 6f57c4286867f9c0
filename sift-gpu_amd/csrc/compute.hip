// compute.hip -- the device stage of sift_compute_batch that prepares the
// caller's keypoint rows for the descriptor kernel (descriptor.hip): it bounds
// the rows by the clamped offsets, validates each row, and sorts the valid
// rows into the two lists the descriptor launches read (launch_compute_prep,
// common.hpp).  A row's image is not needed here (every image of a batch has
// one size): descriptor_kernel finds it from the same offsets, and for a row
// inside [clamp(off[0]), clamp(off[batch])) its scan of the raw offsets lands
// on the image that owns the row under the clamped rule.
#include <algorithm>

#include "match_seg.hpp"

namespace sift {

namespace {

struct PrepArgs {
  Layout L;
  const sift_keypoint* kpts;
  const int* off;  // [batch + 1]
  int batch, kp_cap, max_layer, first_octave;
  float* desc;
  int* err_flag;
  DescLists lists;
};

constexpr int kMaxDetRadius = 40;  // descriptor.hip: (kMaxWinRows - 1) / 2

// One workgroup per run of kComputeChunk consecutive rows, one lane per row.
// The class of a row: -1 nothing to describe (outside the offsets, or invalid),
// 0 the detected-keypoint form, 1 the general form.  A run reserves its part of
// each list with one atomic add, and writes it ranked by (window size, row).
__global__ __launch_bounds__(kComputeChunk) void compute_prep_kernel(PrepArgs A) {
  __shared__ __attribute__((aligned(16))) int keys[kComputeChunk];
  __shared__ signed char cls_s[kComputeChunk];
  __shared__ int base_s[2];
  const int t = threadIdx.x;
  const int lo = clamp_row(A.off[0], A.kp_cap), hi = clamp_row(A.off[A.batch], A.kp_cap);
  const int first = lo / kComputeChunk * kComputeChunk;
  for (int c0 = first + blockIdx.x * kComputeChunk; c0 < hi; c0 += gridDim.x * kComputeChunk) {
    const int i = c0 + t;
    int cls = -1, key = 0;
    if (i >= lo && i < hi) {
      const sift_keypoint kp = A.kpts[i];
      // unpackOctave (src/sift.cpp:724-731), as descriptor_kernel reads it; the
      // pyramid starts at octave first_octave: 0 (the reference never
      // upsamples), or -1 when L is the doubled image's (sift_set_upsample)
      int octave = kp.octave & 255;
      const int layer = (kp.octave >> 8) & 255;
      octave = octave < 128 ? octave : (-128 | octave);
      const int oi = octave - A.first_octave;
      if (oi < 0 || oi >= A.L.n_oct || layer > kLayers + 2 || layer > A.max_layer) {
        atomicOr(A.err_flag, 1);
        float4* row = reinterpret_cast<float4*>(A.desc + (long long)i * kDescLen);
        for (int q = 0; q < kDescLen / 4; ++q) row[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        // the window radius and the keypoint's pixel by descriptor_kernel's own
        // expressions (its setup after unpackOctave)
        const int d = kDescW;
        const float scale = octave >= 0 ? 1.f / (1 << octave) : (float)(1 << -octave);
        const float size = kp.size * scale;
        const float ptx = kp.x * scale, pty = kp.y * scale;
        const float scl = size * 0.5f;
        const Octave& O = A.L.oct[oi];
        const int rows = O.rows, cols = O.cols;
        const int px = cv_round(ptx), py = cv_round(pty);
        const float hist_width = 3.f * scl;
        int radius = cv_round(hist_width * 1.4142135623730951f * (d + 1) * 0.5f);
        const int diag = (int)sqrt(((double)cols) * cols + ((double)rows) * rows);
        radius = radius < diag ? radius : diag;
        // The detected-keypoint form needs a row table (radius <= 40) and a
        // finite gradient under the keypoint's own pixel, where its masked
        // samples gather: an interior pixel (border gradients are never
        // written).  A window of no positive width (size <= 0, NaN) stays with
        // the general form, which is what calDescriptor runs on it.
        const bool det = hist_width > 0.f && radius <= kMaxDetRadius && px >= 1 && px <= cols - 2 && py >= 1 &&
                         py <= rows - 2;
        cls = det ? 0 : 1;
        key = __float_as_int(fabsf(size));  // desc_rank_kernel's key
      }
    }
    __syncthreads();  // the previous run's ranking has read keys and cls_s
    keys[t] = key;
    cls_s[t] = (signed char)cls;
    const int n0 = __syncthreads_count(cls == 0);
    const int n1 = __syncthreads_count(cls == 1);
    if (t == 0) {
      base_s[0] = n0 ? atomicAdd(A.lists.counts, n0) : 0;
      base_s[1] = n1 ? atomicAdd(A.lists.counts + 1, n1) : 0;
    }
    __syncthreads();
    if (cls >= 0) {
      int rank = 0;
      for (int u = 0; u < kComputeChunk; ++u) {
        const int ku = keys[u];
        rank += cls_s[u] == cls && (ku < key || (ku == key && u < t)) ? 1 : 0;
      }
      // every list position is below the number of valid rows, at most kp_cap
      (cls == 0 ? A.lists.det : A.lists.gen)[base_s[cls] + rank] = i;
    }
  }
}

}  // namespace

void launch_compute_prep(hipStream_t st, const Layout& L, const sift_keypoint* kpts, const int* off, int batch,
                         int kp_cap, int max_layer, float* desc, int* err_flag, const DescLists& lists,
                         int first_octave) {
  if (kp_cap <= 0) return;
  (void)hipMemsetAsync(lists.counts, 0, 2 * sizeof(int), st);
  PrepArgs A;
  A.L = L;
  A.kpts = kpts;
  A.off = off;
  A.batch = batch;
  A.kp_cap = kp_cap;
  A.max_layer = max_layer;
  A.first_octave = first_octave;
  A.desc = desc;
  A.err_flag = err_flag;
  A.lists = lists;
  const int chunks = (kp_cap + kComputeChunk - 1) / kComputeChunk + 1;  // + 1: the first run may start below off[0]
  hipLaunchKernelGGL(compute_prep_kernel, dim3(std::min(chunks, 4096)), dim3(kComputeChunk), 0, st, A);
}

}  // namespace sift
