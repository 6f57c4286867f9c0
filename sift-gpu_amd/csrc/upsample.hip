// upsample.hip -- the doubled input image of Lowe's "octave -1" (OpenCV's
// SIFT firstOctave = -1; sift_set_upsample, sift_upsample2x[_device]) for gfx950.
//
// The arithmetic is the library's own statement of
//     cv::resize(src, dst, Size(2 * cols, 2 * rows), 0, 0, INTER_LINEAR)
// on CV_32F (restated in numpy in tests/upsample_inputs.py; parity against
// OpenCV itself is by construction and unpinned -- no OpenCV here).  A
// horizontal pass, then a vertical pass, both in float, every value formed as
// a * w0 + b * w1 with two multiplies and one add, never fused (the library is
// compiled with -ffp-contract=off).  For destination index d of an axis of n
// source samples, the same rule for columns and rows:
//     d even: s = d / 2 - 1,   weights (0.25f, 0.75f) on (S[s], S[s + 1])
//     d odd:  s = (d - 1) / 2, weights (0.75f, 0.25f)
//     s < 0:      the value is S[0], copied (no multiply)
//     s >= n - 1: the value is S[n - 1], copied (no multiply)
//     D[dy][dx] = Hrow[j0][dx] * v0 + Hrow[j1][dx] * v1,
//     Hrow[r][dx] = S[r][i0] * w0 + S[r][i1] * w1.
// So a 1 x 1 image gives four copies, and a 1 x N or N x 1 image doubles both
// axes.
//
// Bound: HBM (4 B read, 16 B written per source pixel).  One lane owns four
// destination columns -- one 16-B store per destination row, a wave 1 KiB of
// a row, eight whole 128-B lines when the row starts on one -- and walks a
// strip of kUpRows source rows down the image, keeping the horizontal pass of
// the previous and the current source row in registers, so a source row is
// read (kUpRows + 2) / kUpRows times.  Destinations whose rows are not 16-B
// aligned take the same walk with scalar stores.  No byte outside the
// 2 rows x 2 cols destination pixels is written: row padding stays untouched.
#include <algorithm>

#include "common.hpp"

namespace sift {

namespace {

constexpr int kUpRows = 8;    // source rows per lane
constexpr int kUpStrips = 4;  // strips per workgroup (threadIdx.y)

struct UpArgs {
  const float* src;
  long long spitch, simg;
  int rows, cols, batch;
  float* dst;
  long long dpitch, dimg;
};

// The horizontal pass of source row r at destination columns 4k .. 4k + 3.
// Source columns 2k - 1 .. 2k + 2 are fetched clamped to the row; a clamped
// value is either the copy the rule asks for or belongs to a column past the
// destination's last, which the caller never stores.
__device__ __forceinline__ void up_hrow(const float* __restrict__ row, int k, int n, float h[4]) {
  const int i = 2 * k;
  const float a = row[i > 0 ? i - 1 : 0], b = row[i];
  const float c = row[i + 1 < n ? i + 1 : n - 1], d = row[i + 2 < n ? i + 2 : n - 1];
  h[0] = i - 1 < 0 ? b : a * 0.25f + b * 0.75f;       // dx = 4k:     s = 2k - 1
  h[1] = i >= n - 1 ? b : b * 0.75f + c * 0.25f;      // dx = 4k + 1: s = 2k
  h[2] = i >= n - 1 ? b : b * 0.25f + c * 0.75f;      // dx = 4k + 2: s = 2k
  h[3] = i + 1 >= n - 1 ? c : c * 0.75f + d * 0.25f;  // dx = 4k + 3: s = 2k + 1
}

template <bool VEC>
__device__ __forceinline__ void up_store(float* __restrict__ p, const float v[4], bool four) {
  if (VEC && four) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    p[0] = v[0];
    p[1] = v[1];
    if (four) {
      p[2] = v[2];
      p[3] = v[3];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(64 * kUpStrips) void upsample2x_kernel(UpArgs A) {
  const int k = blockIdx.x * 64 + threadIdx.x;  // destination columns 4k .. 4k + 3
  const int dcols = 2 * A.cols;
  if (4 * k >= dcols) return;
  const bool four = 4 * k + 3 < dcols;  // else the row ends after 4k + 1 (cols odd)
  for (int b = blockIdx.z; b < A.batch; b += gridDim.z) {
    const float* __restrict__ s = A.src + b * A.simg;
    float* __restrict__ d = A.dst + b * A.dimg + 4 * (long long)k;
    for (long long j0 = ((long long)blockIdx.y * kUpStrips + threadIdx.y) * kUpRows; j0 < A.rows;
         j0 += (long long)gridDim.y * kUpStrips * kUpRows) {
      const int j_end = j0 + kUpRows < A.rows ? (int)j0 + kUpRows : A.rows;
      float prev[4], cur[4], next[4];
      up_hrow(s + (j0 > 0 ? j0 - 1 : 0) * A.spitch, k, A.cols, prev);
      up_hrow(s + j0 * A.spitch, k, A.cols, cur);
      for (int j = (int)j0; j < j_end; ++j) {
        const bool last = j >= A.rows - 1;
        if (!last) up_hrow(s + (long long)(j + 1) * A.spitch, k, A.cols, next);
        float e[4], o[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          e[q] = j == 0 ? cur[q] : prev[q] * 0.25f + cur[q] * 0.75f;  // dy = 2j:     s = j - 1
          o[q] = last ? cur[q] : cur[q] * 0.75f + next[q] * 0.25f;    // dy = 2j + 1: s = j
        }
        up_store<VEC>(d + 2 * (long long)j * A.dpitch, e, four);
        up_store<VEC>(d + (2 * (long long)j + 1) * A.dpitch, o, four);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          prev[q] = cur[q];
          cur[q] = last ? cur[q] : next[q];
        }
      }
    }
  }
}

}  // namespace

void launch_upsample2x(hipStream_t st, const float* src, long long spitch, long long simg, int rows, int cols,
                       float* dst, long long dpitch, long long dimg, int batch) {
  if (batch < 1 || rows < 1 || cols < 1) return;
  const UpArgs A{src, spitch, simg, rows, cols, batch, dst, dpitch, dimg};
  const int groups = (2 * cols + 3) / 4, strip = kUpStrips * kUpRows;
  const dim3 grid((groups + 63) / 64, std::min((rows + strip - 1) / strip, 65535), std::min(batch, 65535));
  const bool vec = !(reinterpret_cast<uintptr_t>(dst) & 15) && dpitch % 4 == 0 && (batch == 1 || dimg % 4 == 0);
  if (vec)
    hipLaunchKernelGGL(upsample2x_kernel<true>, grid, dim3(64, kUpStrips), 0, st, A);
  else
    hipLaunchKernelGGL(upsample2x_kernel<false>, grid, dim3(64, kUpStrips), 0, st, A);
}

}  // namespace sift
