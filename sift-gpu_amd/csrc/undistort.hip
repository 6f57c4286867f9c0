// undistort.hip -- sift_undistort[_batch_device] and
// sift_undistort_points[_segmented[_device]]: every image, or every row of point
// pairs, of a batch taken through a lens model, for gfx950.
//
// The arithmetic is undistort_math.hpp's, the library's own statement of
// cv::undistort (INTER_LINEAR, BORDER_CONSTANT 0; CV_32FC1, CV_8UC1, CV_8UC3)
// and cv::undistortPoints for the 8-coefficient rational model (written out in
// include/sift_hip.h, restated in numpy in tests/undistort_oracle.py; parity
// against OpenCV itself is by construction and unpinned -- no OpenCV here).
// Host and device take every expression from that header.
//
// undistort_kernel.  Bound: HBM, as the warp (f32: 4 B read, 4 B written per
// destination pixel).  It is warp.hip's tile -- four waves, a 256 x
// (4 * kUndRows) destination tile, a lane owns four consecutive pixels of each
// of its wave's rows, 16-B (u8: dword) stores where the rows are aligned,
// XCD-contiguous tile order -- with one difference: the source position of a
// destination pixel depends on the camera alone, so a workgroup forms its
// tile's positions once (one thread forms the camera into LDS, about 60
// double operations and 18 divides; then per pixel five double divides and
// about 45 multiplies and adds), keeps them packed in registers, two ints per
// pixel, and walks with them a group of up to kUndGroup images that share the
// camera.  The double-precision part is paid once per group, not once per
// image; an image costs the sixteen gathers, the blend and the store.  With a
// camera per image a group is one image: the warp's shape.  A camera that
// undistorts to zeros packs every position as "outside": zeros are written and
// nothing is read.  No byte outside the out_rows x out_cols pixels of each
// image is written.
//
// undistort_points_kernel: a (chunk of 256 rows, segment) grid as
// triangulate_kernel's, one row per thread with everything in registers; the
// segment's camera (K^-1, the coefficients, P) is formed once per workgroup
// into LDS.  A segment's chunks past its end leave at once; segments may
// overlap or run backwards, so a row's segment is never searched for.
#include <algorithm>
#include <string.h>

#include "common.hpp"
#include "undistort_math.hpp"

#ifndef SIFT_UNDISTORT_ROWS
#define SIFT_UNDISTORT_ROWS 2  // A/B builds only (tools/build_var.sh): destination rows per wave
#endif
#ifndef SIFT_UNDISTORT_GROUP
#define SIFT_UNDISTORT_GROUP 8  // A/B builds only: images a workgroup walks with one set of positions
#endif

namespace sift {

namespace {

using namespace umath;

constexpr int kUndWaves = 4;                     // waves per workgroup (threadIdx.y)
constexpr int kUndRows = SIFT_UNDISTORT_ROWS;    // destination rows per wave
constexpr int kUndTileH = kUndWaves * kUndRows;  // tile height
constexpr int kUndTileW = 256;                   // tile width: 64 lanes x 4 pixels
constexpr int kUndGroup = SIFT_UNDISTORT_GROUP;  // images per workgroup under a shared camera
static_assert(kUndRows >= 1 && kUndGroup >= 1, "at least one row and one image");

struct UndArgs {
  const unsigned char* src;
  long long spitch, simg;  // bytes
  int rows, cols;
  const double *K, *dist, *newK;  // newK may be null: K
  int per;                        // 1: a camera per image (group == 1)
  int n, group;
  unsigned char* dst;
  long long dpitch, dimg;  // bytes
  int orows, ocols;
  int tiles_x;
  long long tiles_img, total;  // total = tiles_img * number of groups
};

__device__ __forceinline__ unsigned pack4(const unsigned char* b) {
  return (unsigned)b[0] | ((unsigned)b[1] << 8) | ((unsigned)b[2] << 16) | ((unsigned)b[3] << 24);
}

// U8: unsigned char pixels of CH interleaved channels; else float (CH = 1).
template <bool U8, int CH, bool VEC>
__global__ __launch_bounds__(64 * kUndWaves) void undistort_kernel(UndArgs A) {
  __shared__ ImageCam s_cam;
  __shared__ int s_ok;
  // XCD x takes tiles [x per, (x + 1) per), its blocks interleaved over them (warp.hip)
  const long long per = (A.total + 7) / 8, step = gridDim.x >> 3;
  const int xcd = blockIdx.x & 7;
  long long t = xcd * per + (blockIdx.x >> 3);
  const long long t_end = (xcd + 1) * per < A.total ? (xcd + 1) * per : A.total;
  const bool first_thread = threadIdx.x == 0 && threadIdx.y == 0;
  long long cam_have = -1;  // the camera s_cam holds; every bound of this loop is workgroup-uniform
  for (; t < t_end; t += step) {
    const long long g = t / A.tiles_img, rem = t - g * A.tiles_img;
    const int ty = (int)(rem / A.tiles_x), tx = (int)(rem - (long long)ty * A.tiles_x);
    const long long cam = A.per ? g : 0;
    if (cam != cam_have) {
      __syncthreads();  // the previous tile's positions are formed
      if (first_thread)
        s_ok = image_camera(A.K + cam * 9, A.dist + cam * 8, A.newK ? A.newK + cam * 9 : nullptr, s_cam);
      __syncthreads();
      cam_have = cam;
    }
    const int x0 = (tx * 64 + (int)threadIdx.x) * 4;  // this lane's pixels x0 .. x0 + 3
    const int npx = A.ocols - x0 < 4 ? A.ocols - x0 : 4;  // <= 0: none
    const int y0 = ty * kUndTileH + (int)threadIdx.y * kUndRows;

    // the tile's positions, once
    Packed P[kUndRows][4];
    const bool ok = s_ok != 0;
#pragma unroll
    for (int r = 0; r < kUndRows; ++r)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const bool live = ok && q < npx && y0 + r < A.orows;
        P[r][q] = pack(live ? source_coord(s_cam, x0 + q, y0 + r) : Coord{0, 0, 0, 0, false});
      }
    if (npx <= 0) continue;  // after the barriers: a lane past the last column stores nothing

    const long long b0 = g * A.group;
    const int nb = (int)(A.n - b0 < A.group ? A.n - b0 : A.group);
    for (int k = 0; k < nb; ++k) {
      const unsigned char* __restrict__ S = A.src + (b0 + k) * A.simg;
      unsigned char* __restrict__ D = A.dst + (b0 + k) * A.dimg;
#pragma unroll
      for (int r = 0; r < kUndRows; ++r) {
        const int y = y0 + r;
        if (y >= A.orows) break;
        unsigned char* drow = D + (long long)y * A.dpitch;
        if (!U8) {
          float v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) v[q] = wmath::pixel_f32(S, A.rows, A.cols, A.spitch, unpack(P[r][q]));
          float* p = reinterpret_cast<float*>(drow) + x0;
          if (VEC && npx == 4) {
            *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (q < npx) p[q] = v[q];
          }
        } else {
          unsigned char v[4 * CH];
#pragma unroll
          for (int q = 0; q < 4; ++q) wmath::pixel_u8<CH>(S, A.rows, A.cols, A.spitch, unpack(P[r][q]), v + q * CH);
          unsigned char* p = drow + (long long)x0 * CH;
          if (VEC && npx == 4) {
#pragma unroll
            for (int w = 0; w < CH; ++w) reinterpret_cast<unsigned*>(p)[w] = pack4(v + 4 * w);
          } else {
#pragma unroll
            for (int i = 0; i < 4 * CH; ++i)
              if (i < npx * CH) p[i] = v[i];
          }
        }
      }
    }
  }
}

template <bool U8, int CH>
void launch(hipStream_t st, const UndArgs& A, bool vec) {
  // a multiple of 8 (whole XCD runs); beyond 2^24 workgroups the tiles are strided over
  const unsigned grid = (unsigned)std::min<long long>((A.total + 7) / 8 * 8, 1ll << 24);
  if (vec)
    hipLaunchKernelGGL((undistort_kernel<U8, CH, true>), dim3(grid), dim3(64, kUndWaves), 0, st, A);
  else
    hipLaunchKernelGGL((undistort_kernel<U8, CH, false>), dim3(grid), dim3(64, kUndWaves), 0, st, A);
}

constexpr int kPtsThreads = 256;

__device__ inline int clamp_off(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

__global__ __launch_bounds__(kPtsThreads) void undistort_points_kernel(
    const unsigned char* src, unsigned char* dst, long long stride, const int* __restrict__ moff, int n_segments,
    int m_cap, const double* __restrict__ K, const double* __restrict__ dist, const double* __restrict__ Pm, int per,
    int iters, int* __restrict__ ok_out) {
  __shared__ PointCam s_cam;
  __shared__ int s_ok;
  for (int b = blockIdx.y; b < n_segments; b += gridDim.y) {  // uniform over the workgroup
    const int lo = clamp_off(moff[b], m_cap), hi = clamp_off(moff[b + 1], m_cap);
    const long long first = (long long)lo + (long long)blockIdx.x * kPtsThreads;
    if (blockIdx.x != 0 && first >= hi) continue;  // chunk 0 stays: it reports the segment's flag
    const size_t c = per ? (size_t)b : 0;
    __syncthreads();  // the previous segment's camera is no longer read
    if (threadIdx.x == 0) {
      s_ok = point_camera(K + c * 9, dist + c * 8, Pm ? Pm + c * 9 : nullptr, s_cam);
      if (blockIdx.x == 0) ok_out[b] = s_ok;
    }
    __syncthreads();
    const long long i = first + threadIdx.x;
    if (i >= hi) continue;
    const float* in = reinterpret_cast<const float*>(src + i * stride);
    float ou = 0.f, ov = 0.f;
    if (s_ok) undistort_point(s_cam, iters, in[0], in[1], ou, ov);
    float* out = reinterpret_cast<float*>(dst + i * stride);
    out[0] = ou;
    out[1] = ov;
  }
}

}  // namespace

int undistort_group() { return kUndGroup; }

void launch_undistort(hipStream_t st, bool u8, int channels, const void* src, long long spitch, long long simg,
                      int rows, int cols, const double* K, const double* dist, const double* newK, int k_per_segment,
                      int n, void* dst, long long dpitch, long long dimg, int orows, int ocols) {
  if (n < 1 || rows < 1 || cols < 1 || orows < 1 || ocols < 1) return;
  UndArgs A{static_cast<const unsigned char*>(src), spitch, simg, rows, cols, K, dist, newK, k_per_segment ? 1 : 0, n,
            k_per_segment ? 1 : kUndGroup, static_cast<unsigned char*>(dst), dpitch, dimg, orows, ocols, 0, 0, 0};
  A.tiles_x = (ocols + kUndTileW - 1) / kUndTileW;
  A.tiles_img = (long long)A.tiles_x * ((orows + kUndTileH - 1) / kUndTileH);
  A.total = A.tiles_img * ((n + A.group - 1) / A.group);
  const long long align = u8 ? 4 : 16;
  const bool vec = reinterpret_cast<uintptr_t>(dst) % align == 0 && dpitch % align == 0 && (n == 1 || dimg % align == 0);
  if (!u8)
    launch<false, 1>(st, A, vec);
  else if (channels == 1)
    launch<true, 1>(st, A, vec);
  else
    launch<true, 3>(st, A, vec);
}

void launch_undistort_points_seg(hipStream_t st, const void* src, void* dst, long long stride, const int* moff,
                                 int n_segments, int m_cap, const double* K, const double* dist, const double* P,
                                 int k_per_segment, int iters, int* ok) {
  if (n_segments < 1) return;
  const long long chunks = ((long long)m_cap + kPtsThreads - 1) / kPtsThreads;
  const dim3 grid((unsigned)(chunks > 0 ? chunks : 1), (unsigned)(n_segments < 65535 ? n_segments : 65535));
  undistort_points_kernel<<<grid, kPtsThreads, 0, st>>>(static_cast<const unsigned char*>(src),
                                                        static_cast<unsigned char*>(dst), stride, moff, n_segments,
                                                        m_cap, K, dist, P, k_per_segment ? 1 : 0, iters, ok);
}

// One camera, n rows, on the host.  0: the rows are zeros (point_camera's rule).
int undistort_points(const double* K, const double* dist, const double* P, int iters, const void* src, void* dst,
                     size_t stride, int n) {
  PointCam C;
  const bool ok = point_camera(K, dist, P, C);
  const unsigned char* s = static_cast<const unsigned char*>(src);
  unsigned char* d = static_cast<unsigned char*>(dst);
  for (int i = 0; i < n; ++i) {
    float in[2], out[2] = {0.f, 0.f};
    memcpy(in, s + (size_t)i * stride, sizeof(in));
    if (ok) undistort_point(C, iters, in[0], in[1], out[0], out[1]);
    memcpy(d + (size_t)i * stride, out, sizeof(out));
  }
  return ok ? 1 : 0;
}

}  // namespace sift
