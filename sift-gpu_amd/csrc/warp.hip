// warp.hip -- sift_warp_perspective[_segmented_device]: every image of a batch
// warped by its own homography, for gfx950.
//
// The arithmetic is warp_math.hpp's, the library's own statement of
//     cv::warpPerspective(src, dst, H, dsize, INTER_LINEAR [| WARP_INVERSE_MAP],
//                         BORDER_CONSTANT, 0)
// on CV_32FC1, CV_8UC1 and CV_8UC3 (written out in include/sift_hip.h, restated
// in numpy in tests/warp_inputs.py; parity against OpenCV itself is by
// construction and unpinned -- no OpenCV here).  Host and device take every
// expression from that header.
//
// Bound: HBM (f32: 4 B read, 4 B written per destination pixel; u8: 1 or 3 of
// each).  One launch, no scratch.  A workgroup of four waves owns a
// 256 x (4 * kWarpRows) destination tile of one image and forms the image's M
// itself from d_H[b] (about 40 double operations, wave-uniform), so there is
// no pre-kernel and no host value.  Lanes run along x; a lane owns four
// consecutive pixels -- one 16-B store (f32) or one / three dword stores (u8,
// u8 x 3) per row, a wave whole 128-B lines -- and a wave kWarpRows consecutive
// rows, whose terms M1 y, M4 y, M7 y are formed once per row.  The tile is
// several rows tall so that its source footprint under a rotation stays in
// cache, and the tiles are dealt so that each XCD (blocks b and b + 8 share
// one; speed only) takes a contiguous run of the raster-ordered tiles:
// neighbouring tiles of an image meet in one L2.  A tile whose segment is
// absent writes zeros and reads nothing.  Destinations whose rows are not
// 16-B (u8: 4-B) aligned take the same walk with narrower stores.  No byte
// outside the out_rows x out_cols pixels of each image is written.
#include <algorithm>

#include "common.hpp"
#include "warp_math.hpp"

#ifndef SIFT_WARP_ROWS
#define SIFT_WARP_ROWS 2  // A/B builds only (tools/build_var.sh): destination rows per wave
#endif
#ifndef SIFT_WARP_XCD
#define SIFT_WARP_XCD 1  // A/B builds only: 0 = tiles in launch order
#endif

namespace sift {

namespace {

using namespace wmath;

constexpr int kWarpWaves = 4;                       // waves per workgroup (threadIdx.y)
constexpr int kWarpRows = SIFT_WARP_ROWS;           // destination rows per wave
constexpr int kWarpTileH = kWarpWaves * kWarpRows;  // tile height
constexpr int kWarpTileW = 256;                     // tile width: 64 lanes x 4 pixels

struct WarpArgs {
  const unsigned char* src;
  long long spitch, simg;  // bytes
  int rows, cols;
  const double* H;
  const int* found;  // may be null: all found
  int inverse;
  unsigned char* dst;
  long long dpitch, dimg;  // bytes
  int orows, ocols;
  int tiles_x;
  long long tiles_img, total;
};

__device__ __forceinline__ unsigned pack4(const unsigned char* b) {
  return (unsigned)b[0] | ((unsigned)b[1] << 8) | ((unsigned)b[2] << 16) | ((unsigned)b[3] << 24);
}

// U8: unsigned char pixels of CH interleaved channels; else float (CH = 1).
template <bool U8, int CH, bool VEC>
__global__ __launch_bounds__(64 * kWarpWaves) void warp_kernel(WarpArgs A) {
#if SIFT_WARP_XCD
  // XCD x takes tiles [x per, (x + 1) per), its blocks interleaved over them
  const long long per = (A.total + 7) / 8, step = gridDim.x >> 3;
  const int xcd = blockIdx.x & 7;
  long long t = xcd * per + (blockIdx.x >> 3);
  const long long t_end = (xcd + 1) * per < A.total ? (xcd + 1) * per : A.total;
#else
  const long long step = gridDim.x, t_end = A.total;
  long long t = blockIdx.x;
#endif
  for (; t < t_end; t += step) {
    const long long b = t / A.tiles_img, rem = t - b * A.tiles_img;
    const int ty = (int)(rem / A.tiles_x), tx = (int)(rem - (long long)ty * A.tiles_x);
    const int x0 = (tx * 64 + (int)threadIdx.x) * 4;  // this lane's pixels x0 .. x0 + 3
    if (x0 >= A.ocols) continue;
    const int npx = A.ocols - x0 < 4 ? A.ocols - x0 : 4;

    double H[9], M[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = A.H[b * 9 + i];
    bool ok = warp_matrix(H, A.inverse != 0, M);
    if (A.found) ok = ok && A.found[b] != 0;

    const unsigned char* __restrict__ S = A.src + b * A.simg;
    unsigned char* __restrict__ D = A.dst + b * A.dimg;
    const int y0 = ty * kWarpTileH + (int)threadIdx.y * kWarpRows;
    const int y1 = y0 + kWarpRows < A.orows ? y0 + kWarpRows : A.orows;
    for (int y = y0; y < y1; ++y) {
      const RowTerms R = row_terms(M, y);
      unsigned char* drow = D + (long long)y * A.dpitch;
      if (!U8) {
        float v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const Coord c = ok && q < npx ? source_coord(M, R, x0 + q) : Coord{0, 0, 0, 0, false};
          v[q] = pixel_f32(S, A.rows, A.cols, A.spitch, c);
        }
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
        for (int q = 0; q < 4; ++q) {
          const Coord c = ok && q < npx ? source_coord(M, R, x0 + q) : Coord{0, 0, 0, 0, false};
          pixel_u8<CH>(S, A.rows, A.cols, A.spitch, c, v + q * CH);
        }
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

template <bool U8, int CH>
void launch(hipStream_t st, const WarpArgs& A, bool vec) {
  // a multiple of 8 (whole XCD runs); beyond 2^24 workgroups the tiles are strided over
  const unsigned grid = (unsigned)std::min<long long>((A.total + 7) / 8 * 8, 1ll << 24);
  if (vec)
    hipLaunchKernelGGL((warp_kernel<U8, CH, true>), dim3(grid), dim3(64, kWarpWaves), 0, st, A);
  else
    hipLaunchKernelGGL((warp_kernel<U8, CH, false>), dim3(grid), dim3(64, kWarpWaves), 0, st, A);
}

}  // namespace

void launch_warp_perspective(hipStream_t st, bool u8, int channels, const void* src, long long spitch, long long simg,
                             int rows, int cols, const double* H, const int* found, int n_segments, bool inverse,
                             void* dst, long long dpitch, long long dimg, int orows, int ocols) {
  if (n_segments < 1 || rows < 1 || cols < 1 || orows < 1 || ocols < 1) return;
  WarpArgs A{static_cast<const unsigned char*>(src), spitch, simg, rows, cols, H, found, inverse ? 1 : 0,
             static_cast<unsigned char*>(dst), dpitch, dimg, orows, ocols, 0, 0, 0};
  A.tiles_x = (ocols + kWarpTileW - 1) / kWarpTileW;
  A.tiles_img = (long long)A.tiles_x * ((orows + kWarpTileH - 1) / kWarpTileH);
  A.total = A.tiles_img * n_segments;
  const long long align = u8 ? 4 : 16;
  const bool vec = reinterpret_cast<uintptr_t>(dst) % align == 0 && dpitch % align == 0 &&
                   (n_segments == 1 || dimg % align == 0);
  if (!u8)
    launch<false, 1>(st, A, vec);
  else if (channels == 1)
    launch<true, 1>(st, A, vec);
  else
    launch<true, 3>(st, A, vec);
}

}  // namespace sift
