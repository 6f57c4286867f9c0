// common.hpp -- shared host/device definitions for the gfx950 SIFT library.
//
// Everything here that computes is an exact restatement of the reference
// arithmetic (canhld94/SIFT-GPU src/sift.cpp) and of the OpenCV-4.0 helpers it
// calls, so that device results equal the CPU path bit for bit.  The whole
// library is compiled with -ffp-contract=off: every a*b+c below is a separate
// multiply and add, like the reference's x86-64 build (makefile:25, no -march).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sift_hip.h"
#include "gauss_host.hpp"

namespace sift {

// ---- tuning constants, src/sift.cpp:4-47 ---------------------------------
constexpr int kScales = 5;          // nScales = nOctaveLayers + 3
constexpr int kDogPer = 4;          // DoG planes per octave
constexpr int kBorder = 5;          // SIFT_IMG_BORDER
constexpr int kMaxInterp = 5;       // SIFT_MAX_INTERP_STEPS
constexpr int kOriBins = 36;        // SIFT_ORI_HIST_BINS
constexpr int kMaxPeaks = 18;       // strict local maxima of a 36-bin circle
constexpr int kDescW = 4;           // SIFT_DESCR_WIDTH
constexpr int kDescBins = 8;        // SIFT_DESCR_HIST_BINS
constexpr int kDescLen = 128;
constexpr int kMaxOctaves = 12;
constexpr float kDogThreshold = 8.f;  // literal at src/sift.cpp:564
constexpr double kCvPi = 3.1415926535897932384626433832795;

// ---- pyramid layout in HBM ------------------------------------------------
// Per image: octave-major, 5 Gaussian planes then (separately) 4 DoG planes,
// each plane rows x pitch floats, pitch = cols rounded up to 32 floats (128 B,
// one L2 line), so every plane row, plane and image block starts on a line
// boundary: a 64-column strip's row is two whole lines, never a partial-line
// write.  (With 64-B pitches the 1080p image block was 55,251,520 B, an odd
// number of half lines, so every odd image of a batch was misaligned.)
// Invariant: the pitch padding columns [cols, pitch) of every plane hold
// unspecified values.  SIFT_FLAG_FAST's dwordx4 / dwordx2 plane stores
// (pyramid_pc.hip) write whole 4-column groups past cols there, and no kernel
// reads a column >= cols of a Gaussian or DoG plane (every reader bounds its
// columns by cols, and the sub-module API copies planes out row by row with
// cols columns); tests/test_gpu_fast.py::test_pitch_padding_is_never_read
// poisons the padding with NaN and requires unchanged results.
constexpr int kPitchAlign = 32;
struct Octave {
  int rows, cols, pitch;
  int pad_;
  long long g_off[kScales];   // element offset of Gaussian plane s in the image block
  long long d_off[kDogPer];   // element offset of DoG plane s in the image block
};

struct Layout {
  int n_oct;
  int rows, cols;
  int pad_;
  long long g_img;  // elements per image, Gaussian pyramid
  long long d_img;  // elements per image, DoG pyramid
  Octave oct[kMaxOctaves];
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

Layout make_layout(int rows, int cols, int n_oct);

// ---- candidate / keypoint work records -----------------------------------
struct Cand {            // one 26-neighbour extremum, in reference scan order
  int b, ol, r, c;       // image, octave | layer<<8, row, col
};

struct CandOut {         // result of refine + orientation for one candidate
  float x, y, size, response;
  int octave, npeaks, img, ref_r;  // npeaks: 1 if refinement kept it (the count is in DetectBufs::npeaks)
  float angle[kMaxPeaks];
  int ref_c, ref_layer;            // refined integer position / layer (orientation input)
};

// ---- OpenCV scalar helpers --------------------------
__device__ __forceinline__ int cv_round(float v) { return __float2int_rn(v); }
__device__ __forceinline__ int cv_round_d(double v) { return __double2int_rn(v); }
__device__ __forceinline__ int cv_floor(float v) {
  int i = (int)v;
  return i - (i > v);
}
__device__ __forceinline__ float sat_u8(float v) {
  int iv = cv_round(v);
  return (float)(iv < 0 ? 0 : iv > 255 ? 255 : iv);
}

// libm calls on the path, evaluated as (float)f((double)x) on CPU and GPU
// alike (see oracle/sift_oracle.c for the measured glibc deviation).
__device__ __forceinline__ float pow2f_cr(float y) { return (float)exp2((double)y); }
__device__ __forceinline__ float cosf_cr(float x) { return (float)cos((double)x); }
__device__ __forceinline__ float sinf_cr(float x) { return (float)sin((double)x); }

// hal::exp32f, scalar form (EXPTAB_SCALE = 6); tab = 64 floats 2^(j/64)*A0.
struct ExpConsts {
  float A1, A2, A3, A4, lo, hi, post, prescale;
};

template <bool CLAMP = true>  // false: see exp32f_v
__device__ __forceinline__ float exp32f(float v, const float* __restrict__ tab,
                                        const ExpConsts& k) {
  if (CLAMP) {
    v = v < k.lo ? k.lo : v;
    v = k.hi < v ? k.hi : v;
    v = v * k.prescale;
    int vi = cv_round(v);
    v = (v - (float)vi) * k.post;
    int t = (vi >> 6) + 127;
    t = !(t & ~255) ? t : t < 0 ? 0 : 255;
    float sc = __int_as_float(t << 23);
    float poly = (((v + k.A1) * v + k.A2) * v + k.A3) * v + k.A4;
    return sc * tab[vi & 63] * poly;
  } else {
    // see exp32f_v: same bits inside the argument range the callers state
    v = v * k.prescale;
    const float r = rintf(v);  // cv_round's value, kept as a float
    const int vi = (int)r;
    v = (v - r) * k.post;
    float poly = (((v + k.A1) * v + k.A2) * v + k.A3) * v + k.A4;
    return __builtin_amdgcn_ldexpf(tab[vi & 63], vi >> 6) * poly;
  }
}

// The same with the table held one entry per lane (lane j: tab[j]) and read
// with a cross-lane permute instead of an LDS gather; every lane of the wave
// must execute it.
// CLAMP = false is for callers whose argument lies in (-87, 0] (the
// descriptor's -(c^2 + r^2) / 8 over a window: > -1.6; the orientation's:
// > -36): exp32f's input clamp to [lo, hi] never acts there, and the exponent
// t = (vi >> 6) + 127 stays in [1, 127], so its clamp to [0, 255] does not
// act either and 2^(vi >> 6) * tab[...] is an exact power-of-two scaling of a
// normal float -- one v_ldexp_f32 gives the same bits as building the scale
// and multiplying.  (float)cv_round(v) is rintf(v) for |v| < 2^24, so the
// rounded value is kept as a float.  Outside that range the result is
// finite garbage (callers mask it).  The lane permute uses address bits [7:2]
// only, so vi << 2 indexes lane vi & 63.
template <bool CLAMP = true>
__device__ __forceinline__ float exp32f_v(float v, float tab_lane, const ExpConsts& k) {
  if (CLAMP) {
    v = v < k.lo ? k.lo : v;
    v = k.hi < v ? k.hi : v;
    v = v * k.prescale;
    int vi = cv_round(v);
    v = (v - (float)vi) * k.post;
    int t = (vi >> 6) + 127;
    t = !(t & ~255) ? t : t < 0 ? 0 : 255;
    float sc = __int_as_float(t << 23);
    float poly = (((v + k.A1) * v + k.A2) * v + k.A3) * v + k.A4;
    const float tv = __int_as_float(__builtin_amdgcn_ds_bpermute((vi & 63) << 2, __float_as_int(tab_lane)));
    return sc * tv * poly;
  } else {
    v = v * k.prescale;
    const float r = rintf(v);
    const int vi = (int)r;
    v = (v - r) * k.post;
    float poly = (((v + k.A1) * v + k.A2) * v + k.A3) * v + k.A4;
    const float tv = __int_as_float(__builtin_amdgcn_ds_bpermute(vi << 2, __float_as_int(tab_lane)));
    return __builtin_amdgcn_ldexpf(tv, vi >> 6) * poly;
  }
}

// hal::fastAtan2 in degrees.
struct AtanConsts {
  float p1, p3, p5, p7, eps;
};

__device__ __forceinline__ float fast_atan2(float y, float x, const AtanConsts& k) {
  float ax = fabsf(x), ay = fabsf(y);
  float mn = ax < ay ? ax : ay, mx = ax < ay ? ay : ax;
  float c = mn / (mx + k.eps);
  float c2 = c * c;
  float a = (((k.p7 * c2 + k.p5) * c2 + k.p3) * c2 + k.p1) * c;
  if (!(ax >= ay)) a = 90.f - a;
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

__device__ __forceinline__ float magnitude(float x, float y) { return sqrtf(x * x + y * y); }

// Matx33f::solve(b, DECOMP_LU): Cramer's rule with float determinant; a
// singular matrix yields 0 (OpenCV returns Matx::zeros()).
__device__ __forceinline__ void solve3(const float a[9], const float b[3], float x[3]) {
#define A_(i, j) a[(i)*3 + (j)]
  float d = (float)(A_(0, 0) * (A_(1, 1) * A_(2, 2) - A_(2, 1) * A_(1, 2)) -
                    A_(0, 1) * (A_(1, 0) * A_(2, 2) - A_(2, 0) * A_(1, 2)) +
                    A_(0, 2) * (A_(1, 0) * A_(2, 1) - A_(2, 0) * A_(1, 1)));
  if (d == 0) {
    x[0] = x[1] = x[2] = 0;
    return;
  }
  d = 1 / d;
  x[0] = d * (b[0] * (A_(1, 1) * A_(2, 2) - A_(1, 2) * A_(2, 1)) -
              A_(0, 1) * (b[1] * A_(2, 2) - A_(1, 2) * b[2]) +
              A_(0, 2) * (b[1] * A_(2, 1) - A_(1, 1) * b[2]));
  x[1] = d * (A_(0, 0) * (b[1] * A_(2, 2) - A_(1, 2) * b[2]) -
              b[0] * (A_(1, 0) * A_(2, 2) - A_(1, 2) * A_(2, 0)) +
              A_(0, 2) * (A_(1, 0) * b[2] - b[1] * A_(2, 0)));
  x[2] = d * (A_(0, 0) * (A_(1, 1) * b[2] - b[1] * A_(2, 1)) -
              A_(0, 1) * (A_(1, 0) * b[2] - b[1] * A_(2, 0)) +
              b[0] * (A_(1, 0) * A_(2, 1) - A_(1, 1) * A_(2, 0)));
#undef A_
}

// Host-computed constant block shared by every kernel that needs it.
struct MathConsts {
  ExpConsts e;
  AtanConsts t;
  float exptab[64];
};

void host_math_consts(MathConsts* mc);

// ---- persistent-grid sizing ------------------------------------------------
// The work-loop kernels (refinement, orientation, descriptors) split their
// items evenly over the grid.  A grid larger than what the device holds at
// once runs in rounds, and the last, partial round idles the rest of the chip
// (8192 orientation waves on 6144 wave slots = 2 rounds for 1.33 rounds of
// work).  So the grid is the resident count: occupancy API x CUs, a multiple
// of 8 (the kernels' XCD split), cached per kernel; fixed_grid is the
// fallback when the occupancy query fails.
int resident_grid(const void* kernel, int block, size_t lds, int fixed_grid);

// ---- host launchers (defined in the .hip files) --------------------------
struct Plane {          // a device plane (or the input image)
  const float* p;
  long long pitch;      // elements per row
  long long img_stride; // elements per image of the batch
};

// blur.hip
void launch_blur_plane(hipStream_t st, int w, const float* coef, Plane src, float* dst,
                       long long dpitch, long long dimg, int rows, int cols, int batch);
// fuse_next: also write octave o+1's plane 0 (the INTER_NEAREST half of plane
// 2) when blur_fuses_decimation(L, o + 1); the caller then skips the decimation.
void launch_blur_octave(hipStream_t st, const Layout& L, int o, float* gpyr, const float* coefs,
                        const int* wsz, int batch, bool fuse_next = false);
bool blur_fuses_decimation(const Layout& L, int o);
// The same planes for small launches (2 outputs per lane, 32 x 16 tiles;
// round 3): picked when blur_octave_tiles(...) is below the context's limit.
void launch_blur_octave_small(hipStream_t st, const Layout& L, int o, float* gpyr, const float* coefs,
                              const int* wsz, int batch, bool fuse_next = false);
long long blur_octave_tiles(const Layout& L, int o, int batch);
// Exact blur in symmetric scatter form for SIFT_NCL's five fixed tables
// (compile-time constants); sym_tables_match(coefs) checks them against the
// context's base + octave tables before these are used.
bool sym_tables_match(const float* coefs);
void launch_blur_base_sym(hipStream_t st, Plane src, float* dst, long long dpitch, long long dimg, int rows,
                          int cols, int batch);
// no_plane4: planes 1..3 only (three slots, chunks sized from w = 12); plane 4
// keeps whatever it held.
void launch_blur_octave_sym(hipStream_t st, const Layout& L, int o, float* gpyr, int batch, bool fuse_next,
                            bool no_plane4 = false);
void launch_decimate(hipStream_t st, const Layout& L, int o, float* gpyr, int batch);
void launch_dog(hipStream_t st, const Layout& L, int o, const float* gpyr, float* dog, int batch);
void launch_blur_1d(hipStream_t st, int w, const float* coef1d, Plane src, float* tmp, float* dst,
                    long long pitch, long long img, int rows, int cols, int batch);
void launch_synth(hipStream_t st, float* out, int batch, int rows, int cols, long long pitch,
                  long long img_stride, int seed_base);

void launch_bgr8_gray(hipStream_t st, const uint8_t* src, long long sstride, long long simg, int srows, int scols,
                      float* dst, long long dpitch, long long dimg, int drows, int dcols, int batch);
// upsample.hip: the doubled input image of sift_set_upsample (INTER_LINEAR on
// CV_32F, the rule at the head of that file); strides in elements.  Writes the
// 2 rows x 2 cols destination pixels of each image and nothing else.
void launch_upsample2x(hipStream_t st, const float* src, long long spitch, long long simg, int rows, int cols,
                       float* dst, long long dpitch, long long dimg, int batch);
// warp.hip: warpPerspective of every image of a batch by its own homography
// (warp_math.hpp's rule); strides in bytes, simg 0 = one source for every H,
// found may be null.  Writes the orows x ocols destination pixels of each image
// and nothing else.
void launch_warp_perspective(hipStream_t st, bool u8, int channels, const void* src, long long spitch, long long simg,
                             int rows, int cols, const double* H, const int* found, int n_segments, bool inverse,
                             void* dst, long long dpitch, long long dimg, int orows, int ocols);
// undistort.hip: cv::undistort of every image of a batch and cv::undistortPoints of every segment of point rows
// (undistort_math.hpp's rule); strides in bytes, simg 0 = one source for every camera.  K [9], dist [8], newK /
// P [9] (may be null) are one camera (k_per_segment 0) or one per image / segment.  The image call writes the
// orows x ocols destination pixels of each image and nothing else; the point call the (x, y) floats of the
// segments' rows, stride bytes apart (dst may be src), and ok [n_segments].  undistort_points is the host loop
// for one camera (0: zeros); undistort_group the images a workgroup walks under a shared camera.
void launch_undistort(hipStream_t st, bool u8, int channels, const void* src, long long spitch, long long simg,
                      int rows, int cols, const double* K, const double* dist, const double* newK, int k_per_segment,
                      int n, void* dst, long long dpitch, long long dimg, int orows, int ocols);
void launch_undistort_points_seg(hipStream_t st, const void* src, void* dst, long long stride, const int* moff,
                                 int n_segments, int m_cap, const double* K, const double* dist, const double* P,
                                 int k_per_segment, int iters, int* ok);
int undistort_points(const double* K, const double* dist, const double* P, int iters, const void* src, void* dst,
                     size_t stride, int n);
int undistort_group();
int find_homography_ransac(const float* src_xy, const float* dst_xy, int n, double thr, int max_iters,
                           double confidence, double* H, unsigned char* mask_out);
void perspective_transform(const double* H, const float* xy, int n, float* out);
// Segmented forms (device-resident offsets, homography_batch.hip): one
// workgroup per segment; the scratch pieces are scratch.hpp's HomogParts.
struct HomogState;
void launch_homography_seg(hipStream_t st, const float* src_xy, const float* dst_xy, const int* moff, int n_segments,
                           int m_cap, double thr, int max_iters, double confidence, int* subsets, double* models,
                           int* counts, HomogState* state, unsigned char* mask, double* H, int* found,
                           unsigned char* mask_out);
void launch_perspective_seg(hipStream_t st, const double* H, const int* found, int n_segments, const float* xy,
                            int n_pts, float* out);
// affine.hip: estimateAffine2D / estimateAffinePartial2D (RANSAC) on the host; A is 2x3 row-major.
// model: SIFT_MODEL_AFFINE / SIFT_MODEL_SIMILARITY, anything else gives none.
int estimate_affine_ransac(const float* src_xy, const float* dst_xy, int n, int model, double thr, int max_iters,
                           double confidence, double* A, unsigned char* mask_out);
// affine_batch.hip: the same per segment, one workgroup each, no scratch; H is [n_segments][9], last row 0 0 1.
void launch_affine_seg(hipStream_t st, const float* src_xy, const float* dst_xy, const int* moff, int n_segments,
                       int m_cap, int model, double thr, int max_iters, double confidence, double* H, int* found,
                       unsigned char* mask_out);
// fundamental.hip: findFundamentalMat(FM_RANSAC) on the host; F is 3x3 row-major, [dst;1]^T F [src;1] = 0.
int find_fundamental_ransac(const float* src_xy, const float* dst_xy, int n, double thr, int max_iters,
                            double confidence, double* F, unsigned char* mask_out);
// fundamental_batch.hip: the same per segment, one workgroup each, no scratch; F is [n_segments][9].
void launch_fundamental_seg(hipStream_t st, const float* src_xy, const float* dst_xy, const int* moff, int n_segments,
                            int m_cap, double thr, int max_iters, double confidence, double* F, int* found,
                            unsigned char* mask_out);
// pose.hip: recoverPose (cheirality over four candidate poses of E = K_dst^T F K_src) and triangulatePoints
// on the host; pose is [R | t] row-major (12), xyz [n][3], xyzw [n][4]; mask_in, E, mask_out, xyz may be null.
int recover_pose(const double* F, const double* K_src, const double* K_dst, const float* src_xy, const float* dst_xy,
                 int n, const unsigned char* mask_in, double distance_thresh, double* pose, double* E,
                 unsigned char* mask_out, double* xyz, int* n_good);
void triangulate_points(const double* P_src, const double* P_dst, const float* src_xy, const float* dst_xy, int n,
                        double* xyzw);
// pose_batch.hip: the same per segment; one workgroup each, no scratch.  K is one 3x3 (k_per_segment 0) or
// [n_segments][9]; pose is [n_segments][12], E [n_segments][9], xyz [m_cap][3]; P_src / P_dst [n_segments][12].
void launch_recover_pose_seg(hipStream_t st, const float* src_xy, const float* dst_xy, const int* moff, int n_segments,
                             int m_cap, const double* F, const int* found, const double* K_src, const double* K_dst,
                             int k_per_segment, const unsigned char* mask_in, double distance_thresh, double* pose,
                             double* E, int* pose_found, int* n_good, unsigned char* mask_out, double* xyz);
void launch_triangulate_seg(hipStream_t st, const float* src_xy, const float* dst_xy, const int* moff, int n_segments,
                            int m_cap, const double* P_src, const double* P_dst, double* xyzw);
// pnp.hip: solveP3P (up to four poses, returns their number) and solvePnPRansac on the host; xyz is [n][3]
// doubles, xy [n][2] floats, a pose [R | t] row-major (12); row_mask and mask_out may be null.
int solve_p3p(const double* xyz, const float* xy, const double* K, double* poses);
int solve_pnp_ransac(const double* xyz, const float* xy, int n, const unsigned char* row_mask, const double* K,
                     double thr, int max_iters, double confidence, double* pose, unsigned char* mask_out,
                     int* n_inliers);
// pnp_batch.hip: the same per segment; one workgroup each, no scratch.  K is one 3x3 (k_per_segment 0) or
// [n_segments][9]; pose is [n_segments][12].
void launch_pnp_seg(hipStream_t st, const double* xyz, const float* xy, const int* moff, int n_segments, int m_cap,
                    const unsigned char* row_mask, const double* K, int k_per_segment, double thr, int max_iters,
                    double confidence, double* pose, int* found, int* n_inliers, unsigned char* mask_out);
// sift_selftest_math ops 8 / 9: out[i] = update_num_iters(confidence, (good[i] of n[i] pairs), 4, 2000)
void launch_update_num_iters_selftest(hipStream_t st, double confidence, const float* good, const float* n, float* out,
                                      int count);
int knn_splits(int nq, int nt);
void launch_knn_l1(hipStream_t st, const float* q, int nq, const float* t, int nt, int k, int splits,
                   float2* part_d, int2* part_i, int* idx, float* dist);
// Segmented form (device-resident offsets, match.hip): the grid is sized from
// the capacities, knn_seg_max_tiles() query tiles by knn_seg_splits() train
// splits; tile_start is [n_segments + 1] ints of scratch, the partials
// [splits * q_cap] (unused when splits == 1).
int knn_seg_max_tiles(int q_cap, int n_segments);
int knn_seg_splits(int q_cap, int n_segments, int t_cap, bool seg_train);
void launch_knn_l1_seg(hipStream_t st, const float* q, const int* qoff, int n_segments, int q_cap, const float* t,
                       const int* toff, int t_cap, int k, int splits, int* tile_start, float2* part_d, int2* part_i,
                       int* idx, float* dist);
// match_u8.hip: the byte quantiser (rows [0, min(*n_rows, row_cap)), all row_cap
// rows with n_rows null) and the segmented L1 matcher on byte rows -- the grid
// is knn_u8_seg_max_tiles() query tiles by knn_u8_seg_splits() train splits;
// tile_start is [n_segments + 1] ints of scratch, the integer partials
// [splits * q_cap] (unused when splits == 1).  launch_set_offsets writes the two
// offsets of a one-segment call.
void launch_desc_to_u8(hipStream_t st, const float* desc, const int* n_rows, int row_cap, uint8_t* out);
int knn_u8_seg_max_tiles(int q_cap, int n_segments);
int knn_u8_seg_splits(int q_cap, int n_segments, int t_cap, bool seg_train);
void launch_knn_l1_u8_seg(hipStream_t st, const uint8_t* q, const int* qoff, int n_segments, int q_cap,
                          const uint8_t* t, const int* toff, int t_cap, int k, int splits, int* tile_start,
                          int2* part_d, int2* part_i, int* idx, float* dist);
void launch_set_offsets(hipStream_t st, int* off, int a, int b);
// match_l2_u8.hip: the segmented squared-L2 matcher on byte rows (i8 MFMA) --
// the grid is knn_l2_u8_seg_max_tiles() query tiles by knn_l2_u8_seg_splits()
// train splits; tile_start is [n_segments + 1] ints of scratch, q_norm [q_cap]
// and t_norm [t_cap + kL2NormPad] ints (written by the launch's own pre-kernel),
// the integer partials [splits * q_cap] (unused when splits == 1).
constexpr int kL2NormPad = 32;
int knn_l2_u8_seg_max_tiles(int q_cap, int n_segments);
int knn_l2_u8_seg_splits(int q_cap, int n_segments, int t_cap, bool seg_train);
void launch_knn_l2sqr_u8_seg(hipStream_t st, const uint8_t* q, const int* qoff, int n_segments, int q_cap,
                             const uint8_t* t, const int* toff, int t_cap, int k, int splits, int* tile_start,
                             int* q_norm, int* t_norm, int2* part_d, int2* part_i, int* idx, float* dist);
// match_l2_f32.hip: the segmented squared-L2 matcher on float rows (f32 MFMA) --
// the grid is knn_l2_f32_seg_max_tiles() query tiles by knn_l2_f32_seg_splits()
// train splits; tile_start is [n_segments + 1] ints of scratch, q_norm [q_cap]
// and t_norm [t_cap + kL2F32NormPad] floats (written by the launch's own
// pre-kernel), the float partials [splits * q_cap] (unused when splits == 1).
constexpr int kL2F32NormPad = 64;
int knn_l2_f32_seg_max_tiles(int q_cap, int n_segments);
int knn_l2_f32_seg_splits(int q_cap, int n_segments, int t_cap, bool seg_train);
void launch_knn_l2sqr_f32_seg(hipStream_t st, const float* q, const int* qoff, int n_segments, int q_cap,
                              const float* t, const int* toff, int t_cap, int k, int splits, int* tile_start,
                              float* q_norm, float* t_norm, float2* part_d, int2* part_i, int* idx, float* dist);
// Ratio test + ordered compaction + point gather; blk_scan is
// [ratio_blocks(q_cap) + 1] ints of scratch.
int ratio_blocks(int q_cap);
void launch_ratio_matches(hipStream_t st, const int* idx, const float* dist, const int* qoff, int n_segments,
                          int q_cap, double ratio, const sift_keypoint* q_kpts, const sift_keypoint* t_kpts,
                          const int* toff, sift_match* matches, float* src_xy, float* dst_xy, int m_cap, int* moff,
                          int* blk_scan);
// cross_check.hip: the join of a forward ([q_cap][fwd_k]) and a reverse
// ([t_cap][rev_k], column 0 read) matcher result into the ratio stage's
// outputs; ratio 0 = cross-check only; blk_scan is [cross_blocks(q_cap) + 1]
// ints of scratch.
int cross_blocks(int q_cap);
void launch_cross_check(hipStream_t st, const int* idx, const float* dist, int fwd_k, const int* qoff, int n_segments,
                        int q_cap, const int* ridx, int rev_k, const int* toff, int t_cap, double ratio,
                        const sift_keypoint* q_kpts, const sift_keypoint* t_kpts, sift_match* matches, float* src_xy,
                        float* dst_xy, int m_cap, int* moff, int* blk_scan);
// join.hip: the segmented, ordered join of two record tables on a shared keypoint
// index (2-D / 3-D rows for sift_solve_pnp_segmented_device).  Both tables are
// walked in join_max_blocks(cap, n_segments) blocks of 256 rows that never span
// two segments.  Scratch: lookup [max(key_cap, 1)] uint64, a_tiles / b_tiles
// [n_segments + 1] ints, blk_scan [join_max_blocks(b_cap, n_segments) + 1] ints.
int join_max_blocks(int cap, int n_segments);
void launch_join_matches(hipStream_t st, const sift_match* a, const int* aoff, int a_cap, int a_side,
                         const unsigned char* a_mask, const double* a_xyz, const sift_match* b, const int* boff,
                         int b_cap, int b_side, const unsigned char* b_mask, const float* b_xy, const int* koff,
                         int key_cap, int n_segments, double* xyz_out, float* xy_out, int* a_row, int* b_row,
                         unsigned char* b_joined, int j_cap, int* joff, unsigned long long* lookup, int* a_tiles,
                         int* b_tiles, int* blk_scan);
// match_window.hip: the spatially gated segmented matcher.  launch_window_bin
// sorts the train keypoints of every grid (one per train segment, one in all
// for a shared train set) into the cells of an nx x ny grid of side
// 1 / inv_cell: cell_end is [n_grids][nx * ny + 1] ints (after the launch,
// entry c is the end of cell c's run, entry c - 1 its start), cell_rows /
// cell_xy [max(t_cap, 1)] the local train indices and positions in cell order,
// each grid's run starting at its train range's first row.
// launch_knn_window then scores, per query, the admissible rows of the cells
// its window touches.  The grid's shape is scratch.hpp's window_grid(); no
// result depends on it.
struct WindowArgs {
  int metric;  // SIFT_METRIC_*
  const void* q;
  const sift_keypoint* q_kpts;
  const int* qoff;
  int nseg, q_cap;
  const void* t;
  const sift_keypoint* t_kpts;
  const int* toff;  // nullptr: shared train
  int t_cap;
  const double* H;   // nullptr: the query position itself
  const int* found;  // nullptr: every H is used
  float radius;
  int nx, ny;
  float inv_cell;
  int* cell_end;
  int* cell_rows;
  float2* cell_xy;
  int k;
  int* idx;
  float* dist;
};
hipError_t launch_window_bin(hipStream_t st, const WindowArgs& A);
void launch_knn_window(hipStream_t st, const WindowArgs& A);
// match_epipolar.hip: the segmented matcher gated by the window around the
// query's own position and by the epipolar band of the segment's fundamental
// matrix.  W is the windowed matcher's argument block with the same binning
// (launch_window_bin) and W.H = F, [nseg][9] doubles as
// sift_find_fundamental_segmented_device writes them (nullptr: the window
// alone); limit is (float)(band * band), the estimate's own inlier limit.
struct EpipolarArgs {
  WindowArgs W;
  float limit;
};
void launch_knn_epipolar(hipStream_t st, const EpipolarArgs& A);
// pyramid_pc.hip (SIFT_FLAG_FAST): octave o's five planes by the separable
// form, plus octave o+1's plane 0 when pyramid_fuses_decimation(L, o + 1)
// (else decimate first), from a producer wave and three consumer waves
// synchronised by LDS counters; err = the context's sticky word err[3]
// (kErrStall).  fast_taps_match: the compiled-in 1-D taps equal
// fast_taps_host's for these sigmas; pyramid_fast_fits: every plane and the
// input rows below the kernel's dropped-offset range.
void launch_pyramid_pc(hipStream_t st, const Layout& L, int o, float* gpyr, Plane src, int batch, int* err,
                       bool stall_test = false);  // stall_test: the pc_stall_once test hook
bool pyramid_fuses_decimation(const Layout& L, int o);
bool fast_taps_match(float sigma_base, const float* sig);
bool pyramid_fast_fits(const Layout& L, long long src_row_stride);
// Work items of one separable-pyramid launch: n_full strip columns walked
// whole, then the rest in `chunks` row chunks of `chunk` rows.
struct FastPlan {
  int n_full, chunk, chunks;
};
FastPlan fast_plan(int columns, int rows, int slots, int halo);

// One image small enough that the per-keypoint kernels are latency-bound (a
// 1080p image: ~13 K candidates, a few waves per SIMD) runs their one-image
// variants (orient_bin_kernel, the descriptor budgeted for 2 waves per SIMD);
// a batch, or one image above kOneImagePx (an 8K image: 214 K keypoints),
// fills the chip with the batch variants.  SIFT_HIP_ONE_IMAGE_PX overrides the
// limit (A/B runs).
constexpr long long kOneImagePx = 4ll << 20;
bool one_image_variants(const Layout& L, int batch);  // orient.hip

// The detection stages: extrema.hip, scan.hip, refine.hip, orient.hip, emit.hip
// (what only they share is in detect_args.hpp)
struct DetectBufs {
  unsigned* mask;       // candidate bitmask, mask_words_per_image * batch
  int* blk_counts;      // per scan block
  int* cand_total;      // [1]
  int* img_cand_off;    // [batch+1]
  Cand* cands;
  int cand_cap;
  CandOut* couts;
  int* kp_scan;         // per candidate exclusive scan of npeaks, [cand_cap+1]
  int* kp_total;        // [1]
  int* npeaks;          // orientation peaks per candidate, [cand_cap]
  int* scan_tmp;        // exclusive scan of blk_counts, [blk_cap+1]
  int* scan_tiles;      // per-tile sums of the multi-block scan, [scan_tiles_for(max(blk_cap, cand_cap))]
  float* g4patch;       // sparse flow: plane 4 on the 3x3 around the slot's current (r, c), [9 * cand_cap]
  int* rstate;          // sparse flow: Newton iteration a slot waits at for its patch, or -1 (done), [cand_cap]
  int* g4wait;          // sparse flow: two lists of waiting slots, in any order, [2 * cand_cap] (g4_round_kernel);
                        //   the second, which round 1 is the first to write, holds the first fill's list until then
  int* g4stat;          // sparse flow: the call's counters below, [kG4Stats]; cleared at the head of every detection
  int* sel_hist;        // keypoint budget, multi-workgroup form: [max_batch][kSelectPasses][kSelectBins] weight histograms
};
constexpr int kG4StatFirst = 0;  // slots the first fill serves: the length of its list (g4_list_kernel)
constexpr int kG4StatWait = 1;   // [kMaxInterp]: slots waiting after the first step, after round 1, ...
constexpr int kG4StatFills = 6;  // most fills any waiting slot took (its first fill included)
constexpr int kG4Stats = 8;
static_assert(kG4StatWait + kMaxInterp <= kG4StatFills, "one waiting count per round");
// The sparse flow of SIFT_NCL's detection (exact mode, batches): bit o of
// `sparse` marks an octave whose plane 4 was not blurred.  There the extrema
// pass tests layer 2 against DoG 1 and DoG 2 only ("partial candidates"), and
// plane 4 is evaluated point by point -- the reference's 37 x 37 chain,
// g4_fill_kernel -- on the 3x3 around each candidate that sits on layer 2:
// once for the nine DoG 3 comparisons left out, then again whenever a Newton
// step moves a candidate on layer 2 (the waiting lists and g4_round_kernel;
// at most kMaxInterp fills per slot).
// coef4 is the context's table of sig[4] (37 x 37, row-major).  grid > 0
// bounds the fill's and the rounds' grids (SIFT_HIP_G4_GRID, a test hook: a
// multiple of 8; 0 = the resident grid).
struct SparseG4 {
  unsigned sparse;
  const float* coef4;
  int grid;
};
int scan_tiles_for(long long cap);  // scan.hip
// extrema.hip
long long mask_words_per_image(const Layout& L);
int mask_blocks_per_image(const Layout& L);
void launch_extrema(hipStream_t st, const Layout& L, const float* gpyr, float* dog, bool write_dog,
                    float2* grad, const MathConsts* mc, int batch, DetectBufs& D, unsigned sparse = 0);
void launch_grad(hipStream_t st, const Layout& L, const float* gpyr, float2* grad, int batch, int s_lo,
                 int s_hi, const MathConsts* mc);
// refine.hip (refinement, then orient.hip's launch_orient)
void launch_refine_orient(hipStream_t st, const Layout& L, const float* gpyr, const float2* grad,
                          const float* dog, const MathConsts* mc, DetectBufs& D, int batch,
                          SparseG4 sp = SparseG4{0, nullptr, 0});
// Test entry (sift_selftest_g4_points): plane 4's 3x3 patch around each of n
// points of a one-octave layout whose plane 0 holds the source; grid as in
// SparseG4.
void launch_g4_points(hipStream_t st, const Layout& L, const float* gpyr, const float* coef4, const Cand* pts, int n,
                      float* patch, int grid);
// emit.hip.
// half (sift_set_upsample: detection ran on the doubled image): every emitted
// keypoint has x, y and size multiplied by 0.5f and the low byte of its octave
// decremented (255 = octave -1) -- OpenCV's post-pass for firstOctave < 0.
void launch_emit(hipStream_t st, DetectBufs& D, int batch, sift_keypoint* kpts, int kp_cap,
                 int* img_kp_off, bool half = false);
// select.hip: the per-image keypoint budget (sift_set_max_features), between
// launch_refine_orient and launch_emit.  For every image of the batch whose
// keypoint count exceeds n_keep, npeaks becomes 0 in each candidate slot whose
// response is below the image's n_keep-th largest (counted once per keypoint;
// slots that tie with it stay).  grid_form: many workgroups per image and one
// launch per digit pass (one large image) instead of one workgroup per image.
constexpr int kSelectBins = 256, kSelectPasses = 4;
void launch_select_best(hipStream_t st, DetectBufs& D, int batch, int n_keep, bool grid_form);
// detmask.hip: the detection mask of the *_masked entry points
// (KeyPointsFilter::runByPixelsMask), between launch_select_best and
// launch_emit.  Not DetectBufs::mask, the candidate bitmask: this is the
// caller's rows x cols bytes per image, zero = no keypoint here.  Image b's
// bytes start at bytes + b * img_stride (0: one map for the whole batch), rows
// are row_stride bytes apart.  npeaks becomes 0 in every live slot whose
// emitted position rounds (x + 0.5f, y + 0.5f, truncated) to a zero byte or to
// a pixel outside the image.  bytes == nullptr: nothing is launched.
// grid_form: launch_select_best's split for one large image.
// half (sift_set_upsample): the slots hold positions in the doubled image, the
// mask is the original image's rows x cols: the position is multiplied by 0.5f
// first, as launch_emit(half) writes it.
struct DetMask {
  const unsigned char* bytes = nullptr;
  long long row_stride = 0, img_stride = 0;
};
void launch_detmask(hipStream_t st, DetectBufs& D, int batch, const DetMask& dm, int rows, int cols, bool grid_form,
                    bool half = false);
// Device status bits; bit i <-> sticky error word err[i] (DescArgs::err_flag = &err[0],
// emit.hip's status_kernel).
constexpr int kErrAssert = 1;      // keypoint octave/layer outside the pyramid (CV_Assert)
constexpr int kErrWorkspace = 2;   // candidate workspace overflow
constexpr int kErrKpCapacity = 4;  // keypoint total above the output capacity
constexpr int kErrStall = 8;       // a bounded in-kernel wait expired (pyramid_pc.hip); err[3]
void launch_status(hipStream_t st, const int* cand_total, int cand_cap, const int* img_off, int batch, int kp_cap,
                   int* err, int* stat);

// descriptor.hip
void launch_descriptors(hipStream_t st, const Layout& L, const float2* grad, const MathConsts* mc,
                        const sift_keypoint* kpts, const int* img_kp_off, int batch,
                        int kp_cap, float* desc, int first_octave, int* err_flag,
                        bool detected,  // detected: keypoints from this library's detection (radius <= 40)
                        int* perm);     // [kp_cap] scratch: the lane-balance ranking
// compute.hip (sift_compute_batch: descriptors at keypoints the caller holds).
// The prep pass over rows [clamp(off[0]), clamp(off[batch])) of kpts, every
// offset clamped to [0, kp_cap] (match_seg.hpp): with oi = octave -
// first_octave (0, or -1 when L is the doubled image's, sift_set_upsample), a
// row with oi < 0,
// oi >= L.n_oct, layer > 4 or layer > max_layer gets 128 zeros in desc and
// sets err_flag (kErrAssert); every other row goes into one of two index
// lists -- det: the rows descriptor_kernel's detected-keypoint form can take
// (window radius <= 40 and the keypoint's pixel inside the octave's interior),
// gen: the rest -- ranked by window size within each run of kComputeChunk
// consecutive rows, as desc_rank_kernel ranks.  det and gen hold kp_cap ints
// each; counts[0], counts[1] are their lengths (the launch clears them first).
// The order of the runs within a list varies from call to call; it affects
// speed only.
constexpr int kComputeChunk = 256;
struct DescLists {
  int* det;
  int* gen;
  int* counts;  // [2]
};
void launch_compute_prep(hipStream_t st, const Layout& L, const sift_keypoint* kpts, const int* off, int batch,
                         int kp_cap, int max_layer, float* desc, int* err_flag, const DescLists& lists,
                         int first_octave = 0);
// descriptor.hip: the two descriptor launches over those lists
void launch_descriptors_listed(hipStream_t st, const Layout& L, const float2* grad, const MathConsts* mc,
                               const sift_keypoint* kpts, const int* img_kp_off, int batch, int kp_cap, float* desc,
                               int* err_flag, const DescLists& lists, int first_octave = 0);
void launch_math_selftest(hipStream_t st, int op, const float* a, const float* b, float* out, int n,
                          const MathConsts* mc);

}  // namespace sift
