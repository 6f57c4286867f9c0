// pose_batch.hip -- recoverPose and triangulatePoints for every segment of the
// ratio stage's point pairs, on the device in stream order.  The
// result equals recover_pose / triangulate_points (pose.hip) run per segment bit
// for bit: every expression comes from pose_math.hpp, and the only value that
// crosses lanes is an integer count of good rows, so no order of reduction can
// move a bit.
//
// recover_pose_kernel: one workgroup of kPoseThreads lanes per segment, the shape
// of fund_ransac_kernel.  Lane 0 decomposes the segment's F (two 3x3 inverses, a
// 3x3 Jacobi: a few hundred double operations) into LDS; then, candidate by
// candidate, the rows are strided over the lanes, each lane triangulates its rows
// under that candidate (a 4x4 Jacobi, A^T A and V in registers) and counts the
// good ones; the count goes through a wave reduction and one LDS atomic per wave.
// A second pass over the rows takes the winner's solve again and writes the mask
// and the points.  No scratch, no host value.
//
// triangulate_kernel: a (chunk of rows, segment) grid, one DLT solve per thread,
// four doubles stored.  A segment's chunks past its end leave at once; segments
// may overlap or run backwards, so a row's segment is never searched for.
#include "common.hpp"
#include "pose_math.hpp"

namespace sift {

namespace {

using namespace pmath;

constexpr int kPoseThreads = 256;
static_assert(kPoseThreads % 64 == 0 && kPoseThreads <= 1024, "whole waves");

__device__ inline int clamp_off(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

__global__ __launch_bounds__(kPoseThreads) void recover_pose_kernel(
    const float* __restrict__ src_xy, const float* __restrict__ dst_xy, const int* __restrict__ moff, int m_cap,
    const double* __restrict__ F, const int* __restrict__ found, const double* __restrict__ K_src,
    const double* __restrict__ K_dst, int k_stride, const unsigned char* __restrict__ mask_in, double thresh,
    double* __restrict__ pose, double* __restrict__ E, int* __restrict__ pose_found, int* __restrict__ n_good,
    unsigned char* __restrict__ mask_out, double* __restrict__ xyz) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lo = clamp_off(moff[b], m_cap), hi = clamp_off(moff[b + 1], m_cap);
  const int n = hi > lo ? hi - lo : 0;
  const P2* s = reinterpret_cast<const P2*>(src_xy) + lo;
  const P2* d = reinterpret_cast<const P2*>(dst_xy) + lo;
  const unsigned char* on = mask_in ? mask_in + lo : nullptr;

  __shared__ Decomp s_D;
  __shared__ int s_ok, s_cnt[kCandidates];

  if (tid == 0)
    s_ok = thresh_ok(thresh) && found[b] != 0 &&
           decompose(F + (size_t)b * 9, K_src + (size_t)b * k_stride, K_dst + (size_t)b * k_stride, s_D);
  if (tid < kCandidates) s_cnt[tid] = 0;
  __syncthreads();
  bool has = s_ok;  // uniform
  int w = 0, most = 0;
  if (has) {
#pragma unroll 1
    for (int c = 0; c < kCandidates; ++c) {
      double P[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) P[k] = s_D.P[c][k];
      int good = 0;
      for (int i = tid; i < n; i += kPoseThreads) {
        double q[3];
        if (on && !on[i]) continue;
        good += good_point(s_D, P, s[i], d[i], thresh, q);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) good += __shfl_down(good, off, 64);
      if ((tid & 63) == 0 && good) atomicAdd(&s_cnt[c], good);
    }
    __syncthreads();
    int count[kCandidates];
#pragma unroll
    for (int c = 0; c < kCandidates; ++c) count[c] = s_cnt[c];
    w = winner(count);
    most = s_cnt[w];
    has = most >= 1;
  }
  if (tid < 12) pose[(size_t)b * 12 + tid] = has ? s_D.P[w][tid] : 0;
  if (E && tid < 9) E[(size_t)b * 9 + tid] = has ? s_D.E[tid] : 0;
  if (tid == 0) {
    pose_found[b] = has;
    n_good[b] = has ? most : 0;
  }
  if (!mask_out && !xyz) return;
  double P[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = has ? s_D.P[w][k] : 0;
  for (int i = tid; i < n; i += kPoseThreads) {
    double q[3] = {0, 0, 0};
    bool good = has && !(on && !on[i]);
    if (good) good = good_point(s_D, P, s[i], d[i], thresh, q);
    if (mask_out) mask_out[lo + i] = good;
    if (xyz) {
#pragma unroll
      for (int k = 0; k < 3; ++k) xyz[(size_t)(lo + i) * 3 + k] = good ? q[k] : 0;
    }
  }
}

__global__ __launch_bounds__(kPoseThreads) void triangulate_kernel(
    const float* __restrict__ src_xy, const float* __restrict__ dst_xy, const int* __restrict__ moff, int n_segments,
    int m_cap, const double* __restrict__ P_src, const double* __restrict__ P_dst, double* __restrict__ xyzw) {
  const P2* s = reinterpret_cast<const P2*>(src_xy);
  const P2* d = reinterpret_cast<const P2*>(dst_xy);
  for (int b = blockIdx.y; b < n_segments; b += gridDim.y) {
    const int lo = clamp_off(moff[b], m_cap), hi = clamp_off(moff[b + 1], m_cap);
    const long long i = (long long)lo + (long long)blockIdx.x * kPoseThreads + threadIdx.x;
    if (i >= hi) continue;
    double Ps[12], Pd[12], Q[4];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      Ps[k] = P_src[(size_t)b * 12 + k];
      Pd[k] = P_dst[(size_t)b * 12 + k];
    }
    triangulate(Ps, Pd, s[i].x, s[i].y, d[i].x, d[i].y, Q);
#pragma unroll
    for (int k = 0; k < 4; ++k) xyzw[(size_t)i * 4 + k] = Q[k];
  }
}

}  // namespace

void launch_recover_pose_seg(hipStream_t st, const float* src_xy, const float* dst_xy, const int* moff, int n_segments,
                             int m_cap, const double* F, const int* found, const double* K_src, const double* K_dst,
                             int k_per_segment, const unsigned char* mask_in, double distance_thresh, double* pose,
                             double* E, int* pose_found, int* n_good, unsigned char* mask_out, double* xyz) {
  recover_pose_kernel<<<n_segments, kPoseThreads, 0, st>>>(src_xy, dst_xy, moff, m_cap, F, found, K_src, K_dst,
                                                           k_per_segment ? 9 : 0, mask_in, distance_thresh, pose, E,
                                                           pose_found, n_good, mask_out, xyz);
}

void launch_triangulate_seg(hipStream_t st, const float* src_xy, const float* dst_xy, const int* moff, int n_segments,
                            int m_cap, const double* P_src, const double* P_dst, double* xyzw) {
  const dim3 grid((unsigned)(((long long)m_cap + kPoseThreads - 1) / kPoseThreads),
                  (unsigned)(n_segments < 65535 ? n_segments : 65535));
  triangulate_kernel<<<grid, kPoseThreads, 0, st>>>(src_xy, dst_xy, moff, n_segments, m_cap, P_src, P_dst, xyzw);
}

}  // namespace sift
