// match_window.hpp -- what the two gated matchers share (match_window.hip: a
// square window around a predicted position; match_epipolar.hip: that window
// and the band of a fundamental matrix's epipolar lines): the lane group, the
// monotone cell function of the search grid with its range slack, and the three
// metrics' scorers, whose distances are the dense matchers' own bit for bit.
// The binning itself (launch_window_bin) lives in match_window.hip and is
// declared in common.hpp.  Device code; every translation unit instantiates its
// own copy (anonymous namespace, no relocatable device code), like match_seg.hpp.
#pragma once

#include "common.hpp"
#include "match_seg.hpp"

namespace sift {

namespace {

constexpr int kWinGroup = 8;                      // lanes per query
constexpr int kWinBlock = 256;                    // lanes per workgroup
constexpr int kWinQueries = kWinBlock / kWinGroup;  // queries per workgroup
constexpr float kWinSlack = 1.f / 4194304.f;      // 2^-22, see match_window.hip's file comment
static_assert(kDescLen == 16 * kWinGroup, "lane k owns elements 8g + k (floats) or bytes [16k, 16k + 16)");

using Best2 = Top2<float>;  // match_seg.hpp: every metric's distance is a float here, in the dense matchers' order

// Monotone non-decreasing in v; NaN gives 0.
__device__ __forceinline__ int cell_of(float v, float inv_cell, int n) {
  const float f = floorf(v * inv_cell);
  return (int)fminf(fmaxf(f, 0.f), (float)(n - 1));
}
__device__ __forceinline__ int cell_lo(float v, float inv_cell, int n) { return cell_of(v, inv_cell, n); }
__device__ __forceinline__ int cell_hi(float v, float inv_cell, int n) {
  return v != v ? n - 1 : cell_of(v, inv_cell, n);
}

// ---- distances -----------------------------------------------------------------
// What lane `sub` of a group keeps of its query row, and the distance of that
// row to train row `row`, the same bits in all eight lanes.
template <int kMetric>
struct Metric;

template <>
struct Metric<SIFT_METRIC_L1_F32> {
  float q[16];
  __device__ __forceinline__ void load(const void* base, long long row, int sub) {
    const float* p = static_cast<const float*>(base) + row * kDescLen + sub;
#pragma unroll
    for (int g = 0; g < 16; ++g) q[g] = p[8 * g];
  }
  __device__ __forceinline__ float score(const void* base, long long row, int sub) const {
    const float* p = static_cast<const float*>(base) + row * kDescLen + sub;
    float a[16];
#pragma unroll
    for (int g = 0; g < 16; ++g) a[g] = p[8 * g];
    float s = 0.f;  // p[sub] of l1_row
#pragma unroll
    for (int g = 0; g < 16; ++g) s = s + fabsf(q[g] - a[g]);
    s = s + __shfl_xor(s, 4);     // q[k & 3] = p[k] + p[k ^ 4]
    s = s + __shfl_xor(s, 1);     // q0 + q1 | q2 + q3
    return s + __shfl_xor(s, 2);  // (q0 + q1) + (q2 + q3); float addition commutes, so every lane holds these bits
  }
};

__device__ __forceinline__ unsigned group_sum(unsigned s) {
  s += __shfl_xor(s, 4);
  s += __shfl_xor(s, 1);
  return s + __shfl_xor(s, 2);
}

template <>
struct Metric<SIFT_METRIC_L1_U8> {
  uint4 q;
  __device__ __forceinline__ void load(const void* base, long long row, int sub) {
    q = reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(base) + row * kDescLen)[sub];
  }
  __device__ __forceinline__ float score(const void* base, long long row, int sub) const {
    const uint4 a = reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(base) + row * kDescLen)[sub];
    unsigned s = __builtin_amdgcn_sad_u8(q.x, a.x, 0u);
    s = __builtin_amdgcn_sad_u8(q.y, a.y, s);
    s = __builtin_amdgcn_sad_u8(q.z, a.z, s);
    s = __builtin_amdgcn_sad_u8(q.w, a.w, s);
    return (float)group_sum(s);  // <= 32,640: exact
  }
};

// sum of the four byte products of two dwords
__device__ __forceinline__ unsigned dot4(unsigned a, unsigned b, unsigned acc) {
#if __has_builtin(__builtin_amdgcn_udot4)
  return __builtin_amdgcn_udot4(a, b, acc, false);
#else
  return acc + (a & 0xff) * (b & 0xff) + ((a >> 8) & 0xff) * ((b >> 8) & 0xff) +
         ((a >> 16) & 0xff) * ((b >> 16) & 0xff) + (a >> 24) * (b >> 24);
#endif
}

template <>
struct Metric<SIFT_METRIC_L2SQR_U8> {
  uint4 q;
  unsigned qq;  // sum of the squares of the lane's 16 query bytes
  __device__ __forceinline__ void load(const void* base, long long row, int sub) {
    q = reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(base) + row * kDescLen)[sub];
    qq = dot4(q.w, q.w, dot4(q.z, q.z, dot4(q.y, q.y, dot4(q.x, q.x, 0u))));
  }
  // sum (q - a)^2 = sum q^2 + sum a^2 - 2 sum q a over the lane's bytes: each term
  // <= 16 * 255^2, the difference is the non-negative sum of squares itself
  __device__ __forceinline__ float score(const void* base, long long row, int sub) const {
    const uint4 a = reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(base) + row * kDescLen)[sub];
    const unsigned aa = dot4(a.w, a.w, dot4(a.z, a.z, dot4(a.y, a.y, dot4(a.x, a.x, 0u))));
    const unsigned qa = dot4(q.w, a.w, dot4(q.z, a.z, dot4(q.y, a.y, dot4(q.x, a.x, 0u))));
    return (float)group_sum(qq + aa - 2u * qa);  // <= 8,323,200 < 2^24: exact
  }
};

}  // namespace

}  // namespace sift
