// match_u8.hip -- 8-bit descriptors and their brute-force L1 kNN matcher
// (k <= 2) for gfx950: the byte form of match.hip's segmented matcher.
//
// Quantiser: out = saturate_cast<uchar>(desc * 512.f), the byte form the
// reference leaves commented out beside its float descriptor (src/sift.cpp:720,
// SIFT_INT_DESCR_FCTR = 512): the float multiply (exact, a power of two),
// cvRound (ties to even), a clamp to 0..255 -- common.hpp's sat_u8.
//
// Distance: sum |a - b| over 128 unsigned bytes, an integer <= 128 * 255 =
// 32,640, exact in any summation order.  v_sad_u8 forms four element pairs per
// instruction: 32 per (query, train) pair where the float kernel issues 256.
//
// Order: for each query the two smallest (distance, train index) pairs in
// lexicographic order, as in match.hip.  Inside the scoring loop a candidate is
// the one 32-bit key (distance << 17) | (row - first row of the split): the
// distance takes 15 bits, a split holds at most 2^17 rows (knn_u8_seg_splits
// sees to it), keys are distinct, and their unsigned order is the
// lexicographic order -- the top-2 update is min / max / min.  The four waves'
// lists and the splits' lists merge with the explicit (distance, index)
// comparison.
//
// Layout: a workgroup owns 64 x kU8Q queries (kU8Q per lane, 32 VGPRs each)
// and one split of the segment's train rows; wave w scores rows w, w + 4, ...
// of the split.  A train row is the same for every lane of a wave: it is read
// once for the lane's kU8Q queries, either by scalar loads into SGPRs (v_sad_u8
// takes the scalar operand; no LDS and no barrier in the loop) or, the A/B
// alternative kept for tools/bench_match_u8.py (SIFT_HIP_U8_ROUTE=lds), from
// 64-row chunks staged in LDS with broadcast ds_read_b128.  DESIGN.md §6c.
#include "common.hpp"
#include "match_seg.hpp"

#include <stdlib.h>
#include <string.h>

namespace sift {

namespace {

constexpr int kU8Q = 4;                // queries per lane
constexpr int kU8Tile = 64 * kU8Q;     // queries per workgroup
constexpr int kU8TC = 64;              // train rows per split granule (and per LDS chunk)
constexpr int kRowW = kDescLen / 4;    // dwords per row
constexpr int kRowV = kDescLen / 16;   // uint4 per row
constexpr int kIdxBits = 17;           // row bits of a key
constexpr int kSplitRowsMax = 1 << kIdxBits;
constexpr unsigned kEmptyKey = 0xffffffffu;  // distance field 32767 > 32640: above every real key

// ---- quantiser -----------------------------------------------------------------
__device__ __forceinline__ unsigned quant4(float4 v) {
  const unsigned a = (unsigned)sat_u8(v.x * 512.f), b = (unsigned)sat_u8(v.y * 512.f);
  const unsigned c = (unsigned)sat_u8(v.z * 512.f), d = (unsigned)sat_u8(v.w * 512.f);
  return a | (b << 8) | (c << 16) | (d << 24);
}

// One lane per 16 elements: four 16-byte loads, one 16-byte store.  Rows at or
// past min(*n_rows, row_cap) are not written.
__global__ __launch_bounds__(256) void desc_to_u8_kernel(const float4* __restrict__ src,
                                                         const int* __restrict__ n_rows, int row_cap,
                                                         uint4* __restrict__ dst) {
  const int rows = n_rows ? clamp_row(*n_rows, row_cap) : row_cap;
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;  // 16-element group
  if (g >= (long long)rows * kRowV) return;
  const float4* s = src + g * 4;
  uint4 o;
  o.x = quant4(s[0]);
  o.y = quant4(s[1]);
  o.z = quant4(s[2]);
  o.w = quant4(s[3]);
  dst[g] = o;
}

// ---- matcher -------------------------------------------------------------------
using BestI = Top2<int>;  // match_seg.hpp: the decoded list, its order, insert() and write_knn()

__device__ __forceinline__ void decode(unsigned key, int base, int& d, int& i) {
  const bool empty = key == kEmptyKey;
  d = empty ? kEmptyDist<int> : (int)(key >> kIdxBits);
  i = empty ? -1 : (int)(key & (kSplitRowsMax - 1)) + base;
}

struct U8Args {
  const uint8_t* q;
  const int* qoff;
  int nseg, q_cap;
  const uint8_t* t;
  const int* toff;  // nullptr: shared train
  int t_cap;
  const int* tile_start;
  int splits, k;
  int2* part_d;
  int2* part_i;
  int* idx;
  float* dist;
};

// One train row (32 dwords, the same for every lane) against the lane's kU8Q
// queries, then the top-2 update of each by key.
template <typename Row>
__device__ __forceinline__ void score_row(const Row& tr, const unsigned (&qv)[kU8Q][kRowW], int j,
                                          unsigned (&k1)[kU8Q], unsigned (&k2)[kU8Q]) {
  unsigned acc[kU8Q];
#pragma unroll
  for (int s = 0; s < kU8Q; ++s) acc[s] = 0;
#pragma unroll
  for (int w = 0; w < kRowW; ++w) {
    const unsigned tw = tr[w];
#pragma unroll
    for (int s = 0; s < kU8Q; ++s) acc[s] = __builtin_amdgcn_sad_u8(qv[s][w], tw, acc[s]);
  }
#pragma unroll
  for (int s = 0; s < kU8Q; ++s) {
    const unsigned key = (acc[s] << kIdxBits) | (unsigned)j;
    const unsigned hi = key > k1[s] ? key : k1[s];
    k2[s] = hi < k2[s] ? hi : k2[s];
    k1[s] = key < k1[s] ? key : k1[s];
  }
}

// The grid is sized from the capacities as in knn_l1_seg_kernel: grid.x covers
// the most tiles they allow and workgroups past tile_start[nseg] exit; grid.y
// splits every segment's own train range evenly.  Indices are local to the
// train range.  splits == 1 writes idx / dist directly.
template <bool kScalar>
__global__ __launch_bounds__(256) void knn_l1_u8_seg_kernel(U8Args A) {
  __shared__ int md[3][2][kU8Tile];
  __shared__ int mi[3][2][kU8Tile];
  __shared__ uint4 tl[kScalar ? 1 : kU8TC * kRowV];  // 8 KB on the LDS route
  const int tile = blockIdx.x;
  if (tile >= A.tile_start[A.nseg]) return;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = seg_of(A.tile_start, A.nseg, 0x7fffffff, tile);
  const int qe = clamp_row(A.qoff[b + 1], A.q_cap);
  const int q0 = clamp_row(A.qoff[b], A.q_cap) + (tile - A.tile_start[b]) * kU8Tile + lane;  // < qe for lane 0
  int ts = 0, te = A.t_cap;  // train_range() of match_seg.hpp, restated (profiles/match_refactor_isa.txt)
  if (A.toff) {
    ts = clamp_row(A.toff[b], A.t_cap);
    te = clamp_row(A.toff[b + 1], A.t_cap);
    te = te < ts ? ts : te;
  }
  const int per = (((te - ts) + A.splits - 1) / A.splits + kU8TC - 1) / kU8TC * kU8TC;  // <= kSplitRowsMax
  const long long t0l = ts + (long long)blockIdx.y * per;
  int t0 = t0l < te ? (int)t0l : te, t1 = (te - t0) < per ? te : t0 + per;
  t0 = __builtin_amdgcn_readfirstlane(t0);
  t1 = __builtin_amdgcn_readfirstlane(t1);
  unsigned qv[kU8Q][kRowW];
#pragma unroll
  for (int s = 0; s < kU8Q; ++s) {  // slot s: query q0 + 64 s (the last live row stands in past the segment)
    const uint4* qp = reinterpret_cast<const uint4*>(A.q + (long long)min(q0 + 64 * s, qe - 1) * kDescLen);
#pragma unroll
    for (int v = 0; v < kRowV; ++v) {
      const uint4 x = qp[v];
      qv[s][4 * v] = x.x;
      qv[s][4 * v + 1] = x.y;
      qv[s][4 * v + 2] = x.z;
      qv[s][4 * v + 3] = x.w;
    }
  }
  unsigned k1[kU8Q], k2[kU8Q];
#pragma unroll
  for (int s = 0; s < kU8Q; ++s) k1[s] = k2[s] = kEmptyKey;
  if (kScalar) {
    // uniform and never written while the kernel runs: read through the constant
    // address space, i.e. by scalar loads; the next row is requested before the
    // current one is scored
    typedef const __attribute__((address_space(4))) unsigned* RowPtr;
    int r = t0 + wv;
    if (r < t1) {
      unsigned cur[kRowW];
      {
        RowPtr p = (RowPtr)(A.t + (long long)r * kDescLen);
#pragma unroll
        for (int w = 0; w < kRowW; ++w) cur[w] = p[w];
        asm volatile("" ::"s"(cur[0]));  // the first row's wait stays out of the loop, where it would take the next row's too
      }
      for (; r < t1; r += 4) {
        unsigned nxt[kRowW];
        RowPtr p = (RowPtr)(A.t + (long long)(r + 4 < t1 ? r + 4 : r) * kDescLen);
#pragma unroll
        for (int w = 0; w < kRowW; ++w) nxt[w] = p[w];
        __builtin_amdgcn_sched_barrier(0);  // the request stays ahead of the scoring
        score_row(cur, qv, r - t0, k1, k2);
#pragma unroll
        for (int w = 0; w < kRowW; ++w) cur[w] = nxt[w];
      }
    }
  } else {
    for (int c0 = t0; c0 < t1; c0 += kU8TC) {
      const int nrow = min(kU8TC, t1 - c0);
      __syncthreads();
      const uint4* src = reinterpret_cast<const uint4*>(A.t + (long long)c0 * kDescLen);
      for (int u = threadIdx.x; u < nrow * kRowV; u += 256) tl[u] = src[u];
      __syncthreads();
      for (int r = wv; r < nrow; r += 4) {
        const unsigned* tr = reinterpret_cast<const unsigned*>(tl + r * kRowV);
        score_row(tr, qv, c0 + r - t0, k1, k2);
      }
    }
  }
  BestI best[kU8Q];
#pragma unroll
  for (int s = 0; s < kU8Q; ++s) {
    decode(k1[s], t0 - ts, best[s].d1, best[s].i1);
    decode(k2[s], t0 - ts, best[s].d2, best[s].i2);
  }
  if (wv > 0) {
#pragma unroll
    for (int s = 0; s < kU8Q; ++s) {
      md[wv - 1][0][64 * s + lane] = best[s].d1;
      md[wv - 1][1][64 * s + lane] = best[s].d2;
      mi[wv - 1][0][64 * s + lane] = best[s].i1;
      mi[wv - 1][1][64 * s + lane] = best[s].i2;
    }
  }
  __syncthreads();
  if (wv != 0) return;
#pragma unroll
  for (int s = 0; s < kU8Q; ++s) {
    const int qi = q0 + 64 * s;
    if (qi >= qe) continue;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      insert(best[s], md[w][0][64 * s + lane], mi[w][0][64 * s + lane]);
      insert(best[s], md[w][1][64 * s + lane], mi[w][1][64 * s + lane]);
    }
    if (A.splits == 1) {
      write_knn(best[s], qi, A.k, A.idx, A.dist);
    } else {
      const long long o = (long long)blockIdx.y * A.q_cap + qi;
      A.part_d[o] = make_int2(best[s].d1, best[s].d2);
      A.part_i[o] = make_int2(best[s].i1, best[s].i2);
    }
  }
}

__global__ void set_offsets_kernel(int* __restrict__ off, int a, int b) {
  off[0] = a;
  off[1] = b;
}

// SIFT_HIP_U8_ROUTE=lds: the staged-chunk kernel instead of the scalar-load one (A/B runs;
// read at every call, so that one process can alternate the two)
bool lds_route() {
  const char* e = getenv("SIFT_HIP_U8_ROUTE");
  return e && !strcmp(e, "lds");
}

}  // namespace

void launch_desc_to_u8(hipStream_t st, const float* desc, const int* n_rows, int row_cap, uint8_t* out) {
  if (row_cap <= 0) return;
  const long long groups = (long long)row_cap * kRowV;
  hipLaunchKernelGGL(desc_to_u8_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const float4*>(desc), n_rows, row_cap, reinterpret_cast<uint4*>(out));
}

int knn_u8_seg_max_tiles(int q_cap, int n_segments) { return q_cap / kU8Tile + n_segments; }

int knn_u8_seg_splits(int q_cap, int n_segments, int t_cap, bool seg_train) {
  const int gx = knn_u8_seg_max_tiles(q_cap, n_segments);
  int s = (2048 + gx - 1) / gx;  // ~2k workgroups to fill 256 CUs
  // segmented train: an even share of the buffer stands in for the segment size
  const int nt = seg_train ? (t_cap + n_segments - 1) / n_segments : t_cap;
  const int max_s = (nt + kU8TC - 1) / kU8TC;  // at least one granule per split
  s = s < max_s ? s : max_s;
  // a key numbers the rows of a split with kIdxBits bits, whatever the offsets turn out to be
  const int min_s = (t_cap + kSplitRowsMax - 1) / kSplitRowsMax;
  s = s > min_s ? s : min_s;
  return s < 1 ? 1 : s;
}

void launch_knn_l1_u8_seg(hipStream_t st, const uint8_t* q, const int* qoff, int n_segments, int q_cap,
                          const uint8_t* t, const int* toff, int t_cap, int k, int splits, int* tile_start,
                          int2* part_d, int2* part_i, int* idx, float* dist) {
  hipLaunchKernelGGL(seg_tiles_kernel<kU8Tile>, dim3(1), dim3(256), 0, st, qoff, n_segments, q_cap, tile_start);
  const U8Args A{q, qoff, n_segments, q_cap, t, toff, t_cap, tile_start, splits, k, part_d, part_i, idx, dist};
  dim3 grid(knn_u8_seg_max_tiles(q_cap, n_segments), splits);
  if (lds_route())
    hipLaunchKernelGGL(knn_l1_u8_seg_kernel<false>, grid, dim3(256), 0, st, A);
  else
    hipLaunchKernelGGL(knn_l1_u8_seg_kernel<true>, grid, dim3(256), 0, st, A);
  if (splits > 1)
    hipLaunchKernelGGL(knn_seg_merge_kernel<int2>, dim3((q_cap + 255) / 256), dim3(256), 0, st, part_d, part_i, qoff,
                       n_segments, q_cap, splits, k, idx, dist);
}

void launch_set_offsets(hipStream_t st, int* off, int a, int b) {
  hipLaunchKernelGGL(set_offsets_kernel, dim3(1), dim3(1), 0, st, off, a, b);
}

}  // namespace sift
