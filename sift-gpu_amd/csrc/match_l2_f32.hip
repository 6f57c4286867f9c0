// match_l2_f32.hip -- brute-force squared-L2 kNN matcher (k <= 2) on float
// descriptors for gfx950, with the products on the f32 matrix pipe
// (v_mfma_f32_32x32x2_f32).  Same contract as match.hip's segmented L1 matcher.
//
// The rule (include/sift_hip.h): with pi the element order below and
//   chain(x, y) = fmaf(x[pi127], y[pi127], ... fmaf(x[pi0], y[pi0], 0.0f)),
//   d = fmaf(-2.0f, chain(q, t), chain(q, q) + chain(t, t)),  d < 0 ? 0 : d.
// The f32 MFMA is bit for bit a k-ordered fmaf chain with one rounding per
// product, so the accumulator of a 32 x 32 tile after its 64 steps IS chain(q,
// t); the norms come from one pre-kernel that walks the same order with explicit
// fmaf.  Every (q, t) distance is formed inside one tile over all 128 elements,
// from a zero accumulator, so splits, waves and the place of a tile never change
// a value.
//
// pi: a lane loads 16 bytes at a time.  Step s = 4 c + j of the 64 MFMA steps
// takes k = 0 from the lower half-wave (h = 0) and k = 1 from the upper one, and
// lane (r, h) supplies float j of its c-th load, elements [8 c + 4 h, +4) of row
// r.  So position 2 s + h of the chain is element 8 c + 4 h + j:
//   pi = 0 4 1 5 2 6 3 7, 8 12 9 13 10 14 11 15, ..., 120 124 121 125 122 126 123 127
// Both operands and the norms use it.
//
// Tile: D = A.B with A = 32 train rows, B = 32 queries, the byte kernel's
// accumulator mapping: the query on the lane (col = lane & 31), the train rows in
// its 16 registers (row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)), so a lane's
// running Top2<float> belongs to one query and the two half-waves hold different
// train rows of it.
//
// Layout: a workgroup owns kTileQ = 256 queries and one split of the segment's
// train rows.  Each of its four waves holds the B fragments of 64 queries of its
// own in registers for the whole kernel (2 blocks x 64 VGPRs) and scores them
// against every 64-row train step (2 tiles), four independent accumulators (2 x
// 2 tiles of 32 x 32).  The train step is shared by the four waves through LDS:
// 64 rows x 512 bytes, read back as A fragments with 16-byte reads, the 16-byte
// chunks of a row XOR-swizzled by the row so that the 16 lanes of a read phase
// hit 16 different bank groups.  Two buffers: the next step is requested from
// global memory before the current one is scored and written behind it, one
// barrier per step.  The waves own different queries, so only the half-waves
// merge (one lane exchange); the splits merge with knn_seg_merge_kernel<float2>.
// DESIGN.md §6m.
#include "common.hpp"
#include "match_seg.hpp"

namespace sift {

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kQB = 2;                     // 32-query blocks per wave
constexpr int kTileQ = 4 * 32 * kQB;       // queries per workgroup
constexpr int kTT = 2;                     // 32-row train tiles per step
constexpr int kStep = 32 * kTT;            // train rows per step: the split granule
constexpr int kNormPad = kL2F32NormPad;    // t_norm entries past t_cap a tail step may read (masked)
static_assert(kNormPad >= kStep, "a tail step reads the norms of a whole step");
static_assert(kDescLen == 128, "pi and the 64 MFMA steps are written for 128 elements");
constexpr int kRowChunks = kDescLen / 4;   // 16-byte chunks of a row

// ---- norms ---------------------------------------------------------------------
// chain(x, x) in pi's order, explicit fmaf.  One lane per row: rows [0, q_cap)
// of q inside the live range [clamp(qoff[0]), clamp(qoff[nseg])), every row of t,
// and zeros for the kNormPad entries after them.
__device__ __forceinline__ float norm_chain(const uint4* __restrict__ row) {
  float n = 0.f;
#pragma unroll 4
  for (int c = 0; c < kRowChunks / 2; ++c) {
    const uint4 u = row[2 * c], v = row[2 * c + 1];
    const float a[4] = {__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w)};
    const float b[4] = {__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w)};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      n = __builtin_fmaf(a[j], a[j], n);
      n = __builtin_fmaf(b[j], b[j], n);
    }
  }
  return n;
}

__global__ __launch_bounds__(256) void l2_f32_norms_kernel(const uint4* __restrict__ q, const int* __restrict__ qoff,
                                                           int nseg, int q_cap, const uint4* __restrict__ t, int t_cap,
                                                           float* __restrict__ q_norm, float* __restrict__ t_norm) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row < q_cap) {
    if (row >= clamp_row(qoff[0], q_cap) && row < clamp_row(qoff[nseg], q_cap))
      q_norm[row] = norm_chain(q + row * kRowChunks);
    return;
  }
  const long long r = row - q_cap;
  if (r < t_cap)
    t_norm[r] = norm_chain(t + r * kRowChunks);
  else if (r < (long long)t_cap + kNormPad)
    t_norm[r] = 0.f;
}

// ---- matcher -------------------------------------------------------------------
using BestF = Top2<float>;  // match_seg.hpp: the list, its order, insert() and write_knn()

struct L2F32Args {
  const float* q;
  const int* qoff;
  int nseg, q_cap;
  const float* t;
  const int* toff;  // nullptr: shared train
  int t_cap;
  const int* tile_start;
  const float* q_norm;
  const float* t_norm;  // t_cap + kNormPad entries
  int splits, k;
  float2* part_d;
  int2* part_i;
  int* idx;
  float* dist;
};

// The train rows an accumulator register holds, less the lane's 4 h.
__device__ __forceinline__ constexpr int reg_row(int g) { return (g & 3) + 8 * (g >> 2); }

// Chunk u of row r of a step lives at chunk u ^ (r & 15) of the row's 32.
__device__ __forceinline__ int lds_chunk(int r, int u) { return r * kRowChunks + (u ^ (r & 15)); }

constexpr int kStepChunks = kStep * kRowChunks;   // 2048 16-byte chunks per step
constexpr int kLoads = kStepChunks / 256;         // per thread

// Rows [r0, r0 + kStep) of the split, which ends at t1 > r0: thread i takes
// chunks i, i + 256, ... (a row is 32 consecutive chunks).  A row at or past t1
// reads row t1 - 1 instead; its distances are masked.
__device__ __forceinline__ void fetch_step(const float* __restrict__ t, int r0, int t1, int tid, uint4 (&x)[kLoads]) {
#pragma unroll
  for (int i = 0; i < kLoads; ++i) {
    const int ch = tid + 256 * i, r = min(r0 + ch / kRowChunks, t1 - 1);
    x[i] = reinterpret_cast<const uint4*>(t + (long long)r * kDescLen)[ch % kRowChunks];
  }
}

__device__ __forceinline__ void stash_step(uint4* __restrict__ buf, int tid, const uint4 (&x)[kLoads]) {
#pragma unroll
  for (int i = 0; i < kLoads; ++i) {
    const int ch = tid + 256 * i;
    buf[lds_chunk(ch / kRowChunks, ch % kRowChunks)] = x[i];
  }
}

// One train step against the wave's kQB query blocks.  loc: row r0 less the
// range's start; nvalid: rows of the step inside the split (used by kTail).
template <bool kTail>
__device__ __forceinline__ void score_step(const uint4* __restrict__ buf, const float* __restrict__ tn,
                                           const float (&qf)[kQB][64], const float (&qn)[kQB], int loc, int nvalid,
                                           int lane, BestF (&best)[kQB]) {
  const int col = lane & 31, h = lane >> 5;
  float nt[kTT][16];  // chain(t, t) of the rows of the lane's accumulator registers
#pragma unroll
  for (int u = 0; u < kTT; ++u)
#pragma unroll
    for (int g = 0; g < 16; ++g) nt[u][g] = tn[32 * u + 4 * h + reg_row(g)];
  v16f acc[kQB][kTT];
#pragma unroll
  for (int b = 0; b < kQB; ++b)
#pragma unroll
    for (int u = 0; u < kTT; ++u) acc[b][u] = v16f{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int c = 0; c < kRowChunks / 2; ++c) {
    float a[kTT][4];
#pragma unroll
    for (int u = 0; u < kTT; ++u) {
      const uint4 x = buf[lds_chunk(32 * u + col, 2 * c + h)];
      a[u][0] = __uint_as_float(x.x);
      a[u][1] = __uint_as_float(x.y);
      a[u][2] = __uint_as_float(x.z);
      a[u][3] = __uint_as_float(x.w);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < kQB; ++b)
#pragma unroll
        for (int u = 0; u < kTT; ++u)
          acc[b][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][j], qf[b][4 * c + j], acc[b][u], 0, 0, 0);
  }
#pragma unroll
  for (int b = 0; b < kQB; ++b)
#pragma unroll
    for (int u = 0; u < kTT; ++u)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        const int row = 32 * u + 4 * h + reg_row(g);
        const float s = qn[b] + nt[u][g];
        float d = __builtin_fmaf(-2.0f, acc[b][u][g], s);
        d = d < 0.f ? 0.f : d;  // keeps NaN
        if (kTail) d = row < nvalid ? d : INFINITY;  // never a neighbour
        insert(best[b], d, loc + row);
      }
}

// The grid is sized from the capacities as in the other segmented matchers:
// grid.x covers the most tiles they allow and workgroups past tile_start[nseg]
// exit; grid.y splits every segment's own train range evenly, in granules of
// kStep rows.  Indices are local to the train range.  splits == 1 writes idx /
// dist directly.
__global__ __launch_bounds__(256) void knn_l2sqr_f32_seg_kernel(L2F32Args A) {
  __shared__ uint4 lds[2][kStepChunks];
  const int tile = blockIdx.x;
  if (tile >= A.tile_start[A.nseg]) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 31, h = lane >> 5;
  const int b = seg_of(A.tile_start, A.nseg, 0x7fffffff, tile);
  const int qe = clamp_row(A.qoff[b + 1], A.q_cap);
  // the wave's first query; < qe for wave 0
  const int qw = clamp_row(A.qoff[b], A.q_cap) + (tile - A.tile_start[b]) * kTileQ + wv * (32 * kQB);
  const bool live = qw < qe;  // wave-uniform: a wave past the segment only helps to move train rows
  int ts = 0, te = A.t_cap;  // train_range() of match_seg.hpp, restated
  if (A.toff) {
    ts = clamp_row(A.toff[b], A.t_cap);
    te = clamp_row(A.toff[b + 1], A.t_cap);
    te = te < ts ? ts : te;
  }
  const int per = (((te - ts) + A.splits - 1) / A.splits + kStep - 1) / kStep * kStep;
  const long long t0l = ts + (long long)blockIdx.y * per;
  const int t0 = t0l < te ? (int)t0l : te, t1 = (te - t0) < per ? te : t0 + per;

  float qf[kQB][64];
  float qn[kQB];
  BestF best[kQB];
#pragma unroll
  for (int s = 0; s < kQB; ++s) {  // block s: query qw + 32 s + col (the last live row stands in past the segment)
    const int qi = live ? min(qw + 32 * s + col, qe - 1) : 0;
    const uint4* p = reinterpret_cast<const uint4*>(A.q + (long long)qi * kDescLen) + h;
#pragma unroll
    for (int c = 0; c < kRowChunks / 2; ++c) {
      const uint4 x = live ? p[2 * c] : make_uint4(0, 0, 0, 0);
      qf[s][4 * c + 0] = __uint_as_float(x.x);
      qf[s][4 * c + 1] = __uint_as_float(x.y);
      qf[s][4 * c + 2] = __uint_as_float(x.z);
      qf[s][4 * c + 3] = __uint_as_float(x.w);
    }
    qn[s] = live ? A.q_norm[qi] : 0.f;
    best[s] = top2_empty<float>();
  }

  if (t0 < t1) {
    uint4 x[kLoads];
    fetch_step(A.t, t0, t1, tid, x);
    stash_step(lds[0], tid, x);
    __syncthreads();
    int cur = 0;
    for (int r0 = t0; r0 < t1; r0 += kStep, cur ^= 1) {
      // the last step asks for itself again and writes it behind: nobody reads that buffer
      fetch_step(A.t, r0 + kStep < t1 ? r0 + kStep : r0, t1, tid, x);
      if (live) {
        const int nvalid = t1 - r0;
        if (nvalid >= kStep)
          score_step<false>(lds[cur], A.t_norm + r0, qf, qn, r0 - ts, nvalid, lane, best);
        else
          score_step<true>(lds[cur], A.t_norm + r0, qf, qn, r0 - ts, nvalid, lane, best);
      }
      stash_step(lds[cur ^ 1], tid, x);
      __syncthreads();
    }
  }
  if (!live) return;
  // the other half-wave scored the other rows of the same queries
#pragma unroll
  for (int s = 0; s < kQB; ++s) {
    const float d1 = __shfl_xor(best[s].d1, 32), d2 = __shfl_xor(best[s].d2, 32);
    const int i1 = __shfl_xor(best[s].i1, 32), i2 = __shfl_xor(best[s].i2, 32);
    insert(best[s], d1, i1);
    insert(best[s], d2, i2);
  }
  if (h != 0) return;
#pragma unroll
  for (int s = 0; s < kQB; ++s) {
    const int qi = qw + 32 * s + col;
    if (qi >= qe) continue;
    if (A.splits == 1) {
      write_knn(best[s], qi, A.k, A.idx, A.dist);
    } else {
      const long long o = (long long)blockIdx.y * A.q_cap + qi;
      A.part_d[o] = make_float2(best[s].d1, best[s].d2);
      A.part_i[o] = make_int2(best[s].i1, best[s].i2);
    }
  }
}

}  // namespace

int knn_l2_f32_seg_max_tiles(int q_cap, int n_segments) { return q_cap / kTileQ + n_segments; }

int knn_l2_f32_seg_splits(int q_cap, int n_segments, int t_cap, bool seg_train) {
  const int gx = knn_l2_f32_seg_max_tiles(q_cap, n_segments);
  int s = (1024 + gx - 1) / gx;  // ~1k workgroups: one per CU at a time (256 CUs), four rounds
  // segmented train: an even share of the buffer stands in for the segment size
  const int nt = seg_train ? (t_cap + n_segments - 1) / n_segments : t_cap;
  const int max_s = (nt + kStep - 1) / kStep;  // at least one granule per split
  s = s < max_s ? s : max_s;
  return s < 1 ? 1 : s;
}

void launch_knn_l2sqr_f32_seg(hipStream_t st, const float* q, const int* qoff, int n_segments, int q_cap,
                              const float* t, const int* toff, int t_cap, int k, int splits, int* tile_start,
                              float* q_norm, float* t_norm, float2* part_d, int2* part_i, int* idx, float* dist) {
  hipLaunchKernelGGL(seg_tiles_kernel<kTileQ>, dim3(1), dim3(256), 0, st, qoff, n_segments, q_cap, tile_start);
  const long long rows = (long long)q_cap + t_cap + kNormPad;
  hipLaunchKernelGGL(l2_f32_norms_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const uint4*>(q), qoff, n_segments, q_cap, reinterpret_cast<const uint4*>(t),
                     t_cap, q_norm, t_norm);
  const L2F32Args A{q,      qoff,   n_segments, q_cap, t,      toff,   t_cap, tile_start,
                    q_norm, t_norm, splits,     k,     part_d, part_i, idx,   dist};
  dim3 grid(knn_l2_f32_seg_max_tiles(q_cap, n_segments), splits);
  hipLaunchKernelGGL(knn_l2sqr_f32_seg_kernel, grid, dim3(256), 0, st, A);
  if (splits > 1)
    hipLaunchKernelGGL(knn_seg_merge_kernel<float2>, dim3((q_cap + 255) / 256), dim3(256), 0, st, part_d, part_i, qoff,
                       n_segments, q_cap, splits, k, idx, dist);
}

}  // namespace sift
