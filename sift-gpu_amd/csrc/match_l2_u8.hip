// match_l2_u8.hip -- brute-force squared-L2 kNN matcher (k <= 2) on 8-bit
// descriptors for gfx950, with the products on the matrix pipe
// (v_mfma_i32_32x32x32_i8).  Same contract as match_u8.hip's L1 matcher.
//
// Distance: sum (a - b)^2 over 128 unsigned bytes, an integer <= 128 * 255^2 =
// 8,323,200 < 2^23.  MFMA i8 operands are signed, so every byte is biased to
// x' = x ^ 0x80 = x - 128 (once per loaded dword); differences are unchanged and
//   d = |q'|^2 + |t'|^2 - 2 q'.t',   |q'.t'| <= 2^21, each norm <= 2^21,
// all exact in int32.  The norms come from one small pre-kernel (one int per
// row of both buffers, in context scratch); the products are integer MFMA, so
// nothing depends on a summation order.
//
// Tile: D = A.B with A = 32 train rows, B = 32 queries, K = 128 as four
// 32x32x32 steps.  The accumulator has the query on the lane (col = lane & 31)
// and the train rows in its 16 registers (row = (reg & 3) + 8 (reg >> 2) +
// 4 (lane >> 5)), so a lane's running top-2 belongs to one query and the two
// half-waves hold different train rows of it.  Both operands are loaded with
// the same k map -- lane (r, h), step s: bytes [32 s + 16 h, +16) of row r --
// so whatever order the hardware gives the 16 bytes of a lane, the sum runs
// over all 128 element pairs.
//
// Selection: a candidate is the one 32-bit key (d << 9) | (row - chunk base):
// d takes 23 bits, a chunk is 512 rows, keys are distinct and their unsigned
// order is the (distance, index) order, so the update is min / max / min.  At
// the end of every chunk the two keys are decoded and folded into the lane's
// (distance, index) top-2 with the explicit comparison, and the keys start
// again: the index bits bound the chunk, not the split, whatever the offsets
// hold.  Only a wave's last tile can hold rows past its range; that tile takes
// the path that replaces their keys by the empty key.
//
// Layout: a workgroup owns 32 x kQB queries, held as B fragments by each of its
// four waves (16 VGPRs per 32 queries), and one split of the segment's train
// rows; wave w scores the w-th quarter of the split, 32 rows at a time straight
// from global memory into A fragments (the next tile is requested before the
// current one is scored; no LDS and no barrier in the loop).  The half-waves
// merge by one lane exchange, the waves through LDS, the splits by the integer
// merge kernel.  DESIGN.md §6d.
#include "common.hpp"
#include "match_seg.hpp"

namespace sift {

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kQB = 4;                   // 32-query blocks per wave
constexpr int kL2Tile = 32 * kQB;        // queries per workgroup
constexpr int kTR = 32;                  // train rows per MFMA tile
constexpr int kGran = 4 * kTR;           // train rows per split granule: one tile per wave
constexpr int kLocBits = 9;              // row bits of a key
constexpr int kChunk = 1 << kLocBits;    // rows scored between two folds
constexpr int kNormPad = kL2NormPad;     // t_norm entries past t_cap a tail tile may read (zeros, masked)
static_assert(kNormPad >= kTR, "a tail tile reads the norms of a whole tile");
constexpr unsigned kBias = 0x80808080u;
constexpr unsigned kEmptyKey = 0xffffffffu;  // above (8,323,200 << 9) | 511

// ---- norms ---------------------------------------------------------------------
__device__ __forceinline__ int sq4(unsigned w) {
  w ^= kBias;
  const int a = (signed char)(w & 0xff), b = (signed char)((w >> 8) & 0xff);
  const int c = (signed char)((w >> 16) & 0xff), d = (signed char)(w >> 24);
  return a * a + b * b + c * c + d * d;
}

// Eight lanes per row, 16 bytes each: q_norm[i] = |q'_i|^2 for i < q_cap,
// t_norm[j] = |t'_j|^2 for j < t_cap and 0 for the kNormPad entries after them.
__global__ __launch_bounds__(256) void l2_norms_kernel(const uint4* __restrict__ q, int q_cap,
                                                       const uint4* __restrict__ t, int t_cap,
                                                       int* __restrict__ q_norm, int* __restrict__ t_norm) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long row = g >> 3;
  const int part = (int)(g & 7);
  if (row >= (long long)q_cap + t_cap + kNormPad) return;  // whole groups of eight lanes leave together
  const bool is_q = row < q_cap;
  const long long r = is_q ? row : row - q_cap;
  int v = 0;
  if (is_q || r < t_cap) {
    const uint4 x = (is_q ? q : t)[r * 8 + part];
    v = sq4(x.x) + sq4(x.y) + sq4(x.z) + sq4(x.w);
  }
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  if (part == 0) (is_q ? q_norm : t_norm)[r] = v;
}

// ---- matcher -------------------------------------------------------------------
using BestI = Top2<int>;  // match_seg.hpp: the decoded list, its order, insert() and write_knn()

__device__ __forceinline__ void fold(BestI& b, unsigned key, int base) {
  if (key != kEmptyKey) insert(b, (int)(key >> kLocBits), (int)(key & (kChunk - 1)) + base);
}

struct L2Args {
  const uint8_t* q;
  const int* qoff;
  int nseg, q_cap;
  const uint8_t* t;
  const int* toff;  // nullptr: shared train
  int t_cap;
  const int* tile_start;
  const int* q_norm;
  const int* t_norm;  // t_cap + kNormPad entries
  int splits, k;
  int2* part_d;
  int2* part_i;
  int* idx;
  float* dist;
};

// One operand fragment: bytes [32 s + 16 h, +16) of a row, s = 0..3, biased.
__device__ __forceinline__ void load_frags(const uint8_t* __restrict__ row, int h, v4i (&f)[4]) {
  const uint4* p = reinterpret_cast<const uint4*>(row) + h;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const uint4 x = p[2 * s];
    f[s] = v4i{(int)(x.x ^ kBias), (int)(x.y ^ kBias), (int)(x.z ^ kBias), (int)(x.w ^ kBias)};
  }
}

// The train rows an accumulator register holds, less the lane's 4 h.
__device__ __forceinline__ constexpr int reg_row(int g) { return (g & 3) + 8 * (g >> 2); }

struct TrainTile {
  v4i a[4];    // A fragments of row r0 + (lane & 31), clamped into the range
  int tn[16];  // |t'|^2 of the rows of the lane's 16 accumulator registers
};

// Rows [r0, r0 + 32) of the wave's range, which ends at w1 > r0.  A row at or
// past w1 reads row w1 - 1 instead (its key is masked by the tail path); the
// norms are read in place: t_norm has kNormPad entries past t_cap >= w1.
__device__ __forceinline__ void load_tile(const L2Args& A, int r0, int w1, int lane, TrainTile& T) {
  const int r = min(r0 + (lane & 31), w1 - 1), h = lane >> 5;
  load_frags(A.t + (long long)r * kDescLen, h, T.a);
  const int* n = A.t_norm + r0 + 4 * h;
#pragma unroll
  for (int g = 0; g < 16; ++g) T.tn[g] = n[reg_row(g)];
}

// One train tile against the wave's kQB query blocks.  loc: row r0 + 4 h less
// the chunk base; nvalid: rows of the tile inside the range (used by kTail).
template <bool kTail>
__device__ __forceinline__ void score_tile(const TrainTile& T, const v4i (&qf)[kQB][4], const unsigned (&qn9)[kQB],
                                           int loc, int nvalid, int h, unsigned (&k1)[kQB], unsigned (&k2)[kQB]) {
  unsigned tk[16];  // (|t'|^2 << 9) + the row's place in the chunk
#pragma unroll
  for (int g = 0; g < 16; ++g) tk[g] = ((unsigned)T.tn[g] << kLocBits) + (unsigned)(loc + reg_row(g));
#pragma unroll
  for (int b = 0; b < kQB; ++b) {
    v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(T.a[s], qf[b][s], acc, 0, 0, 0);
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      // ((|q'|^2 + |t'|^2 - 2 q'.t') << 9) + place; |q'.t'| <= 2^21 fits the 24-bit multiply
      unsigned key = (tk[g] + qn9[b]) + (unsigned)__mul24(acc[g], -(2 << kLocBits));
      if (kTail) key = reg_row(g) + 4 * h < nvalid ? key : kEmptyKey;
      const unsigned hi = key > k1[b] ? key : k1[b];
      k2[b] = hi < k2[b] ? hi : k2[b];
      k1[b] = key < k1[b] ? key : k1[b];
    }
  }
}

// The grid is sized from the capacities as in knn_l1_u8_seg_kernel: grid.x
// covers the most tiles they allow and workgroups past tile_start[nseg] exit;
// grid.y splits every segment's own train range evenly, in granules of kGran
// rows.  Indices are local to the train range.  splits == 1 writes idx / dist
// directly.
__global__ __launch_bounds__(256) void knn_l2sqr_u8_seg_kernel(L2Args A) {
  __shared__ int md[3][2][kL2Tile];
  __shared__ int mi[3][2][kL2Tile];
  const int tile = blockIdx.x;
  if (tile >= A.tile_start[A.nseg]) return;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int col = lane & 31, h = lane >> 5;
  const int b = seg_of(A.tile_start, A.nseg, 0x7fffffff, tile);
  const int qe = clamp_row(A.qoff[b + 1], A.q_cap);
  const int q0 = clamp_row(A.qoff[b], A.q_cap) + (tile - A.tile_start[b]) * kL2Tile + col;  // < qe for lane 0
  int ts = 0, te = A.t_cap;  // train_range() of match_seg.hpp, restated (profiles/match_refactor_isa.txt)
  if (A.toff) {
    ts = clamp_row(A.toff[b], A.t_cap);
    te = clamp_row(A.toff[b + 1], A.t_cap);
    te = te < ts ? ts : te;
  }
  const int per = (((te - ts) + A.splits - 1) / A.splits + kGran - 1) / kGran * kGran;
  const long long t0l = ts + (long long)blockIdx.y * per;
  const int t0 = t0l < te ? (int)t0l : te, t1 = (te - t0) < per ? te : t0 + per;
  // wave wv's quarter [w0, w1) of the split, a multiple of kTR rows unless it ends the range
  int w0 = (t1 - t0) < wv * (per / 4) ? t1 : t0 + wv * (per / 4);
  int w1 = (t1 - w0) < per / 4 ? t1 : w0 + per / 4;
  w0 = __builtin_amdgcn_readfirstlane(w0);
  w1 = __builtin_amdgcn_readfirstlane(w1);

  v4i qf[kQB][4];
  unsigned qn9[kQB];
#pragma unroll
  for (int s = 0; s < kQB; ++s) {  // block s: query q0 + 32 s (the last live row stands in past the segment)
    const int qi = min(q0 + 32 * s, qe - 1);
    load_frags(A.q + (long long)qi * kDescLen, h, qf[s]);
    qn9[s] = (unsigned)A.q_norm[qi] << kLocBits;
  }
  BestI best[kQB];
#pragma unroll
  for (int s = 0; s < kQB; ++s) best[s] = top2_empty<int>();

  if (w0 < w1) {
    unsigned k1[kQB], k2[kQB];
#pragma unroll
    for (int s = 0; s < kQB; ++s) k1[s] = k2[s] = kEmptyKey;
    TrainTile cur;
    load_tile(A, w0, w1, lane, cur);
    int c0 = w0;  // chunk base
    for (int r0 = w0; r0 < w1; r0 += kTR) {
      TrainTile nxt;
      load_tile(A, r0 + kTR < w1 ? r0 + kTR : r0, w1, lane, nxt);
      const int nvalid = w1 - r0, loc = r0 - c0 + 4 * h;
      if (nvalid >= kTR)
        score_tile<false>(cur, qf, qn9, loc, nvalid, h, k1, k2);
      else
        score_tile<true>(cur, qf, qn9, loc, nvalid, h, k1, k2);
      cur = nxt;
      if (r0 + kTR - c0 == kChunk || r0 + kTR >= w1) {  // the chunk is full, or the range ends
#pragma unroll
        for (int s = 0; s < kQB; ++s) {
          fold(best[s], k1[s], c0 - ts);
          fold(best[s], k2[s], c0 - ts);
          k1[s] = k2[s] = kEmptyKey;
        }
        c0 = r0 + kTR;
      }
    }
  }
  // the other half-wave scored the other rows of the same queries
#pragma unroll
  for (int s = 0; s < kQB; ++s) {
    const int d1 = __shfl_xor(best[s].d1, 32), i1 = __shfl_xor(best[s].i1, 32);
    const int d2 = __shfl_xor(best[s].d2, 32), i2 = __shfl_xor(best[s].i2, 32);
    insert(best[s], d1, i1);
    insert(best[s], d2, i2);
  }
  if (wv > 0 && h == 0) {
#pragma unroll
    for (int s = 0; s < kQB; ++s) {
      md[wv - 1][0][32 * s + col] = best[s].d1;
      md[wv - 1][1][32 * s + col] = best[s].d2;
      mi[wv - 1][0][32 * s + col] = best[s].i1;
      mi[wv - 1][1][32 * s + col] = best[s].i2;
    }
  }
  __syncthreads();
  if (wv != 0 || h != 0) return;
#pragma unroll
  for (int s = 0; s < kQB; ++s) {
    const int qi = q0 + 32 * s;
    if (qi >= qe) continue;
#pragma unroll
    for (int w = 0; w < 3; ++w) {
      insert(best[s], md[w][0][32 * s + col], mi[w][0][32 * s + col]);
      insert(best[s], md[w][1][32 * s + col], mi[w][1][32 * s + col]);
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

}  // namespace

int knn_l2_u8_seg_max_tiles(int q_cap, int n_segments) { return q_cap / kL2Tile + n_segments; }

// No bound from the key: its index bits number the rows of a chunk, not of a split.
int knn_l2_u8_seg_splits(int q_cap, int n_segments, int t_cap, bool seg_train) {
  const int gx = knn_l2_u8_seg_max_tiles(q_cap, n_segments);
  int s = (2048 + gx - 1) / gx;  // ~2k workgroups to fill 256 CUs
  // segmented train: an even share of the buffer stands in for the segment size
  const int nt = seg_train ? (t_cap + n_segments - 1) / n_segments : t_cap;
  const int max_s = (nt + kGran - 1) / kGran;  // at least one granule per split
  s = s < max_s ? s : max_s;
  return s < 1 ? 1 : s;
}

void launch_knn_l2sqr_u8_seg(hipStream_t st, const uint8_t* q, const int* qoff, int n_segments, int q_cap,
                             const uint8_t* t, const int* toff, int t_cap, int k, int splits, int* tile_start,
                             int* q_norm, int* t_norm, int2* part_d, int2* part_i, int* idx, float* dist) {
  hipLaunchKernelGGL(seg_tiles_kernel<kL2Tile>, dim3(1), dim3(256), 0, st, qoff, n_segments, q_cap, tile_start);
  const long long groups = ((long long)q_cap + t_cap + kNormPad) * 8;
  hipLaunchKernelGGL(l2_norms_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const uint4*>(q), q_cap, reinterpret_cast<const uint4*>(t), t_cap, q_norm,
                     t_norm);
  const L2Args A{q,      qoff,   n_segments, q_cap, t,      toff,   t_cap, tile_start,
                 q_norm, t_norm, splits,     k,     part_d, part_i, idx,   dist};
  dim3 grid(knn_l2_u8_seg_max_tiles(q_cap, n_segments), splits);
  hipLaunchKernelGGL(knn_l2sqr_u8_seg_kernel, grid, dim3(256), 0, st, A);
  if (splits > 1)
    hipLaunchKernelGGL(knn_seg_merge_kernel<int2>, dim3((q_cap + 255) / 256), dim3(256), 0, st, part_d, part_i, qoff,
                       n_segments, q_cap, splits, k, idx, dist);
}

}  // namespace sift
