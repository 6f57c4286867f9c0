// join.hip -- the segmented, ordered join of two sift_match tables on the index
// of the keypoint they share: table A's records carry 3-D points (what
// sift_recover_pose_segmented_device leaves by pair row), table B's the next
// view's pixels, and the joined rows are the 2-D / 3-D rows that
// sift_solve_pnp_segmented_device takes.  The rule is include/sift_hip.h's
// (sift_join_matches); the host form of one segment is join_rule.hpp.
// DESIGN.md §6s.
//
// Shape: the ratio and cross-check stages' ordered compaction (count per block,
// one-workgroup scan of block_scan.hpp, emit that tests again and ranks inside
// the block; no atomic decides the order) behind a scatter that elects each
// key's winner with one 64-bit vector atomicMin per candidate A row.  Both
// tables are walked in blocks of kRB rows that never span two segments (tile
// tables as in match_seg.hpp), so the segment, its row range and its key slice
// are found once per block, uniformly, not once per record.  Launches: the
// lookup fill (hipMemsetAsync), the two tile tables, scatter, count, scan, emit.
// No floating arithmetic beyond the `+ 0.0f` of the rank; the gathered doubles
// and floats move as bits.  Bound: memory -- 16-byte record loads, one byte of
// mask, one 8-byte gather from the lookup per live row, and per joined row 24 +
// 8 bytes gathered and 24 + 8 + 4 + 4 written.
#include "common.hpp"
#include "block_scan.hpp"
#include "match_seg.hpp"

namespace sift {

namespace {

constexpr int kRB = 256;  // rows per block of the stage (scratch.hpp's kJoinRows)
constexpr unsigned long long kNoWinner = ~0ull;

// One table of records with its segments.
struct JoinTable {
  const sift_match* rec;
  const int* off;
  int cap, side;  // side: SIFT_JOIN_QUERY / SIFT_JOIN_TRAIN, the index that names the shared view's keypoint
  const unsigned char* mask;
  int* tiles;     // [nseg + 1], written by join_tiles_kernel
};

// The shared views' keypoints: segment s owns lookup[klo, klo + nkeys).
struct JoinKeys {
  const int* off;
  int cap;
  unsigned long long* lookup;
};

// Workgroup 0: table A's tile table; workgroup 1: table B's (seg_tiles_kernel's scan).
__global__ __launch_bounds__(256) void join_tiles_kernel(JoinTable A, JoinTable B, int nseg) {
  const JoinTable T = blockIdx.x ? B : A;
  const int total = wg_scan_chunks<256>(
      nseg,
      [&](int s) {
        const int lo = clamp_row(T.off[s], T.cap), hi = clamp_row(T.off[s + 1], T.cap);
        return hi > lo ? (hi - lo + kRB - 1) / kRB : 0;
      },
      [&](int s, int x) { T.tiles[s] = x; });
  if (threadIdx.x == 0) T.tiles[nseg] = total;
}

// What a block of a table works on: its segment's key slice and this thread's row.
struct JoinRow {
  int row;        // absolute row of the table; -1: none (past the segment's end)
  int klo, nkeys;
};

// Block `tile` of table T (tile < T.tiles[nseg]): every value but row is uniform.
__device__ __forceinline__ JoinRow join_row(const JoinTable& T, const JoinKeys& K, int nseg, int tile) {
  const int s = seg_of(T.tiles, nseg, 0x7fffffff, tile);
  const int lo = clamp_row(T.off[s], T.cap), hi = clamp_row(T.off[s + 1], T.cap);
  const int klo = clamp_row(K.off[s], K.cap), khi = clamp_row(K.off[s + 1], K.cap);
  const int row = lo + (tile - T.tiles[s]) * kRB + (int)threadIdx.x;  // <= hi + kRB <= cap + kRB: no overflow
  return {row < hi ? row : -1, klo, khi - klo};
}

// The record as one 16-byte load: x = query, y = train, z = the distance's bits, w = segment (not read).
__device__ __forceinline__ int4 load_record(const sift_match* rec, int row) {
  return *reinterpret_cast<const int4*>(rec + row);
}

// The row's key if the row is live (it exists, its mask byte is set, its key lies
// in the segment's slice), else -1.  klo + key < klo + nkeys <= K.cap.
__device__ __forceinline__ int live_key(const JoinTable& T, const JoinRow& R, int4& rec) {
  if (R.row < 0) return -1;
  if (T.mask && !T.mask[R.row]) return -1;
  rec = load_record(T.rec, R.row);
  const int key = T.side ? rec.y : rec.x;
  return key >= 0 && key < R.nkeys ? key : -1;
}

// One thread per A row: a candidate bids ((uint64)bits(distance + 0.0f) << 32) | row
// for its key.  distance >= 0 is false for NaN; the sum turns -0.0 into +0.0.
__global__ __launch_bounds__(kRB) void join_scatter_kernel(JoinTable A, JoinKeys K, int nseg) {
  const int tile = blockIdx.x;
  if (tile >= A.tiles[nseg]) return;
  const JoinRow R = join_row(A, K, nseg, tile);
  int4 rec;
  const int key = live_key(A, R, rec);
  if (key < 0) return;
  const float d = __int_as_float(rec.z);
  if (!(d >= 0.f)) return;
  const unsigned long long bid =
      ((unsigned long long)__float_as_uint(d + 0.0f) << 32) | (unsigned long long)(unsigned)R.row;
  atomicMin(K.lookup + R.klo + key, bid);
}

// B row R joins iff it is live and its key has a winner; win gets the lookup entry.
__device__ __forceinline__ bool join_keep(const JoinTable& B, const JoinKeys& K, const JoinRow& R,
                                          unsigned long long& win) {
  int4 rec;
  const int key = live_key(B, R, rec);
  if (key < 0) return false;
  win = K.lookup[R.klo + key];
  return win != kNoWinner;
}

// blk_cnt[tile] = joined rows of block `tile`, 0 for the blocks past the last one.
__global__ __launch_bounds__(kRB) void join_count_kernel(JoinTable B, JoinKeys K, int nseg,
                                                         int* __restrict__ blk_cnt) {
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int tile = blockIdx.x;
  bool keep = false;
  if (tile < B.tiles[nseg]) {  // uniform
    unsigned long long win;
    keep = join_keep(B, K, join_row(B, K, nseg, tile), win);
  }
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wcnt[wv] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[tile] = (wcnt[0] + wcnt[1]) + (wcnt[2] + wcnt[3]);
}

struct JoinOut {
  const double* a_xyz;  // [a_cap][3], read at the winner's row
  const float* b_xy;    // [b_cap][2], read at the B row
  double* xyz;
  float* xy;
  int* a_row;
  int* b_row;
  unsigned char* b_joined;
  int j_cap;
  int* joff;
};

// Blocks [0, max_tiles): one B row per thread, ranked inside the block in row
// order behind the scanned block counts.  Blocks past max_tiles: one thread per
// segment boundary s writes joff[s] = the joined rows of the blocks before
// segment s's first; a table whose overlapping segments need more than
// max_tiles blocks loses the blocks past them, and joff counts what was written.
__global__ __launch_bounds__(kRB) void join_emit_kernel(JoinTable B, JoinKeys K, int nseg,
                                                        const int* __restrict__ blk_pre, int max_tiles, JoinOut O) {
  __shared__ int wcnt[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int tile = blockIdx.x;
  if (tile >= max_tiles) {
    const int s = (tile - max_tiles) * kRB + (int)threadIdx.x;
    if (s <= nseg) O.joff[s] = blk_pre[min(B.tiles[s], max_tiles)];
    return;
  }
  if (tile >= B.tiles[nseg]) return;
  const JoinRow R = join_row(B, K, nseg, tile);
  unsigned long long win = kNoWinner;
  const bool keep = join_keep(B, K, R, win);
  if (O.b_joined && R.row >= 0) O.b_joined[R.row] = keep;
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wcnt[wv] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int pos = blk_pre[tile] + __popcll(m & ((1ull << lane) - 1ull));
  for (int w = 0; w < wv; ++w) pos += wcnt[w];
  if (pos >= O.j_cap) return;
  const int w = (int)(unsigned)win;  // an A row some candidate wrote: < a_cap
  if (O.xyz) {
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(O.a_xyz) + 3ll * w;
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(O.xyz) + 3ll * pos;
    dst[0] = src[0];
    dst[1] = src[1];
    dst[2] = src[2];
  }
  if (O.xy) reinterpret_cast<uint2*>(O.xy)[pos] = reinterpret_cast<const uint2*>(O.b_xy)[R.row];
  if (O.a_row) O.a_row[pos] = w;
  if (O.b_row) O.b_row[pos] = R.row;
}

}  // namespace

int join_max_blocks(int cap, int n_segments) { return cap / kRB + n_segments; }

void launch_join_matches(hipStream_t st, const sift_match* a, const int* aoff, int a_cap, int a_side,
                         const unsigned char* a_mask, const double* a_xyz, const sift_match* b, const int* boff,
                         int b_cap, int b_side, const unsigned char* b_mask, const float* b_xy, const int* koff,
                         int key_cap, int n_segments, double* xyz_out, float* xy_out, int* a_row, int* b_row,
                         unsigned char* b_joined, int j_cap, int* joff, unsigned long long* lookup, int* a_tiles,
                         int* b_tiles, int* blk_scan) {
  const JoinTable A{a, aoff, a_cap, a_side, a_mask, a_tiles}, B{b, boff, b_cap, b_side, b_mask, b_tiles};
  const JoinKeys K{koff, key_cap, lookup};
  const JoinOut O{a_xyz, b_xy, xyz_out, xy_out, a_row, b_row, b_joined, j_cap, joff};
  const int a_max = join_max_blocks(a_cap, n_segments), b_max = join_max_blocks(b_cap, n_segments);
  if (key_cap > 0) (void)hipMemsetAsync(lookup, 0xff, (size_t)key_cap * sizeof(unsigned long long), st);
  hipLaunchKernelGGL(join_tiles_kernel, dim3(2), dim3(256), 0, st, A, B, n_segments);
  hipLaunchKernelGGL(join_scatter_kernel, dim3(a_max), dim3(kRB), 0, st, A, K, n_segments);
  hipLaunchKernelGGL(join_count_kernel, dim3(b_max), dim3(kRB), 0, st, B, K, n_segments, blk_scan);
  hipLaunchKernelGGL(ratio_scan_kernel, dim3(1), dim3(1024), 0, st, blk_scan, b_max);
  hipLaunchKernelGGL(join_emit_kernel, dim3(b_max + (n_segments + 1 + kRB - 1) / kRB), dim3(kRB), 0, st, B, K,
                     n_segments, blk_scan, b_max, O);
}

}  // namespace sift
