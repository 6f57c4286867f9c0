// scan.hip -- the exclusive scan of the detection stages (candidates per mask
// chunk, orientation peaks per candidate) and the gather of per-image offsets.
#include "detect_args.hpp"
#include "wave_scan.hpp"

namespace sift {

// ---- exclusive scan (reduce / scan of tile sums / down-sweep) ---------------
// out[i] = sum(in[0..i)), out[n] = total (also *total_out if given).  n from
// n_dev (clamped to cap) if given, else n_host.  The grid is sized from cap on
// the host; tiles past n contribute 0 and write nothing.
constexpr int kScanT = 256, kScanPer = 16, kScanTile = kScanT * kScanPer;

__device__ __forceinline__ int scan_n(const int* n_dev, int n_host, int cap) {
  const int n = n_dev ? *n_dev : n_host;
  return n < cap ? n : cap;
}

__device__ __forceinline__ int block_sum(int v, int* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
  if (lane == 0) red[wv] = v;
  __syncthreads();
  int t = 0;
  for (int k = 0; k < kScanT / 64; ++k) t += red[k];
  return t;
}

__global__ __launch_bounds__(kScanT) void scan_reduce_kernel(const int* __restrict__ in, const int* n_dev,
                                                             int n_host, int cap, int* __restrict__ tsum) {
  __shared__ int red[kScanT / 64];
  const int n = scan_n(n_dev, n_host, cap);
  const long long base = (long long)blockIdx.x * kScanTile;
  int s = 0;
  if (base < n)
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
      const long long i = base + k * kScanT + threadIdx.x;
      s += i < n ? in[i] : 0;
    }
  s = block_sum(s, red);
  if (threadIdx.x == 0) tsum[blockIdx.x] = s;
}

// exclusive scan of the tile sums in place (one workgroup); out[n] = total
__global__ __launch_bounds__(1024) void scan_tiles_kernel(int* __restrict__ tsum, int ntiles, const int* n_dev,
                                                          int n_host, int cap, int* __restrict__ out,
                                                          int* total_out) {
  const int total = wg_scan_chunks<1024>(ntiles, [&](int i) { return tsum[i]; }, [&](int i, int x) { tsum[i] = x; });
  if (threadIdx.x == 0) {
    out[scan_n(n_dev, n_host, cap)] = total;
    if (total_out) *total_out = total;
  }
}

__global__ __launch_bounds__(kScanT) void scan_down_kernel(const int* __restrict__ in, const int* n_dev,
                                                           int n_host, int cap, const int* __restrict__ tsum,
                                                           int* __restrict__ out) {
  __shared__ int wsum[kScanT / 64];
  const int n = scan_n(n_dev, n_host, cap);
  const long long base = (long long)blockIdx.x * kScanTile;
  if (base >= n) return;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // thread tid owns the kScanPer consecutive elements [base + tid*kScanPer, ...)
  int v[kScanPer];
  int s = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    const long long i = base + (long long)tid * kScanPer + k;
    v[k] = i < n ? in[i] : 0;
    s += v[k];
  }
  // wave_scan_incl() + wg_scan<kScanT / 64>().before restated: the calls change this kernel's text (profiles/detect_split_isa.txt)
  int incl = s;
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(incl, off);
    if (lane >= off) incl += t;
  }
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  int run = tsum[blockIdx.x] + incl - s;
  for (int k = 0; k < wv; ++k) run += wsum[k];
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    const long long i = base + (long long)tid * kScanPer + k;
    if (i < n) out[i] = run;
    run += v[k];
  }
}

// The same exclusive scan in one workgroup for short lists (one image's
// candidate blocks and orientation peaks): one launch instead of three, on a
// path whose launches are latency-bound.  Thread t owns the `per` consecutive
// elements [t * per, t * per + per) (per <= 64, in registers); out[n] = total.
// The gather of the per-image offsets (ScanGather; gather_offsets_kernel's
// contract) follows in the same launch.
constexpr int kScanSmallMax = 1024 * 64;  // one 1080p image: 64,800 candidates
__global__ __launch_bounds__(1024) void scan_small_kernel(const int* __restrict__ in, const int* n_dev, int n_host,
                                                          int cap, int* __restrict__ out, int* total_out,
                                                          ScanGather g) {
  __shared__ int wsum[16];
  const int n = scan_n(n_dev, n_host, cap);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // a multiple of 4 (<= kScanSmallMax / 1024): the chunk is read as int4s, all
  // in flight at once -- a loop of dependent loads cost ~13 us for a 1080p
  // image's ~50 K candidates (round 6)
  const int per = ((n + 1023) / 1024 + 3) & ~3;
  const int i0 = tid * per;
  const bool vec = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
  int v[kScanSmallMax / 1024];
#pragma unroll
  for (int k = 0; k < kScanSmallMax / 1024; k += 4) {
    if (k < per && vec && i0 + k + 3 < n) {
      const int4 q = *reinterpret_cast<const int4*>(in + i0 + k);
      v[k] = q.x;
      v[k + 1] = q.y;
      v[k + 2] = q.z;
      v[k + 3] = q.w;
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[k + u] = k < per && i0 + k + u < n ? in[i0 + k + u] : 0;
    }
  }
  int s = 0;
#pragma unroll
  for (int k = 0; k < kScanSmallMax / 1024; ++k) s += v[k];
  const int incl = wave_scan_incl(s, lane);
  // wg_scan<16>() restated, `run` as its accumulator (profiles/detect_split_isa.txt)
  if (lane == 63) wsum[wv] = incl;
  __syncthreads();
  int run = incl - s, tot = 0;
  for (int k = 0; k < 16; ++k) {
    run += k < wv ? wsum[k] : 0;
    tot += wsum[k];
  }
#pragma unroll
  for (int k = 0; k < kScanSmallMax / 1024; ++k)
    if (k < per && i0 + k < n) {
      out[i0 + k] = run;
      run += v[k];
    }
  if (tid == 0) {
    out[n] = tot;
    if (total_out) *total_out = tot;
  }
  if (g.gout) {  // the gather of the per-image offsets, after the whole scan is written
    __syncthreads();
    for (int b = tid; b <= g.batch; b += 1024) {
      int i = b * g.stride;
      if (g.idx) i = g.idx[b] < n ? g.idx[b] : n;
      g.gout[b] = out[i];
    }
  }
}

// out[b] = scan[b*stride] (idx == nullptr) or scan[min(idx[b], n)] with n the
// clamped length of the scanned list, for b = 0..batch (any batch: the block
// strides over it).
__global__ void gather_offsets_kernel(const int* __restrict__ scan, const int* __restrict__ idx,
                                      int stride, int batch, const int* n_dev, int cap,
                                      int* __restrict__ out) {
  int n = 0;
  if (idx) {
    n = *n_dev;
    n = n < cap ? n : cap;
  }
  for (int b = threadIdx.x; b <= batch; b += blockDim.x) {
    if (!idx) {
      out[b] = scan[(long long)b * stride];
    } else {
      const int i = idx[b];
      out[b] = scan[i < n ? i : n];
    }
  }
}

int scan_tiles_for(long long cap) { return (int)((cap + kScanTile - 1) / kScanTile); }

void launch_scan(hipStream_t st, const int* in, int* out, const int* n_dev, int n_host, int cap, int* total_out,
                 int* tsum, ScanGather g) {
  if (cap <= kScanSmallMax) {
    hipLaunchKernelGGL(scan_small_kernel, dim3(1), dim3(1024), 0, st, in, n_dev, n_host, cap, out, total_out, g);
    return;
  }
  const int nt = scan_tiles_for(cap) > 0 ? scan_tiles_for(cap) : 1;
  hipLaunchKernelGGL(scan_reduce_kernel, dim3(nt), dim3(kScanT), 0, st, in, n_dev, n_host, cap, tsum);
  hipLaunchKernelGGL(scan_tiles_kernel, dim3(1), dim3(1024), 0, st, tsum, nt, n_dev, n_host, cap, out, total_out);
  hipLaunchKernelGGL(scan_down_kernel, dim3(nt), dim3(kScanT), 0, st, in, n_dev, n_host, cap, tsum, out);
  if (g.gout)  // the three-kernel scan, then the gather as its own launch
    hipLaunchKernelGGL(gather_offsets_kernel, dim3(1), dim3(256), 0, st, out, g.idx, g.stride, g.batch,
                       g.idx ? n_dev : nullptr, cap, g.gout);
}

}  // namespace sift
