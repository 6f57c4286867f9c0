// select.hip -- the per-image keypoint budget of SIFT_NCL (sift_set_max_features):
// cv::KeyPointsFilter::retainBest on the device, placed between orientation
// and the keypoint scan.
//
// Every candidate slot ci of image b (slots [img_cand_off[b], img_cand_off[b+1])
// clamped to cand_cap) stands for npeaks[ci] keypoints that share one
// response, couts[ci].response.  With K the image's keypoint count and n the
// budget: K <= n keeps everything; otherwise T is the n-th largest response
// counted with multiplicity, and every slot with response >= T keeps all its
// keypoints (ties at the cut are kept, so the kept count can exceed n).  The
// dropped slots get npeaks = 0, and the scan, the emission and the descriptor
// pass that follow see a shorter list -- same order, same bytes per keypoint.
//
// T comes from a weighted radix select, most significant digit first: the key
// is the response's float bits as an unsigned integer (responses are >= 0, so
// the bits order like the values), the weight is npeaks.  Each pass builds a
// 256-bin histogram of weights over the keys that share the prefix fixed so
// far, finds the digit at which the weight counted from the top bin reaches
// what is still wanted, and appends it to the prefix; four passes fix T's 32
// bits.  Integer adds only: the result does not depend on the order in which
// the lanes arrive.  A NaN response is a key like any other.
//
// Two forms with the same result:
//  - select_block_kernel: one workgroup per image, histogram in LDS, all four
//    passes and the mark in one launch (a batch: ~10^4 slots per image);
//  - select_hist_kernel x 4 + select_mark_kernel: many workgroups per image,
//    LDS partial histograms added to a global one, one launch per pass (one
//    large image: up to ~10^6 slots).  No workgroup waits for another: pass p
//    re-derives the prefix from the finished histograms of passes 0..p-1.
#include <algorithm>

#include "common.hpp"
#include "wave_scan.hpp"

namespace sift {

namespace {

constexpr int kSelBits = 8;
static_assert((1 << kSelBits) == kSelectBins && kSelBits * kSelectPasses == 32, "four byte digits");

struct SelShared {
  int wsum[kSelectBins / 64];
  int digit, rest, total;
};

// For a histogram of kSelectBins weights: the largest digit d whose suffix sum
// S(d) = hist[d] + ... + hist[255] reaches `want` (1 <= want <= S(0)), and
// rest = want - S(d + 1), what is still wanted inside bin d (1 <= rest <=
// hist[d]).  total = S(0).  If S(0) < want: digit 0, rest 0.  Every thread of
// the workgroup (>= 256 threads, whole waves) calls it and gets the same values.
__device__ __forceinline__ void select_digit(const int* hist, int want, SelShared& s, int& digit, int& rest,
                                             int& total) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int v = 0, incl = 0;
  if (tid == 0) {
    s.digit = 0;
    s.rest = 0;
  }
  if (tid < kSelectBins) {  // waves 0..3, whole
    v = hist[kSelectBins - 1 - tid];
    incl = wave_scan_incl(v, lane);
    if (lane == 63) s.wsum[wv] = incl;
  }
  __syncthreads();
  if (tid < kSelectBins) {
    for (int k = 0; k < wv; ++k) incl += s.wsum[k];
    // incl = S(255 - tid), incl - v = S(256 - tid)
    if (incl >= want && incl - v < want) {
      s.digit = kSelectBins - 1 - tid;
      s.rest = want - (incl - v);
    }
    if (tid == kSelectBins - 1) s.total = incl;
  }
  __syncthreads();
  digit = s.digit;
  rest = s.rest;
  total = s.total;
  __syncthreads();  // s is written again by the next call
}

struct SelSeg {
  int lo, hi;
};
__device__ __forceinline__ SelSeg select_segment(const int* __restrict__ img_cand_off, int b, int cand_cap) {
  int lo = img_cand_off[b], hi = img_cand_off[b + 1];
  lo = lo < 0 ? 0 : lo < cand_cap ? lo : cand_cap;
  hi = hi < lo ? lo : hi < cand_cap ? hi : cand_cap;
  return SelSeg{lo, hi};
}

// The high bits that pass `pass` requires to equal the prefix (none in pass 0).
__device__ __forceinline__ unsigned select_fixed_mask(int pass) {
  return pass == 0 ? 0u : ~0u << (32 - kSelBits * pass);
}

// hist[digit of key] += npeaks over the slots lo + first, lo + first + stride, ...
// of [lo, hi) whose key has the prefix.
__device__ __forceinline__ void select_accumulate(const CandOut* __restrict__ couts, const int* npeaks, SelSeg g,
                                                  int first, int stride, int pass, unsigned prefix, int* hist) {
  const unsigned fixed = select_fixed_mask(pass);
  const int shift = 32 - kSelBits * (pass + 1);
  for (long long ci = (long long)g.lo + first; ci < g.hi; ci += stride) {
    const int w = npeaks[ci];
    if (w <= 0) continue;
    const unsigned key = __float_as_uint(couts[ci].response);
    if ((key & fixed) == prefix) atomicAdd(&hist[(key >> shift) & (kSelectBins - 1)], w);
  }
}

__device__ __forceinline__ void select_mark(const CandOut* __restrict__ couts, int* npeaks, SelSeg g, int first,
                                            int stride, unsigned threshold) {
  for (long long ci = (long long)g.lo + first; ci < g.hi; ci += stride)
    if (npeaks[ci] > 0 && __float_as_uint(couts[ci].response) < threshold) npeaks[ci] = 0;
}

constexpr int kSelBlockT = 1024;
__global__ __launch_bounds__(kSelBlockT) void select_block_kernel(const CandOut* __restrict__ couts, int* npeaks,
                                                                 const int* __restrict__ img_cand_off, int cand_cap,
                                                                 int n_keep) {
  __shared__ int hist[kSelectBins];
  __shared__ SelShared s;
  const SelSeg g = select_segment(img_cand_off, blockIdx.x, cand_cap);
  const int tid = threadIdx.x;
  unsigned prefix = 0;
  int want = n_keep;
  for (int pass = 0; pass < kSelectPasses; ++pass) {
    if (tid < kSelectBins) hist[tid] = 0;
    __syncthreads();
    select_accumulate(couts, npeaks, g, tid, kSelBlockT, pass, prefix, hist);
    __syncthreads();
    int digit, rest, total;
    select_digit(hist, want, s, digit, rest, total);
    if (pass == 0 && total <= n_keep) return;  // K <= n: the image keeps everything
    prefix |= (unsigned)digit << (32 - kSelBits * (pass + 1));
    want = rest;
  }
  select_mark(couts, npeaks, g, tid, kSelBlockT, prefix);
}

// ---- the multi-workgroup form ---------------------------------------------------
// hist: [batch][kSelectPasses][kSelectBins] ints, zero before pass 0.
constexpr int kSelGridT = 256;
__global__ __launch_bounds__(kSelGridT) void select_zero_kernel(int* __restrict__ hist, int n) {
  const int i = blockIdx.x * kSelGridT + threadIdx.x;
  if (i < n) hist[i] = 0;
}

// The prefix and the wanted weight after passes 0..upto-1, from their finished
// histograms; false when the image keeps everything.
__device__ __forceinline__ bool select_chain(const int* H, int upto, int n_keep, SelShared& s, unsigned& prefix,
                                             int& want) {
  prefix = 0;
  want = n_keep;
  for (int p = 0; p < upto; ++p) {
    int digit, rest, total;
    select_digit(H + p * kSelectBins, want, s, digit, rest, total);
    if (p == 0 && total <= n_keep) return false;
    prefix |= (unsigned)digit << (32 - kSelBits * (p + 1));
    want = rest;
  }
  return true;
}

__global__ __launch_bounds__(kSelGridT) void select_hist_kernel(const CandOut* __restrict__ couts, const int* npeaks,
                                                                const int* __restrict__ img_cand_off, int cand_cap,
                                                                int n_keep, int* hist_all, int pass) {
  __shared__ int hist[kSelectBins];
  __shared__ SelShared s;
  const SelSeg g = select_segment(img_cand_off, blockIdx.y, cand_cap);
  const int first = blockIdx.x * kSelGridT;
  if (first >= g.hi - g.lo) return;  // no slot of this image for this workgroup
  int* H = hist_all + (size_t)blockIdx.y * kSelectPasses * kSelectBins;
  unsigned prefix;
  int want;
  if (!select_chain(H, pass, n_keep, s, prefix, want)) return;
  const int tid = threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
  select_accumulate(couts, npeaks, g, first + tid, (int)gridDim.x * kSelGridT, pass, prefix, hist);
  __syncthreads();
  if (hist[tid]) atomicAdd(&H[pass * kSelectBins + tid], hist[tid]);
}

__global__ __launch_bounds__(kSelGridT) void select_mark_kernel(const CandOut* __restrict__ couts, int* npeaks,
                                                                const int* __restrict__ img_cand_off, int cand_cap,
                                                                int n_keep, const int* hist_all) {
  __shared__ SelShared s;
  const SelSeg g = select_segment(img_cand_off, blockIdx.y, cand_cap);
  const int first = blockIdx.x * kSelGridT;
  if (first >= g.hi - g.lo) return;
  unsigned prefix;
  int want;
  if (!select_chain(hist_all + (size_t)blockIdx.y * kSelectPasses * kSelectBins, kSelectPasses, n_keep, s, prefix,
                    want))
    return;
  select_mark(couts, npeaks, g, first + (int)threadIdx.x, (int)gridDim.x * kSelGridT, prefix);
}

}  // namespace

void launch_select_best(hipStream_t st, DetectBufs& D, int batch, int n_keep, bool grid_form) {
  if (n_keep <= 0 || batch < 1) return;
  if (!grid_form) {
    hipLaunchKernelGGL(select_block_kernel, dim3(batch), dim3(kSelBlockT), 0, st, D.couts, D.npeaks, D.img_cand_off,
                       D.cand_cap, n_keep);
    return;
  }
  // eight strides of a workgroup over the whole list at most, 1024 workgroups per image at most
  const int gx = std::min(1024, std::max(1, (D.cand_cap + kSelGridT * 8 - 1) / (kSelGridT * 8)));
  const int words = batch * kSelectPasses * kSelectBins;
  hipLaunchKernelGGL(select_zero_kernel, dim3((words + kSelGridT - 1) / kSelGridT), dim3(kSelGridT), 0, st, D.sel_hist,
                     words);
  for (int pass = 0; pass < kSelectPasses; ++pass)
    hipLaunchKernelGGL(select_hist_kernel, dim3(gx, batch), dim3(kSelGridT), 0, st, D.couts, D.npeaks, D.img_cand_off,
                       D.cand_cap, n_keep, D.sel_hist, pass);
  hipLaunchKernelGGL(select_mark_kernel, dim3(gx, batch), dim3(kSelGridT), 0, st, D.couts, D.npeaks, D.img_cand_off,
                     D.cand_cap, n_keep, D.sel_hist);
}

}  // namespace sift
