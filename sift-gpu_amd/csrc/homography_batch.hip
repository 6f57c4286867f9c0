// homography_batch.hip -- findHomography(RANSAC) for every segment of the
// ratio stage's point pairs, and perspectiveTransform of shared points by
// every segment's H, on the device in stream order.  The
// result equals find_homography_ransac (homography.hip) run per segment bit for
// bit: every expression comes from homography_math.hpp, and the three places
// where the serial algorithm depends on hypothesis order are replayed in that
// order by one lane:
//   * the RNG stream (cv::RNG(~0), duplicate rejection, check_subset retries,
//     the 10000-attempt limit) -- lane 0 accepts a round of kHomogRound subsets;
//   * the running best (good > max(max_good, 3), strict, in iteration order) and
//   * the shrinking niters (updated after each win; hypotheses at
//     iter >= niters do not exist) -- lane 0 walks the round's inlier counts.
// Between those points a round is independent work: kHomogRound lanes solve
// their 4-point DLTs (9x9 cyclic Jacobi, A and V in registers), then the
// workgroup scores every hypothesis against every pair (ballot + popcount).
// Hypotheses past the final niters are computed and dropped: nothing later
// consumes the RNG.
//
// Two kernels, one workgroup per segment each:
//   homog_ransac_kernel  rounds -> HomogState (best model, found, max_good) and
//                        the best hypothesis's inlier mask (scratch);
//   homog_refine_kernel  refit on the inliers, 10 LM steps, normalisation, the
//                        outputs.  Its sums over the inliers (centroid, scale,
//                        LtL; JtJ, Jtr, cost) are double chains in pair order:
//                        the per-pair terms are formed 64 pairs at a time in
//                        LDS, then one lane per accumulator adds its terms in
//                        order, skipping non-inliers -- the chain the host
//                        runs over its compacted arrays.
#include "common.hpp"
#include "homography_math.hpp"
#include "scratch.hpp"

namespace sift {

namespace {

using namespace hmath;

constexpr int kRansacThreads = 256;
constexpr int kRefineThreads = 128;
constexpr int kChunk = 64;  // pairs whose terms are formed at once (homog_refine_kernel)

__device__ inline int clamp_off(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

__global__ __launch_bounds__(kRansacThreads) void homog_ransac_kernel(
    const float* __restrict__ src_xy, const float* __restrict__ dst_xy, const int* __restrict__ moff, int m_cap,
    double thr, int max_iters, double confidence, int params_ok, int* __restrict__ subsets,
    double* __restrict__ models, int* __restrict__ counts, HomogState* __restrict__ state,
    unsigned char* __restrict__ mask) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lo = clamp_off(moff[b], m_cap), hi = clamp_off(moff[b + 1], m_cap);
  const int n = hi > lo ? hi - lo : 0;
  HomogState* st = state + b;
  if (!params_ok || n < 4) {  // the whole workgroup leaves
    if (tid == 0) st->found = 0, st->max_good = 0;
    return;
  }
  const P2* s = reinterpret_cast<const P2*>(src_xy) + lo;
  const P2* d = reinterpret_cast<const P2*>(dst_xy) + lo;
  int* sub = subsets + (size_t)b * kHomogRound * 4;
  double* mod = models + (size_t)b * kHomogRound * 9;
  int* cnt = counts + (size_t)b * kHomogRound;
  const float t = inlier_limit(thr);
  __shared__ int s_njobs, s_win, s_done;
  // lane 0's serial state
  Rng rng{~0ull};
  int niters = max_iters, max_good = 0, base = 0;
  bool exhausted = false;  // getSubset gave up: no later hypothesis exists

  for (;;) {
    if (tid == 0) {  // the RNG stream: this round's subsets
      int njobs = 0;
      if (n == 4) {
        for (int i = 0; i < 4; ++i) sub[i] = i;
        njobs = 1;
      } else {
        for (; njobs < kHomogRound; ++njobs) {
          int idx[4];
          P2 ms[4], md[4];
          if (!get_subset(rng, s, d, n, idx, ms, md)) {
            exhausted = true;
            break;
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) sub[njobs * 4 + i] = idx[i];
        }
      }
      s_njobs = njobs;
    }
    __syncthreads();
    const int njobs = s_njobs;
    if (tid < njobs) {  // one 4-point DLT per lane
      P2 ms[4], md[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = sub[tid * 4 + i];
        ms[i] = s[r];
        md[i] = d[r];
      }
      double H[9];
      const bool ok = run_kernel<4>(ms, md, 4, H);
      if (ok) {
#pragma unroll
        for (int k = 0; k < 9; ++k) mod[tid * 9 + k] = H[k];
      }
      cnt[tid] = ok ? 0 : -1;
    }
    __syncthreads();
    if (n > 4) {  // score: a wave per hypothesis, 64 pairs at a time
      for (int h = wave; h < njobs; h += kRansacThreads / 64) {
        if (cnt[h] < 0) continue;
        double H[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) H[k] = mod[h * 9 + k];
        int good = 0;
        for (int i0 = 0; i0 < n; i0 += 64) {
          const int i = i0 + lane;
          const bool in = i < n && is_inlier(H, s[i], d[i], t);
          good += __popcll(__ballot(in));
        }
        if (lane == 0) cnt[h] = good;
      }
    }
    __syncthreads();
    if (tid == 0) {  // the winner rule, in iteration order
      int win = -1, done = 0;
      if (n == 4) {
        done = 1;
        if (cnt[0] >= 0) win = 0, max_good = 4;
      } else {
        for (int h = 0; h < njobs; ++h) {
          if (base + h >= niters) break;
          const int good = cnt[h];
          if (good < 0) continue;
          if (wins(good, max_good)) {
            max_good = good;
            win = h;
            niters = update_num_iters(confidence, (double)(n - good) / n, 4, niters);
          }
        }
        base += njobs;
        done = exhausted || base >= niters;
      }
      s_win = win;
      s_done = done;
    }
    __syncthreads();
    const int win = s_win, done = s_done;
    if (win >= 0) {  // keep the round's last winner: its model and its mask
      if (tid < 9) st->best[tid] = mod[win * 9 + tid];
      if (n > 4) {
        double H[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) H[k] = mod[win * 9 + k];
        for (int i = tid; i < n; i += kRansacThreads) mask[lo + i] = is_inlier(H, s[i], d[i], t);
      }
    }
    if (done) break;
    __syncthreads();
  }
  if (tid == 0) st->found = max_good > 0, st->max_good = max_good;
}

// Ordered sums over the inliers: kAcc accumulators, accumulator a held by
// thread a.  terms(i, out) forms pair i's kAcc terms.  Returns thread a's sum
// (threads >= kAcc return 0).
template <int kAcc, typename F>
__device__ inline double ordered_sums(double* s_terms, unsigned char* s_on, const unsigned char* inl, int n, F terms) {
  const int tid = threadIdx.x;
  double acc = 0;
  for (int i0 = 0; i0 < n; i0 += kChunk) {
    if (tid < kChunk) {
      const int i = i0 + tid;
      const bool on = i < n && inl[i];
      s_on[tid] = on;
      if (on) {
        double out[kAcc];
        terms(i, out);
#pragma unroll
        for (int a = 0; a < kAcc; ++a) s_terms[tid * kAcc + a] = out[a];
      }
    }
    __syncthreads();
    if (tid < kAcc) {
      const int m = n - i0 < kChunk ? n - i0 : kChunk;
      for (int k = 0; k < m; ++k)
        if (s_on[k]) acc += s_terms[k * kAcc + tid];
    }
    __syncthreads();
  }
  return acc;
}

__global__ __launch_bounds__(kRefineThreads) void homog_refine_kernel(
    const float* __restrict__ src_xy, const float* __restrict__ dst_xy, const int* __restrict__ moff, int m_cap,
    int params_ok, const HomogState* __restrict__ state, const unsigned char* __restrict__ mask,
    double* __restrict__ H_out, int* __restrict__ found_out, unsigned char* __restrict__ mask_out) {
  static_assert(kLmSums <= kRefineThreads && kDltSums <= kRefineThreads && kChunk <= kRefineThreads, "one thread per sum");
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lo = clamp_off(moff[b], m_cap), hi = clamp_off(moff[b + 1], m_cap);
  const int n = hi > lo ? hi - lo : 0;
  const HomogState* st = state + b;
  double* Hb = H_out + (size_t)b * 9;
  if (!params_ok || n < 4 || !st->found) {  // none: H zeroed, the oracle's zero mask
    if (tid < 9) Hb[tid] = 0;
    if (tid == 0) found_out[b] = 0;
    if (mask_out)
      for (int i = tid; i < n; i += kRefineThreads) mask_out[lo + i] = 0;
    return;
  }
  if (n == 4) {  // the direct fit: no refit, no LM
    if (tid == 0) {
      double best[9];
      for (int k = 0; k < 9; ++k) best[k] = st->best[k];
      normalise_h(best, Hb);
      found_out[b] = 1;
    }
    if (mask_out && tid < 4) mask_out[lo + tid] = 1;
    return;
  }
  const P2* s = reinterpret_cast<const P2*>(src_xy) + lo;
  const P2* d = reinterpret_cast<const P2*>(dst_xy) + lo;
  const unsigned char* inl = mask + lo;
  const int count = st->max_good;  // the inliers of the best hypothesis

  __shared__ double s_terms[kChunk * (kLmSums > kDltSums ? kLmSums : kDltSums)];
  __shared__ unsigned char s_on[kChunk];
  __shared__ Norm s_norm;
  __shared__ double s_sums[kLmSums], s_H[9], s_Hn[9], s_A[8 * 9], s_dx[8];
  __shared__ int s_ok;

  if (tid < 9) s_H[tid] = st->best[tid];
  // refit: runKernel on the inliers
  if (tid < 4) {
    double c = 0;
    for (int i = 0; i < n; ++i)
      if (inl[i]) centroid_add(c, norm_coord(s[i], d[i], tid));
    centroid_finish(c, count);
    s_norm.c[tid] = c;
    double sp = 0;
    for (int i = 0; i < n; ++i)
      if (inl[i]) spread_add(sp, norm_coord(s[i], d[i], tid), c);
    s_norm.s[tid] = sp;
  }
  __syncthreads();
  if (tid == 0) s_ok = spread_finish(s_norm, count);
  __syncthreads();
  if (s_ok) {  // uniform
    const Norm nm = s_norm;
    const double sum = ordered_sums<kDltSums>(s_terms, s_on, inl, n, [&](int i, double* out) {
      double Lx[9], Ly[9];
      dlt_rows(nm, s[i], d[i], Lx, Ly);
      int a = 0;
#pragma unroll
      for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int k = j; k < 9; ++k) out[a++] = dlt_product(Lx, Ly, j, k);
    });
    if (tid < kDltSums) s_sums[tid] = sum;
    __syncthreads();
    if (tid == 0) {
      double LtL[9][9], refit[9];
      int a = 0;
#pragma unroll
      for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int k = j; k < 9; ++k) LtL[j][k] = s_sums[a++];
      if (dlt_finish(nm, LtL, refit)) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s_H[k] = refit[k];
      }
    }
  }
  __syncthreads();
  // Levenberg-Marquardt; lane 0 holds lambda and the cost
  double lambda = kLmLambda0;
  double c0 = ordered_sums<1>(s_terms, s_on, inl, n, [&](int i, double* out) { out[0] = lm_cost_term(s_H, s[i], d[i]); });
  for (int it = 0; it < kLmSteps; ++it) {
    const double sum = ordered_sums<kLmSums>(s_terms, s_on, inl, n, [&](int i, double* out) {
      double Jx[8], Jy[8], rx, ry;
      lm_rows(s_H, s[i], d[i], Jx, Jy, rx, ry);
#pragma unroll
      for (int a = 0; a < 8; ++a) {
#pragma unroll
        for (int c = 0; c < 8; ++c) out[a * 8 + c] = lm_jtj(Jx, Jy, a, c);
        out[64 + a] = lm_jtr(Jx, Jy, a, rx, ry);
      }
    });
    if (tid < kLmSums) s_sums[tid] = sum;
    __syncthreads();
    if (tid == 0) {
      s_ok = lm_solve(s_sums, s_sums + 64, lambda, s_A, s_dx);
      if (s_ok) lm_candidate(s_H, s_dx, s_Hn);
    }
    __syncthreads();
    if (!s_ok) break;  // uniform
    const double c1 = ordered_sums<1>(s_terms, s_on, inl, n, [&](int i, double* out) { out[0] = lm_cost_term(s_Hn, s[i], d[i]); });
    if (tid == 0) {
      const bool accepted = lm_accept(c1, c0);
      if (accepted) {
        for (int k = 0; k < 9; ++k) s_H[k] = s_Hn[k];
        c0 = c1;
      }
      lambda = lm_lambda_next(lambda, accepted);
    }
    __syncthreads();
  }
  if (tid == 0) {
    normalise_h(s_H, Hb);
    found_out[b] = 1;
  }
  if (mask_out)
    for (int i = tid; i < n; i += kRefineThreads) mask_out[lo + i] = inl[i];
}

__global__ void perspective_seg_kernel(const double* __restrict__ H, const int* __restrict__ found, int n_segments,
                                       const float* __restrict__ xy, int n_pts, float* __restrict__ out) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)n_segments * n_pts) return;
  const int b = (int)(g / n_pts), i = (int)(g % n_pts);
  float o[2] = {0.f, 0.f};
  if (found[b]) {
    double Hb[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Hb[k] = H[(size_t)b * 9 + k];
    perspective_point(Hb, xy[2 * i], xy[2 * i + 1], o);
  }
  out[2 * g] = o[0];
  out[2 * g + 1] = o[1];
}

// The libm-dependent site on the device's own pow / log (sift_selftest_math ops 8, 9).
__global__ __launch_bounds__(256) void update_num_iters_selftest_kernel(double confidence, const float* __restrict__ good,
                                                                         const float* __restrict__ n,
                                                                         float* __restrict__ out, int count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int g = (int)good[i], m = (int)n[i];
  out[i] = (float)update_num_iters(confidence, (double)(m - g) / m, 4, 2000);
}

}  // namespace

void launch_update_num_iters_selftest(hipStream_t st, double confidence, const float* good, const float* n, float* out,
                                      int count) {
  update_num_iters_selftest_kernel<<<(count + 255) / 256, 256, 0, st>>>(confidence, good, n, out, count);
}

void launch_homography_seg(hipStream_t st, const float* src_xy, const float* dst_xy, const int* moff, int n_segments,
                           int m_cap, double thr, int max_iters, double confidence, int* subsets, double* models,
                           int* counts, HomogState* state, unsigned char* mask, double* H, int* found,
                           unsigned char* mask_out) {
  const int params_ok = confidence > 0 && confidence < 1 && max_iters >= 1;
  homog_ransac_kernel<<<n_segments, kRansacThreads, 0, st>>>(src_xy, dst_xy, moff, m_cap, thr, max_iters, confidence,
                                                            params_ok, subsets, models, counts, state, mask);
  homog_refine_kernel<<<n_segments, kRefineThreads, 0, st>>>(src_xy, dst_xy, moff, m_cap, params_ok, state, mask, H,
                                                            found, mask_out);
}

void launch_perspective_seg(hipStream_t st, const double* H, const int* found, int n_segments, const float* xy,
                            int n_pts, float* out) {
  const long long total = (long long)n_segments * n_pts;
  perspective_seg_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(H, found, n_segments, xy, n_pts, out);
}

}  // namespace sift
