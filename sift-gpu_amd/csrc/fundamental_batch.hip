// fundamental_batch.hip -- findFundamentalMat(FM_RANSAC) for every segment of
// the ratio stage's point pairs, on the device in stream order.
// The result equals find_fundamental_ransac (fundamental.hip) run per segment
// bit for bit: every expression comes from fundamental_math.hpp, and the three
// places where the serial algorithm depends on hypothesis order are replayed in
// that order by one lane, as in affine_batch.hip:
//   * the RNG stream -- lane 0 accepts a round of up to kFundRound subsets;
//   * the running best (good > max(max_good, 7), strict, in iteration order);
//   * the shrinking niters -- lane 0 walks the round's inlier counts.
// Between those points a round is independent work, one hypothesis per lane.
// The solve is the heavy part here (a normalised 8-point solve: a 9x9 and a 3x3
// cyclic Jacobi, A^T A and V in registers as in homog_ransac_kernel); the
// scoring follows the affine kernel: the nine float coefficients stay in VGPRs,
// the segment's pairs are walked as wave-uniform data (scalar loads), and the
// inlier count is a lane-private integer: no ballot, no model in memory.
// Hypotheses past the final niters are computed and dropped: nothing later
// consumes the RNG.
//
// One kernel, one workgroup of kFundRound threads per segment.  Its tail takes
// the best hypothesis's mask again from its model (the same floats, the same
// test), forms the refit's 4 + 2 + 45 sums as double chains in pair order -- the
// per-pair terms 64 pairs at a time in LDS, then one lane per accumulator adds
// its terms in order, skipping non-inliers: the chain the host runs over its
// compacted inliers -- and one lane finishes the solve.  No scratch: a round's
// subsets and counts live in LDS.
#include "common.hpp"
#include "fundamental_math.hpp"
#include "scratch.hpp"

namespace sift {

namespace {

using namespace fmath;

constexpr int kThreads = kFundRound;
constexpr int kChunk = 64;  // pairs whose refit terms are formed at once
constexpr int m = kModelPoints;
static_assert(kThreads % 64 == 0 && kThreads <= 1024 && kChunk <= kThreads && kProducts <= kThreads,
              "one thread per hypothesis / sum");

__device__ inline int clamp_off(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

// Ordered sums over the pairs with on(i): kAcc accumulators, accumulator a held
// by thread a.  terms(i, out) forms pair i's kAcc terms.  Returns thread a's
// sum (threads >= kAcc return 0).  affine_batch.hip's scheme, restated.
template <int kAcc, typename On, typename T>
__device__ inline double ordered_sums(double* s_terms, unsigned char* s_on, int n, On on, T terms) {
  const int tid = threadIdx.x;
  double acc = 0;
  for (int i0 = 0; i0 < n; i0 += kChunk) {
    if (tid < kChunk) {
      const int i = i0 + tid;
      const bool in = i < n && on(i);
      s_on[tid] = in;
      if (in) {
        double out[kAcc];
        terms(i, out);
#pragma unroll
        for (int a = 0; a < kAcc; ++a) s_terms[tid * kAcc + a] = out[a];
      }
    }
    __syncthreads();
    if (tid < kAcc) {
      const int cnt = n - i0 < kChunk ? n - i0 : kChunk;
      for (int k = 0; k < cnt; ++k)
        if (s_on[k]) acc += s_terms[k * kAcc + tid];
    }
    __syncthreads();
  }
  return acc;
}

__global__ __launch_bounds__(kThreads) void fund_ransac_kernel(
    const float* __restrict__ src_xy, const float* __restrict__ dst_xy, const int* __restrict__ moff, int m_cap,
    double thr, int max_iters, double confidence, int params_ok, double* __restrict__ F_out,
    int* __restrict__ found_out, unsigned char* __restrict__ mask_out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lo = clamp_off(moff[b], m_cap), hi = clamp_off(moff[b + 1], m_cap);
  const int n = hi > lo ? hi - lo : 0;
  double* Fb = F_out + (size_t)b * 9;

  __shared__ int s_sub[kFundRound * m], s_cnt[kFundRound];
  __shared__ int s_njobs, s_win, s_done, s_max_good, s_scaled;
  __shared__ double s_best[9], s_dist[kDists], s_sums[kProducts];
  __shared__ Norm s_norm;
  __shared__ double s_terms[kChunk * kProducts];
  __shared__ unsigned char s_on[kChunk];

  bool found = params_ok && n >= m;  // uniform
  if (found) {
    const P2* s = reinterpret_cast<const P2*>(src_xy) + lo;
    const P2* d = reinterpret_cast<const P2*>(dst_xy) + lo;
    const float t = hmath::inlier_limit(thr);
    // lane 0's serial state
    Rng rng{~0ull};
    int niters = max_iters, max_good = 0, base = 0;
    bool exhausted = false;  // getSubset gave up: no later hypothesis exists

    for (;;) {
      if (tid == 0) {  // the RNG stream: this round's subsets
        int njobs = 0;
        if (n == m) {
          for (int i = 0; i < m; ++i) s_sub[i] = i;
          njobs = 1;
        } else {
          const int want = niters - base < kFundRound ? niters - base : kFundRound;
          for (; njobs < want; ++njobs) {
            int idx[m];
            P2 ms[m], md[m];
            if (!get_subset8(rng, s, d, n, idx, ms, md)) {
              exhausted = true;
              break;
            }
#pragma unroll
            for (int i = 0; i < m; ++i) s_sub[njobs * m + i] = idx[i];
          }
        }
        s_njobs = njobs;
      }
      __syncthreads();
      const int njobs = s_njobs;
      // one 8-point solve per lane; a lane without a model scores NaNs, which no pair passes
      double F[9] = {0};
      float f[9];
      bool ok = false;
      if (tid < njobs) {
        P2 ms[m], md[m];
#pragma unroll
        for (int i = 0; i < m; ++i) {
          const int r = s_sub[tid * m + i];
          ms[i] = s[r];
          md[i] = d[r];
        }
        ok = solve<m>(ms, md, m, F);
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) f[k] = ok ? (float)F[k] : __builtin_nanf("");
      int good = 0;
      if (n > m) {  // score: the pairs by scalar loads, the hypothesis in this lane's registers
#pragma unroll 2
        for (int i = 0; i < n; ++i) {
          const P2 p = s[i], q = d[i];
          good += is_inlier(f, p.x, p.y, q.x, q.y, t);
        }
      }
      s_cnt[tid] = ok ? good : -1;
      __syncthreads();
      if (tid == 0) {  // the winner rule, in iteration order
        int win = -1, done = 0;
        if (n == m) {
          done = 1;
          if (s_cnt[0] >= 0) win = 0, max_good = m;
        } else {
          for (int h = 0; h < njobs; ++h) {
            if (base + h >= niters) break;
            const int g = s_cnt[h];
            if (g < 0) continue;
            if (wins(g, max_good)) {
              max_good = g;
              win = h;
              niters = hmath::update_num_iters(confidence, (double)(n - g) / n, m, niters);
            }
          }
          base += njobs;
          done = exhausted || base >= niters;
        }
        s_win = win;
        s_done = done;
        s_max_good = max_good;
      }
      __syncthreads();
      if (tid == s_win) {  // keep the round's last winner
#pragma unroll
        for (int k = 0; k < 9; ++k) s_best[k] = F[k];
      }
      if (s_done) break;
      __syncthreads();  // s_win / s_done are read before lane 0 writes the next round's
    }
    __syncthreads();
    found = s_max_good > 0;
  }

  if (!found) {  // none: F zeroed, a zero mask
    if (tid < 9) Fb[tid] = 0;
    if (tid == 0) found_out[b] = 0;
    if (mask_out)
      for (int i = tid; i < n; i += kThreads) mask_out[lo + i] = 0;
    return;
  }
  if (n > m) {  // the mask of the best hypothesis, then the same solve over it
    const P2* s = reinterpret_cast<const P2*>(src_xy) + lo;
    const P2* d = reinterpret_cast<const P2*>(dst_xy) + lo;
    const float t = hmath::inlier_limit(thr);
    const int count = s_max_good;
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = (float)s_best[k];
    auto on = [&](int i) { return is_inlier(f, s[i].x, s[i].y, d[i].x, d[i].y, t); };
    if (mask_out)
      for (int i = tid; i < n; i += kThreads) mask_out[lo + i] = on(i);
    const double c = ordered_sums<kCoords>(s_terms, s_on, n, on, [&](int i, double* out) {
#pragma unroll
      for (int a = 0; a < kCoords; ++a) out[a] = coord(s[i], d[i], a);
    });
    if (tid < kCoords) s_norm.c[tid] = c / count;
    __syncthreads();
    const double dist = ordered_sums<kDists>(s_terms, s_on, n, on,
                                             [&](int i, double* out) { dist_terms(s_norm.c, s[i], d[i], out); });
    if (tid < kDists) s_dist[tid] = dist;
    __syncthreads();
    if (tid == 0) {
      double k[kDists];
      const bool scaled = scale_finish(s_dist, count, k);
      if (scaled) s_norm.k[0] = k[0], s_norm.k[1] = k[1];
      s_scaled = scaled;
    }
    __syncthreads();
    if (s_scaled) {  // uniform
      const double sum = ordered_sums<kProducts>(s_terms, s_on, n, on,
                                                 [&](int i, double* out) { product_terms(s_norm, s[i], d[i], out); });
      if (tid < kProducts) s_sums[tid] = sum;
      __syncthreads();
      if (tid == 0) {
        double AtA[9][9], R[9];
        const Norm nm = s_norm;
        int q = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j)
#pragma unroll
          for (int k = 0; k < 9; ++k) AtA[j][k] = k >= j ? s_sums[q++] : 0;
        if (finish(nm, AtA, R)) {
#pragma unroll
          for (int k = 0; k < 9; ++k) s_best[k] = R[k];
        }
      }
    }
  } else if (mask_out && tid < m) {
    mask_out[lo + tid] = 1;
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) Fb[k] = s_best[k];
    found_out[b] = 1;
  }
}

}  // namespace

void launch_fundamental_seg(hipStream_t st, const float* src_xy, const float* dst_xy, const int* moff, int n_segments,
                            int m_cap, double thr, int max_iters, double confidence, double* F, int* found,
                            unsigned char* mask_out) {
  const int params_ok = confidence > 0 && confidence < 1 && max_iters >= 1;
  fund_ransac_kernel<<<n_segments, kThreads, 0, st>>>(src_xy, dst_xy, moff, m_cap, thr, max_iters, confidence,
                                                      params_ok, F, found, mask_out);
}

}  // namespace sift
