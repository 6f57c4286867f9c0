// pnp_batch.hip -- solvePnPRansac (P3P) for every segment of a batch's 3-D / 2-D
// rows, on the device in stream order.  The result equals
// solve_pnp_ransac (pnp.hip) run per segment bit for bit: every expression
// comes from pnp_math.hpp, and the three places where the serial algorithm
// depends on hypothesis order are replayed in that order by one lane, as in
// fundamental_batch.hip:
//   * the RNG stream -- lane 0 draws a round of up to kPnpRound subsets;
//   * the running best (good > max(max_good, 3), strict, in iteration order);
//   * the shrinking niters -- lane 0 walks the round's inlier counts.
// Between those points a round is independent work, one hypothesis per lane: a
// P3P solve (a 3 x 3 Jacobi, a bisected cubic, up to four depth refinements) on
// the lane's four rows, then the score: the pose stays in the lane's registers,
// the segment's rows are walked as wave-uniform data (scalar loads of three
// doubles, two floats and the mask byte), and the inlier count is a lane-private
// integer: no ballot, no model in memory.  Hypotheses past the final niters are
// computed and dropped: nothing later consumes the RNG.
//
// One kernel, one workgroup of kPnpRound threads per segment; the segment's K
// and K^-1 are formed once into LDS.  The tail takes the best hypothesis's mask
// again from its pose (the same doubles, the same test), counts nothing new,
// and runs the refit: per Gauss-Newton step the 28 per-row terms 64 rows at a
// time in LDS, one lane per accumulator adding its terms in row order and
// skipping non-inliers -- the chain the host runs --, and one lane solves the
// 6 x 6 and judges the step.  No scratch: a round's subsets and counts live in
// LDS.
#include "common.hpp"
#include "pnp_math.hpp"
#include "scratch.hpp"

namespace sift {

namespace {

using namespace pnpmath;

constexpr int kThreads = kPnpRound;
constexpr int kChunk = 64;  // rows whose refit terms are formed at once
constexpr int m = kModelPoints;
static_assert(kThreads % 64 == 0 && kThreads <= 1024 && kChunk <= kThreads && kRefitSums <= kThreads,
              "one thread per hypothesis / sum");

__device__ inline int clamp_off(int v, int cap) { return v < 0 ? 0 : (v > cap ? cap : v); }

// Ordered sums over the rows with on(i): kAcc accumulators, accumulator a held
// by thread a.  terms(i, out) forms row i's kAcc terms.  Returns thread a's
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

__global__ __launch_bounds__(kThreads) void pnp_ransac_kernel(
    const double* __restrict__ xyz_all, const float* __restrict__ xy_all, const int* __restrict__ moff, int m_cap,
    const unsigned char* __restrict__ row_mask, const double* __restrict__ K_all, int k_stride, double thr,
    int max_iters, double confidence, int params_ok, double* __restrict__ pose_out, int* __restrict__ found_out,
    int* __restrict__ n_inliers_out, unsigned char* __restrict__ mask_out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int lo = clamp_off(moff[b], m_cap), hi = clamp_off(moff[b + 1], m_cap);
  const int n = hi > lo ? hi - lo : 0;
  const double* xyz = xyz_all + (size_t)lo * 3;
  const P2* pix = reinterpret_cast<const P2*>(xy_all) + lo;
  const unsigned char* on = row_mask ? row_mask + lo : nullptr;
  double* Pb = pose_out + (size_t)b * 12;

  __shared__ int s_sub[kPnpRound * m], s_cnt[kPnpRound];
  __shared__ int s_njobs, s_win, s_done, s_max_good, s_calibrated, s_go;
  __shared__ Calib s_cal;
  __shared__ double s_best[12], s_cur[12], s_cand[12], s_held[kRefitSums], s_sums[kRefitSums];
  __shared__ double s_terms[kChunk * kRefitSums];
  __shared__ unsigned char s_on[kChunk];

  if (tid == 0) {
    s_calibrated = calibrate(K_all + (size_t)b * k_stride, s_cal);
    s_max_good = 0;
  }
  __syncthreads();
  bool found = params_ok && n >= m && s_calibrated;  // uniform
  const double t2 = inlier_limit(thr);
  if (found) {
    // lane 0's serial state
    Rng rng{~0ull};
    int niters = max_iters, max_good = 0, base = 0;

    for (;;) {
      if (tid == 0) {  // the RNG stream: this round's subsets
        int njobs = 0;
        if (n == m) {
#pragma unroll
          for (int i = 0; i < m; ++i) s_sub[i] = i;
          njobs = 1;
        } else {
          const int want = niters - base < kPnpRound ? niters - base : kPnpRound;
          for (; njobs < want; ++njobs) {
            int idx[m];
            draw_subset(rng, n, idx);
#pragma unroll
            for (int i = 0; i < m; ++i) s_sub[njobs * m + i] = idx[i];
          }
        }
        s_njobs = njobs;
      }
      __syncthreads();
      const int njobs = s_njobs;
      // one hypothesis per lane; a lane without a model scores NaNs, which no row passes
      double P[12];
      bool ok = false;
      if (tid < njobs) {
        double x[12];
        P2 p[m];
        ok = true;
#pragma unroll
        for (int i = 0; i < m; ++i) {
          const int r = s_sub[tid * m + i];
          if (on && !on[r]) ok = false;
#pragma unroll
          for (int k = 0; k < 3; ++k) x[3 * i + k] = xyz[(size_t)r * 3 + k];
          p[i] = pix[r];
        }
        if (ok) ok = hypothesis(s_cal, x, p, P);
      }
      if (!ok) {
#pragma unroll
        for (int k = 0; k < 12; ++k) P[k] = __builtin_nan("");
      }
      int good = 0;
      if (n > m) {  // score: the rows by scalar loads, the hypothesis in this lane's registers
        double Kr[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) Kr[k] = s_cal.K[k];
        for (int i = 0; i < n; ++i) {
          const double x[3] = {xyz[(size_t)i * 3], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2]};
          const bool in = is_inlier(Kr, P, x, pix[i], t2);
          good += (on && !on[i]) ? 0 : (int)in;
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
            if (hmath::wins(g, max_good)) {
              max_good = g;
              win = h;
              niters = hmath::update_num_iters(confidence, (double)(n - g) / n, m, niters);
            }
          }
          base += njobs;
          done = base >= niters;
        }
        s_win = win;
        s_done = done;
        s_max_good = max_good;
      }
      __syncthreads();
      if (tid == s_win) {  // keep the round's last winner
#pragma unroll
        for (int k = 0; k < 12; ++k) s_best[k] = P[k];
      }
      if (s_done) break;
      __syncthreads();  // s_win / s_done are read before lane 0 writes the next round's
    }
    __syncthreads();
    found = s_max_good > 0;
  }

  if (!found) {  // none: a pose of zeros, a zero mask
    if (tid < 12) Pb[tid] = 0;
    if (tid == 0) found_out[b] = 0, n_inliers_out[b] = 0;
    if (mask_out)
      for (int i = tid; i < n; i += kThreads) mask_out[lo + i] = 0;
    return;
  }
  if (n > m) {  // the mask of the best hypothesis, then the refit over it
    double Kr[9], Pw[12];
#pragma unroll
    for (int k = 0; k < 9; ++k) Kr[k] = s_cal.K[k];
#pragma unroll
    for (int k = 0; k < 12; ++k) Pw[k] = s_best[k];
    auto in = [&](int i) { return !(on && !on[i]) && is_inlier(Kr, Pw, xyz + (size_t)i * 3, pix[i], t2); };
    if (mask_out)
      for (int i = tid; i < n; i += kThreads) mask_out[lo + i] = in(i);
    if (tid < 12) s_cur[tid] = s_best[tid];
    __syncthreads();
    double sum = ordered_sums<kRefitSums>(s_terms, s_on, n, in, [&](int i, double* out) {
      refit_terms(s_cal.Ki, s_cur, xyz + (size_t)i * 3, pix[i], out);
    });
    if (tid < kRefitSums) s_held[tid] = sum;
    __syncthreads();
#pragma unroll 1
    for (int step = 0; step < kRefitSteps; ++step) {
      if (tid == 0) {
        double held[kRefitSums], cur[12], cand[12];
#pragma unroll
        for (int k = 0; k < kRefitSums; ++k) held[k] = s_held[k];
#pragma unroll
        for (int k = 0; k < 12; ++k) cur[k] = s_cur[k];
        const bool go = refit_candidate(held, cur, cand);
        if (go) {
#pragma unroll
          for (int k = 0; k < 12; ++k) s_cand[k] = cand[k];
        }
        s_go = go;
      }
      __syncthreads();
      if (!s_go) break;  // uniform
      sum = ordered_sums<kRefitSums>(s_terms, s_on, n, in, [&](int i, double* out) {
        refit_terms(s_cal.Ki, s_cand, xyz + (size_t)i * 3, pix[i], out);
      });
      if (tid < kRefitSums) s_sums[tid] = sum;
      __syncthreads();
      const bool keep = refit_accept(s_sums[kRefitSums - 1], s_held[kRefitSums - 1]);  // uniform
      __syncthreads();  // every lane has read the two costs
      if (!keep) break;
      if (tid < 12) s_cur[tid] = s_cand[tid];
      if (tid < kRefitSums) s_held[tid] = s_sums[tid];
      __syncthreads();
    }
    if (tid == 0) {
      double cur[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) cur[k] = s_cur[k];
      if (finite_n(cur, 12)) {
#pragma unroll
        for (int k = 0; k < 12; ++k) s_best[k] = cur[k];
      }
    }
  } else if (mask_out && tid < m) {
    mask_out[lo + tid] = 1;
  }
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 12; ++k) Pb[k] = s_best[k];
    found_out[b] = 1;
    n_inliers_out[b] = s_max_good;
  }
}

}  // namespace

void launch_pnp_seg(hipStream_t st, const double* xyz, const float* xy, const int* moff, int n_segments, int m_cap,
                    const unsigned char* row_mask, const double* K, int k_per_segment, double thr, int max_iters,
                    double confidence, double* pose, int* found, int* n_inliers, unsigned char* mask_out) {
  const int params_ok = confidence > 0 && confidence < 1 && max_iters >= 1;
  pnp_ransac_kernel<<<n_segments, kThreads, 0, st>>>(xyz, xy, moff, m_cap, row_mask, K, k_per_segment ? 9 : 0, thr,
                                                     max_iters, confidence, params_ok, pose, found, n_inliers,
                                                     mask_out);
}

}  // namespace sift
