// orient.hip -- orientation assignment (calcOrientationHist and the peaks,
// reference src/sift.cpp:389-451, 524-541): the batch kernel and the one-image
// kernel.
#include <float.h>
#include <stdlib.h>

#include <algorithm>

#include "detect_args.hpp"

namespace sift {

// Orientation: the batch kernel (orient_slots_kernel below) gives each 8-lane
// group candidates; lanes 8g..8g+7 of a group add their samples to the
// group's 36-bin histograms in raster order, lane q at step q.
constexpr int kOGrp = 8;

__device__ __forceinline__ int ori_radius(float size, int o) {
  const float scl = size * 0.5f / (1 << o);
  return cv_round(3 * 1.5f * scl);
}

// Orientation histograms, one wave per candidate, bins bucketed (round 4;
// the one-image path).
//
// The reference's only ordering constraint (src/sift.cpp:429-437) is that each
// bin receives its terms in window raster order; different bins are
// independent chains.  The batch kernel walks a window one sample per step
// (8 samples per batch, each added after the previous one's LDS round trip),
// so a radius-17 window is a 1,225-step chain and one image's launch is as
// long as its longest such walk.  Here a wave takes a candidate and 64
// consecutive raster samples per batch: every lane forms its sample's bin and
// value, the wave ranks each sample among the earlier samples of the same bin
// (a 6-bit match over ballots), scatters the value to [rank][bin] in LDS, and
// lane b (b < 36) then adds its bin's values in rank order into a register
// accumulator that runs across the batches.  The chain is now the largest
// per-batch bin count, summed over the batches, and every bin still gets
// exactly the reference's adds in the reference's order.  Invalid samples
// (outside the image interior, src/sift.cpp:405,410) join no bin; the masked
// reads past a bin's count add +0.0 to a sum that is >= +0 (exact no-op).
// (A per-XCD dynamic candidate fetch was bit-exact and 16 % slower: each
// draw is a returning atomic that sits in vmcnt order ahead of the
// candidate's gathers; tools/patches/r5_variants.patch.)
//
// One wave (one workgroup) per candidate slot: the dispatcher hands the next
// candidate to whichever slot frees, instead of a fixed stride per resident
// wave (round 4's form: tools/patches/detect_split_variants.patch).
__global__ __launch_bounds__(64) void orient_bin_kernel(RefArgs A) {
  __shared__ float vals[64][kOriBins];  // [rank][bin]: owner reads are conflict free
  __shared__ int cnt[64];
  __shared__ float hist[kOriBins + 4], sm[kOriBins + 4];
  const int lane = threadIdx.x;
  int n = *A.cand_total;
  if (n > A.cand_cap) n = A.cand_cap;
  const ExpConsts ek = A.mc->e;
  const float etab_lane = A.mc->exptab[lane];
  const unsigned long long below = (1ull << lane) - 1ull;
  cnt[lane] = 0;
  const int ci = blockIdx.x;
  if (ci < n) {
    const CandOut& co = A.couts[ci];
    if (co.npeaks == 0) {  // refinement rejected it
      if (lane == 0) A.npeaks[ci] = 0;
      return;
    }
    const int o = A.cands[ci].ol & 255;
    const Octave& O = A.L.oct[o];
    const int pitch = O.pitch, rr = co.ref_r, rc = co.ref_c;
    // ---- calcOrientationHist, src/sift.cpp:389-437 ----
    const float scl = co.size * 0.5f / (1 << o);
    const int radius = cv_round(3 * 1.5f * scl);
    const float sigma = 1.5f * scl;
    const float escale = -1.f / (2.f * sigma * sigma);
    const float2* gwin = A.grad + co.img * A.L.g_img + O.g_off[co.ref_layer];
    const int D = 2 * radius + 1;
    // the window's valid rectangle (y in [1, rows - 2], x in [1, cols - 2],
    // src/sift.cpp:405,410): the pixels the reference skips are not
    // enumerated, so the rest keep their raster order and a sample needs no
    // range test (a kept candidate lies >= 5 px inside, so the rectangle is
    // >= min(rad + 5, cols - 2) >= 9 columns wide)
    const int i0 = max(0, 1 - rr + radius), i1 = min(D - 1, O.rows - 2 - rr + radius);
    const int j0 = max(0, 1 - rc + radius), j1 = min(D - 1, O.cols - 2 - rc + radius);
    const int W = max(j1 - j0 + 1, 1), ns = max(j1 - j0 + 1, 0) * max(i1 - i0 + 1, 0);
    // lane's sample index base + lane as (si, sj) of the window, moved on by
    // 64 = q W + rem per batch
    int si = i0 + lane / W, sj = j0 + lane - (lane / W) * W;
    const int q64 = 64 / W, r64 = 64 - q64 * W, jend = j0 + W;
    float acc = 0.f;  // lane b < 36: bin b's running sum
    // the batch at (si, sj): validity and the gather (issued one batch ahead,
    // so its latency runs under the previous batch's bucketing)
    auto gather = [&](int base_, bool& ok_, float2& mo_) {
      const int y = rr + si - radius, x = rc + sj - radius;
      ok_ = base_ + lane < ns;
      mo_ = gwin[ok_ ? (long long)y * pitch + x : (long long)rr * pitch + rc];  // (Mag, Ori)
    };
    auto step64 = [&]() {
      si += q64;
      sj += r64;
      if (sj >= jend) {
        sj -= W;
        ++si;
      }
    };
    bool ok_n;
    float2 mo_n;
    gather(0, ok_n, mo_n);
    for (int base = 0; base < ns; base += 64) {
      const int i = si - radius, j = sj - radius;
      const bool ok = ok_n;
      const float2 mo = mo_n;
      step64();
      if (base + 64 < ns) gather(base + 64, ok_n, mo_n);
      // |argument| <= 2 * 17^2 / (2 * 2.85^2) < 36: exp32f's input clamp never acts
      const float wgt = exp32f_v<false>((i * i + j * j) * escale, etab_lane, ek);
      // Ori in [0, 360]: bin in [0, 36], the reference's wraps reduce to 36 -> 0
      const int bin = cv_round((kOriBins / 360.f) * mo.y);
      const float val = wgt * mo.x;
      const int key = ok ? (bin != kOriBins ? bin : 0) : 63;
      // lanes with the same key: match over the key's 6 bits
      unsigned long long m = ~0ull;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const unsigned long long bk = __ballot((key >> k) & 1);
        m &= ((key >> k) & 1) ? bk : ~bk;
      }
      const int rank = __popcll(m & below), total = __popcll(m);
      if (ok) {
        vals[rank][key] = val;
        if (rank == total - 1) cnt[key] = total;
      }
      wave_sync();
      int c = 0;
      if (lane < kOriBins) {
        c = cnt[lane];
        cnt[lane] = 0;
      }
      // bin lane's values in rank (= raster) order, 4 reads in flight
      for (int r = 0; __ballot(r < c); r += 4) {
        float v4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v4[u] = (r + u < c) ? vals[r + u][lane] : 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = acc + v4[u];
      }
      wave_sync();
    }
    // ---- smoothing (src/sift.cpp:440-451), max, peaks (src/sift.cpp:524-541) ----
    if (lane < kOriBins) hist[lane] = acc;
    wave_sync();
    float h = -1.f;
    if (lane < kOriBins) {
      const float* th = hist;
      const int t = lane;
      const int jm2 = (t + kOriBins - 2) % kOriBins, jp2 = (t + 2) % kOriBins;
      const int jm1 = (t + kOriBins - 1) % kOriBins, jp1 = (t + 1) % kOriBins;
      h = (th[jm2] + th[jp2]) * (1.f / 16.f) + (th[jm1] + th[jp1]) * (4.f / 16.f) + th[t] * (6.f / 16.f);
      sm[t] = h;
    }
    float mx = h;
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) mx = fmaxf(mx, __shfl_xor(mx, k));
    wave_sync();
    const float mag_thr = (float)(mx * 0.8f);
    bool pk = false;
    float ang = 0.f;
    if (lane < kOriBins) {
      const int t = lane;
      const int l = t > 0 ? t - 1 : kOriBins - 1;
      const int r2 = t < kOriBins - 1 ? t + 1 : 0;
      const float hl = sm[l], hr = sm[r2];
      if (h > hl && h > hr && h >= mag_thr) {
        float bn = t + 0.5f * (hl - hr) / (hl - 2 * h + hr);
        bn = bn < 0 ? kOriBins + bn : bn >= kOriBins ? bn - kOriBins : bn;
        float a = 360.f - (float)((360.f / kOriBins) * bn);
        if (fabsf(a - 360.f) < FLT_EPSILON) a = 0.f;
        ang = a;
        pk = true;
      }
    }
    const unsigned long long pmask = __ballot(pk);
    CandOut* cw = A.couts + ci;
    if (pk) cw->angle[__popcll(pmask & below)] = ang;
    if (lane == 0) A.npeaks[ci] = __popcll(pmask);
  }
}

// Orientation histograms, kOSlots candidates per lane group (default kernel).
//
// One candidate per group (round 1's orient_kernel) is bound by its histogram
// chain: a group's 8 samples of a batch are applied one after the other (each read-modify-write waits for the
// previous one's LDS round trip, ~100 cycles), and a wave's run time is the
// sum of its chains, which more resident waves cannot shorten.  Here each
// group carries kOSlots candidates at once -- 8 x kOSlots per wave -- with one
// histogram each, so every step of the chain issues kOSlots independent reads,
// one wait, kOSlots adds and kOSlots writes: the same ordered sums, kOSlots
// chains in flight per wave.  The gathers of the next batch are issued before
// the current batch's chain (software pipeline).  Lane q of a group adds its
// sample at step q, as before, so every bin receives its terms in the
// reference's raster order (src/sift.cpp:429-437); an invalid sample adds +0.0
// to bin 0 (exact no-op: every bin is >= +0).
template <int kOSlots>
#ifndef SIFT_ORIENT_WPE
#define SIFT_ORIENT_WPE 6  // A/B builds only (tools/build_var.sh): waves per SIMD orient_slots_kernel<2> is budgeted for
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kOSlots == 2 ? SIFT_ORIENT_WPE : 1))) void orient_slots_kernel(
    RefArgs A) {
  constexpr int SB = kOGrp * kOSlots;   // candidates per sub-batch
  constexpr int NSB = 64 / SB;          // sub-batches per ranked chunk
  constexpr int CH = NSB * SB;          // candidates per ranked chunk (<= 64: one per lane)
  __shared__ float oh[kOSlots][kOGrp][kOriBins + 4];
  __shared__ float sm[kOGrp][kOriBins + 4];
  __shared__ int sord[SB];
  __shared__ float etab[64];  // exp32f table, LDS-resident (gathered per sample)
  const int lane = threadIdx.x & 63;
  const int g = lane >> 3, q = lane & 7;
  int n = *A.cand_total;
  if (n > A.cand_cap) n = A.cand_cap;
  const ExpConsts ek = A.mc->e;
  etab[lane] = A.mc->exptab[lane];
  wave_sync();

  // XCD-aware contiguous split of the raster-ordered candidates (speed only)
  const int xcd = blockIdx.x & 7, nslot = gridDim.x >> 3, wslot = blockIdx.x >> 3;
  const int per = ((n + 7) / 8 + CH - 1) / CH * CH;
  const int c0 = xcd * per;
  const int cend = min(n, (xcd + 1) * per);
  const int chend = c0 + (max(cend - c0, 0) + CH - 1) / CH * CH;
  for (int cb = c0 + wslot * SB; cb < chend; cb += nslot * SB) {
    // lane balance: the chunk's CH candidates ranked by window radius, this
    // sub-batch takes SB consecutive ranks (XOR with the pass index: no wave
    // always draws the largest)
    const int rel = (cb - c0) / SB, pass = rel / nslot;
    const int kc = c0 + (rel / NSB) * CH, win = ((rel % NSB) ^ (pass % NSB)) * SB;
    {
      const int kk = kc + lane;
      int key = 0x1ffffff;  // past the end: ranked last
      if (lane < CH && kk < cend) {
        const CandOut& co = A.couts[kk];
        key = co.npeaks ? min(max(ori_radius(co.size, A.cands[kk].ol & 255), 0), 0xffffff) : 0;
      }
      key = (key << 6) | lane;
      int rank = 0;
#pragma unroll
      for (int m = 0; m < 64; ++m) rank += __builtin_amdgcn_readlane(key, m) < key ? 1 : 0;
      if (rank >= win && rank < win + SB) sord[rank - win] = kk;
      wave_sync();
    }
    // per slot: the window's top-left gradient address (gwin, pitch) and the
    // sample walk (si, sj) over the window's valid rectangle -- interior
    // pixels only, src/sift.cpp:405,410, the pixels the reference skips are
    // never enumerated, so the raster order of the rest is unchanged and a
    // sample needs no per-pixel range test: [j0, jend) x rows from si
    int radius[kOSlots], ns[kOSlots], Dw[kOSlots], si[kOSlots], sj[kOSlots], pitch[kOSlots], jend[kOSlots];
    float escale[kOSlots];
    const float2* gwin[kOSlots];
    int nmax = 0;
#pragma unroll
    for (int u = 0; u < kOSlots; ++u) {
      const int ci = sord[u * kOGrp + g];
      bool ok = false;
      int o = 0, rl = 0, b = 0, rr = 0, rc = 0;
      float size = 0.f;
      if (ci < cend) {
        const CandOut& co = A.couts[ci];
        ok = co.npeaks != 0;
        o = A.cands[ci].ol & 255;
        size = co.size;
        rr = co.ref_r;
        rc = co.ref_c;
        rl = co.ref_layer;
        b = co.img;
      }
      const Octave& O = A.L.oct[o];
      pitch[u] = (int)O.pitch;
      // ---- calcOrientationHist setup, src/sift.cpp:389-402 ----
      const float scl = size * 0.5f / (1 << o);
      const int rad = ok ? cv_round(3 * 1.5f * scl) : 0;
      radius[u] = rad;
      const float sigma = 1.5f * scl;
      escale[u] = -1.f / (2.f * sigma * sigma);
      // (rr, rc) is an interior pixel (refinement keeps it >= 5 from the
      // border), so the window centre is a valid address for every slot
      gwin[u] = A.grad + b * A.L.g_img + O.g_off[ok ? rl : 0] + (long long)(rr - rad) * pitch[u] + (rc - rad);
      const int D = 2 * rad + 1;
      // y = rr + si - rad in [1, rows - 2], x = rc + sj - rad in [1, cols - 2]
      const int i0 = max(0, 1 - rr + rad), i1 = min(D - 1, O.rows - 2 - rr + rad);
      const int j0 = max(0, 1 - rc + rad), j1 = min(D - 1, O.cols - 2 - rc + rad);
      const int wv = j1 - j0 + 1, hv = i1 - i0 + 1;
      ns[u] = ok && wv > 0 && hv > 0 ? wv * hv : 0;
      // a kept candidate lies >= 5 px inside its octave (cols >= 11) and
      // rad = cvRound(4.5 scl) >= 8, so wv >= min(rad + 5, cols - 2) >= 9 > 8:
      // one advance wraps at most once; rejected: never wraps
      Dw[u] = ns[u] ? wv : 0x40000000;
      jend[u] = ns[u] ? j1 + 1 : 0x40000000;
      // lane q walks samples s = q, q+8, ... as (row si, column sj) of the rectangle
      si[u] = i0;
      sj[u] = j0 + q;
      while (sj[u] >= jend[u]) {
        sj[u] -= Dw[u];
        ++si[u];
      }
      nmax = max(nmax, ns[u]);
      for (int t = q; t < kOriBins; t += 8) oh[u][g][t] = 0.f;
    }
    int okbits = 0;  // slot u's candidate is kept (bit u): read by the epilogue's rolled loop
#pragma unroll
    for (int u = 0; u < kOSlots; ++u) okbits |= ns[u] > 0 ? 1 << u : 0;
    nmax = max(nmax, __shfl_xor(nmax, 8));
    nmax = max(nmax, __shfl_xor(nmax, 16));
    nmax = max(nmax, __shfl_xor(nmax, 32));
    wave_sync();
    // one batch (one sample per lane and slot): the gather, branch-free (the
    // window centre for an invalid sample), and the weight W = exp32f, which
    // depends on the position only (src/sift.cpp:424); w = -1 marks an invalid
    // sample (exp32f > 0 for every window position)
    float2 mo[kOSlots];
    float wt[kOSlots];
    auto fetch = [&](int base) {
#pragma unroll
      for (int u = 0; u < kOSlots; ++u) {
        const int i = si[u] - radius[u], j = sj[u] - radius[u];
        const bool okv = base + q < ns[u];
        // 24-bit products, 32-bit offsets (full-rate VALU; a window's offsets are < 2^31)
        mo[u] = gwin[u][(unsigned)(okv ? __mul24(si[u], pitch[u]) + sj[u] : __mul24(radius[u], pitch[u] + 1))];  // (Mag, Ori)
        // |argument| <= 2 * 17^2 / (2 * 2.85^2) < 36: exp32f's input clamp never acts
        const float w = exp32f<false>((__mul24(i, i) + __mul24(j, j)) * escale[u], etab, ek);
        wt[u] = okv ? w : -1.f;
        sj[u] += 8;  // at most one wrap (above)
        if (sj[u] >= jend[u]) {
          sj[u] -= Dw[u];
          ++si[u];
        }
      }
    };
    if (nmax > 0) fetch(0);
    for (int base = 0; base < nmax; base += 8) {
      int bin[kOSlots];
      float val[kOSlots];
#pragma unroll
      for (int u = 0; u < kOSlots; ++u) {
        // src/sift.cpp:426-432: Ori = fastAtan2 (precomputed), bin, W * Mag
        // Ori in [0, 360] (fastAtan2 of this library's gradients) puts bn in
        // [0, 36]: the reference's two wraps reduce to 36 -> 0, folded into
        // the validity select
        const int bn = cv_round((kOriBins / 360.f) * mo[u].y);
        const bool okv = wt[u] > 0.f;
        bin[u] = okv && bn != kOriBins ? bn : 0;
        val[u] = okv ? wt[u] * mo[u].x : 0.f;
      }
      if (base + 8 < nmax) fetch(base + 8);  // next batch's gathers fly during this chain
      // step jj: lane jj of every group adds its kOSlots samples into the
      // slots' histograms (kOSlots independent rows: reads, one wait, adds,
      // writes); the wave's LDS operations stay in program order, so step
      // jj + 1 reads what step jj wrote.  Each step tests a fresh opaque copy
      // of q behind a compiler barrier: with plain q == jj guards -- eight
      // mutually exclusive blocks for one thread -- hipcc rebuilt the steps as
      // a switch on q and ran them out of order (measured: 3 % of the angles
      // a few ulps off).  (A branch-free form, the other lanes updating a
      // scratch word, measured 1.54 ms against 1.42: its scratch accesses
      // share banks with the histogram rows.)
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        int qv = q;
        asm volatile("; orient step %1" : "+v"(qv) : "n"(jj) : "memory");
        if (qv == jj) {
          float h[kOSlots];
#pragma unroll
          for (int u = 0; u < kOSlots; ++u) h[u] = oh[u][g][bin[u]];
#pragma unroll
          for (int u = 0; u < kOSlots; ++u) oh[u][g][bin[u]] = h[u] + val[u];
        }
      }
    }
    wave_sync();
#pragma unroll 1
    for (int u = 0; u < kOSlots; ++u) {
      // smoothing (src/sift.cpp:440-451), max, peaks (src/sift.cpp:524-541)
      float mx = -1.f;
      for (int t = q; t < kOriBins; t += 8) {
        const float* th = oh[u][g];
        const int jm2 = (t + kOriBins - 2) % kOriBins, jp2 = (t + 2) % kOriBins;
        const int jm1 = (t + kOriBins - 1) % kOriBins, jp1 = (t + 1) % kOriBins;
        const float h = (th[jm2] + th[jp2]) * (1.f / 16.f) + (th[jm1] + th[jp1]) * (4.f / 16.f) +
                        th[t] * (6.f / 16.f);
        sm[g][t] = h;
        mx = fmaxf(mx, h);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 1));
      mx = fmaxf(mx, __shfl_xor(mx, 2));
      mx = fmaxf(mx, __shfl_xor(mx, 4));
      wave_sync();
      const float mag_thr = (float)(mx * 0.8f);
      unsigned long long pmask = 0;
      float ang[5];
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        const int t = q + 8 * m;
        ang[m] = 0.f;
        if (t < kOriBins && ((okbits >> u) & 1)) {
          const int l = t > 0 ? t - 1 : kOriBins - 1;
          const int r2 = t < kOriBins - 1 ? t + 1 : 0;
          const float h = sm[g][t], hl = sm[g][l], hr = sm[g][r2];
          if (h > hl && h > hr && h >= mag_thr) {
            float bn = t + 0.5f * (hl - hr) / (hl - 2 * h + hr);
            bn = bn < 0 ? kOriBins + bn : bn >= kOriBins ? bn - kOriBins : bn;
            float a = 360.f - (float)((360.f / kOriBins) * bn);
            if (fabsf(a - 360.f) < FLT_EPSILON) a = 0.f;
            ang[m] = a;
            pmask |= 1ull << t;
          }
        }
      }
      pmask |= __shfl_xor(pmask, 1);
      pmask |= __shfl_xor(pmask, 2);
      pmask |= __shfl_xor(pmask, 4);
      const int ci = sord[u * kOGrp + g];
      if (ci < cend) {
        CandOut* co = A.couts + ci;
#pragma unroll
        for (int m = 0; m < 5; ++m) {
          const int t = q + 8 * m;
          if (t < kOriBins && ((pmask >> t) & 1ull))
            co->angle[__popcll(pmask & ((1ull << t) - 1ull))] = ang[m];
        }
        // co->npeaks keeps the refine pass's kept flag (other waves rank
        // their chunk from it); the peak count goes to A.npeaks only
        const int np = ((okbits >> u) & 1) ? __popcll(pmask) : 0;
        if (q == 0) A.npeaks[ci] = np;
      }
      wave_sync();
    }
  }
}

bool one_image_variants(const Layout& L, int batch) {
  static const long long lim = [] {
    const char* e = getenv("SIFT_HIP_ONE_IMAGE_PX");
    return e ? atoll(e) : kOneImagePx;
  }();
  return batch == 1 && (long long)L.rows * L.cols <= lim;
}

void launch_orient(hipStream_t st, const RefArgs& A, int batch) {
  // batches: two candidates per lane group (orient_slots_kernel<2>; three
  // slots 1.65, four 1.53-1.57 vs 1.48-1.50 ms, round 5); one image: one wave
  // per candidate with bucketed bins (orient_bin_kernel, round 4), whose chain
  // is a window's largest per-batch bin counts instead of its whole sample
  // walk.  Every variant is bit-identical (the losers are kept as
  // tools/patches/r5_variants.patch).
  // One image: a workgroup (one wave) per candidate slot, so the dispatcher
  // gives the next candidate to whichever wave slot frees first -- a fixed
  // stride per resident wave left the waves alive 40 % of the launch on
  // average (61.6 vs 41.8 us for one 1080p image, round 6; rejected
  // candidates exit after one load).
  if (one_image_variants(A.L, batch)) {
    hipLaunchKernelGGL(orient_bin_kernel, dim3(std::max(1, A.cand_cap)), dim3(64), 0, st, A);
  } else {
    // (one 8K image: 4 resident grids were 457 -> 520 us here, unlike the
    // descriptor's; profiles/r6_one_image_grids_ab.txt)
    hipLaunchKernelGGL(orient_slots_kernel<2>,
                       dim3(resident_grid((const void*)orient_slots_kernel<2>, 64, 0, 8192)), dim3(64), 0, st, A);
  }
}

}  // namespace sift
