// extrema.hip -- the extrema walk (DoG fused with the 26-neighbour test,
// reference src/sift.cpp:280, 493-511), the candidate bitmask and its ordered
// compaction into the candidate list; the standalone gradient planes.
#include <algorithm>

#include "detect_args.hpp"

namespace sift {

// ---- candidate bitmask: one bit per (octave, layer, row, col) -------------
// Plane (o, layer) holds rows x wpr 32-bit words (wpr = ceil(cols/32)), bit c%32
// of word r*wpr + c/32; planes follow in (o, layer) order.  Word order within an
// image is therefore exactly the reference's scan order (src/sift.cpp:556-557,
// 487-491), which makes the ordered compaction a plain scan over words.
constexpr int kMaxSeg = 2 * kMaxOctaves;
#ifndef SIFT_WORD_CHUNK
#define SIFT_WORD_CHUNK 512  // A/B builds only (tools/build_var.sh); round 6: 2048 -> 512, one image's mask_expand 11.4 -> 4.9 us
#endif
constexpr int kWordChunk = SIFT_WORD_CHUNK;  // mask words per workgroup in the count/expand passes

struct MaskLayout {
  int n;                          // segments = n_oct * 2
  int bpw;                        // count/expand workgroups per image
  long long w_img;                // words per image
  long long start[kMaxSeg + 1];
  int o[kMaxSeg], layer[kMaxSeg], wpr[kMaxSeg];
};

static MaskLayout make_mask(const Layout& L) {
  MaskLayout M{};
  long long t = 0;
  int n = 0;
  for (int o = 0; o < L.n_oct; ++o)
    for (int layer = 1; layer <= kLayers; ++layer) {
      M.start[n] = t;
      M.o[n] = o;
      M.layer[n] = layer;
      M.wpr[n] = (L.oct[o].cols + 31) / 32;
      t += (long long)L.oct[o].rows * M.wpr[n];
      ++n;
    }
  M.start[n] = t;
  M.n = n;
  M.w_img = t;
  M.bpw = (int)((t + kWordChunk - 1) / kWordChunk);
  if (M.bpw == 0) M.bpw = 1;
  return M;
}

long long mask_words_per_image(const Layout& L) { return make_mask(L).w_img; }
int mask_blocks_per_image(const Layout& L) { return make_mask(L).bpw; }

// ---- pass 1: DoG (src/sift.cpp:280) fused with the 26-neighbour test --------
// One wave owns a 64-column strip (64-aligned, so its ballots are exactly two
// mask words per row) of one octave and walks a chunk of rows.  Each row of
// the five Gaussian planes (or the caller's DoG planes) is loaded once --
// lanes 0 and 1 also fetch the columns x0-1 and x0+64 -- one row ahead of its
// use, turned into the four DoG rows + Gaussian layers 1, 2 and put into a
// three-row LDS ring; row y is then tested and its gradients written as soon
// as row y+1 is in the ring.  Against round 1's 64x16 tiles (a workgroup per
// tile, 29 KB of LDS, 1.16x the rows with the halo; 2.26 vs 1.56 ms per step,
// tools/patches/r5_variants.patch): no 2-row halo per tile (rows are read
// once per chunk), the loads of the next row fly while the current one is
// tested, and a wave needs 4.9 KB of LDS, so 8 waves per SIMD stay resident.
// Same values, same bits (the 26-neighbour test only compares; the gradients
// and DoG are the same float expressions).
constexpr int kWCols = 64 + 4;  // ring row: column x0 - 1 + c at c (c = 0..65)

struct WalkArgs {
  Layout L;
  MaskLayout M;
  const float* gpyr;
  const float* dog;
  float2* grad;
  const MathConsts* mc;
  unsigned* mask;
  int wave_start[kMaxOctaves + 1];  // first wave (blockIdx.x) of octave o
  int strips[kMaxOctaves];
  int chunk;                        // rows per wave
  unsigned sparse;                  // bit o: octave o has no plane 4 (FROM_G only): layer 2 is tested without DoG 3
};

// src/sift.cpp:493-511 at ring column c: lo/cu/hi[k] = row y - 1 + k of the
// layer below / at / above the tested one; ties pass.
__device__ __forceinline__ bool ring_extremum(const float* const (&lo)[3], const float* const (&cu)[3],
                                              const float* const (&hi)[3], int c) {
  const float v = cu[1][c];
  if (!(fabsf(v) > kDogThreshold)) return false;
  bool ok = true;
  if (v > 0) {
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        ok = ok && v >= lo[dy][c + dx] && v >= hi[dy][c + dx];
        if (dy != 1 || dx != 0) ok = ok && v >= cu[dy][c + dx];
      }
  } else if (v < 0) {
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        ok = ok && v <= lo[dy][c + dx] && v <= hi[dy][c + dx];
        if (dy != 1 || dx != 0) ok = ok && v <= cu[dy][c + dx];
      }
  } else {
    ok = false;
  }
  return ok;
}

template <bool FROM_G>
__global__ __launch_bounds__(64) void extrema_walk_kernel(WalkArgs A) {
  __shared__ float ring[3][6][kWCols];  // planes: DoG 0..3, Gaussian layers 1, 2
  const int lane = threadIdx.x;
  const int b = blockIdx.y;
  // XCD-aware order (speed only): blocks b and b + 8 share an XCD, so XCD x
  // takes the contiguous run [x P, (x + 1) P) of the (octave, chunk, strip)
  // raster order and neighbouring strips -- which fetch each other's edge
  // columns -- meet in the same L2
  const int per_xcd = (int)(gridDim.x >> 3);
  const int t = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
  if (t >= A.wave_start[A.L.n_oct]) return;
  int o = 0;
  while (o + 1 < A.L.n_oct && A.wave_start[o + 1] <= t) ++o;
  const int local = t - A.wave_start[o];
  const Octave& O = A.L.oct[o];
  const int x0 = (local % A.strips[o]) * 64, y0 = (local / A.strips[o]) * A.chunk;
  const int y1 = min(y0 + A.chunk, O.rows);
  const int rows = O.rows, cols = O.cols;
  const long long pitch = O.pitch;
  const float* g = A.gpyr + b * A.L.g_img;
  const float* dg = FROM_G ? nullptr : A.dog + b * A.L.d_img;
  // no plane 4 in this octave (uniform): it is not loaded, DoG 3 is not formed
  // and layer 2 passes on its other 17 neighbours (a partial candidate; the
  // nine DoG 3 comparisons follow in refine_step_kernel<true>)
  const bool sp = FROM_G && ((A.sparse >> o) & 1u);
  const int xm = x0 + lane;                       // this lane's column
  const int xh = lane == 0 ? x0 - 1 : x0 + 64;    // halo column of lanes 0, 1
  const bool hl = lane < 2;
  const int xmc = min(xm, cols - 1), xhc = min(max(xh, 0), cols - 1);
  // loads of row r (clamped addresses; out-of-image values are zeroed when the
  // row is put): G1, G2 and then G0, G3, G4 (FROM_G) or the DoG planes 0..3
  auto load = [&](int r, float (&v)[6], float (&h)[6]) {
    const long long rp = (long long)min(max(r, 0), rows - 1) * pitch;
    const long long pm = rp + xmc, ph = rp + xhc;
    v[0] = g[O.g_off[1] + pm];
    v[1] = g[O.g_off[2] + pm];
    if (FROM_G) {
      v[2] = g[O.g_off[0] + pm];
      v[3] = g[O.g_off[3] + pm];
      v[4] = sp ? 0.f : g[O.g_off[4] + pm];
    } else {
#pragma unroll
      for (int k = 0; k < kDogPer; ++k) v[2 + k] = dg[O.d_off[k] + pm];
    }
    if (hl) {
      h[0] = g[O.g_off[1] + ph];
      h[1] = g[O.g_off[2] + ph];
      if (FROM_G) {
        h[2] = g[O.g_off[0] + ph];
        h[3] = g[O.g_off[3] + ph];
        h[4] = sp ? 0.f : g[O.g_off[4] + ph];
      } else {
#pragma unroll
        for (int k = 0; k < kDogPer; ++k) h[2 + k] = dg[O.d_off[k] + ph];
      }
    }
  };
  // DoG (src/sift.cpp:280: dog = g[i+1] - g[i]) and the Gaussian layers into
  // ring slot s at column c; 0 outside the image, as the tile kernel
  // the lane's own column of the ring, kept in registers as well: od[slot][k]
  // = DoG plane k, og[slot][l] = Gaussian layer 1 + l (slots are compile-time
  // constants in the unrolled walk below)
  float od[3][kDogPer], og[3][2];
  auto put1 = [&](int s, int c, const float (&v)[6], bool ok, float (&d)[kDogPer], float (&gg)[2]) {
    const float g1 = ok ? v[0] : 0.f, g2 = ok ? v[1] : 0.f;
    if (FROM_G) {
      const float g0 = ok ? v[2] : 0.f, g3 = ok ? v[3] : 0.f, g4 = ok ? v[4] : 0.f;
      d[0] = g1 - g0;
      d[1] = g2 - g1;
      d[2] = g3 - g2;
      d[3] = g4 - g3;
    } else {
#pragma unroll
      for (int k = 0; k < kDogPer; ++k) d[k] = ok ? v[2 + k] : 0.f;
    }
    gg[0] = g1;
    gg[1] = g2;
#pragma unroll
    for (int k = 0; k < kDogPer; ++k) ring[s][k][c] = d[k];
    ring[s][4][c] = g1;
    ring[s][5][c] = g2;
  };
  auto put = [&](int s, int r, const float (&v)[6], const float (&h)[6]) {
    const bool rok = r >= 0 && r < rows;
    put1(s, lane + 1, v, rok && xm < cols, od[s], og[s]);
    if (hl) {
      float dh[kDogPer], gh[2];
      put1(s, lane == 0 ? 0 : 65, h, rok && xh >= 0 && xh < cols, dh, gh);
    }
  };
  const AtanConsts ak = A.mc->t;
  float2* gr = A.grad + b * A.L.g_img;
  const int wpr = A.M.wpr[2 * o];
  const long long mbase = b * A.M.w_img;
  // row y from ring slots su (y-1), sm (y), sd (y+1)
  auto process = [&](int y, int su, int sm, int sd) {
    const int c = lane + 1;
    if (y > 0 && y < rows - 1 && xm > 0 && xm < cols - 1) {
#pragma unroll
      for (int ls = 0; ls < 2; ++ls) {
        const float dx = (float)(ring[sm][4 + ls][c + 1] - ring[sm][4 + ls][c - 1]);
        const float dy = (float)(og[su][ls] - og[sd][ls]);
        gr[O.g_off[1 + ls] + (long long)y * pitch + xm] = make_float2(magnitude(dx, dy), fast_atan2(dy, dx, ak));
      }
    }
    // src/sift.cpp:493-511, both detection layers: v at (y, x) of DoG plane
    // 1 (layer 1) / 2 (layer 2) is an extremum when |v| > 8 and v >= (<=)
    // all 26 neighbours -- ties pass -- i.e. v >= the max (v <= the min) of
    // the neighbours (finite values: the order of the comparisons does not
    // matter).  Branch-free: per plane the max / min of the 3x3 block,
    // without its centre for the two planes whose centres are tested.
    const int s3[3] = {su, sm, sd};
    float mx9[kDogPer], mn9[kDogPer], mx8[2], mn8[2];
#pragma unroll
    for (int k = 0; k < kDogPer; ++k) {
      float l3[3], r3[3];
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        l3[dy] = ring[s3[dy]][k][c - 1];
        r3[dy] = ring[s3[dy]][k][c + 1];
      }
      const float own_ud_max = fmaxf(od[su][k], od[sd][k]), own_ud_min = fminf(od[su][k], od[sd][k]);
      const float side_max = fmaxf(fmaxf(fmaxf(l3[0], l3[1]), l3[2]), fmaxf(fmaxf(r3[0], r3[1]), r3[2]));
      const float side_min = fminf(fminf(fminf(l3[0], l3[1]), l3[2]), fminf(fminf(r3[0], r3[1]), r3[2]));
      const float m8x = fmaxf(side_max, own_ud_max), m8n = fminf(side_min, own_ud_min);
      mx9[k] = fmaxf(m8x, od[sm][k]);
      mn9[k] = fminf(m8n, od[sm][k]);
      if (k == 1 || k == 2) {
        mx8[k - 1] = m8x;
        mn8[k - 1] = m8n;
      }
    }
    const bool inside = y >= kBorder && y < rows - kBorder && xm >= kBorder && xm < cols - kBorder;
    bool f[2];
#pragma unroll
    for (int l = 0; l < 2; ++l) {
      const float v = od[sm][1 + l];
      float nmax = fmaxf(mx9[l], mx8[l]), nmin = fminf(mn9[l], mn8[l]);
      if (!(sp && l == 1)) {
        nmax = fmaxf(nmax, mx9[l + 2]);
        nmin = fminf(nmin, mn9[l + 2]);
      }
      f[l] = inside && fabsf(v) > kDogThreshold && ((v > 0 && v >= nmax) || (v < 0 && v <= nmin));
    }
    const unsigned long long m1 = __ballot(f[0]), m2 = __ballot(f[1]);
    if (lane == 0 || lane == 32) {
      const int w = x0 / 32 + (lane >> 5);
      if (w < wpr) {
        const long long base = mbase + (long long)y * wpr + w;
        A.mask[base + A.M.start[2 * o]] = (unsigned)(m1 >> lane);
        A.mask[base + A.M.start[2 * o + 1]] = (unsigned)(m2 >> lane);
      }
    }
  };
  // rows y0-1 .. y1 enter the ring in order (row y0-1+i in slot i % 3); row y
  // is processed once row y+1 is in.  Three register sets rotate, so the
  // loads of the next two rows are in flight while a row is processed.
  float va[6], ha[6], vb[6], hb[6], vc[6], hc[6];
  load(y0 - 1, va, ha);
  load(y0, vb, hb);
  load(y0 + 1, vc, hc);
  // ring slot of row r: (r - y0 + 1) % 3, i.e. set a <-> slot 0, b <-> 1, c <-> 2
  auto step = [&](int r, float (&v)[6], float (&h)[6], int sr) {
    wave_sync();  // the previous process() read slot sr (row r - 3) at other lanes' columns
    put(sr, r, v, h);
    wave_sync();
    if (r + 3 <= y1) load(r + 3, v, h);
    if (r >= y0 + 1) process(r - 1, (sr + 1) % 3, (sr + 2) % 3, sr);
  };
  for (int r = y0 - 1; r <= y1; r += 3) {
    step(r, va, ha, 0);
    if (r + 1 > y1) break;
    step(r + 1, vb, hb, 1);
    if (r + 2 > y1) break;
    step(r + 2, vc, hc, 2);
  }
}

// ---- pass 2: ordered compaction of the bitmask ----------------------------
__global__ __launch_bounds__(256) void mask_count_kernel(const unsigned* __restrict__ mask, long long w_img,
                                                         int bpw, int* __restrict__ blk_counts,
                                                         int* __restrict__ g4stat) {
  __shared__ int wsum[4];
  const int b = blockIdx.y;
  // the sparse flow's counters start every detection at 0 (inside the captured sequence)
  if (blockIdx.x == 0 && b == 0 && threadIdx.x < kG4Stats) g4stat[threadIdx.x] = 0;
  const long long base = (long long)blockIdx.x * kWordChunk;
  const unsigned* m = mask + b * w_img;
  int cnt = 0;
#pragma unroll
  for (int it = 0; it < kWordChunk / 256; ++it) {
    const long long w = base + it * 256 + threadIdx.x;
    if (w < w_img) cnt += __popc(m[w]);
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) blk_counts[b * bpw + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(256) void mask_expand_kernel(MaskLayout M, const unsigned* __restrict__ mask,
                                                          const int* __restrict__ blk_off,
                                                          Cand* __restrict__ cands, int cap) {
  __shared__ int wcnt[4];
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long base = (long long)blockIdx.x * kWordChunk;
  const unsigned* m = mask + b * M.w_img;
  int run = blk_off[b * M.bpw + blockIdx.x];
  // every word of the chunk in flight at once (the loop below synchronises per step)
  unsigned words[kWordChunk / 256];
#pragma unroll
  for (int it = 0; it < kWordChunk / 256; ++it) {
    const long long w = base + it * 256 + threadIdx.x;
    words[it] = w < M.w_img ? m[w] : 0u;
  }
#pragma unroll
  for (int it = 0; it < kWordChunk / 256; ++it) {
    const long long w = base + it * 256 + threadIdx.x;
    unsigned bits = words[it];
    const int cnt = __popc(bits);
    // wave_scan.hpp's wave_scan_incl() + wg_scan<4>() restated: the calls change this kernel's text (profiles/detect_split_isa.txt)
    int incl = cnt;
    for (int off = 1; off < 64; off <<= 1) {
      const int tt = __shfl_up(incl, off);
      if (lane >= off) incl += tt;
    }
    if (lane == 63) wcnt[wv] = incl;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < wv; ++k) before += wcnt[k];
    const int tot = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    if (bits) {
      int s = 0;
      while (s + 1 < M.n && M.start[s + 1] <= w) ++s;
      const long long wi = w - M.start[s];
      const int r = (int)(wi / M.wpr[s]);
      const int c0 = (int)(wi % M.wpr[s]) * 32;
      int pos = run + before + incl - cnt;
      const int ol = M.o[s] | (M.layer[s] << 8);
      while (bits) {
        const int bit = __builtin_ctz(bits);
        bits &= bits - 1;
        if (pos < cap) cands[pos] = Cand{b, ol, r, c0 + bit};
        ++pos;
      }
    }
    run += tot;
    __syncthreads();
  }
}

// Standalone gradient planes for scales [s_lo, s_hi] (sub-module entry points
// whose pyramids come from the caller).
__global__ __launch_bounds__(256) void grad_kernel(const float* __restrict__ gpyr, float2* __restrict__ grad,
                                                   long long g_img, long long g_off, int pitch, int rows,
                                                   int cols, int nscale, long long plane,
                                                   const MathConsts* __restrict__ mc) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const int b = blockIdx.z / nscale, s = blockIdx.z % nscale;
  if (!(y > 0 && y < rows - 1 && x > 0 && x < cols - 1)) return;
  const long long off = b * g_img + g_off + s * plane + (long long)y * pitch + x;
  const float* p = gpyr + off;
  const float dx = (float)(p[1] - p[-1]);
  const float dy = (float)(p[-pitch] - p[pitch]);
  grad[off] = make_float2(magnitude(dx, dy), fast_atan2(dy, dx, mc->t));
}

void launch_grad(hipStream_t st, const Layout& L, const float* gpyr, float2* grad, int batch, int s_lo,
                 int s_hi, const MathConsts* mc) {
  for (int o = 0; o < L.n_oct; ++o) {
    const Octave& O = L.oct[o];
    const int ns = s_hi - s_lo + 1;
    dim3 grid((O.cols + 63) / 64, (O.rows + 3) / 4, batch * ns);
    hipLaunchKernelGGL(grad_kernel, grid, dim3(256), 0, st, gpyr, grad, L.g_img, O.g_off[s_lo], O.pitch,
                       O.rows, O.cols, ns, (long long)O.rows * O.pitch, mc);
  }
}

void launch_extrema(hipStream_t st, const Layout& L, const float* gpyr, float* dog, bool write_dog,
                    float2* grad, const MathConsts* mc, int batch, DetectBufs& D, unsigned sparse) {
  WalkArgs W;
  W.sparse = write_dog ? sparse : 0u;
  W.L = L;
  W.M = make_mask(L);
  W.gpyr = gpyr;
  W.dog = dog;
  W.grad = grad;
  W.mc = mc;
  W.mask = D.mask;
  // rows per wave: about 64 K waves over the launch (measured on the
  // 64 x 1080p batch: 16 K 1.70 ms, 32 K 1.60, 64 K 1.56), at least
  // SIFT_EXTREMA_MIN_CHUNK rows (a chunk re-reads 2 rows)
  long long strip_rows = 0;
  for (int o = 0; o < L.n_oct; ++o) strip_rows += (long long)((L.oct[o].cols + 63) / 64) * L.oct[o].rows;
  constexpr long long target = 65536;  // waves per launch (16 K / 32 K / 64 K measured in round 2)
#ifndef SIFT_EXTREMA_MIN_CHUNK
#define SIFT_EXTREMA_MIN_CHUNK 4  // A/B builds only (tools/build_var.sh); one 1080p image: 4 rows 28.9 us, 8 30.7 (round 6)
#endif
  W.chunk = (int)std::min<long long>(512, std::max<long long>(SIFT_EXTREMA_MIN_CHUNK, strip_rows * batch / target));
  int w = 0;
  for (int o = 0; o < L.n_oct; ++o) {
    W.wave_start[o] = w;
    W.strips[o] = (L.oct[o].cols + 63) / 64;
    w += W.strips[o] * ((L.oct[o].rows + W.chunk - 1) / W.chunk);
  }
  W.wave_start[L.n_oct] = w;
  const int wg = (w + 7) / 8 * 8;  // whole XCD runs (extra waves exit)
  if (write_dog)
    hipLaunchKernelGGL(extrema_walk_kernel<true>, dim3(wg, batch), dim3(64), 0, st, W);
  else
    hipLaunchKernelGGL(extrema_walk_kernel<false>, dim3(wg, batch), dim3(64), 0, st, W);
  const MaskLayout& M = W.M;
  hipLaunchKernelGGL(mask_count_kernel, dim3(M.bpw, batch), dim3(256), 0, st, D.mask, M.w_img, M.bpw,
                     D.blk_counts, D.g4stat);
  const int nblk = M.bpw * batch;
  launch_scan(st, D.blk_counts, D.scan_tmp, nullptr, nblk, nblk, D.cand_total, D.scan_tiles,
              ScanGather{nullptr, M.bpw, batch, D.img_cand_off});
  hipLaunchKernelGGL(mask_expand_kernel, dim3(M.bpw, batch), dim3(256), 0, st, M, D.mask, D.scan_tmp,
                     D.cands, D.cand_cap);
}

}  // namespace sift
