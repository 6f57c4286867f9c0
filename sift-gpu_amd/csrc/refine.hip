// refine.hip -- sub-pixel refinement (adjustLocalExtrema, reference
// src/sift.cpp:287-388): the dense pass, and the sparse flow that evaluates the
// widest Gaussian plane point by point where a candidate reads it.
#include <limits.h>

#include <algorithm>

#include "detect_args.hpp"

namespace sift {

// adjustLocalExtrema (src/sift.cpp:287-388) for one candidate.
struct Refined {
  bool ok;
  bool pending;  // SPARSE: stopped before iteration `it` at (layer 2, r, c), whose patch is not filled yet
  int it;
  int layer, r, c, octave;
  float x, y, size, response;
};

// Writes a slot's refinement result: the refined keypoint fields and the
// orientation pass's inputs (refined r, c, layer; npeaks = 1 if kept).
__device__ __forceinline__ void store_refined(CandOut* co, const Refined& R, int img, bool kept) {
  co->x = R.x;
  co->y = R.y;
  co->size = R.size;
  co->response = R.response;
  co->octave = R.octave;
  co->img = img;
  co->npeaks = kept ? 1 : 0;
  co->ref_r = R.r;
  co->ref_c = R.c;
  co->ref_layer = R.layer;
}

// DoG value of layer l at (yy, xx): the stored DoG plane, or -- FROM_G -- the
// difference of the Gaussian planes l+1 and l that buildDoGPyramid stores
// (src/sift.cpp:276; the same float subtraction, so bit-identical).
//
// SPARSE (FROM_G; the octave has no plane 4): the walk starts at iteration it0
// and takes plane 4 from `patch` -- its 3x3 around (pr, pc), g4_fill_kernel's
// floats, the plane's own bit for bit -- whenever the cube reaches it, i.e. on
// layer 2.  On layer 2 at any other position it returns `pending` with its
// state before that iteration; the caller has the patch filled there and
// calls again.  The arithmetic is the same term for term.
template <bool FROM_G, bool SPARSE = false>
__device__ __forceinline__ Refined refine_candidate(const Layout& Lay, const float* __restrict__ dimg,
                                                    const float* __restrict__ gimg, int o, int layer, int r,
                                                    int c, int it0 = 0, const float* __restrict__ patch = nullptr,
                                                    int pr = -1, int pc = -1) {
  static_assert(FROM_G || !SPARSE, "the sparse flow forms DoG from the Gaussian planes");
  const Octave& O = Lay.oct[o];
  const long long pitch = O.pitch;
  const float img_scale = 1. / 255;
  const float deriv_scale = img_scale * 0.5f;
  const float second_scale = img_scale;
  const float cross_scale = img_scale * 0.25f;
  float xi = 0, xr = 0, xc = 0, contr = 0;
  Refined R{};
  R.ok = true;
  int it = it0;
  // The 3x3 neighbourhood of (r, c) in DoG layers layer-1 .. layer+1, loaded
  // once per Newton step as one 12-byte row per plane and row (FROM_G: four
  // Gaussian planes, DoG = g[l+1] - g[l], src/sift.cpp:276 -- the same float
  // subtraction as the stored DoG, bit-identical).  (r, c) stays >= 5 from
  // the border and layer in [1, 2], so every row lies inside its plane.
  struct Row3 {
    float a, b, c;
  };
  float cube[3][3][3];  // [layer - (cur - 1)][dy + 1][dx + 1]
  int cube_layer = -1, cube_r = -1, cube_c = -1;
  auto load_cube = [&](int cur, int rr_, int cc_) {
    if (cur == cube_layer && rr_ == cube_r && cc_ == cube_c) return;
    cube_layer = cur;
    cube_r = rr_;
    cube_c = cc_;
    const long long base = (long long)(rr_ - 1) * pitch + (cc_ - 1);
    if (FROM_G) {
      Row3 gv[4][3];
#pragma unroll
      for (int pl = 0; pl < 4; ++pl)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          if (SPARSE && cur - 1 + pl == kScales - 1)  // plane 4: the patch at (pr, pc) == (rr_, cc_)
            gv[pl][dy] = Row3{patch[3 * dy], patch[3 * dy + 1], patch[3 * dy + 2]};
          else
            gv[pl][dy] = *reinterpret_cast<const Row3*>(gimg + O.g_off[cur - 1 + pl] + base + dy * pitch);
        }
#pragma unroll
      for (int l = 0; l < 3; ++l)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          cube[l][dy][0] = gv[l + 1][dy].a - gv[l][dy].a;
          cube[l][dy][1] = gv[l + 1][dy].b - gv[l][dy].b;
          cube[l][dy][2] = gv[l + 1][dy].c - gv[l][dy].c;
        }
    } else {
#pragma unroll
      for (int l = 0; l < 3; ++l)
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
          const Row3 v = *reinterpret_cast<const Row3*>(dimg + O.d_off[cur - 1 + l] + base + dy * pitch);
          cube[l][dy][0] = v.a;
          cube[l][dy][1] = v.b;
          cube[l][dy][2] = v.c;
        }
    }
  };
// DoG value of layer pl at (yy, xx): every use is within one of (layer, r, c),
// so the cube indices fold to constants
#define AT(pl, yy, xx) cube[(pl) - (layer - 1)][(yy) - r + 1][(xx) - c + 1]
  for (; it < kMaxInterp; ++it) {
    if (SPARSE && layer == kLayers && (r != pr || c != pc)) {
      R.pending = true;
      R.it = it;
      R.layer = layer;
      R.r = r;
      R.c = c;
      return R;
    }
    load_cube(layer, r, c);
    const int cur = layer, lo = layer - 1, hi = layer + 1;
    const float g[3] = {(AT(cur, r, c + 1) - AT(cur, r, c - 1)) * deriv_scale,
                        (AT(cur, r + 1, c) - AT(cur, r - 1, c)) * deriv_scale,
                        (AT(hi, r, c) - AT(lo, r, c)) * deriv_scale};
    const float v2 = (float)AT(cur, r, c) * 2;
    const float dxx = (AT(cur, r, c + 1) + AT(cur, r, c - 1) - v2) * second_scale;
    const float dyy = (AT(cur, r + 1, c) + AT(cur, r - 1, c) - v2) * second_scale;
    const float dss = (AT(hi, r, c) + AT(lo, r, c) - v2) * second_scale;
    const float dxy = (AT(cur, r + 1, c + 1) - AT(cur, r + 1, c - 1) - AT(cur, r - 1, c + 1) +
                       AT(cur, r - 1, c - 1)) * cross_scale;
    const float dxs = (AT(hi, r, c + 1) - AT(hi, r, c - 1) - AT(lo, r, c + 1) + AT(lo, r, c - 1)) *
                      cross_scale;
    const float dys = (AT(hi, r + 1, c) - AT(hi, r - 1, c) - AT(lo, r + 1, c) + AT(lo, r - 1, c)) *
                      cross_scale;
    const float H[9] = {dxx, dxy, dxs, dxy, dyy, dys, dxs, dys, dss};
    float X[3];
    solve3(H, g, X);
    xi = -X[2];
    xr = -X[1];
    xc = -X[0];
    if (fabsf(xi) < 0.5f && fabsf(xr) < 0.5f && fabsf(xc) < 0.5f) break;
    if (fabsf(xi) > (float)(INT_MAX / 3) || fabsf(xr) > (float)(INT_MAX / 3) ||
        fabsf(xc) > (float)(INT_MAX / 3)) {
      R.ok = false;
      return R;
    }
    c += cv_round(xc);
    r += cv_round(xr);
    layer += cv_round(xi);
    if (layer < 1 || layer > kLayers || c < kBorder || c >= O.cols - kBorder || r < kBorder ||
        r >= O.rows - kBorder) {
      R.ok = false;
      return R;
    }
  }
  if (it >= kMaxInterp) {
    R.ok = false;
    return R;
  }
  {
    load_cube(layer, r, c);  // unchanged since the last step's load (the loop left without moving)
    const int cur = layer, lo = layer - 1, hi = layer + 1;
    const float g0 = (AT(cur, r, c + 1) - AT(cur, r, c - 1)) * deriv_scale;
    const float g1 = (AT(cur, r + 1, c) - AT(cur, r - 1, c)) * deriv_scale;
    const float g2 = (AT(hi, r, c) - AT(lo, r, c)) * deriv_scale;
    float t = 0;  // Matx::dot: s = 0; s += a_i * b_i
    t = t + g0 * xc;
    t = t + g1 * xr;
    t = t + g2 * xi;
    contr = AT(cur, r, c) * img_scale + t * 0.5f;
    if (fabsf(contr) * kLayers < (float)0.04) {
      R.ok = false;
      return R;
    }
    const float v2 = AT(cur, r, c) * 2.f;
    const float dxx = (AT(cur, r, c + 1) + AT(cur, r, c - 1) - v2) * second_scale;
    const float dyy = (AT(cur, r + 1, c) + AT(cur, r - 1, c) - v2) * second_scale;
    const float dxy = (AT(cur, r + 1, c + 1) - AT(cur, r + 1, c - 1) - AT(cur, r - 1, c + 1) +
                       AT(cur, r - 1, c - 1)) * cross_scale;
    const float tr = dxx + dyy;
    const float det = dxx * dyy - dxy * dxy;
    const float et = 10.f;
    if (det <= 0 || tr * tr * et >= (et + 1) * (et + 1) * det) {
      R.ok = false;
      return R;
    }
  }
#undef AT
  R.layer = layer;
  R.r = r;
  R.c = c;
  R.x = (c + xc) * (1 << o);
  R.y = (r + xr) * (1 << o);
  R.octave = o + (layer << 8) + (cv_round_d((xi + 0.5) * 255) << 16);
  R.size = (float)kSigma * pow2f_cr((layer + xi) / kLayers) * (1 << o) * 2;
  R.response = fabsf(contr);
  return R;
}

// Refinement: one lane per candidate.
__global__ __launch_bounds__(256) void refine_kernel(RefArgs A) {
  int n = *A.cand_total;
  if (n > A.cand_cap) n = A.cand_cap;
  for (int ci = blockIdx.x * 256 + threadIdx.x; ci < n; ci += gridDim.x * 256) {
    const Cand cd = A.cands[ci];
    const Refined R = A.dog_from_g ? refine_candidate<true>(A.L, nullptr, A.gpyr + cd.b * A.L.g_img, cd.ol & 255,
                                                            cd.ol >> 8, cd.r, cd.c)
                                   : refine_candidate<false>(A.L, A.dog + cd.b * A.L.d_img, nullptr, cd.ol & 255,
                                                             cd.ol >> 8, cd.r, cd.c);
    // store_refined(A.couts + ci, R, cd.b, R.ok) restated: the call is +176
    // instructions here (profiles/detect_split_isa.txt)
    CandOut* co = A.couts + ci;
    co->x = R.x;
    co->y = R.y;
    co->size = R.size;
    co->response = R.response;
    co->octave = R.octave;
    co->img = cd.b;
    co->npeaks = R.ok ? 1 : 0;
    co->ref_r = R.r;
    co->ref_c = R.c;
    co->ref_layer = R.layer;
  }
}

// ---- sparse flow: plane 4 point by point (SparseG4, common.hpp) -------------
// g4_fill_group: Gaussian_Blur(plane 0, sig[4]) (src/sift.cpp:110-153,
// 257-258) on the 3x3 around a candidate, for up to kG4Cands slots at a time.
// Every output runs the reference's chain -- acc = +0; kernel rows ascending,
// columns ascending, one multiply and one add per tap; source 0 outside
// [0, rows-1) x [0, cols-1) (:116); / 8192 -- which is blur_tile's and
// sym_walk's chain for that pixel, so the floats are the dense plane's.
//
// Lane 3q + dy owns output row dy of slot q, its three outputs (dx = 0..2) as
// three chains side by side.  Kernel row a of output row dy reads row a + dy
// of the slot's 39 x 39 source window, so the window's rows pass through a
// four-row LDS ring, one new row per step (the 64 lanes load the group's
// 21 x 39 row segments, coalesced, one step ahead).  A step's kernel row is
// uniform across the wave: its 37 floats come from the scalar cache into SGPRs
// (as in blur_tile), not from LDS.  Per step and lane: 10 ds_read_b128, 111
// multiplies, 111 adds.
//
// Ring layout: row rr of slot q starts at word q * 180 + rr * 44, i.e. at the
// 16-byte slot 45 q + 11 rr; a ds_read_b128 is served in four 16-lane groups
// ({0-3, 12-15, 20-27}, ...) over 16 such slots (mod 16).  With these two odd
// pitches no slot is asked for by more than two of a group's distinct rows at
// any step (every step and group enumerated); the plain 160 / 40 pitches gave
// only the eight even slots, four rows deep.
constexpr int kG4W = 18, kG4K = 2 * kG4W + 1, kG4Win = kG4K + 2;
constexpr int kG4Cols = 40;                // words read per window row (b128 reads); staging element pitch
constexpr int kG4RowPitch = 44;            // ring row pitch
constexpr int kG4CandPitch = 4 * kG4RowPitch + 4;  // ring pitch of a slot's four rows
constexpr int kG4Cands = 21;               // slots per wave pass (3 lanes each)
constexpr int kG4Loads = (kG4Cands * kG4Cols + 63) / 64;  // staged elements per lane and row
static_assert(kG4Win <= kG4Cols && kG4Cols <= kG4RowPitch && kG4Cols % 4 == 0 && 3 * kG4Cands <= 64, "fill layout");
static_assert((kG4RowPitch / 4) % 2 == 1 && (kG4CandPitch / 4) % 2 == 1, "odd slot pitches (bank rule above)");

struct G4Lds {
  float ring[kG4Cands * kG4CandPitch];
  int ci[kG4Cands], r[kG4Cands], c[kG4Cands];  // the pass's slots (ci < 0: none) and the centre of each patch
};

// One pass over the slots S.ci / S.r / S.c (written before a wave_sync): acc =
// the unscaled chains of lane 3q + dy's output row.  Ends on a wave_sync, so
// the caller may rewrite S at once.
__device__ __forceinline__ void g4_fill_group(G4Lds& S, const Layout& L, const float* __restrict__ gpyr,
                                              const Cand* __restrict__ cands, const float* __restrict__ coef4,
                                              int lane, float (&acc)[3]) {
  const int q = min(lane / 3, kG4Cands - 1), dy = lane - 3 * (lane / 3);
  // staging: element e = k * 64 + lane of the group's row is column e % 40
  // of slot e / 40; its source column, row range and ring word
  const float* sp[kG4Loads];
  int row0[kG4Loads], spitch[kG4Loads], lim[kG4Loads], loff[kG4Loads];
#pragma unroll
  for (int k = 0; k < kG4Loads; ++k) {
    const int e = k * 64 + lane, eq = e / kG4Cols, col = e - eq * kG4Cols;
    sp[k] = gpyr;
    row0[k] = 0;
    spitch[k] = 0;
    lim[k] = 0;  // no row passes
    loff[k] = -1;
    const int ci = eq < kG4Cands && col < kG4Win ? S.ci[eq] : -1;
    if (ci >= 0) {
      const Cand cd = cands[ci];
      const Octave& O = L.oct[cd.ol & 255];
      const int x = S.c[eq] - (kG4W + 1) + col;
      loff[k] = eq * kG4CandPitch + col;
      row0[k] = S.r[eq] - (kG4W + 1);
      if (x >= 0 && x < O.cols - 1) {  // getSubMatrix's column rule; the row rule is lim
        sp[k] = gpyr + cd.b * L.g_img + O.g_off[0] + x;
        spitch[k] = O.pitch;
        lim[k] = O.rows - 1;
      }
    }
  }
  float nv[kG4Loads];
  auto fetch = [&](int s) {  // window row s
#pragma unroll
    for (int k = 0; k < kG4Loads; ++k) {
      const int row = row0[k] + s;
      nv[k] = (unsigned)row < (unsigned)lim[k] ? sp[k][(long long)row * spitch[k]] : 0.f;
    }
  };
  auto stage = [&](int s) {
#pragma unroll
    for (int k = 0; k < kG4Loads; ++k)
      if (loff[k] >= 0) S.ring[loff[k] + (s & 3) * kG4RowPitch] = nv[k];
  };
  fetch(0);
  stage(0);
  fetch(1);
  stage(1);
  fetch(2);
  acc[0] = acc[1] = acc[2] = 0.f;
  // step a: window rows a .. a + 2 are needed; row a + 2 goes into the ring
  // slot row a - 2 left (last read at step a - 2), rows a - 1 .. a + 1 of
  // step a - 1's reads sit in the other three
  for (int a = 0; a < kG4K; ++a) {
    stage(a + 2);
    wave_sync();
    if (a + 3 < kG4Win) fetch(a + 3);
    float x[kG4Cols];
    const float4* w4 = reinterpret_cast<const float4*>(S.ring + q * kG4CandPitch + ((a + dy) & 3) * kG4RowPitch);
#pragma unroll
    for (int i = 0; i < kG4Cols / 4; ++i) {
      const float4 v = w4[i];
      x[4 * i] = v.x;
      x[4 * i + 1] = v.y;
      x[4 * i + 2] = v.z;
      x[4 * i + 3] = v.w;
    }
    // uniform and never written while a kernel runs: read through the constant
    // address space, i.e. by scalar loads (the wave fences above would
    // otherwise make these vector loads)
    const __attribute__((address_space(4))) float* kr =
        (const __attribute__((address_space(4))) float*)(coef4 + a * kG4K);
#pragma unroll
    for (int b = 0; b < kG4K; ++b) {
      const float k = kr[b];
      float t[3];
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) t[dx] = x[b + dx] * k;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) acc[dx] = acc[dx] + t[dx];
    }
  }
  wave_sync();  // the next pass's first stores follow this pass's last reads
}

// The groups of kG4Cands list entries one wave of a resident grid (one wave
// per block, a multiple of 8 blocks) serves: g, g + step, ... below end.
// XCD-aware (blocks b and b + 8 share an XCD): each XCD takes a contiguous
// eighth of the groups and its waves hold consecutive ones at any moment, so
// the overlapping windows of neighbouring entries meet in one L2 (speed only:
// a patch is addressed by its slot).
struct G4Groups {
  int g, end, step;
};
__device__ __forceinline__ G4Groups g4_groups(int ngroups) {
  const int xcd = blockIdx.x & 7, per = (ngroups + 7) / 8;
  return G4Groups{xcd * per + (int)(blockIdx.x >> 3), min((xcd + 1) * per, ngroups), (int)(gridDim.x >> 3)};
}

// The first fill's list: every partial candidate (layer 2 of a sparse
// octave) below min(*cand_total, cand_cap), a wave's 64 consecutive slots
// consecutive and the waves in the order of their atomic adds (near slot
// order, which serves locality only).  Its length is stat[kG4StatFirst].
__global__ __launch_bounds__(256) void g4_list_kernel(const Cand* __restrict__ cands,
                                                      const int* __restrict__ cand_total, int cand_cap,
                                                      unsigned sparse, int* __restrict__ list,
                                                      int* __restrict__ stat) {
  int n = *cand_total;
  if (n > cand_cap) n = cand_cap;
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  const long long ci = (long long)blockIdx.x * 256 + threadIdx.x;
  bool need = false;
  if (ci < n) {
    const int ol = cands[ci].ol;
    need = (ol >> 8) == kLayers && ((sparse >> (ol & 255)) & 1u);
  }
  const unsigned long long m = __ballot(need);
  if (m) {
    const int leader = __ffsll((long long)m) - 1;
    int at = 0;
    if (lane == leader) at = atomicAdd(stat + kG4StatFirst, __popcll(m));
    at = __shfl(at, leader);
    if (need) list[at + __popcll(m & below)] = (int)ci;  // at most n <= cand_cap entries: distinct slots below n
  }
}

struct FillArgs {
  Layout L;
  const float* gpyr;
  const float* coef4;
  const Cand* cands;
  const int* list;   // the slots to serve, *count of them (g4_list_kernel); nullptr: slots 0 .. n_host - 1
  const int* count;
  int n_host, cand_cap;
  float* patch;
};

// First fill: the listed slots at their detected position, kG4Cands per wave
// pass, the passes handed out by g4_groups.
__global__ __launch_bounds__(64) void g4_fill_kernel(FillArgs A) {
  __shared__ __attribute__((aligned(16))) G4Lds S;
  const int lane = threadIdx.x;
  int n = A.list ? *A.count : A.n_host;
  if (n > A.cand_cap) n = A.cand_cap;
  const int q = min(lane / 3, kG4Cands - 1), dy = lane - 3 * (lane / 3);
  const G4Groups G = g4_groups((n + kG4Cands - 1) / kG4Cands);
  for (int g = G.g; g < G.end; g += G.step) {
    const int e0 = g * kG4Cands, ng = min(kG4Cands, n - e0);
    if (lane < kG4Cands) {
      const int ci = lane < ng ? (A.list ? A.list[e0 + lane] : e0 + lane) : -1;
      S.ci[lane] = ci;
      if (ci >= 0) {
        const Cand cd = A.cands[ci];
        S.r[lane] = cd.r;
        S.c[lane] = cd.c;
      }
    }
    wave_sync();
    const int cq = S.ci[q];  // read before the next pass rewrites S
    float acc[3];
    g4_fill_group(S, A.L, A.gpyr, A.cands, A.coef4, lane, acc);
    if (lane < 3 * ng) {
      float* p = A.patch + (long long)cq * 9 + 3 * dy;
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) p[dx] = acc[dx] / 8192.f;
    }
  }
}

// First step of adjustLocalExtrema in the sparse flow, one lane per candidate
// slot.  A partial candidate first takes the nine DoG 3 comparisons the
// extrema pass left out (src/sift.cpp:493-511, same threshold side and >= / <=
// rule: v is compared with plane 4's patch minus plane 3) and is rejected like
// a refinement rejection when one fails, so the slot and keypoint order stay
// the reference's.  A slot whose walk reaches a layer-2 position that has no
// patch yet is left pending (rstate = its iteration, ref_r / ref_c = the
// position) and appended to the first waiting list -- in any order, a patch
// is addressed by its slot -- with one atomic add per wave; g4_round_kernel
// takes those further.
__global__ __launch_bounds__(256) void refine_step_kernel(RefArgs A) {
  int n = *A.cand_total;
  if (n > A.cand_cap) n = A.cand_cap;
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int ci = blockIdx.x * 256 + threadIdx.x; ci < n; ci += gridDim.x * 256) {
    const Cand cd = A.cands[ci];
    const int o = cd.ol & 255;
    const int layer = cd.ol >> 8, r = cd.r, c = cd.c;
    const bool sp = (A.sparse >> o) & 1u;
    const float* gimg = A.gpyr + cd.b * A.L.g_img;
    const float* patch = A.patch + (long long)ci * 9;
    // the patch holds (r, c) exactly when the slot sits on layer 2: a partial
    // candidate's first fill
    const bool have = sp && layer == kLayers;
    bool ok = true;
    if (have) {
      const Octave& O = A.L.oct[o];
      const float* g3 = gimg + O.g_off[3] + (long long)(r - 1) * O.pitch + (c - 1);
      const float* g2 = gimg + O.g_off[2] + (long long)r * O.pitch + c;
      const float v = g3[O.pitch + 1] - *g2;  // DoG 2 at (r, c), as the extrema pass formed it
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const float d3 = patch[3 * dy + dx] - g3[dy * (long long)O.pitch + dx];
          ok = ok && (v > 0 ? v >= d3 : v <= d3);
        }
    }
    Refined R{};
    if (ok) {
      R = sp ? refine_candidate<true, true>(A.L, nullptr, gimg, o, layer, r, c, 0, patch, have ? r : -1, have ? c : -1)
             : refine_candidate<true, false>(A.L, nullptr, gimg, o, layer, r, c);
    }
    const bool pending = ok && R.pending;
    A.rstate[ci] = pending ? R.it : -1;
    store_refined(A.couts + ci, R, cd.b, ok && R.ok && !pending);
    const unsigned long long m = __ballot(pending);
    if (m) {  // uniform over the lanes still in the loop
      const int leader = __ffsll((long long)m) - 1;
      int at = 0;
      if (lane == leader) at = atomicAdd(A.g4stat + kG4StatWait, __popcll(m));
      at = __shfl(at, leader);
      if (pending) A.wait[at + __popcll(m & below)] = ci;
    }
  }
}

// A later round of the sparse refinement (round = 1 .. kMaxInterp - 1) over
// the compacted list the round before left: a wave takes kG4Cands entries,
// fills each one's patch at its recorded (r, c) and resumes its walk at its
// recorded iteration (lane q walks entry q, the patch handed over in LDS).  A
// slot that waits again goes onto the next round's list.  Each resumed walk
// runs at least the iteration it waited at (its patch is there now), a slot
// enters the first list at iteration >= 1, so after round kMaxInterp - 1 none
// waits (launch_refine_orient).  (One launch looping over its group until no
// member waited cost as many passes as the group's deepest slot: 1.07 ms
// against the 1.02 ms of the uncompacted rounds it replaced.  g4_groups' XCD
// order over the round lists measured no faster: tools/patches/
// detect_split_variants.patch.)
__global__ __launch_bounds__(64) void g4_round_kernel(RefArgs A, int round) {
  __shared__ __attribute__((aligned(16))) G4Lds S;
  __shared__ float pt[kG4Cands * 9];
  const int lane = threadIdx.x;
  const int* in = A.wait + (long long)((round - 1) & 1) * A.cand_cap;
  int* out = A.wait + (long long)(round & 1) * A.cand_cap;
  int cnt = A.g4stat[kG4StatWait + round - 1];
  if (cnt > A.cand_cap) cnt = A.cand_cap;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int q = lane / 3, dy = lane - 3 * q;
  int most = 0;
  const G4Groups G{(int)blockIdx.x, (cnt + kG4Cands - 1) / kG4Cands, (int)gridDim.x};
  for (int g = G.g; g < G.end; g += G.step) {
    const int g0 = g * kG4Cands, ng = min(kG4Cands, cnt - g0);
    int ci = -1, it = 0, r = 0, c = 0;
    Cand cd{};
    if (lane < ng) {
      ci = in[g0 + lane];
      cd = A.cands[ci];
      it = A.rstate[ci];
      r = A.couts[ci].ref_r;
      c = A.couts[ci].ref_c;
    }
    if (lane < kG4Cands) {
      S.ci[lane] = ci;
      S.r[lane] = r;
      S.c[lane] = c;
    }
    wave_sync();
    float acc[3];
    g4_fill_group(S, A.L, A.gpyr, A.cands, A.coef4, lane, acc);
    if (q < kG4Cands) {
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) pt[q * 9 + 3 * dy + dx] = acc[dx] / 8192.f;
    }
    wave_sync();
    bool pending = false;
    if (ci >= 0) {
      Refined R = refine_candidate<true, true>(A.L, nullptr, A.gpyr + cd.b * A.L.g_img, cd.ol & 255, kLayers, r, c, it,
                                               pt + lane * 9, r, c);
      pending = R.pending && round + 1 < kMaxInterp;
      if (R.pending && !pending) R = Refined{};  // not reached (see above): out of iterations, rejected
      A.rstate[ci] = pending ? R.it : -1;
      store_refined(A.couts + ci, R, cd.b, R.ok && !pending);
      // fills this slot took: one per round, and a partial candidate's first fill
      if (!pending) most = max(most, round + ((cd.ol >> 8) == kLayers ? 1 : 0));
    }
    const unsigned long long m = __ballot(pending);
    if (m) {
      int at = 0;
      if (lane == 0) at = atomicAdd(A.g4stat + kG4StatWait + round, __popcll(m));
      at = __shfl(at, 0);
      if (pending) out[at + __popcll(m & below)] = ci;
    }
    wave_sync();  // pt and S are rewritten by the next group
  }
  for (int off = 32; off > 0; off >>= 1) most = max(most, __shfl_xor(most, off));
  if (lane == 0 && most > 0) atomicMax(A.g4stat + kG4StatFills, most);
}

// Grid of a g4_groups kernel: the resident count, or SparseG4::grid's bound.
static unsigned g4_grid(const void* kernel, int bound) {
  return (unsigned)(bound > 0 ? bound : resident_grid(kernel, 64, 0, 2048));
}

void launch_refine_orient(hipStream_t st, const Layout& L, const float* gpyr, const float2* grad,
                          const float* dog, const MathConsts* mc, DetectBufs& D, int batch, SparseG4 sp) {
  RefArgs A;
  A.sparse = dog == nullptr ? sp.sparse : 0u;
  A.coef4 = sp.coef4;
  A.patch = D.g4patch;
  A.rstate = D.rstate;
  A.wait = D.g4wait;
  A.g4stat = D.g4stat;
  A.L = L;
  A.gpyr = gpyr;
  A.grad = grad;
  A.dog = dog;
  A.dog_from_g = dog == nullptr;
  A.mc = mc;
  A.cands = D.cands;
  A.cand_total = D.cand_total;
  A.cand_cap = D.cand_cap;
  A.couts = D.couts;
  A.npeaks = D.npeaks;
  if (A.sparse) {
    // First fill and first step over every slot, then kMaxInterp - 1 rounds
    // over compacted lists of the slots whose walk moved on layer 2 (about a
    // fifth of the first fill's slots enter the first list): a slot's walk
    // loads the cube once per iteration, each load can need one new patch, the
    // first step leaves a slot at iteration >= 1 and every round takes it at
    // least one iteration further, so none waits after the last.
    // The first fill's slots go onto a list first (the second waiting list's
    // space, which nothing uses before round 1), so that a resident grid can
    // hand them out in groups of kG4Cands.
    int* flist = D.g4wait + D.cand_cap;
    hipLaunchKernelGGL(g4_list_kernel, dim3((unsigned)std::max(1, (D.cand_cap + 255) / 256)), dim3(256), 0, st,
                       D.cands, D.cand_total, D.cand_cap, A.sparse, flist, D.g4stat);
    FillArgs F{L, gpyr, sp.coef4, D.cands, flist, D.g4stat + kG4StatFirst, 0, D.cand_cap, D.g4patch};
    hipLaunchKernelGGL(g4_fill_kernel, dim3(g4_grid((const void*)g4_fill_kernel, sp.grid)), dim3(64), 0, st, F);
    hipLaunchKernelGGL(refine_step_kernel, dim3(resident_grid((const void*)refine_step_kernel, 256, 0, 2048)),
                       dim3(256), 0, st, A);
    // a wave per kG4Cands waiting slots, striding when the list is longer than the grid; the others leave at once
    const int tcap = sp.grid > 0 ? sp.grid : 8192;
    const dim3 tgrid((unsigned)std::min(tcap, std::max(1, (D.cand_cap + kG4Cands - 1) / kG4Cands)));
    for (int round = 1; round < kMaxInterp; ++round) hipLaunchKernelGGL(g4_round_kernel, tgrid, dim3(64), 0, st, A, round);
  } else {
    hipLaunchKernelGGL(refine_kernel, dim3(resident_grid((const void*)refine_kernel, 256, 0, 2048)), dim3(256), 0, st, A);
  }
  launch_orient(st, A, batch);
}

void launch_g4_points(hipStream_t st, const Layout& L, const float* gpyr, const float* coef4, const Cand* pts, int n,
                      float* patch, int grid) {
  FillArgs F{L, gpyr, coef4, pts, nullptr, nullptr, n, n, patch};
  hipLaunchKernelGGL(g4_fill_kernel, dim3(g4_grid((const void*)g4_fill_kernel, grid)), dim3(64), 0, st, F);
}

}  // namespace sift
