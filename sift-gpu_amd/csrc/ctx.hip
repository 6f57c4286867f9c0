// ctx.hip -- the context behind the C ABI (include/sift_hip.h): pyramid
// layout, occupancy cache, math constants, creation / destruction / setters,
// device workspace growth, the status protocol and per-stage HIP-event
// profiling.  Host code only.
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>

#include "graph.hpp"

namespace sift {

// The defaults the tests read (tests/adversarial_inputs.py): a fresh context
// holds max(kCandidateFloor, pixels / kPixelsPerCandidate) candidate slots per
// image, and kKeypointsPerCandidateSlot keypoints per slot in its own buffer.
constexpr long long kCandidateFloor = 16384;
constexpr long long kPixelsPerCandidate = 32;
constexpr int kKeypointsPerCandidateSlot = 2;

Layout make_layout(int rows, int cols, int n_oct) {
  Layout L;
  memset(&L, 0, sizeof(L));
  L.n_oct = n_oct;
  L.rows = rows;
  L.cols = cols;
  long long g = 0, d = 0;
  int r = rows, c = cols;
  for (int o = 0; o < n_oct; ++o, halve(r, c)) {
    Octave& O = L.oct[o];
    O.rows = r;
    O.cols = c;
    O.pitch = round_up(c > 0 ? c : 1, kPitchAlign);
    const long long plane = (long long)O.rows * O.pitch;
    for (int s = 0; s < kScales; ++s) O.g_off[s] = g + s * plane;
    for (int s = 0; s < kDogPer; ++s) O.d_off[s] = d + s * plane;
    g += kScales * plane;
    d += kDogPer * plane;
  }
  L.g_img = g;
  L.d_img = d;
  return L;
}

int resident_grid(const void* kernel, int block, size_t lds, int fixed_grid) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, int> cache;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fixed_grid;
  std::lock_guard<std::mutex> lk(mu);
  const auto key = std::make_pair(kernel, dev);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int per_cu = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per_cu < 1 ||
      cus < 1)
    return fixed_grid;
  const int g = std::max(8, per_cu * cus / 8 * 8);
  cache[key] = g;
  return g;
}

void host_math_consts(MathConsts* mc) {
  const double A0 = .9670371139572337719125840413672004409288e-2;
  const double prescale = 1.4426950408889634073599246810019 * 64;
  const double maxval = 3000. * 64;
  mc->e.A4 = (float)(1.000000000000002438532970795181890933776 / A0);
  mc->e.A3 = (float)(.6931471805521448196800669615864773144641 / A0);
  mc->e.A2 = (float)(.2402265109513301490103372422686535526573 / A0);
  mc->e.A1 = (float)(.5550339366753125211915322047004666939128e-1 / A0);
  mc->e.lo = (float)(-maxval / prescale);
  mc->e.hi = (float)(maxval / prescale);
  mc->e.post = (float)(1. / 64);
  mc->e.prescale = (float)prescale;
  for (int j = 0; j < 64; ++j) mc->exptab[j] = (float)((double)exp2l((long double)j / 64.0L) * A0);
  const float deg = (float)(180 / kCvPi);
  mc->t.p1 = 0.9997878412794807f * deg;
  mc->t.p3 = -0.3258083974640975f * deg;
  mc->t.p5 = 0.1555786518463281f * deg;
  mc->t.p7 = -0.04432655554792128f * deg;
  mc->t.eps = (float)DBL_EPSILON;
}

hipEvent_t get_event(sift_ctx* c) {
  if (!c->pool.empty()) {
    hipEvent_t e = c->pool.back();
    c->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

int check_dims(sift_ctx* c, int rows, int cols, int n_oct, int batch) {
  if (rows <= 0 || cols <= 0) return fail(c, SIFT_E_INVALID, "image dimensions must be positive");
  if (n_oct < 1 || n_oct > kMaxOctaves) return fail(c, SIFT_E_INVALID, "n_octaves out of range");
  if ((rows >> (n_oct - 1)) < 1 || (cols >> (n_oct - 1)) < 1)
    return fail(c, SIFT_E_INVALID,
                "image too small: every octave must keep at least one row and column "
                "(the reference's resize to an empty Size throws)");
  if (rows > c->max_rows || cols > c->max_cols || batch > c->max_batch || n_oct > c->max_oct)
    return fail(c, SIFT_E_SIZE, "image/batch exceeds the context's creation limits");
  if (batch < 1) return fail(c, SIFT_E_INVALID, "batch must be >= 1");
  return SIFT_OK;
}

int enter(sift_ctx* c, bool bufs_ok, const char* null_msg, int rows, int cols, int n_oct, int batch) {
  if (!c) return SIFT_E_INVALID;
  if (!bufs_ok) return fail(c, SIFT_E_INVALID, null_msg);
  if (int rc = check_dims(c, rows, cols, n_oct, batch)) return rc;
  (void)hipSetDevice(c->device);
  return SIFT_OK;
}

// SIFT_FLAG_FAST preconditions: pyramid_pc.hip's literal taps equal the host
// formula, and every plane and the input rows stay below the buffer offset
// its dropped loads and stores use (without the size check a plane
// of ~530 M pixels would read real pixels as padding and write inside itself).
int check_fast(sift_ctx* c, const Layout& L, long long src_row_stride) {
  if (!(c->flags & SIFT_FLAG_FAST)) return SIFT_OK;
  if (!c->fast_ok) return fail(c, SIFT_E_INVALID, "SIFT_FLAG_FAST: compiled-in separable taps differ from the host's");
  if (!pyramid_fast_fits(L, src_row_stride))
    return fail(c, SIFT_E_SIZE,
                "SIFT_FLAG_FAST: the octave-0 plane or the input rows exceed the separable pyramid's "
                "2,130,706,432-byte buffer-offset range");
  return SIFT_OK;
}

// coefficient scratch for arbitrary sigma
int ensure_coef_gen(sift_ctx* c, size_t n) {
  HIP_TRY(c, c->d_coef_gen.grow(n));
  return SIFT_OK;
}

int ensure_kp(sift_ctx* c, int need) {
  if (need <= c->kp_cap) return SIFT_OK;
  drop_graphs(c);  // captured sequences name the old buffers
  c->kp_cap = 0;
  HIP_TRY(c, c->d_kpts.grow((size_t)need));
  HIP_TRY(c, c->d_desc.grow((size_t)need * kDescLen));
  c->kp_cap = need;
  return SIFT_OK;
}

// The descriptor's ranking scratch (one int per keypoint the descriptor pass
// can see); grown before any capture (captured sequences name the buffer).
int ensure_perm(sift_ctx* c, int need) {
  if (need <= (int)c->d_perm.count()) return SIFT_OK;
  drop_graphs(c);
  HIP_TRY(c, c->d_perm.grow((size_t)need));
  return SIFT_OK;
}

int ensure_match(sift_ctx* c, size_t bytes) {
  if (bytes <= c->d_match.count()) return SIFT_OK;
  if (c->d_match.get()) HIP_TRY(c, hipStreamSynchronize(c->stream));  // queued work may still use the old block
  if (c->d_match.grow(bytes) != hipSuccess) return fail(c, SIFT_E_NOMEM, "match scratch");
  return SIFT_OK;
}

// Candidate-list workspace for cap extrema (all images of a batch), plus the
// internal keypoint buffer at kKeypointsPerCandidateSlot keypoints per slot.
// Captured sequences carry cand_cap, so they go even when nothing moves.
int alloc_candidates(sift_ctx* c, int cap) {
  drop_graphs(c);
  const size_t scan_n = (size_t)std::max<long long>(c->blk_cap, cap) + 1;
  const bool ok = c->cands.grow((size_t)cap) == hipSuccess && c->couts.grow((size_t)cap) == hipSuccess &&
                  c->kp_scan.grow((size_t)cap + 1) == hipSuccess && c->npeaks.grow((size_t)cap) == hipSuccess &&
                  c->scan_tmp.grow(scan_n) == hipSuccess &&
                  c->scan_tiles.grow((size_t)scan_tiles_for((long long)scan_n) + 1) == hipSuccess &&
                  c->g4patch.grow((size_t)cap * 9) == hipSuccess && c->rstate.grow((size_t)cap) == hipSuccess &&
                  c->g4wait.grow((size_t)cap * 2) == hipSuccess && c->g4stat.grow(kG4Stats) == hipSuccess;
  c->D = DetectBufs{c->mask,    c->blk_counts, c->cand_total, c->img_cand_off, c->cands,    ok ? cap : 0,
                    c->couts,   c->kp_scan,    c->kp_total,   c->npeaks,       c->scan_tmp, c->scan_tiles,
                    c->g4patch, c->rstate,     c->g4wait,     c->g4stat,       c->sel_hist};
  if (!ok) return fail(c, SIFT_E_NOMEM, "candidate workspace allocation failed");
  HIP_TRY(c, hipMemset(c->g4stat, 0, kG4Stats * sizeof(int)));  // sift_g4_fill_stats before any detection
  return ensure_kp(c, (int)std::min<long long>((long long)cap * kKeypointsPerCandidateSlot, 1 << 28));
}

// End of every compute sequence: status_kernel folds the candidate and
// keypoint capacity checks into the sticky error word and the status block is
// copied to pinned host memory on the same stream, so the host learns the
// counts from the one stream synchronisation it already does.
// img_off == nullptr: no keypoint count (calDescriptor); check_cand false: no
// candidate check (no detection ran).
void enqueue_status(sift_ctx* c, bool check_cand, const int* img_off, int batch, int kp_cap) {
  launch_status(c->stream, check_cand ? c->D.cand_total : nullptr, c->D.cand_cap, img_off, batch, kp_cap, c->d_err,
                c->d_stat);
  (void)hipMemcpyAsync(c->h_stat, c->d_stat, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream);
}

// After a stream sync: interprets the pinned status block of the last
// compute call -- its own bits (sticky = false: host entry points) or every
// bit not yet reported (sticky = true: sift_sync) -- restricted to mask, and
// clears the device words of the bits it consumes.  kp_internal: keypoint
// overflow of the context's own buffer is the caller's growth case.
int take_status(sift_ctx* c, bool sticky, int mask, bool kp_internal) {
  const int ct = c->h_stat[0], n = c->h_stat[1];
  int e = (sticky ? c->h_stat[3] : c->h_stat[2]) & mask;
  for (int i = 0; i < 4; ++i)
    if (e & (1 << i)) HIP_TRY(c, hipMemsetAsync(c->d_err + i, 0, sizeof(int), c->stream));
  c->h_stat[2] &= ~e;
  c->h_stat[3] &= ~e;
  if (kp_internal) e &= ~kErrKpCapacity;
  if (!e) return SIFT_OK;
  if (e & kErrWorkspace)
    return fail(c, SIFT_E_WORKSPACE,
                "candidate workspace overflow: capacity " + std::to_string(c->D.cand_cap) + " < " +
                    std::to_string(ct) + " extrema (sift_set_candidate_capacity, or a larger context)");
  if (e & kErrStall)
    return fail(c, SIFT_E_HIP, "an in-kernel pipeline wait expired (pyramid_pc.hip): the SIFT_FLAG_FAST planes are invalid");
  if (e & kErrAssert)
    return fail(c, SIFT_E_INVALID,
                "keypoint octave/layer outside the pyramid (CV_Assert at src/sift.cpp:744)");
  return fail(c, SIFT_E_CAPACITY, "keypoint total " + std::to_string(n) +
                                      " exceeds the output capacity (see d_img_offsets[batch])");
}

}  // namespace sift

using namespace sift;

namespace {

const char* const kStageNames[] = {
#define X(id, name) name,
    SIFT_STAGES(X)
#undef X
};

void drain_profile(sift_ctx* c) {
  if (c->recs.empty()) return;
  (void)hipStreamSynchronize(c->stream);
  for (auto& r : c->recs) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, r.a, r.b);
    c->acc_ms[r.stage] += ms;
    c->acc_flops[r.stage] += r.flops;
    c->acc_bytes[r.stage] += r.bytes;
    c->acc_n[r.stage] += 1;
    c->pool.push_back(r.a);
    c->pool.push_back(r.b);
  }
  c->recs.clear();
}

int max_octaves_for(int rows, int cols) {
  int n = 0;
  while (n < kMaxOctaves && (rows >> n) >= 1 && (cols >> n) >= 1) ++n;
  return n;
}

}  // namespace

extern "C" {

int sift_graph_stats(const sift_ctx* c, long long* captures, long long* updates, long long* instantiations) {
  if (!c || !captures || !updates || !instantiations) return SIFT_E_INVALID;
  *captures = c->graph_captures;
  *updates = c->graph_updates;
  *instantiations = c->graph_instantiations;
  return SIFT_OK;
}

const char* sift_version(void) { return "sift-hip 0.2 (gfx950; exact + SIFT_FLAG_FAST separable pyramid)"; }

int sift_octave_shapes(int rows, int cols, int n_octaves, int* orows, int* ocols) {
  if (n_octaves < 1 || n_octaves > kMaxOctaves || !orows || !ocols) return SIFT_E_INVALID;
  for (int o = 0; o < n_octaves; ++o, halve(rows, cols)) {
    orows[o] = rows;
    ocols[o] = cols;
  }
  return SIFT_OK;
}

size_t sift_packed_size(int rows, int cols, int n_octaves, int per) {
  size_t t = 0;
  for (int o = 0; o < n_octaves; ++o, halve(rows, cols)) t += (size_t)per * rows * cols;
  return t;
}

int sift_ctx_create(int device, int max_rows, int max_cols, int max_batch, unsigned flags,
                    sift_ctx** out) {
  if (!out || max_rows < 1 || max_cols < 1 || max_batch < 1) return SIFT_E_INVALID;
  *out = nullptr;
  // descriptor.hip gathers with 32-bit element offsets inside one plane
  // (row * pitch + col): an octave-0 plane must stay below 2^31 elements
  if ((long long)max_rows * round_up(max_cols, kPitchAlign) >= (1ll << 31)) return SIFT_E_SIZE;
  if (hipSetDevice(device) != hipSuccess) return SIFT_E_HIP;
  sift_ctx* c = new sift_ctx();
  c->device = device;
  c->flags = flags;
  c->max_rows = max_rows;
  c->max_cols = max_cols;
  c->max_batch = max_batch;
  c->max_oct = max_octaves_for(max_rows, max_cols);
  auto bail = [&](int code) {  // frees whatever the context owns so far
    sift_ctx_destroy(c);
    return code;
  };
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail(SIFT_E_HIP);
  c->own_stream = true;
  const Layout L = make_layout(max_rows, max_cols, c->max_oct);
  c->in_pitch = round_up(max_cols, kPitchAlign);
  c->in_img = c->in_pitch * max_rows;
  c->gpyr_elems = L.g_img * max_batch;
  c->dog_elems = L.d_img * max_batch;
  if (c->d_in.grow((size_t)c->in_img * max_batch) != hipSuccess ||
      c->d_gpyr.grow((size_t)c->gpyr_elems) != hipSuccess || c->d_dog.grow((size_t)c->dog_elems) != hipSuccess ||
      c->d_tmp.grow((size_t)c->in_img) != hipSuccess || c->d_grad.grow((size_t)c->gpyr_elems) != hipSuccess)
    return bail(SIFT_E_NOMEM);
  // Gaussian coefficients: base sigma sqrt(1.6^2 + 0.2^2) (src/sift.cpp:237)
  // and sig[1..4] (src/sift.cpp:240-245), each through getGaussianKernel(float).
  std::vector<float> coefs;
  float sig_f[4] = {0, 0, 0, 0};
  float sb = 0;
  sift_sigmas(&sb, sig_f);
  {
    const int ks = gaussian_kernel_host(sb, nullptr);
    c->w_base = ks / 2;
    c->coef_base_off = 0;
    coefs.resize(ks * ks);
    gaussian_kernel_host(sb, coefs.data());
    c->coef_oct_off = coefs.size();
    for (int i = 1; i < kScales; ++i) {
      const float sg = sig_f[i - 1];
      const int kk = gaussian_kernel_host(sg, nullptr);
      c->wsz[i - 1] = kk / 2;
      const size_t at = coefs.size();
      coefs.resize(at + kk * kk);
      gaussian_kernel_host(sg, coefs.data() + at);
    }
  }
  if (c->w_base != 4 || c->wsz[0] != 4 || c->wsz[1] != 8 || c->wsz[2] != 12 || c->wsz[3] != 18)
    return bail(SIFT_E_INVALID);  // the octave kernel is unrolled for these widths
  {
    // the scatter-form blur carries these tables as literals; the gather-form
    // kernels (same chain, twice the multiplies) stay as the path for any
    // mismatch and for A/B runs (SIFT_HIP_BLUR_GATHER=1)
    const char* e = getenv("SIFT_HIP_BLUR_GATHER");
    c->sym_blur = sym_tables_match(coefs.data()) && !(e && atoi(e) != 0);
    // a scatter walk is a tall column strip (its halo is recomputed per
    // chunk), so it needs many strips to fill the chip; small launches (one
    // 1080p or 8K image, the last octaves of a batch) keep the 2-D tiles.
    // SIFT_HIP_SYM_MIN=0 forces it (tests).
    const char* m = getenv("SIFT_HIP_SYM_MIN");
    if (m) c->sym_min = atoi(m);
    const char* r = getenv("SIFT_HIP_SYM_ROWS_MIN");
    if (r) c->sym_rows = atoi(r);
    const char* sm = getenv("SIFT_HIP_SMALL_MAX");
    if (sm) c->small_max = atoll(sm);
    // the sparse flow's point evaluation reads sig[4]'s table from d_coef,
    // which sym_tables_match ties to the scatter blur's literals
    const char* dg = getenv("SIFT_HIP_DENSE_G4");
    c->sparse_g4 = c->sym_blur && !(dg && atoi(dg) != 0);
    // test hook: small inputs reach the fill's striding and uneven XCD ranges
    const char* gg = getenv("SIFT_HIP_G4_GRID");
    const int g = gg ? atoi(gg) : 0;
    c->g4_grid = g == 8 || g == 16 ? g : 0;
    // the keypoint budget's select: 0 = always the multi-workgroup form
    const char* sel = getenv("SIFT_HIP_SELECT_BLOCK_MAX");
    if (sel) c->select_block_max = atoll(sel);
  }
  // SIFT_FLAG_FAST: pyramid_pc.hip carries its 1-D taps as literals; a
  // mismatch with the host formula makes the flag an error (enqueue-time check)
  c->fast_ok = fast_taps_match(sb, sig_f);
  {
    const char* th = getenv("SIFT_HIP_TEST_HOOKS");
    const std::string hooks = "," + std::string(th ? th : "") + ",";
    c->poison_pad = hooks.find(",poison_pad,") != std::string::npos;
    c->stall_once = hooks.find(",pc_stall_once,") != std::string::npos;
  }
  MathConsts mc;
  host_math_consts(&mc);
  if (c->d_coef.grow(coefs.size()) != hipSuccess || c->d_mc.grow(1) != hipSuccess ||
      c->d_err.grow(4) != hipSuccess || c->d_stat.grow(4) != hipSuccess || c->h_stat.grow(4) != hipSuccess)
    return bail(SIFT_E_NOMEM);
  memset(c->h_stat, 0, 4 * sizeof(int));
  if (hipMemcpy(c->d_coef, coefs.data(), coefs.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(c->d_mc, &mc, sizeof(mc), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(c->d_err, 0, 4 * sizeof(int)) != hipSuccess)
    return bail(SIFT_E_HIP);
  // detection workspace
  const long long px = (long long)max_rows * max_cols;
  const long long cap = std::max(kCandidateFloor, px / kPixelsPerCandidate) * max_batch;
  if (cap > (1ll << 30)) return bail(SIFT_E_NOMEM);
  c->blk_cap = mask_blocks_per_image(L) * max_batch;
  if (c->mask.grow((size_t)mask_words_per_image(L) * max_batch) != hipSuccess ||
      c->blk_counts.grow(c->blk_cap) != hipSuccess || c->cand_total.grow(1) != hipSuccess ||
      c->img_cand_off.grow(max_batch + 1) != hipSuccess || c->kp_total.grow(1) != hipSuccess ||
      c->sel_hist.grow((size_t)max_batch * kSelectPasses * kSelectBins) != hipSuccess ||
      c->d_img_off.grow(max_batch + 1) != hipSuccess || alloc_candidates(c, (int)cap) != SIFT_OK)
    return bail(SIFT_E_NOMEM);
  if (hipMemset(c->D.cand_total, 0, sizeof(int)) != hipSuccess) return bail(SIFT_E_HIP);
  *out = c;
  return SIFT_OK;
}

// Only what has an order is spelled out: the device, the stream's queued work,
// events and graphs, then every buffer with the context itself, and the
// stream last.
int sift_ctx_destroy(sift_ctx* c) {
  if (!c) return SIFT_OK;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (auto& r : c->recs) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  for (auto e : c->pool) (void)hipEventDestroy(e);
  drop_graphs(c);
  const hipStream_t owned = c->own_stream ? c->stream : nullptr;
  delete c;
  if (owned) (void)hipStreamDestroy(owned);
  return SIFT_OK;
}

const char* sift_last_error(const sift_ctx* c) { return c ? c->err.c_str() : "null context"; }

int sift_set_stream(sift_ctx* c, void* s) {
  if (!c) return SIFT_E_INVALID;
  if (c->own_stream && c->stream) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamDestroy(c->stream);
  }
  drop_graphs(c);  // captured on the old stream
  c->stream = (hipStream_t)s;
  c->own_stream = false;
  return SIFT_OK;
}

void* sift_get_stream(sift_ctx* c) { return c ? (void*)c->stream : nullptr; }

int sift_set_flags(sift_ctx* c, unsigned flags) {
  if (!c) return SIFT_E_INVALID;
  c->flags = flags;
  return SIFT_OK;
}

int sift_set_octaves(sift_ctx* c, int n) {
  if (!c) return SIFT_E_INVALID;
  if (n < 1 || n > c->max_oct) return fail(c, SIFT_E_INVALID, "n_octaves out of range");
  c->n_oct = n;
  return SIFT_OK;
}

int sift_set_max_features(sift_ctx* c, int n_per_image) {
  if (!c) return SIFT_E_INVALID;
  if (n_per_image < 0) return fail(c, SIFT_E_INVALID, "max_features must be >= 0");
  c->max_features = n_per_image;  // part of the SIFT_NCL graph key: no captured sequence is replayed with another budget
  return SIFT_OK;
}

int sift_set_upsample(sift_ctx* c, int on) {
  if (!c) return SIFT_E_INVALID;
  c->upsample = on != 0;  // part of the SIFT_NCL and sift_compute graph keys, like the budget
  return SIFT_OK;
}

int sift_set_candidate_capacity(sift_ctx* c, int per_image) {
  if (!c) return SIFT_E_INVALID;
  if (per_image < 1 || (long long)per_image * c->max_batch > (1ll << 30))
    return fail(c, SIFT_E_INVALID, "candidate capacity out of range");
  (void)hipSetDevice(c->device);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->last_n = -1;
  return alloc_candidates(c, per_image * c->max_batch);
}

int sift_sync(sift_ctx* c) {
  if (!c) return SIFT_E_INVALID;
  (void)hipSetDevice(c->device);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return take_status(c, true, kAllErr);
}

int sift_get_stage_stats(sift_ctx* c, sift_stage_stat* out, int cap, int* n, int reset) {
  if (!c) return SIFT_E_INVALID;
  drain_profile(c);
  int k = 0;
  for (int s = 0; s < ST_N; ++s) {
    if (!c->acc_n[s]) continue;
    if (out && k < cap) {
      memset(&out[k], 0, sizeof(out[k]));
      strncpy(out[k].name, kStageNames[s], sizeof(out[k].name) - 1);
      out[k].launches = c->acc_n[s];
      out[k].ms = c->acc_ms[s];
      out[k].flops = c->acc_flops[s];
      out[k].bytes = c->acc_bytes[s];
    }
    ++k;
  }
  if (n) *n = k;
  if (reset)
    for (int s = 0; s < ST_N; ++s) c->acc_ms[s] = c->acc_flops[s] = c->acc_bytes[s] = c->acc_n[s] = 0;
  return SIFT_OK;
}

}  // extern "C"
