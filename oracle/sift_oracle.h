/*
 * sift_oracle.h -- CPU restatement of the reference SIFT hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing in the shipped library links, loads or
 * calls this code.  Only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg may use it, and only as the checker / CPU baseline.
 *
 * What it restates: canhld94/SIFT-GPU src/sift.cpp (the whole SIFT_NCL path,
 * file:line cited per function in sift_oracle.c) plus the OpenCV-4.0
 * internals that file calls (cvRound, cvFloor, saturate_cast<uchar>,
 * hal::exp32f, hal::fastAtan2, hal::magnitude32f, Matx33f::solve(DECOMP_LU),
 * resize(INTER_NEAREST)) as documented in SURVEY.md Appendix A.
 *
 * PINNED TO THE REFERENCE'S SOURCE: src/sift.cpp's own text, compiled with its
 * makefile's flags over stand-in OpenCV primitives (oracle/cvmini/,
 * oracle/ref_build.py), is compared with this restatement bit for bit in
 * tests/test_reference_source.py, and its recorded outputs
 * (tests/golden/ref_*.npz) with the GPU.  They agree on every plane and every
 * keypoint field; the only differences are the libm calls (powf, cosf, sinf)
 * that sift_oracle.c replaces on purpose.  NOT pinned: the OpenCV primitives
 * themselves (both sides restate them from SURVEY.md Appendix A), SIMD
 * dispatch inside real OpenCV, the front end's resize, BFMatcher,
 * findHomography.  The other fixtures in tests/golden/ are vectors produced
 * by this oracle.
 *
 * Arithmetic contract: compiled with -O2 -ffp-contract=off, no -march, no
 * -ffast-math -- the reference's own makefile:25 flags (-O3, no -march) give
 * IEEE single precision with separate multiply and add on x86-64 (SSE2).
 */
#ifndef SIFT_ORACLE_H_
#define SIFT_ORACLE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Layout-identical to cv::KeyPoint (5 floats + 2 int32 = 28 bytes). */
typedef struct so_keypoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} so_keypoint;

#define SO_N_SCALES 5  /* nOctaveLayers + 3, src/sift.cpp:5 */
#define SO_N_DOG 4     /* nScales - 1 */

/* Octave shapes: octave o+1 is Size(cols/2, rows/2) of octave o
 * (src/sift.cpp:254).  Fills rows[o], cols[o] for o < n_octaves. */
void so_octave_shapes(int rows, int cols, int n_octaves, int* orows, int* ocols);

/* Packed pyramid layout: plane (o, s) starts at element off[o*per+s] where
 * per = 5 for the Gaussian pyramid and 4 for DoG.  Returns total elements. */
size_t so_pyramid_offsets(int rows, int cols, int n_octaves, int per, size_t* off);

/* 2-D Gaussian coefficients x8192 (src/sift.cpp:95-108).  coeff must hold
 * ksize*ksize floats (ksize <= 2*floor(3*sigma)+1).  Returns ksize. */
int so_gaussian_kernel(float sigma, float* coeff);

/* Gaussian_Blur (src/sift.cpp:123-153). */
void so_gaussian_blur(const float* src, int rows, int cols, double sigma, float* dst);

/* Gaussian_Blur_1D (src/sift.cpp:157-217), taps k in [-w, w-1]. */
void so_gaussian_blur_1d(const float* src, int rows, int cols, double sigma, float* dst);

/* resize(..., INTER_NEAREST) to (drows, dcols) (src/sift.cpp:254). */
void so_resize_nn(const float* src, int srows, int scols, float* dst, int drows, int dcols);

/* buildGaussianPyramid (src/sift.cpp:229-263), packed output (5 planes per
 * octave, correct o*5+s indexing -- identical to the reference at 5). */
void so_build_gaussian_pyramid(const float* img, int rows, int cols, int n_octaves, float* gpyr);

/* The library's SIFT_FLAG_FAST separable pyramid (agreement mode, not the
 * reference's arithmetic), in its exact operation order; packed like
 * so_build_gaussian_pyramid. */
void so_fast_pyramid(const float* img, int rows, int cols, int n_octaves, float* gpyr);

/* buildDoGPyramid (src/sift.cpp:265-283), packed output (4 planes/octave). */
void so_build_dog_pyramid(const float* gpyr, int rows, int cols, int n_octaves, float* dog);

/* findScaleSpaceExtrema (src/sift.cpp:547-577).  Writes up to cap keypoints
 * and returns the total count found (may exceed cap). */
int so_find_scale_space_extrema(const float* gpyr, const float* dog, int rows, int cols,
                                int n_octaves, so_keypoint* kps, int cap);

/* Branch counters of the last so_find_scale_space_extrema call (so_sift
 * included), for tests that must know which paths an input reaches.  Purely
 * additive: counting changes no result.  The extrema stage is serial, the
 * counters are plain globals (not thread-safe across concurrent calls). */
enum {
  SO_ST_RAW = 0,       /* 26-neighbour extrema above the threshold (scan_layer) */
  SO_ST_REJ_HUGE,      /* an offset above INT_MAX/3 (src/sift.cpp:335-337)      */
  SO_ST_REJ_LAYER,     /* moved out of layers 1..nOctaveLayers (:344)           */
  SO_ST_REJ_BORDER,    /* moved into the image border (:345-347)                */
  SO_ST_REJ_MAXIT,     /* no convergence in SIFT_MAX_INTERP_STEPS (:351)        */
  SO_ST_REJ_CONTRAST,  /* |contrast| * nOctaveLayers < 0.04 (:365)              */
  SO_ST_REJ_DET,       /* det <= 0 (:377)                                       */
  SO_ST_REJ_EDGE,      /* edge ratio (:377), det > 0                            */
  SO_ST_MOVED_LAYER,   /* converged after a step that changed the layer         */
  SO_ST_MOVED_RC,      /* converged after a step that changed r or c            */
  SO_ST_POS,           /* raw extrema with v > 0                                */
  SO_ST_NEG,           /* raw extrema with v < 0                                */
  SO_ST_KEPT,          /* candidates that passed adjustLocalExtrema             */
  SO_ST_CLIPPED,       /* kept, orientation window clipped by the interior      */
  SO_ST_MAX_RADIUS,    /* largest orientation radius (a maximum, not a count)   */
  SO_ST_PEAKS,         /* [19] kept candidates with 0..18 orientation peaks     */
  SO_ST_KP = SO_ST_PEAKS + 19, /* [8][2] keypoints of octave o (< 8), layer 1..2 */
  SO_ST_KP_OCTAVES = 8,
  SO_STATS_LEN = SO_ST_KP + SO_ST_KP_OCTAVES * 2
};
/* Copies min(n, SO_STATS_LEN) counters into out; returns SO_STATS_LEN. */
int so_extrema_stats(long long* out, int n);
void so_extrema_stats_reset(void);

/* calDescriptor (src/sift.cpp:733-753): n rows of 128 floats. */
void so_calc_descriptors(const float* gpyr, int rows, int cols, int n_octaves,
                         const so_keypoint* kps, int n, float* desc, int first_octave);

/* SIFT_NCL (src/sift.cpp:59-91).  *kps / *desc are malloc'd; caller frees
 * with so_free.  Returns the keypoint count. */
int so_sift(const float* img, int rows, int cols, int n_octaves, so_keypoint** kps, float** desc);
void so_free(void* p);

/* Number of OpenMP threads for the descriptor loop (src/sift.cpp:738). */
void so_set_threads(int n);

/* Test-only switch, off by default (0): when on, powf (src/sift.cpp:384) and
 * cosf / sinf (:583-584) are libm's, as in the reference's text, instead of
 * (float)f((double)x).  Used only to compare this file with the reference's own
 * source byte for byte; so_helper ops 3-5 keep the default definition. */
void so_set_libm(int on);
int so_get_libm(void);
/* Test-only: the descriptor's orientation bin wrapped modulo n (circular) instead of once. */
void so_set_wrap_mod(int on);

/* Synthetic integer-exact test image, SURVEY.md 8(d) row d2. */
void so_synth_image(int b, int rows, int cols, float* out);

/* OpenCV-internal helpers, exported for unit tests. */
void so_exp32f(const float* x, float* y, int n);
void so_fast_atan2(const float* y, const float* x, float* out, int n);
void so_magnitude32f(const float* x, const float* y, float* out, int n);
int so_solve3(const float* a9, const float* b3, float* x3); /* 1 ok, 0 singular (x=0) */
int so_cv_round(float v);
/* Element-wise helper evaluation with the same op codes as the library's
 * sift_selftest_math: 0 exp32f, 1 fastAtan2(a,b), 2 magnitude(a,b),
 * 3 (float)cos((double)a), 4 (float)sin((double)a), 5 (float)exp2((double)a),
 * 6 cvRound(a), 7 cvFloor(a). */
void so_helper(int op, const float* a, const float* b, float* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* SIFT_ORACLE_H_ */
