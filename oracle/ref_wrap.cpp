/*
 * ref_wrap.cpp -- extern "C" entry points over the reference's own
 * src/sift.cpp, compiled unmodified over the stand-in headers of
 * oracle/cvmini/ (recipe: oracle/ref_build.py).  TEST INFRASTRUCTURE ONLY.
 *
 * Signatures and packed layouts mirror the so_* functions of sift_oracle.h,
 * so that oracle/refsrc.py and oracle/oracle.py are interchangeable in a
 * test.  buildGaussianPyramid and SIFT_NCL with 5 octaves only: src/sift.cpp:248
 * indexes gpyr[o*nOctaves + i], which is right only when nOctaves == nScales.
 * buildDoGPyramid, findScaleSpaceExtrema and calDescriptor index by nScales and
 * take any count of 1 .. 12 octaves.
 */
#include "sift.hpp"

#include <math.h>
#include <string.h>

namespace {

const int kScales = 5, kDog = 4, kMaxOctaves = 12;

void cap_threads() {
  if (omp_get_max_threads() > 16) omp_set_num_threads(16);
}

Mat view(const float* p, int rows, int cols) {
  return Mat(rows, cols, CV_32FC1, const_cast<float*>(p));
}

/* Headers over a packed pyramid: plane (o, s) at o*per + s, octave o+1 is
 * Size(cols/2, rows/2) of octave o (src/sift.cpp:254). */
std::vector<Mat> views(const float* packed, int rows, int cols, int n_octaves, int per) {
  std::vector<Mat> v;
  size_t off = 0;
  for (int o = 0; o < n_octaves; ++o) {
    for (int s = 0; s < per; ++s) {
      v.push_back(view(packed + off, rows, cols));
      off += (size_t)rows * cols;
    }
    rows /= 2;
    cols /= 2;
  }
  return v;
}

void pack(const std::vector<Mat>& planes, float* out) {
  size_t off = 0;
  for (size_t i = 0; i < planes.size(); ++i) {
    const size_t n = planes[i].total();
    if (n) memcpy(out + off, planes[i].data, n * sizeof(float));
    off += n;
  }
}

}  // namespace

extern "C" {

typedef struct rs_keypoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} rs_keypoint;

void rs_gaussian_blur(const float* src, int rows, int cols, double sigma, float* dst) {
  cap_threads();
  Mat s = view(src, rows, cols), d;
  Gaussian_Blur(s, d, sigma);
  memcpy(dst, d.data, d.total() * sizeof(float));
}

void rs_gaussian_blur_1d(const float* src, int rows, int cols, double sigma, float* dst) {
  cap_threads();
  Mat s = view(src, rows, cols), d;
  Gaussian_Blur_1D(s, d, sigma);
  memcpy(dst, d.data, d.total() * sizeof(float));
}

int rs_build_gaussian_pyramid(const float* img, int rows, int cols, int n_octaves, float* gpyr) {
  if (n_octaves != kScales) return -1;
  cap_threads();
  Mat im = view(img, rows, cols);
  std::vector<Mat> g;
  buildGaussianPyramid(im, g, n_octaves);
  pack(g, gpyr);
  return 0;
}

int rs_build_dog_pyramid(const float* gpyr, int rows, int cols, int n_octaves, float* dog) {
  if (n_octaves < 1 || n_octaves > kMaxOctaves) return -1;
  cap_threads();
  std::vector<Mat> g = views(gpyr, rows, cols, n_octaves, kScales), d;
  buildDoGPyramid(g, d, n_octaves);
  pack(d, dog);
  return 0;
}

/* Writes up to cap keypoints; returns the count found (may exceed cap), -1 for
 * an octave count outside 1 .. 12. */
int rs_find_scale_space_extrema(const float* gpyr, const float* dog, int rows, int cols, int n_octaves,
                                rs_keypoint* kps, int cap) {
  if (n_octaves < 1 || n_octaves > kMaxOctaves) return -1;
  cap_threads();
  std::vector<Mat> g = views(gpyr, rows, cols, n_octaves, kScales);
  std::vector<Mat> d = views(dog, rows, cols, n_octaves, kDog);
  std::vector<KeyPoint> found;
  findScaleSpaceExtrema(g, d, found, n_octaves);
  const int n = (int)found.size();
  if (n) memcpy(kps, found.data(), sizeof(KeyPoint) * (size_t)(n < cap ? n : cap));
  return n;
}

int rs_calc_descriptors(const float* gpyr, int rows, int cols, int n_octaves, const rs_keypoint* kps, int n,
                        float* desc, int first_octave) {
  if (n_octaves < 1 || n_octaves > kMaxOctaves) return -1;
  cap_threads();
  std::vector<Mat> g = views(gpyr, rows, cols, n_octaves, kScales);
  std::vector<KeyPoint> k((size_t)n);
  if (n) memcpy(k.data(), kps, sizeof(KeyPoint) * (size_t)n);
  Mat out = view(desc, n, 128);
  calDescriptor(g, k, out, first_octave);
  return 0;
}

/* SIFT_NCL.  *kps / *desc are malloc'd; free with rs_free. */
int rs_sift(const float* img, int rows, int cols, int n_octaves, rs_keypoint** kps, float** desc) {
  if (n_octaves != kScales) return -1;
  cap_threads();
  Mat im = view(img, rows, cols), d;
  std::vector<KeyPoint> found;
  SIFT_NCL(im, found, d);
  const size_t n = found.size();
  *kps = (rs_keypoint*)malloc(sizeof(rs_keypoint) * (n ? n : 1));
  *desc = (float*)malloc(sizeof(float) * 128 * (n ? n : 1));
  if (n) {
    memcpy(*kps, found.data(), sizeof(KeyPoint) * n);
    memcpy(*desc, d.data, sizeof(float) * 128 * n);
  }
  return (int)n;
}

void rs_free(void* p) { free(p); }

/* Matx33f::solve(b, DECOMP_LU) of the stand-in header; zeros when singular. */
void rs_solve3(const float* a, const float* b, float* x) {
  Matx33f A(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]);
  Vec3f r = A.solve(Vec3f(b[0], b[1], b[2]), DECOMP_LU);
  x[0] = r[0];
  x[1] = r[1];
  x[2] = r[2];
}

/* The stand-in header's primitives and the libm calls as src/sift.cpp makes
 * them, with the op codes of so_helper: 0 exp32f, 1 fastAtan2(a, b),
 * 2 magnitude32f(a, b), 3 cosf(a), 4 sinf(a), 5 powf(2.f, a), 6 cvRound(a),
 * 7 cvFloor(a). */
void rs_helper(int op, const float* a, const float* b, float* out, int n) {
  switch (op) {
    case 0: cv::hal::exp32f(a, out, n); return;
    case 1: cv::hal::fastAtan2(a, b, out, n, true); return;
    case 2: cv::hal::magnitude32f(a, b, out, n); return;
    default: break;
  }
  for (int i = 0; i < n; ++i) {
    float r;
    switch (op) {
      case 3: r = cosf(a[i]); break;
      case 4: r = sinf(a[i]); break;
      case 5: r = powf(2.f, a[i]); break;
      case 6: r = (float)cvRound(a[i]); break;
      default: r = (float)cvFloor(a[i]); break;
    }
    out[i] = r;
  }
}

/* saturate_cast<uchar>(a), as a float. */
void rs_saturate_u8(const float* a, float* out, int n) {
  for (int i = 0; i < n; ++i) out[i] = (float)saturate_cast<uchar>(a[i]);
}

void rs_resize_nn(const float* src, int srows, int scols, float* dst, int drows, int dcols) {
  Mat s = view(src, srows, scols), d;
  resize(s, d, Size(dcols, drows), 0, 0, INTER_NEAREST);
  memcpy(dst, d.data, d.total() * sizeof(float));
}

}  // extern "C"
