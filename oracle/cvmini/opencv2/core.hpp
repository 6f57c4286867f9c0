/*
 * cvmini -- stand-in for the slice of OpenCV 4.0 that the reference's
 * src/sift.cpp uses, so that its own translation unit compiles unchanged
 * without OpenCV (oracle/ref_build.py).  TEST INFRASTRUCTURE ONLY.
 *
 * This is the one real header; every other file under cvmini/ forwards here.
 * The primitives (cvRound, cvFloor, saturate_cast<uchar>, hal::exp32f,
 * hal::fastAtan2, hal::magnitude32f, Matx33f::solve(DECOMP_LU),
 * resize(INTER_NEAREST)) are written from SURVEY.md Appendix A, independently
 * of oracle/sift_oracle.c: a third statement of the same semantics, checked
 * against the other two in tests/test_reference_source.py.
 *
 * Deliberately absent: scalar cv::exp / cv::sqrt / cv::pow.  The reference's
 * exp(...), sqrt(...) and pow(...) on doubles must resolve to libm, as they do
 * with the real headers.
 *
 * Everything is evaluated with separate multiply and add (the reference's
 * flags have no -march, so x86-64 has no FMA to contract into).
 */
#ifndef CVMINI_OPENCV2_CORE_HPP_
#define CVMINI_OPENCV2_CORE_HPP_

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <cfloat>
#include <chrono>
#include <climits>
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#if defined(__SSE2__)
#include <emmintrin.h>
#endif

#define CV_PI 3.1415926535897932384626433832795
#define CV_8U 0
#define CV_32F 5
#define CV_8UC1 0
#define CV_32FC1 5

#define CV_Assert(expr)                                                              \
  do {                                                                               \
    if (!(expr)) ::cv::cvmini_fail(#expr, __FILE__, __LINE__);                       \
  } while (0)

namespace cv {

typedef unsigned char uchar;
typedef int64_t int64;

inline void cvmini_fail(const char* expr, const char* file, int line) {
  throw std::runtime_error(std::string("CV_Assert(") + expr + ") failed at " + file + ":" + std::to_string(line));
}

enum { DECOMP_LU = 0 };
enum { INTER_NEAREST = 0, INTER_LINEAR = 1 };

/* ---- rounding helpers ------------------------------------------------------
 * cvRound is SSE2 cvtss2si / cvtsd2si: the current MXCSR rounding mode, which
 * is round-half-to-even by default; NaN and out-of-range give INT_MIN. */
inline int cvRound(float v) {
#if defined(__SSE2__)
  return _mm_cvtss_si32(_mm_set_ss(v));
#else
  return (int)std::nearbyint(v);
#endif
}
inline int cvRound(double v) {
#if defined(__SSE2__)
  return _mm_cvtsd_si32(_mm_set_sd(v));
#else
  return (int)std::nearbyint(v);
#endif
}
inline int cvRound(int v) { return v; }
/* cvFloor: the mathematical floor, as an int. */
inline int cvFloor(float v) { return (int)std::floor(v); }
inline int cvFloor(double v) { return (int)std::floor(v); }
inline int cvFloor(int v) { return v; }

template <typename T>
inline T saturate_cast(float v);
template <>
inline uchar saturate_cast<uchar>(float v) {
  const int iv = cvRound(v);
  return (uchar)(iv > 255 ? 255 : iv > 0 ? iv : 0);
}
template <>
inline int saturate_cast<int>(float v) {
  return cvRound(v);
}

inline int64 getTickCount() {
  return (int64)std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}
inline double getTickFrequency() { return 1e9; }

/* ---- points, sizes, keypoints ---------------------------------------------- */
struct Point {
  int x, y;
  Point() : x(0), y(0) {}
  Point(int x_, int y_) : x(x_), y(y_) {}
};
struct Point2f {
  float x, y;
  Point2f() : x(0), y(0) {}
  Point2f(float x_, float y_) : x(x_), y(y_) {}
};
struct Size {
  int width, height;
  Size() : width(0), height(0) {}
  Size(int w, int h) : width(w), height(h) {}
};

/* {Point2f pt; float size, angle, response; int octave, class_id;}: 28 bytes. */
class KeyPoint {
 public:
  KeyPoint() : pt(0, 0), size(0), angle(-1), response(0), octave(0), class_id(-1) {}
  KeyPoint(Point2f p, float sz, float ang = -1, float resp = 0, int oct = 0, int cls = -1)
      : pt(p), size(sz), angle(ang), response(resp), octave(oct), class_id(cls) {}
  Point2f pt;
  float size;
  float angle;
  float response;
  int octave;
  int class_id;
};
static_assert(sizeof(KeyPoint) == 28, "cv::KeyPoint layout");

/* ---- Mat: continuous, refcounted planes ----------------------------------- */
struct MatSize {
  int r, c;
  bool operator==(const MatSize& o) const { return r == o.r && c == o.c; }
  bool operator!=(const MatSize& o) const { return !(*this == o); }
};

class Mat {
 public:
  int rows, cols;
  uchar* data;
  MatSize size;

  Mat() : rows(0), cols(0), data(nullptr), size{0, 0}, type_(CV_32F) {}
  Mat(int r, int c, int type) : rows(0), cols(0), data(nullptr), size{0, 0}, type_(CV_32F) { create(r, c, type); }
  /* A header over memory the caller owns (never freed here). */
  Mat(int r, int c, int type, void* ext)
      : rows(r), cols(c), data(static_cast<uchar*>(ext)), size{r, c}, type_(type) {}

  void create(int r, int c, int type) {
    if (r == rows && c == cols && type == type_ && data) return;
    if (type != CV_32F && type != CV_8U) throw std::runtime_error("cvmini: unsupported Mat type");
    const size_t n = (size_t)r * c * elem(type);
    buf_ = std::shared_ptr<uchar>(new uchar[n ? n : 1], std::default_delete<uchar[]>());
    data = buf_.get();
    rows = r;
    cols = c;
    size = MatSize{r, c};
    type_ = type;
  }
  void release() {
    buf_.reset();
    data = nullptr;
    rows = cols = 0;
    size = MatSize{0, 0};
  }
  int type() const { return type_; }
  bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
  size_t step1() const { return (size_t)cols; }
  size_t total() const { return (size_t)rows * cols; }
  template <typename T>
  T* ptr(int i = 0) {
    return reinterpret_cast<T*>(data + (size_t)i * cols * elem(type_));
  }
  template <typename T>
  const T* ptr(int i = 0) const {
    return reinterpret_cast<const T*>(data + (size_t)i * cols * elem(type_));
  }
  template <typename T>
  T& at(int i, int j) {
    return ptr<T>(i)[j];
  }
  template <typename T>
  const T& at(int i, int j) const {
    return ptr<T>(i)[j];
  }
  /* a - b, element by element, for CV_32FC1 (the DoG). */
  friend Mat operator-(const Mat& a, const Mat& b) {
    if (a.size != b.size || a.type_ != CV_32F || b.type_ != CV_32F)
      throw std::runtime_error("cvmini: operator- needs equal-size CV_32FC1 Mats");
    Mat d(a.rows, a.cols, CV_32F);
    const float *pa = a.ptr<float>(), *pb = b.ptr<float>();
    float* pd = d.ptr<float>();
    for (size_t i = 0; i < a.total(); ++i) pd[i] = pa[i] - pb[i];
    return d;
  }

 private:
  static size_t elem(int t) { return t == CV_32F ? 4 : 1; }
  std::shared_ptr<uchar> buf_;
  int type_;
};

class _InputArray {
 public:
  _InputArray(const Mat& m) : m_(&m) {}
  Mat getMat() const { return *m_; }

 private:
  const Mat* m_;
};

class _OutputArray {
 public:
  _OutputArray(Mat& m) : m_(&m) {}
  void create(int r, int c, int type) const { m_->create(r, c, type); }
  Mat getMat() const { return *m_; }
  Mat& getMatRef() const { return *m_; }

 private:
  Mat* m_;
};

typedef const _InputArray& InputArray;
typedef const _OutputArray& OutputArray;

/* ---- resize, INTER_NEAREST only ------------------------------------------
 * ifx = 1 / (dst_w / src_w) in double; sx = min(floor(x * ifx), src_w - 1);
 * the same down the rows. */
inline void resize(InputArray src_, OutputArray dst_, Size dsize, double = 0, double = 0,
                   int interpolation = INTER_LINEAR) {
  if (interpolation != INTER_NEAREST) throw std::runtime_error("cvmini: resize supports INTER_NEAREST only");
  const Mat src = src_.getMat();
  if (src.type() != CV_32F) throw std::runtime_error("cvmini: resize needs CV_32FC1");
  Mat out(dsize.height, dsize.width, CV_32F);
  const double scale_x = (double)dsize.width / src.cols, scale_y = (double)dsize.height / src.rows;
  const double ifx = 1. / scale_x, ify = 1. / scale_y;
  std::vector<int> xofs((size_t)dsize.width);
  for (int x = 0; x < dsize.width; ++x) {
    const int sx = cvFloor(x * ifx);
    xofs[(size_t)x] = sx < src.cols - 1 ? sx : src.cols - 1;
  }
  for (int y = 0; y < dsize.height; ++y) {
    int sy = cvFloor(y * ify);
    if (sy > src.rows - 1) sy = src.rows - 1;
    const float* s = src.ptr<float>(sy);
    float* d = out.ptr<float>(y);
    for (int x = 0; x < dsize.width; ++x) d[x] = s[xofs[(size_t)x]];
  }
  dst_.getMatRef() = out;
}

/* ---- small fixed matrices -------------------------------------------------- */
struct Matx31f {
  float val[3];
  Matx31f() { val[0] = val[1] = val[2] = 0; }
  Matx31f(float a, float b, float c) {
    val[0] = a;
    val[1] = b;
    val[2] = c;
  }
  float operator()(int i) const { return val[i]; }
  float& operator()(int i) { return val[i]; }
  /* Matx::dot: s = 0; s += a_i * b_i, in the element type. */
  float dot(const Matx31f& m) const {
    float s = 0;
    for (int i = 0; i < 3; ++i) s += val[i] * m.val[i];
    return s;
  }
};

struct Vec3f : Matx31f {
  Vec3f() {}
  Vec3f(float a, float b, float c) : Matx31f(a, b, c) {}
  Vec3f(const Matx31f& m) : Matx31f(m) {}
  float operator[](int i) const { return val[i]; }
  float& operator[](int i) { return val[i]; }
};

struct Matx33f {
  float val[9];
  Matx33f() {
    for (int i = 0; i < 9; ++i) val[i] = 0;
  }
  Matx33f(float v0, float v1, float v2, float v3, float v4, float v5, float v6, float v7, float v8) {
    const float v[9] = {v0, v1, v2, v3, v4, v5, v6, v7, v8};
    for (int i = 0; i < 9; ++i) val[i] = v[i];
  }
  float operator()(int i, int j) const { return val[i * 3 + j]; }
  float& operator()(int i, int j) { return val[i * 3 + j]; }

  /* Matx * Vec: s = 0; s += a(i,k) * b(k). */
  Vec3f operator*(const Matx31f& b) const {
    Vec3f r;
    for (int i = 0; i < 3; ++i) {
      float s = 0;
      for (int k = 0; k < 3; ++k) s += (*this)(i, k) * b(k);
      r(i) = s;
    }
    return r;
  }

  /* solve(b, DECOMP_LU) on a 3 x 3 system: the closed form.  d = (float)det(A)
   * by cofactor expansion along row 0 in float; d == 0 gives zeros; otherwise
   * x(i) = (1/d) * (the Cramer numerator of column i), each expanded along
   * row 0 of A with b substituted. */
  Vec3f solve(const Matx31f& b, int method) const {
    if (method != DECOMP_LU) throw std::runtime_error("cvmini: solve supports DECOMP_LU only");
    const Matx33f& a = *this;
    const double det = a(0, 0) * (a(1, 1) * a(2, 2) - a(2, 1) * a(1, 2)) -
                       a(0, 1) * (a(1, 0) * a(2, 2) - a(2, 0) * a(1, 2)) +
                       a(0, 2) * (a(1, 0) * a(2, 1) - a(2, 0) * a(1, 1));
    float d = (float)det;
    Vec3f x;
    if (d == 0) return x;
    d = 1 / d;
    x(0) = d * (b(0) * (a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)) -
                a(0, 1) * (b(1) * a(2, 2) - a(1, 2) * b(2)) +
                a(0, 2) * (b(1) * a(2, 1) - a(1, 1) * b(2)));
    x(1) = d * (a(0, 0) * (b(1) * a(2, 2) - a(1, 2) * b(2)) -
                b(0) * (a(1, 0) * a(2, 2) - a(1, 2) * a(2, 0)) +
                a(0, 2) * (a(1, 0) * b(2) - b(1) * a(2, 0)));
    x(2) = d * (a(0, 0) * (a(1, 1) * b(2) - b(1) * a(2, 1)) -
                a(0, 1) * (a(1, 0) * b(2) - b(1) * a(2, 0)) +
                b(0) * (a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0)));
    return x;
  }
};

/* ---- buffers and per-thread storage ---------------------------------------- */
template <typename T>
class AutoBuffer {
 public:
  explicit AutoBuffer(size_t n) : v_(n ? n : 1) {}
  operator T*() { return v_.data(); }
  operator const T*() const { return v_.data(); }
  size_t size() const { return v_.size(); }

 private:
  std::vector<T> v_;
  AutoBuffer(const AutoBuffer&);
  AutoBuffer& operator=(const AutoBuffer&);
};

/* Serial use only: one slot, the caller's. */
template <typename T>
class TLSData {
 public:
  TLSData() {}
  T* get() const { return &slot_; }
  T& getRef() const { return slot_; }
  void gather(std::vector<T*>& out) const { out.push_back(&slot_); }

 private:
  mutable T slot_;
  TLSData(const TLSData&);
  TLSData& operator=(const TLSData&);
};

template <typename T>
using Ptr = std::shared_ptr<T>;

/* ---- hal ------------------------------------------------------------------- */
namespace hal {

/* exp32f with a 64-entry table (EXPTAB_SCALE = 6):
 *   x clamped to +-3000*64 / (log2(e)*64); x *= log2(e)*64 (float);
 *   xi = round(x); f = (x - xi) / 64; t = clamp((xi >> 6) + 127, 0, 255);
 *   y = float(t << 23) * tab[xi & 63] * ((((f + A1) f + A2) f + A3) f + A4),
 * tab[i] = (float)(2^(i/64) * A0), A1..A4 = (float)(c_k / A0). */
struct ExpTab32f {
  float tab[64];
  ExpTab32f() {
    const double A0 = 0.009670371139572338;
    for (int i = 0; i < 64; ++i) tab[i] = (float)((double)powl(2.0L, (long double)i / 64) * A0);
  }
};

inline void exp32f(const float* src, float* dst, int n) {
  static const ExpTab32f T;
  const double A0 = 0.009670371139572338;
  const float A1 = (float)(0.05550339366753125 / A0), A2 = (float)(0.2402265109513301 / A0);
  const float A3 = (float)(0.6931471805521448 / A0), A4 = (float)(1.000000000000002 / A0);
  const double log2e = 1.4426950408889634;
  const float prescale = (float)(log2e * 64), postscale = (float)(1. / 64);
  const float maxv = (float)(3000. * 64 / (log2e * 64)), minv = -maxv;
  for (int i = 0; i < n; ++i) {
    float x = src[i];
    x = x < minv ? minv : x;
    x = x > maxv ? maxv : x;
    x *= prescale;
    const int xi = cvRound(x);
    const float f = (x - (float)xi) * postscale;
    int t = (xi >> 6) + 127;
    t = t < 0 ? 0 : t > 255 ? 255 : t;
    const uint32_t bits = (uint32_t)t << 23;
    float scale;
    memcpy(&scale, &bits, sizeof scale);
    const float tail = (((f + A1) * f + A2) * f + A3) * f + A4;
    dst[i] = (scale * T.tab[xi & 63]) * tail;
  }
}

/* fastAtan2 in degrees: a 7th-order odd polynomial in min/max of |x|, |y|,
 * unfolded by octant; the result lies in [0, 360]. */
inline void fastAtan2(const float* Y, const float* X, float* angle, int n, bool in_degrees) {
  if (!in_degrees) throw std::runtime_error("cvmini: fastAtan2 supports degrees only");
  const float scale = (float)(180 / CV_PI);
  const float p1 = 0.9997878412794807f * scale, p3 = -0.3258083974640975f * scale;
  const float p5 = 0.1555786518463281f * scale, p7 = -0.04432655554792128f * scale;
  const float eps = (float)DBL_EPSILON;
  for (int i = 0; i < n; ++i) {
    const float x = X[i], y = Y[i];
    const float ax = std::abs(x), ay = std::abs(y);
    float a, c, c2;
    if (ax >= ay) {
      c = ay / (ax + eps);
      c2 = c * c;
      a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
      c = ax / (ay + eps);
      c2 = c * c;
      a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    angle[i] = a;
  }
}

inline void magnitude32f(const float* x, const float* y, float* dst, int n) {
  for (int i = 0; i < n; ++i) {
    const float x0 = x[i], y0 = y[i];
    dst[i] = std::sqrt(x0 * x0 + y0 * y0);
  }
}

}  // namespace hal

/* ---- link-only stubs for SITF_BuildIn_OpenCV -------------------------------- */
namespace xfeatures2d {
class SIFT {
 public:
  static Ptr<SIFT> create() { throw std::runtime_error("cvmini: cv::xfeatures2d::SIFT is a stub"); }
  void detectAndCompute(InputArray, InputArray, std::vector<KeyPoint>&, OutputArray, bool = false) {
    throw std::runtime_error("cvmini: cv::xfeatures2d::SIFT is a stub");
  }
  void clear() { throw std::runtime_error("cvmini: cv::xfeatures2d::SIFT is a stub"); }
};
}  // namespace xfeatures2d

}  // namespace cv

#endif /* CVMINI_OPENCV2_CORE_HPP_ */
