// undistort_rule.cpp -- csrc/undistort_math.hpp on the host, stand-alone: reads the
// cases tests/undistort_inputs.py::write_cases wrote, runs each with the header's
// own functions in the kernels' order (the camera once, then the pixels or the
// rows) and writes the flag and the bytes for read_results.  Plain host C++ with
// its own main: the place for an address / undefined-behaviour sanitizer build of
// the rule.
//   undistort_rule <cases file> <results file>
// A case is eight int32 and 26 doubles (K, dist, newK or P), then its bytes:
//   image:  {0, pixel, channels, rows, cols, out_rows, out_cols, has_newK}, the packed source
//   points: {1, n, stride, iters, has_P, in_place, 0, 0}, n * stride bytes of rows
// The result of an image is one int32 (the camera's flag) and the packed
// destination; of points one int32 and n * stride bytes (not in place: 0xCD
// wherever the rule writes nothing).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sift-gpu_amd/csrc/undistort_math.hpp"

using namespace sift::umath;
namespace wmath = sift::wmath;

namespace {

bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

Coord coord(const ImageCam& C, bool ok, int x, int y) {
  // through the packed form, as the kernel keeps it
  return unpack(pack(ok ? source_coord(C, x, y) : Coord{0, 0, 0, 0, false}));
}

template <int CH>
void image_u8(const unsigned char* S, int rows, int cols, const ImageCam& C, bool ok, unsigned char* D, int orows,
              int ocols) {
  for (int y = 0; y < orows; ++y)
    for (int x = 0; x < ocols; ++x)
      wmath::pixel_u8<CH>(S, rows, cols, (long long)cols * CH, coord(C, ok, x, y), D + ((size_t)y * ocols + x) * CH);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: undistort_rule <cases> <results>\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) {
    fprintf(stderr, "cannot open the files\n");
    return 2;
  }
  int n_cases = 0;
  for (;;) {
    int32_t h[8];
    const size_t got = fread(h, 1, sizeof(h), in);
    if (got == 0) break;
    double cam[26];
    if (got != sizeof(h) || !read_exact(in, cam, sizeof(cam))) {
      fprintf(stderr, "case %d: truncated header\n", n_cases);
      return 1;
    }
    const double *K = cam, *dist = cam + 9, *third = cam + 17;
    if (h[0] == 0) {
      const int pixel = h[1], ch = h[2], rows = h[3], cols = h[4], orows = h[5], ocols = h[6];
      const size_t bpp = pixel == 0 ? sizeof(float) : (size_t)ch;
      if (rows < 1 || cols < 1 || orows < 1 || ocols < 1 ||
          !((pixel == 0 && ch == 1) || (pixel == 1 && (ch == 1 || ch == 3)))) {
        fprintf(stderr, "case %d: bad header\n", n_cases);
        return 1;
      }
      // the source as floats so that its rows are aligned for either pixel type
      std::vector<float> src(((size_t)rows * cols * bpp + 3) / 4);
      if (!read_exact(in, src.data(), (size_t)rows * cols * bpp)) {
        fprintf(stderr, "case %d: truncated image\n", n_cases);
        return 1;
      }
      const unsigned char* S = reinterpret_cast<const unsigned char*>(src.data());
      ImageCam C;
      const bool ok = image_camera(K, dist, h[7] ? third : nullptr, C);
      std::vector<float> dst(((size_t)orows * ocols * bpp + 3) / 4);
      unsigned char* D = reinterpret_cast<unsigned char*>(dst.data());
      if (pixel == 0) {
        for (int y = 0; y < orows; ++y)
          for (int x = 0; x < ocols; ++x)
            dst[(size_t)y * ocols + x] = wmath::pixel_f32(S, rows, cols, (long long)cols * 4, coord(C, ok, x, y));
      } else if (ch == 1) {
        image_u8<1>(S, rows, cols, C, ok, D, orows, ocols);
      } else {
        image_u8<3>(S, rows, cols, C, ok, D, orows, ocols);
      }
      const int32_t ok32 = ok ? 1 : 0;
      fwrite(&ok32, sizeof(ok32), 1, out);
      fwrite(D, 1, (size_t)orows * ocols * bpp, out);
    } else if (h[0] == 1) {
      const int n = h[1], iters = h[3];
      const size_t stride = (size_t)h[2];
      if (n < 0 || !stride_ok(stride) || !iters_ok(iters)) {
        fprintf(stderr, "case %d: bad header\n", n_cases);
        return 1;
      }
      std::vector<float> src((size_t)n * stride / 4);
      if (!read_exact(in, src.data(), (size_t)n * stride)) {
        fprintf(stderr, "case %d: truncated rows\n", n_cases);
        return 1;
      }
      std::vector<float> other((size_t)n * stride / 4);
      if (n) memset(other.data(), 0xCD, (size_t)n * stride);
      std::vector<float>& dst = h[5] ? src : other;
      PointCam C;
      const bool ok = point_camera(K, dist, h[4] ? third : nullptr, C);
      for (int i = 0; i < n; ++i) {
        const float* p = src.data() + (size_t)i * stride / 4;
        float ou = 0.f, ov = 0.f;
        if (ok) undistort_point(C, iters, p[0], p[1], ou, ov);
        float* q = dst.data() + (size_t)i * stride / 4;
        q[0] = ou;
        q[1] = ov;
      }
      const int32_t ok32 = ok ? 1 : 0;
      fwrite(&ok32, sizeof(ok32), 1, out);
      if (n) fwrite(dst.data(), 1, (size_t)n * stride, out);
    } else {
      fprintf(stderr, "case %d: unknown kind\n", n_cases);
      return 1;
    }
    ++n_cases;
  }
  fclose(in);
  if (fclose(out) != 0) return 1;
  printf("undistort rule ok: %d cases\n", n_cases);
  return 0;
}
