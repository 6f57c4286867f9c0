// warp_rule.cpp -- csrc/warp_math.hpp on the host, stand-alone: reads the cases
// tests/warp_inputs.py::write_cases wrote, warps each with the header's own
// functions in the kernel's order (M once, the row terms once per row, then
// the pixels) and writes M, ok and the warped image for read_results.  Plain
// host C++ with its own main: the place for an address / undefined-behaviour
// sanitizer build of the rule.
//   warp_rule <cases file> <results file>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sift-gpu_amd/csrc/warp_math.hpp"

using namespace sift::wmath;

namespace {

bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

template <int CH>
void warp_u8(const unsigned char* S, int rows, int cols, const double* M, bool ok, unsigned char* D, int orows,
             int ocols) {
  for (int y = 0; y < orows; ++y) {
    const RowTerms R = row_terms(M, y);
    for (int x = 0; x < ocols; ++x) {
      const Coord c = ok ? source_coord(M, R, x) : Coord{0, 0, 0, 0, false};
      pixel_u8<CH>(S, rows, cols, (long long)cols * CH, c, D + ((size_t)y * ocols + x) * CH);
    }
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: warp_rule <cases> <results>\n");
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
    double H[9], M[9];
    if (got != sizeof(h) || !read_exact(in, H, sizeof(H))) {
      fprintf(stderr, "case %d: truncated header\n", n_cases);
      return 1;
    }
    const int pixel = h[0], ch = h[1], rows = h[2], cols = h[3], orows = h[4], ocols = h[5];
    const bool inverse = h[6] != 0, found = h[7] != 0;
    const size_t bpp = pixel == 0 ? sizeof(float) : (size_t)ch;
    if (rows < 1 || cols < 1 || orows < 1 || ocols < 1 || !((pixel == 0 && ch == 1) || (pixel == 1 && (ch == 1 || ch == 3)))) {
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
    const bool m_ok = warp_matrix(H, inverse, M);
    const bool ok = m_ok && found;
    std::vector<float> dst(((size_t)orows * ocols * bpp + 3) / 4);
    unsigned char* D = reinterpret_cast<unsigned char*>(dst.data());
    if (pixel == 0) {
      for (int y = 0; y < orows; ++y) {
        const RowTerms R = row_terms(M, y);
        for (int x = 0; x < ocols; ++x) {
          const Coord c = ok ? source_coord(M, R, x) : Coord{0, 0, 0, 0, false};
          dst[(size_t)y * ocols + x] = pixel_f32(S, rows, cols, (long long)cols * 4, c);
        }
      }
    } else if (ch == 1) {
      warp_u8<1>(S, rows, cols, M, ok, D, orows, ocols);
    } else {
      warp_u8<3>(S, rows, cols, M, ok, D, orows, ocols);
    }
    const int32_t ok32 = m_ok ? 1 : 0;
    fwrite(M, sizeof(double), 9, out);
    fwrite(&ok32, sizeof(ok32), 1, out);
    fwrite(D, 1, (size_t)orows * ocols * bpp, out);
    ++n_cases;
  }
  fclose(in);
  if (fclose(out) != 0) return 1;
  printf("warp rule ok: %d cases\n", n_cases);
  return 0;
}
