// compute_cli.cpp -- the five-argument SIFT_NCL of include/sift.hpp
// (detectAndCompute's useProvidedKeypoints) beside the detect calls.
//   compute_cli <in.pgm>
// Prints the keypoint count and four digests of descriptor bytes: the
// three-argument call's, the five-argument call with useProvidedKeypoints true on
// those keypoints (and a mask of zeros, which it must ignore), the five-argument
// call with false and an empty mask, and true on the first half of the keypoints.
// The provided keypoints must come back unchanged; the exit code says which step
// failed.
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "sift.hpp"

static bool read_pgm(const char* path, Mat& gray) {
  std::ifstream f(path, std::ios::binary);
  std::string magic;
  int w = 0, h = 0, mx = 0;
  f >> magic >> w >> h >> mx;
  f.get();
  if (magic != "P5" || mx != 255 || w <= 0 || h <= 0) return false;
  std::vector<unsigned char> px((size_t)w * h);
  f.read(reinterpret_cast<char*>(px.data()), px.size());
  if (!f) return false;
  gray = Mat(h, w, DATATYPE);
  for (int i = 0; i < h; ++i)
    for (int j = 0; j < w; ++j) gray.at<data_t>(i, j) = (data_t)px[(size_t)i * w + j];
  return true;
}

// FNV-1a over the n x 128 descriptor floats
static unsigned long long digest(Mat& d, int n) {
  unsigned long long h = 1469598103934665603ull;
  if (n == 0) return h;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(d.ptr<float>(0));
  for (size_t i = 0; i < (size_t)n * 128 * sizeof(float); ++i) h = (h ^ p[i]) * 1099511628211ull;
  return h;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cout << "Usage: ./compute_cli <in.pgm>" << std::endl;
    return -1;
  }
  Mat gray;
  if (!read_pgm(argv[1], gray)) return 1;
  Mat zeros(gray.rows, gray.cols, CV_8UC1), empty;
  for (int i = 0; i < gray.rows; ++i)
    for (int j = 0; j < gray.cols; ++j) zeros.at<unsigned char>(i, j) = 0;
  try {
    std::vector<KeyPoint> k3, kf, none;
    Mat d3, dp, df, dh, dn;
    SIFT_NCL(gray, k3, d3);
    const int n = (int)k3.size();
    std::vector<KeyPoint> kp = k3;
    SIFT_NCL(gray, zeros, kp, dp, true);
    if ((int)kp.size() != n || (n && memcmp(kp.data(), k3.data(), sizeof(KeyPoint) * n) != 0)) return 3;
    SIFT_NCL(gray, empty, kf, df, false);
    if ((int)kf.size() != n) return 4;
    std::vector<KeyPoint> half(k3.begin(), k3.begin() + n / 2);
    SIFT_NCL(gray, empty, half, dh, true);
    SIFT_NCL(gray, empty, none, dn, true);  // no keypoint: an empty result, no device call
    if (!none.empty() || dn.rows != 0) return 5;
    printf("%d %016llx %016llx %016llx %016llx\n", n, digest(d3, n), digest(dp, n), digest(df, n),
           digest(dh, n / 2));
  } catch (const std::exception& e) {
    std::cerr << "error: " << e.what() << std::endl;
    return 2;
  }
  return 0;
}
