// detect_mask_cli.cpp -- the four-argument SIFT_NCL of include/sift.hpp
// (detectAndCompute's mask argument) beside the three-argument call.
//   detect_mask_cli <in.pgm> <out.bin>
// The mask keeps the left half plane (columns below cols / 2, value 1).  Writes,
// for the three-argument call, then the four-argument call with that mask, then
// the four-argument call with an empty mask: int32 n, n x 28-byte KeyPoints,
// n x 128 float descriptors.  A CV_32F mask and a mask of another size must
// throw; the exit code says which step failed.
#include <stdio.h>

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

static void dump(FILE* out, const std::vector<KeyPoint>& keypoints, Mat& descriptors) {
  const int n = (int)keypoints.size();
  fwrite(&n, sizeof(int), 1, out);
  if (n) {
    fwrite(keypoints.data(), sizeof(KeyPoint), n, out);
    fwrite(descriptors.ptr<float>(0), sizeof(float) * 128, n, out);
  }
}

template <typename F>
static bool throws(F&& f) {
  try {
    f();
  } catch (const std::exception&) {
    return true;
  }
  return false;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cout << "Usage: ./detect_mask_cli <in.pgm> <out.bin>" << std::endl;
    return -1;
  }
  Mat gray;
  if (!read_pgm(argv[1], gray)) return 1;
  Mat mask(gray.rows, gray.cols, CV_8UC1);
  for (int i = 0; i < gray.rows; ++i)
    for (int j = 0; j < gray.cols; ++j) mask.at<unsigned char>(i, j) = j < gray.cols / 2 ? 1 : 0;
  FILE* out = fopen(argv[2], "wb");
  if (!out) return 3;
  try {
    std::vector<KeyPoint> k3, k4, k0;
    Mat d3, d4, d0;
    SIFT_NCL(gray, k3, d3);
    dump(out, k3, d3);
    SIFT_NCL(gray, mask, k4, d4);
    dump(out, k4, d4);
    Mat empty;
    SIFT_NCL(gray, empty, k0, d0);
    dump(out, k0, d0);
    printf("%d %d %d keypoints\n", (int)k3.size(), (int)k4.size(), (int)k0.size());
    Mat fmask(gray.rows, gray.cols, CV_32FC1), small(gray.rows - 1, gray.cols, CV_8UC1);
    if (!throws([&] { SIFT_NCL(gray, fmask, k0, d0); })) return 4;
    if (!throws([&] { SIFT_NCL(gray, small, k0, d0); })) return 5;
  } catch (const std::exception& e) {
    std::cerr << "error: " << e.what() << std::endl;
    fclose(out);
    return 2;
  }
  fclose(out);
  return 0;
}
