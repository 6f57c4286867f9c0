// join_rule.hpp -- the join of two sift_match tables on the keypoint they share,
// for ONE segment on the host, behind sift_join_matches: the rule of
// include/sift_hip.h written as the serial loop it describes.  A batch whose
// tables are already on the device is join.hip's.  Plain host C++ (no HIP
// include), so that tests/cpp/join_rule.cpp runs it under the sanitizers as a
// program of its own.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/sift_hip.h"

namespace sift {

constexpr uint64_t kJoinNoWinner = ~0ull;  // a lookup entry no candidate has reached

// The key a record names on the given side.
inline int join_key(const sift_match& r, int side) { return side == SIFT_JOIN_TRAIN ? r.train : r.query; }

// ((uint64)bits(distance + 0.0f) << 32) | row: for distance >= 0 the bits order
// as the floats do, -0.0 becomes +0.0 by the sum, and +inf (0x7f800000) stays
// below kJoinNoWinner.
inline uint64_t join_rank(float distance, int row) {
  const float d = distance + 0.0f;
  uint32_t bits;
  memcpy(&bits, &d, sizeof(bits));
  return ((uint64_t)bits << 32) | (uint32_t)row;
}

// Returns the number of joined rows; every output may be null.  The caller has
// checked the arguments (sift_join_matches).
inline int join_matches(const sift_match* a, int na, int a_key_side, const unsigned char* a_mask, const double* a_xyz,
                        const sift_match* b, int nb, int b_key_side, const unsigned char* b_mask, const float* b_xy,
                        int n_keys, double* xyz_out, float* xy_out, int* a_row, int* b_row, unsigned char* b_joined) {
  std::vector<uint64_t> lookup((size_t)(n_keys > 0 ? n_keys : 0), kJoinNoWinner);
  for (int i = 0; i < na; ++i) {
    const int key = join_key(a[i], a_key_side);
    if ((a_mask && !a_mask[i]) || key < 0 || key >= n_keys || !(a[i].distance >= 0)) continue;
    const uint64_t r = join_rank(a[i].distance, i);
    if (r < lookup[key]) lookup[key] = r;
  }
  int n = 0;
  for (int i = 0; i < nb; ++i) {
    const int key = join_key(b[i], b_key_side);
    const bool joined = !(b_mask && !b_mask[i]) && key >= 0 && key < n_keys && lookup[key] != kJoinNoWinner;
    if (b_joined) b_joined[i] = joined;
    if (!joined) continue;
    const int w = (int)(uint32_t)lookup[key];
    if (xyz_out) memcpy(xyz_out + (size_t)n * 3, a_xyz + (size_t)w * 3, 3 * sizeof(double));
    if (xy_out) memcpy(xy_out + (size_t)n * 2, b_xy + (size_t)i * 2, 2 * sizeof(float));
    if (a_row) a_row[n] = w;
    if (b_row) b_row[n] = i;
    ++n;
  }
  return n;
}

}  // namespace sift
