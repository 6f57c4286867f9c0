// pose.hip -- recoverPose and triangulatePoints for ONE set of point pairs on the
// host, behind sift_recover_pose and sift_triangulate_points: host code like
// fundamental.hip, for the same reason.  A batch whose point pairs are already
// on the device is pose_batch.hip's; both take every expression from
// pose_math.hpp (the rule is written out there), and this file keeps only the
// serial control flow.
#include <string.h>

#include "common.hpp"
#include "pose_math.hpp"

namespace sift {

using namespace pmath;

int recover_pose(const double* F, const double* K_src, const double* K_dst, const float* src_xy, const float* dst_xy,
                 int n, const unsigned char* mask_in, double distance_thresh, double* pose, double* E,
                 unsigned char* mask_out, double* xyz, int* n_good) {
  const P2* s = reinterpret_cast<const P2*>(src_xy);
  const P2* d = reinterpret_cast<const P2*>(dst_xy);
  memset(pose, 0, 12 * sizeof(double));
  if (E) memset(E, 0, 9 * sizeof(double));
  if (mask_out) memset(mask_out, 0, (size_t)n);
  if (xyz) memset(xyz, 0, (size_t)n * 3 * sizeof(double));
  *n_good = 0;
  Decomp D;
  if (!thresh_ok(distance_thresh) || !decompose(F, K_src, K_dst, D)) return 0;
  int count[kCandidates] = {0, 0, 0, 0};
  for (int c = 0; c < kCandidates; ++c)
    for (int i = 0; i < n; ++i) {
      double q[3];
      if (mask_in && !mask_in[i]) continue;
      count[c] += good_point(D, D.P[c], s[i], d[i], distance_thresh, q);
    }
  const int w = winner(count);
  if (count[w] < 1) return 0;
  for (int i = 0; i < n; ++i) {
    double q[3];
    if (mask_in && !mask_in[i]) continue;
    if (!good_point(D, D.P[w], s[i], d[i], distance_thresh, q)) continue;
    if (mask_out) mask_out[i] = 1;
    if (xyz) memcpy(xyz + (size_t)i * 3, q, sizeof(q));
  }
  memcpy(pose, D.P[w], 12 * sizeof(double));
  if (E) memcpy(E, D.E, 9 * sizeof(double));
  *n_good = count[w];
  return 1;
}

void triangulate_points(const double* P_src, const double* P_dst, const float* src_xy, const float* dst_xy, int n,
                        double* xyzw) {
  const P2* s = reinterpret_cast<const P2*>(src_xy);
  const P2* d = reinterpret_cast<const P2*>(dst_xy);
  for (int i = 0; i < n; ++i) triangulate(P_src, P_dst, s[i].x, s[i].y, d[i].x, d[i].y, xyzw + (size_t)i * 4);
}

}  // namespace sift
