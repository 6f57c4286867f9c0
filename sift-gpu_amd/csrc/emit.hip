// emit.hip -- ordered keypoint emission from the scan of the per-candidate
// peak counts, and the end-of-call status block.
#include "detect_args.hpp"

namespace sift {

// ---- ordered keypoint emission ------------------------------------------------
// HALF (sift_set_upsample): the candidates are the doubled image's; the
// keypoint goes out in the original image's frame -- x, y and size times 0.5f
// (exact) and the octave byte one lower, 255 for octave -1 -- which is what
// SIFT::detectAndCompute does to every keypoint when firstOctave < 0.
template <bool HALF>
__global__ __launch_bounds__(256) void emit_kernel(const CandOut* __restrict__ couts,
                                                   const int* __restrict__ kp_scan,
                                                   const int* __restrict__ cand_total, int cand_cap,
                                                   sift_keypoint* __restrict__ kpts, int kp_cap) {
  int n = *cand_total;
  if (n > cand_cap) n = cand_cap;
  for (int ci = blockIdx.x * 256 + threadIdx.x; ci < n; ci += gridDim.x * 256) {
    const int base = kp_scan[ci];
    const int np = kp_scan[ci + 1] - base;
    if (np == 0) continue;
    const CandOut& co = couts[ci];
    for (int k = 0; k < np; ++k) {
      const int pos = base + k;
      if (pos >= kp_cap) break;
      sift_keypoint kp;
      kp.x = HALF ? co.x * 0.5f : co.x;
      kp.y = HALF ? co.y * 0.5f : co.y;
      kp.size = HALF ? co.size * 0.5f : co.size;
      kp.angle = co.angle[k];
      kp.response = co.response;
      kp.octave = HALF ? (co.octave & ~255) | ((co.octave - 1) & 255) : co.octave;
      kp.class_id = -1;
      kpts[pos] = kp;
    }
  }
}

// End-of-call status (one lane).  err[0..2] are sticky words (assertion,
// candidate workspace overflow, keypoint capacity exceeded); this call's own
// overflows are added to them.  stat = {candidates, keypoints, this call's
// bits, all sticky bits} (bit i <-> err[i]), copied by the host to pinned
// memory in the same stream, so it arrives with the stream synchronisation.
__global__ void status_kernel(const int* __restrict__ cand_total, int cand_cap, const int* __restrict__ img_off,
                              int batch, int kp_cap, int* __restrict__ err, int* __restrict__ stat) {
  if (threadIdx.x != 0) return;
  const int ct = cand_total ? *cand_total : 0;
  const int n = img_off ? img_off[batch] : 0;
  const int fresh = (err[0] ? kErrAssert : 0) | (ct > cand_cap ? kErrWorkspace : 0) | (n > kp_cap ? kErrKpCapacity : 0) |
                    (err[3] ? kErrStall : 0);
  if (fresh & kErrWorkspace) err[1] = 1;
  if (fresh & kErrKpCapacity) err[2] = 1;
  stat[0] = ct;
  stat[1] = n;
  stat[2] = fresh;
  stat[3] = (err[0] ? kErrAssert : 0) | (err[1] ? kErrWorkspace : 0) | (err[2] ? kErrKpCapacity : 0) |
            (err[3] ? kErrStall : 0);
}

void launch_status(hipStream_t st, const int* cand_total, int cand_cap, const int* img_off, int batch, int kp_cap,
                   int* err, int* stat) {
  hipLaunchKernelGGL(status_kernel, dim3(1), dim3(64), 0, st, cand_total, cand_cap, img_off, batch, kp_cap, err,
                     stat);
}

void launch_emit(hipStream_t st, DetectBufs& D, int batch, sift_keypoint* kpts, int kp_cap,
                 int* img_kp_off, bool half) {
  // kp_scan = exclusive scan of npeaks over the (clamped) candidate list
  launch_scan(st, D.npeaks, D.kp_scan, D.cand_total, 0, D.cand_cap, D.kp_total, D.scan_tiles,
              ScanGather{D.img_cand_off, 0, batch, img_kp_off});
  if (half)
    hipLaunchKernelGGL(emit_kernel<true>, dim3(1024), dim3(256), 0, st, D.couts, D.kp_scan, D.cand_total,
                       D.cand_cap, kpts, kp_cap);
  else
    hipLaunchKernelGGL(emit_kernel<false>, dim3(1024), dim3(256), 0, st, D.couts, D.kp_scan, D.cand_total,
                       D.cand_cap, kpts, kp_cap);
}

}  // namespace sift
