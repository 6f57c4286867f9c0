// detmask.hip -- the detection mask of SIFT_NCL (the *_masked entry points):
// cv::KeyPointsFilter::runByPixelsMask on the device, placed where
// SIFT::detectAndCompute applies it -- after the keypoint budget (select.hip),
// before the keypoint scan.
//
// A detection mask is rows x cols bytes per image, the size of the image:
// zero means "no keypoint here".  Every candidate slot ci of image b (slots
// [img_cand_off[b], img_cand_off[b+1]) clamped to cand_cap, as select.hip
// takes them) with npeaks[ci] > 0 stands for npeaks[ci] keypoints that share
// one position, couts[ci].x / .y -- the coordinates the emission writes.  The
// slot is dropped whole (npeaks = 0) iff
//     bytes[(int)(y + 0.5f)][(int)(x + 0.5f)] == 0,
// the sum formed in float and truncated toward zero (so a sum in (-1, 0) is
// index 0).  An index outside [0, rows) x [0, cols), or one formed from a NaN
// coordinate, drops the slot; that test comes first, so no byte outside the
// image's rows x cols is ever read.  The scan, the emission and the descriptor
// pass that follow see a shorter list -- same order, same bytes per keypoint.
// With sift_set_upsample the slots hold positions in the doubled image and the
// mask stays the original image's: x and y are multiplied by 0.5f (exact)
// before the rule, which is then the rule on the emitted coordinates.
//
// One byte gather per live slot; the slots of an image are strided over by
// `parts` workgroups (1 for a batch's ~10^4 slots per image, more for one large
// image: launch_select_best's split).  The grid is (batch, parts), never one
// workgroup per slot of the capacity.
#include <algorithm>

#include "common.hpp"

namespace sift {

namespace {

constexpr int kDetMaskT = 256;

__global__ __launch_bounds__(kDetMaskT) void detmask_kernel(const CandOut* __restrict__ couts, int* npeaks,
                                                            const int* __restrict__ img_cand_off, int cand_cap,
                                                            DetMask dm, int rows, int cols, float pos_scale) {
  const int b = blockIdx.x;
  int lo = img_cand_off[b], hi = img_cand_off[b + 1];
  lo = lo < 0 ? 0 : lo < cand_cap ? lo : cand_cap;
  hi = hi < lo ? lo : hi < cand_cap ? hi : cand_cap;
  const unsigned char* img = dm.bytes + (long long)b * dm.img_stride;
  const long long stride = (long long)gridDim.y * kDetMaskT;
  const float frows = (float)rows, fcols = (float)cols;  // exact: the dimensions are far below 2^24
  for (long long ci = (long long)lo + blockIdx.y * kDetMaskT + threadIdx.x; ci < hi; ci += stride) {
    if (npeaks[ci] <= 0) continue;
    // pos_scale: 1.f, or 0.5f (exact) for candidates of the doubled image -- the emitted position
    const float fx = couts[ci].x * pos_scale + 0.5f, fy = couts[ci].y * pos_scale + 0.5f;
    // the range test on the floats, before the conversion: a NaN fails every
    // comparison, and (int) is taken only of a value in (-1, cols) / (-1, rows)
    bool keep = fx > -1.0f && fx < fcols && fy > -1.0f && fy < frows;
    if (keep) keep = img[(long long)(int)fy * dm.row_stride + (int)fx] != 0;
    if (!keep) npeaks[ci] = 0;
  }
}

}  // namespace

void launch_detmask(hipStream_t st, DetectBufs& D, int batch, const DetMask& dm, int rows, int cols, bool grid_form,
                    bool half) {
  if (!dm.bytes || batch < 1) return;
  // launch_select_best's split: eight strides of a workgroup over the whole list at most
  const int parts = grid_form ? std::min(1024, std::max(1, (D.cand_cap + kDetMaskT * 8 - 1) / (kDetMaskT * 8))) : 1;
  hipLaunchKernelGGL(detmask_kernel, dim3(batch, parts), dim3(kDetMaskT), 0, st, D.couts, D.npeaks, D.img_cand_off,
                     D.cand_cap, dm, rows, cols, half ? 0.5f : 1.f);
}

}  // namespace sift
