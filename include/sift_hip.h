/*
 * sift_hip.h -- C ABI of libsift_hip.so, the MI355X (gfx950) SIFT detect+compute
 * library.  Plain C types only: no OpenCV, no C++ and no torch types cross
 * this boundary, so any FFI (ctypes, cgo, JNI, N-API) can bind it.
 *
 * Each entry point names the reference interface it replaces
 * (canhld94/SIFT-GPU include/sift.hpp, src/sift.cpp).  The C++ drop-in that
 * restores the reference's own signatures on top of this ABI is
 * include/sift.hpp (implemented in sift-gpu_amd/cpp/sift_shim.cpp).
 *
 * Conventions
 *  - Every function returns SIFT_OK (0) or a negative SIFT_E_* code; the
 *    message is available from sift_last_error(ctx).  Nothing calls exit().
 *  - A context owns device workspace sized at creation for images up to
 *    max_rows x max_cols and batches up to max_batch, plus one HIP stream.
 *    A context is not thread-safe: use one per host thread.
 *  - "host" entry points take and return host memory and synchronise; the
 *    "_device" / "_batch" entry points take device pointers, enqueue on the
 *    context stream and return immediately (call sift_sync to wait).
 *  - Results equal the reference CPU path bit for bit in the default (exact)
 *    mode.  SIFT_FLAG_FAST selects the separable LDS-tiled pyramid, which is
 *    not bit-exact.
 */
#ifndef SIFT_HIP_H_
#define SIFT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIFT_OK 0
#define SIFT_E_INVALID (-1)   /* bad argument */
#define SIFT_E_HIP (-2)       /* HIP runtime error */
#define SIFT_E_CAPACITY (-3)  /* output capacity too small; required count reported */
#define SIFT_E_SIZE (-4)      /* image/batch larger than the context was created for */
#define SIFT_E_NOMEM (-5)     /* device allocation failed */
#define SIFT_E_WORKSPACE (-6) /* the context's internal candidate workspace overflowed
                                 (an input far more textured than the context was sized
                                 for): no result is held, *n_out = -1; create the context
                                 with a larger max size.  Not the two-call sizing case. */

#define SIFT_FLAG_FAST 0x1u     /* separable fused pyramid (not bit-exact) */
#define SIFT_FLAG_PROFILE 0x2u  /* per-stage HIP-event timing, see sift_get_stage_stats */
#define SIFT_FLAG_VERBOSE 0x4u  /* print the reference's phase timings (src/sift.cpp:70,80,88) */
#define SIFT_FLAG_NO_GRAPH 0x8u /* launch every kernel directly instead of replaying the context's
                                   cached hipGraph of the compute sequence (graphs are also off
                                   under SIFT_FLAG_PROFILE / SIFT_FLAG_VERBOSE) */

#define SIFT_DESC_LEN 128
#define SIFT_N_SCALES 5         /* Gaussian planes per octave */
#define SIFT_N_DOG 4            /* DoG planes per octave */

/* Layout-identical to cv::KeyPoint {Point2f pt; float size, angle, response;
 * int octave, class_id;} = 28 bytes.  octave packs o | layer<<8 | xi<<16
 * exactly as src/sift.cpp:383 does. */
typedef struct sift_keypoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} sift_keypoint;

typedef struct sift_ctx sift_ctx;

typedef struct sift_stage_stat {
  char name[32];
  int launches;
  double ms;     /* summed device time over launches (HIP events) */
  double flops;  /* algorithmic flops summed over launches */
  double bytes;  /* algorithmic HBM bytes summed over launches */
} sift_stage_stat;

/* ---- context ------------------------------------------------------------ */
int sift_ctx_create(int device, int max_rows, int max_cols, int max_batch, unsigned flags,
                    sift_ctx** out);
int sift_ctx_destroy(sift_ctx* ctx);
const char* sift_last_error(const sift_ctx* ctx);
/* Use an external HIP stream (hipStream_t) instead of the context's own. */
int sift_set_stream(sift_ctx* ctx, void* hip_stream);
void* sift_get_stream(sift_ctx* ctx);
int sift_set_flags(sift_ctx* ctx, unsigned flags);
/* Number of octaves (default 5, the literal at src/sift.cpp:67,68,78). */
int sift_set_octaves(sift_ctx* ctx, int n_octaves);
/* Waits for the context stream, then reports the sticky device status of the
 * calls since the last report: SIFT_E_WORKSPACE (candidate workspace
 * overflow), SIFT_E_CAPACITY (a batch call's keypoint total exceeded its
 * kp_cap), SIFT_E_INVALID (calDescriptor's CV_Assert, src/sift.cpp:744). */
int sift_sync(sift_ctx* ctx);
/* Candidate (26-neighbour extremum) slots per image of the batch; the default
 * is max(16384, max_rows * max_cols / 32), about 5x the extrema of a textured
 * 1080p image.  Reallocates the workspace (synchronises). */
int sift_set_candidate_capacity(sift_ctx* ctx, int per_image);
/* Per-image keypoint budget of SIFT_NCL -- OpenCV's SIFT::create(nfeatures),
 * which the reference leaves at "all".  n_per_image = 0 (the default) keeps
 * every keypoint and launches nothing extra.  With n > 0, for each image of a
 * call whose keypoint count K (every orientation peak is one keypoint)
 * exceeds n: let T be the n-th largest response among the K keypoints,
 * counted with multiplicity; every keypoint with response >= T is kept, the
 * others are dropped (cv::KeyPointsFilter::retainBest).  So an image keeps at
 * least n keypoints and more than n exactly when responses tie at the cut --
 * the peaks of one extremum share a response, so this is common -- and
 * batch * n rows is NOT a bound on a batch's total.  An image with K <= n is
 * unchanged.  The kept keypoints stay in the unlimited order (OpenCV's own
 * order after retainBest is unspecified): each image's output is a
 * subsequence of its unlimited output, and each kept keypoint's 28 bytes and
 * 128 descriptor floats are the unlimited run's bit for bit.  The selection
 * runs on the device before the descriptors, so dropped keypoints cost no
 * descriptor work.  d_img_offsets, the counts, *n_out and every capacity
 * rule (kp_cap: only the first kp_cap rows written, the true total in
 * d_img_offsets[batch], SIFT_E_CAPACITY from sift_sync; the host calls'
 * two-call sizing) refer to the kept keypoints: a kp_cap too small for the
 * unlimited total but large enough for the kept total succeeds.  NaN
 * responses (NaN images) select an unspecified, in-bounds subset.
 * Applies to sift_detect_compute, sift_detect_compute_batch (exact and
 * SIFT_FLAG_FAST) and sift_multi_step; not to sift_find_scale_space_extrema
 * (OpenCV filters in detectAndCompute, not there).  n_per_image < 0 or a NULL
 * context: SIFT_E_INVALID, the setting is unchanged. */
int sift_set_max_features(sift_ctx* ctx, int n_per_image);
/* The upsampled first octave: Lowe's "octave -1", SIFT::create()'s default
 * firstOctave = -1, which the reference leaves out (its createInitialImage
 * ignores doubleSize).  on == 0 (the default) launches nothing, allocates
 * nothing and leaves every output as it is.  With on != 0, sift_detect_compute,
 * sift_detect_compute_masked, sift_detect_compute_batch[_masked], sift_compute
 * and sift_compute_batch double each image on the device into a buffer the
 * context owns (sift_upsample2x_device's rule, below; the buffer is allocated by
 * the first upsampled call) and run their sequence, unchanged, on the
 * 2 rows x 2 cols image: the reference's base blur sqrt(1.6^2 + 0.2^2) -- not
 * OpenCV's sqrt(sigma^2 - 1) for a doubled image, which is out of scope -- the
 * context's octave count applied to the doubled image (a caller who wants the
 * same coarsest octave sets one more), exact mode and SIFT_FLAG_FAST alike.
 * The context must have been created for the doubled shape: 2 rows > max_rows
 * or 2 cols > max_cols is SIFT_E_SIZE, and the candidate capacity and the
 * SIFT_E_WORKSPACE rule are the doubled image's.
 * Keypoints come out in the original image's frame, by OpenCV's post-pass in
 * detectAndCompute for firstOctave < 0, applied where the keypoints are
 * emitted: x, y and size are multiplied by 0.5f (exact), the low byte of
 * octave is decremented -- (octave & ~255) | ((octave - 1) & 255), so 255 is
 * octave -1 -- and angle, response and class_id are unchanged.  Each image's
 * keypoints are the doubled run's, in its order; each descriptor row is the
 * doubled run's bit for bit (the descriptor stage runs with first_octave = -1,
 * and unpackOctave maps each emitted row back onto the doubled pyramid exactly).
 * The keypoint budget selects as in the doubled run (responses are unchanged).
 * A detection mask stays rows x cols of the original image and is read at the
 * emitted coordinates, mask[(int)(y + 0.5f)][(int)(x + 0.5f)].
 * sift_compute[_batch]: keypoints are in original-image coordinates, the
 * pyramid is the doubled image's, first_octave is -1, and the valid octaves
 * are -1 .. n_octaves - 2; with the setting off a row with octave -1 stays an
 * invalid row.  The setting is part of the graph-cache key of both sequences.
 * Not applied by sift_find_scale_space_extrema (OpenCV rescales in
 * detectAndCompute, not there) nor by the other sub-module calls.  sift_multi_*
 * has no such setting: multi.hip calls no library function beyond those it
 * already did (tests/cpp/multi_sim.cpp links it against its own stand-ins).
 * A NULL context: SIFT_E_INVALID. */
int sift_set_upsample(sift_ctx* ctx, int on);
const char* sift_version(void);
/* hipGraph cache counters of this context: sequences captured, cached
 * executables patched in place (hipGraphExecUpdate: same shape, other
 * buffers) and executables instantiated.  The cache holds 4 shapes; a call
 * whose shape (batch, dims, strides, kp_cap, octaves, flags) and buffers both
 * match a cached entry replays it with no capture at all, so callers that can
 * keep their device buffers stable (or rotate among a few) pay no capture. */
int sift_graph_stats(const sift_ctx* ctx, long long* captures, long long* updates, long long* instantiations);

/* ---- layout helpers ----------------------------------------------------- */
/* Octave shapes: octave o+1 = Size(cols/2, rows/2) of octave o (src/sift.cpp:254). */
int sift_octave_shapes(int rows, int cols, int n_octaves, int* orows, int* ocols);
/* Elements of a packed pyramid (planes back to back, no padding): per = 5
 * (Gaussian, index o*5+s) or 4 (DoG, index o*4+s). */
size_t sift_packed_size(int rows, int cols, int n_octaves, int per);

/* ---- full detect + compute ---------------------------------------------- */
/* Replaces SIFT_NCL (include/sift.hpp:41, src/sift.cpp:59-91).
 * img: host, rows x cols CV_32FC1 values, row_stride_bytes apart.
 * kpts/desc: host, capacity cap keypoints / cap x 128 floats.  *n_out gets the
 * keypoint count; if it exceeds cap, nothing is copied and SIFT_E_CAPACITY is
 * returned (call again with cap >= *n_out). */
int sift_detect_compute(sift_ctx* ctx, const float* img, int rows, int cols,
                        size_t row_stride_bytes, sift_keypoint* kpts, float* desc, int cap,
                        int* n_out);

/* Copies the keypoints/descriptors of the last host-API call that produced
 * them (sift_detect_compute or sift_find_scale_space_extrema) without
 * recomputing: the second half of the two-call sizing pattern.  desc may be
 * NULL (extrema only).  SIFT_E_CAPACITY if cap < count (*n_out = count). */
int sift_copy_results(sift_ctx* ctx, sift_keypoint* kpts, float* desc, int cap, int* n_out);

/* Batch mode on device-resident images.  d_imgs: batch images
 * of rows x cols, row_stride elements between rows and img_stride elements
 * between images.  Outputs (device, caller-owned): keypoints of image b occupy
 * [d_img_offsets[b], d_img_offsets[b+1]) of d_kpts/d_desc (rows of 128).  Only
 * the first kp_cap keypoints are written; d_img_offsets[batch] holds the true
 * total, so a caller detects overflow after sift_sync.  Asynchronous. */
int sift_detect_compute_batch(sift_ctx* ctx, const float* d_imgs, int batch, int rows, int cols,
                              size_t row_stride, size_t img_stride, sift_keypoint* d_kpts,
                              float* d_desc, int kp_cap, int* d_img_offsets);

/* ---- detection mask: detectAndCompute(image, mask, ...) ------------------------
 * The mask argument of OpenCV's feature detectors, applied on the device where
 * SIFT::detectAndCompute applies it (cv::KeyPointsFilter::runByPixelsMask).  A
 * mask is rows x cols bytes, the size of the image it belongs to: zero means
 * "no keypoint here", any other value keeps the keypoint.  A keypoint with
 * emitted coordinates (x, y) is dropped iff
 *     mask[(int)(y + 0.5f)][(int)(x + 0.5f)] == 0,
 * the sums formed in float and truncated toward zero.  An index outside
 * [0, rows) x [0, cols), or one formed from a NaN coordinate, drops the
 * keypoint, and no byte outside the mask's rows x cols is ever read (OpenCV
 * leaves that case undefined; this rule is the library's own).  The orientation
 * peaks of one extremum share x and y, so they are kept or dropped together.
 * Order with the keypoint budget: as in OpenCV, retainBest(nfeatures) runs
 * first and the mask after it.  With sift_set_max_features(n) the cut threshold
 * is computed over ALL keypoints of the image, masked-out ones included, and
 * the mask then removes from the survivors -- so an image may end with fewer
 * than n keypoints although unmasked ones were cut.
 * The kept keypoints stay in the unmasked order: each image's output is a
 * subsequence of its unmasked output, and each kept keypoint's 28 bytes and 128
 * descriptor floats are the unmasked run's bit for bit.  The filter runs before
 * the emission and the descriptors, so dropped keypoints cost neither.
 * d_img_offsets, *n_out, the host calls' two-call sizing, sift_copy_results and
 * every capacity rule (only the first kp_cap rows written, the true total in
 * d_img_offsets[batch], SIFT_E_CAPACITY from sift_sync) refer to the kept
 * keypoints: a kp_cap too small for the unmasked total but large enough for
 * the kept total succeeds.  Exact mode and SIFT_FLAG_FAST, with and without
 * SIFT_FLAG_NO_GRAPH / _PROFILE / _VERBOSE; not sift_find_scale_space_extrema
 * (OpenCV filters in detectAndCompute, not there).  A mask of another size
 * than the image is not supported.
 *
 * sift_detect_compute_batch with masks.  d_masks: device bytes, image b's mask
 * at d_masks + b * mask_img_stride with rows mask_row_stride apart, both in
 * bytes; mask_img_stride == 0 is one mask shared by every image of the batch.
 * d_masks == NULL is sift_detect_compute_batch exactly (the mask strides are
 * ignored, nothing extra is launched); with a mask, mask_row_stride < cols is
 * SIFT_E_INVALID.  Asynchronous: the masks, like the images, must stay valid
 * until the stream reaches the call.  In the context's graph cache a masked and
 * an unmasked call of one shape are two entries, and another mask buffer with
 * the same strides is an in-place update of the cached executable. */
int sift_detect_compute_batch_masked(sift_ctx* ctx, const float* d_imgs, int batch, int rows, int cols,
                                     size_t row_stride, size_t img_stride, const uint8_t* d_masks,
                                     size_t mask_row_stride, size_t mask_img_stride, sift_keypoint* d_kpts,
                                     float* d_desc, int kp_cap, int* d_img_offsets);
/* sift_detect_compute with a host mask (rows mask_row_stride_bytes apart; 0
 * means cols; less than cols is SIFT_E_INVALID).  mask == NULL is
 * sift_detect_compute exactly.  The mask is uploaded into a buffer the context
 * owns (max_rows x max_cols bytes, allocated by the first masked call).
 * *n_out, the two-call sizing and sift_copy_results report the kept count. */
int sift_detect_compute_masked(sift_ctx* ctx, const float* img, int rows, int cols, size_t row_stride_bytes,
                               const uint8_t* mask, size_t mask_row_stride_bytes, sift_keypoint* kpts,
                               float* desc, int cap, int* n_out);

/* ---- provided keypoints: detectAndCompute(..., useProvidedKeypoints = true) ------
 * OpenCV's Feature2D::compute(): describe images at keypoints the caller already
 * holds -- the keypoints of the previous frame carried into this one, a dense
 * grid, another detector's points.  Nothing is detected and no keypoint field is
 * changed (the orientation is taken as given, as OpenCV takes it).
 *
 * sift_compute_batch.  Images as for sift_detect_compute_batch.  d_kpts: kp_cap
 * rows, only read.  d_desc: kp_cap x 128 floats.  d_kp_offsets: batch + 1 device
 * ints, exactly what sift_detect_compute_batch leaves in d_img_offsets: image b
 * owns rows [clamp(off[b]), clamp(off[b+1])), every bound clamped to
 * [0, kp_cap]; empty images are allowed, and descriptor rows before
 * clamp(off[0]) or at and past clamp(off[batch]) are never written.
 * Row k's 128 floats are calDescriptor (src/sift.cpp:733-753) of keypoint k in
 * the pyramid SIFT_NCL builds for its image (the context's octave count,
 * firstOctave 0): in exact mode, bit for bit what sift_build_gaussian_pyramid +
 * sift_calc_descriptors(..., first_octave = 0) give, and for keypoints that
 * sift_detect_compute_batch emitted on the same images, the descriptors that
 * call wrote (under SIFT_FLAG_FAST too, on the fast pyramid).  Angles follow
 * sift_calc_descriptors' contract (the bin wraps modulo 8).
 * firstOctave: OpenCV derives it from the keypoints and upsamples the image for
 * a negative octave; the reference never upsamples, so unless
 * sift_set_upsample is on the pyramid starts at octave 0 and a row with a
 * negative octave is an invalid row.  With sift_set_upsample on, the pyramid
 * is the doubled image's, firstOctave is -1, the rows stay in original-image
 * coordinates and the valid octaves are -1 .. n_octaves - 2 (see there).
 * max_layer, 0 .. 4 (else SIFT_E_INVALID), is the caller's promise that no row
 * names a scale above it: only scales 0 .. max_layer are differentiated, and
 * with max_layer <= 3 the widest blur (w = 18) is not computed where the blur
 * form in use can leave it out.  4 admits every scale the reference allows; 3
 * covers every keypoint a SIFT detection emits.
 * Invalid rows: octave < 0, octave >= the context's octave count (with
 * sift_set_upsample on: octave < -1, octave >= the count - 1), layer > 4 or
 * layer > max_layer.  Such a row gets 128 zeros and sets the sticky assertion
 * bit, which sift_sync reports as SIFT_E_INVALID once; other rows are not
 * affected.
 * Asynchronous on the context stream: no synchronisation and no host read of an
 * offset (the ranking scratch grows, with a wait, only for a kp_cap above every
 * earlier call's).  In the graph cache the sequence has its own entries, keyed
 * by the shape, kp_cap, the octave count, the flags and max_layer; other
 * buffers of the same shape update the cached executable in place.  Under
 * SIFT_FLAG_PROFILE its stages are the pyramid's, "gradient", "compute_prep" and
 * "descriptor".  The keypoint budget and the detection masks do not apply.
 * batch == 0 or kp_cap == 0: SIFT_OK, nothing is enqueued.  kp_cap above 2^30 is
 * SIFT_E_SIZE. */
int sift_compute_batch(sift_ctx* ctx, const float* d_imgs, int batch, int rows, int cols, size_t row_stride,
                       size_t img_stride, const sift_keypoint* d_kpts, const int* d_kp_offsets, int kp_cap,
                       int max_layer, float* d_desc);
/* The same from host memory, synchronous: one image (rows row_stride_bytes
 * apart, 0 = cols * 4), n keypoints in, n x 128 floats out.  SIFT_E_INVALID if
 * any row was invalid -- the n rows are written all the same, the invalid ones
 * as zeros.  n == 0 is SIFT_OK.  Like sift_calc_descriptors it uses the
 * context's keypoint buffer, so sift_copy_results has nothing to copy after it. */
int sift_compute(sift_ctx* ctx, const float* img, int rows, int cols, size_t row_stride_bytes,
                 const sift_keypoint* kpts, int n, int max_layer, float* desc);

/* Synthetic integer-exact test images, written on device:
 * image b uses seed 0x5EED0000 + seed_base + b.  Asynchronous. */
int sift_synth_images(sift_ctx* ctx, float* d_out, int batch, int rows, int cols,
                      size_t row_stride, size_t img_stride, int seed_base);

/* ---- multi-GPU batch mode (BASELINE configs[3]) ----------
 * The reference's only parallelism is OpenMP over descriptors
 * (src/sift.cpp:738); here the images of a batch are sharded over the GPUs of
 * one node by contiguous ranges, each device runs sift_detect_compute_batch on
 * its shard, and the keypoint records are gathered to the first device over
 * RCCL (ncclSend / ncclRecv, xGMI) one step behind the compute.  One process
 * drives every device (ncclCommInitAll); a multi context is not thread-safe. */
typedef struct sift_multi sift_multi;
#define SIFT_MULTI_SELF_P2P 0x100u /* sift_multi_create flag: device 0's own records also go through RCCL
                                      (self send/recv) instead of a DMA copy -- tests the p2p path on one GPU */
/* Shard arithmetic: device `index` of n takes the contiguous images
 * [*first, *first + *count) = [floor(index * batch / n), floor((index + 1) * batch / n)).
 * No GPU needed. */
int sift_multi_shard(int batch, int n_devices, int index, int* first, int* count);
/* Global per-image offsets [sum(counts) + 1] from each shard's own offsets
 * [counts[i] + 1] (records concatenated in device order).  No GPU needed. */
int sift_multi_merge_offsets(const int* const* shard_offsets, const int* counts, int n_devices,
                             int* global_offsets);
/* Per device: streams_per_device sift_ctx contexts, each with its own HIP
 * stream (0 = the default, 2: each step's shard runs as that many contiguous
 * sub-batches whose stages overlap, as bench.py's streams do), two result
 * slots per context sharing kp_cap_per_device records per slot, and a
 * gather stream; on devices[0] the gather buffers (n_devices x
 * kp_cap_per_device records, and descriptors when gather_desc); RCCL
 * communicators over the devices.  Device indices must be distinct (RCCL:
 * one rank per device). */
int sift_multi_create(const int* devices, int n_devices, int max_rows, int max_cols, int max_batch_per_device,
                      unsigned flags, int streams_per_device, int kp_cap_per_device, int gather_desc,
                      sift_multi** out);
int sift_multi_destroy(sift_multi* m);
const char* sift_multi_last_error(const sift_multi* m);
/* The first context of device index i (sift_synth_images on that device, ...). */
sift_ctx* sift_multi_context(sift_multi* m, int index);
/* sift_set_octaves / sift_set_flags / sift_set_max_features on every context. */
int sift_multi_set_octaves(sift_multi* m, int n_octaves);
int sift_multi_set_flags(sift_multi* m, unsigned flags);
int sift_multi_set_max_features(sift_multi* m, int n_per_image);
/* One step: device i detects + describes counts[i] images resident on it
 * (d_imgs[i], strides in elements as in sift_detect_compute_batch) into its
 * result slots, and the previous step's records are gathered to devices[0].
 * The images must be complete when the step is enqueued (the contexts'
 * streams do not wait for the caller's producers: synchronise them first).
 * Asynchronous, except that the host waits for the previous step's per-image
 * offsets (one step behind, so normally without blocking). */
int sift_multi_step(sift_multi* m, const float* const* d_imgs, const int* counts, int rows, int cols,
                    size_t row_stride, size_t img_stride);
/* sift_multi_step with detection masks (sift_detect_compute_batch_masked on
 * every device): d_masks[i] is device i's masks, resident on it, counts[i]
 * masks mask_img_stride bytes apart (0: one mask for all of that device's
 * images), rows mask_row_stride bytes apart.  d_masks == NULL, or a NULL entry,
 * means no mask on that device.  With several streams per device each
 * sub-batch takes its own slice of the masks.  mask_row_stride < cols with any
 * mask given is SIFT_E_INVALID, refused before anything is enqueued. */
int sift_multi_step_masked(sift_multi* m, const float* const* d_imgs, const uint8_t* const* d_masks,
                           const int* counts, int rows, int cols, size_t row_stride, size_t img_stride,
                           size_t mask_row_stride, size_t mask_img_stride);
/* Gathers the last step, drains every stream and reports the contexts' sticky
 * status (as sift_sync).  A step or flush that fails after enqueueing work
 * (a device error, a keypoint count above a context's share of
 * kp_cap_per_device) leaves the result slots undefined: later steps and
 * flushes return SIFT_E_INVALID and the multi context must be destroyed. */
int sift_multi_flush(sift_multi* m);
/* The last gathered step on devices[0]: device pointers to its records (and
 * descriptors, or NULL without gather_desc) in global image order, and the
 * global per-image offsets [batch_total + 1] into host memory (offsets may be
 * NULL).  Valid until the next sift_multi_step. */
int sift_multi_gathered(sift_multi* m, const sift_keypoint** d_kpts, const float** d_desc, int* offsets,
                        int offsets_cap, int* batch_total, long long* step);
/* Host copy of the last gathered step's records (and descriptors, desc may be
 * NULL): *n_out gets the record count; SIFT_E_CAPACITY if cap < count.
 * Synchronous. */
int sift_multi_copy_gathered(sift_multi* m, sift_keypoint* kpts, float* desc, int cap, int* n_out);
/* Steps enqueued, records gathered and RCCL p2p transfers posted so far
 * (device 0's own pieces are DMA copies unless SIFT_MULTI_SELF_P2P). */
int sift_multi_stats(const sift_multi* m, long long* steps, long long* records, long long* transfers);
/* RCCL's NCCL_VERSION_CODE at run time (ncclGetVersion), -1 on error. */
int sift_multi_rccl_version(void);

/* ---- sub-module entry points (host memory, synchronous) ----------------- */
/* Gaussian_Blur (include/sift.hpp:47, src/sift.cpp:123-153).  Both blurs take
 * 0 < sigma <= 100 (SIFT_E_INVALID otherwise, NaN included), kernel half-width
 * w = floor(3 sigma) in 0 .. 300.  w = 0 is the reference's own arithmetic: the
 * 2-D blur multiplies by the single tap 1 / (2 pi sigma^2), the 1-D blur's tap
 * loop is empty and the result is all zeros; a plane with one row or one
 * column blurs to zeros (the getSubMatrix border rule, :116). */
int sift_gaussian_blur(sift_ctx* ctx, const float* src, int rows, int cols, double sigma,
                       float* dst);
/* Gaussian_Blur_1D (include/sift.hpp:49, src/sift.cpp:170-217). */
int sift_gaussian_blur_1d(sift_ctx* ctx, const float* src, int rows, int cols, double sigma,
                          float* dst);
/* buildGaussianPyramid (include/sift.hpp:51, src/sift.cpp:229-263); gpyr is
 * packed, sift_packed_size(rows, cols, n_octaves, 5) floats. */
int sift_build_gaussian_pyramid(sift_ctx* ctx, const float* img, int rows, int cols,
                                int n_octaves, float* gpyr);
/* buildDoGPyramid (include/sift.hpp:55, src/sift.cpp:265-283); packed in/out. */
int sift_build_dog_pyramid(sift_ctx* ctx, const float* gpyr, int rows, int cols, int n_octaves,
                           float* dog);
/* findScaleSpaceExtrema (include/sift.hpp:59, src/sift.cpp:547-577); packed
 * pyramids in; keypoints out with the same count/capacity rule as above. */
int sift_find_scale_space_extrema(sift_ctx* ctx, const float* gpyr, const float* dog, int rows,
                                  int cols, int n_octaves, sift_keypoint* kpts, int cap,
                                  int* n_out);
/* calDescriptor (include/sift.hpp:64, src/sift.cpp:733-753).  A keypoint's
 * octave byte is signed (254 = -2); with oi = octave - first_octave, a row with
 * oi < 0, oi >= n_octaves or layer > 4 makes the call return SIFT_E_INVALID
 * (the CV_Assert of :744, and the bounds of gpyr it does not check).  Angles in
 * [0, 720] are the reference's contract: its single wrap of the orientation bin
 * covers 360 - angle in [-360, 360], and beyond that it adds samples outside
 * their histogram cell.  The library wraps the bin modulo 8 (the circular
 * histogram) for every angle, which is the reference's result inside the
 * contract; outside it the call succeeds, the row's descriptor is that
 * histogram's, and other rows are not affected.  NaN angles give an
 * unspecified (in-bounds) bin. */
int sift_calc_descriptors(sift_ctx* ctx, const float* gpyr, int rows, int cols, int n_octaves,
                          const sift_keypoint* kpts, int n, float* desc, int first_octave);

/* ---- image front end ----------------------------------- */
/* Replaces the conversion half of the application's readImage
 * (src/main.cpp:79-87): decoded 8-bit BGR bytes (imread's layout) ->
 * optional INTER_LINEAR resize to out_rows x out_cols (the scene's
 * Size(960, 960); no resize when the sizes are equal) -> cvtColor
 * COLOR_RGB2GRAY on those BGR bytes -> CV_32F.  Decoding stays with the
 * caller.  Host buffers (synchronous), gray is out_rows x out_cols floats;
 * rows are row_stride >= 3 * cols bytes apart and only the
 * (rows - 1) * row_stride + 3 * cols bytes a strided view owns are read: */
int sift_bgr8_to_gray(sift_ctx* ctx, const uint8_t* bgr, int rows, int cols, size_t row_stride, int out_rows,
                      int out_cols, float* gray);
/* Device buffers, a batch of images, enqueued on the context stream (the
 * output can be the input of sift_detect_compute_batch). Strides in bytes. */
int sift_bgr8_to_gray_device(sift_ctx* ctx, const uint8_t* d_bgr, int batch, int rows, int cols,
                             size_t row_stride, size_t img_stride, int out_rows, int out_cols, float* d_gray,
                             size_t out_row_stride, size_t out_img_stride);

/* ---- the doubled image (sift_set_upsample's first step, usable on its own) --
 * dst = cv::resize(src, Size(2 * cols, 2 * rows), 0, 0, INTER_LINEAR) on
 * CV_32F, stated here as the library's own rule (restated in numpy in
 * tests/upsample_inputs.py); parity against OpenCV itself is by construction
 * and unpinned, as for the homography (no OpenCV here).  A horizontal pass,
 * then a vertical pass, both in float, every value formed as a * w0 + b * w1
 * with two multiplies and one add, never fused.  For destination index d along
 * an axis of n source samples S (columns and rows alike):
 *     d even: s = d / 2 - 1,   weights (0.25f, 0.75f) on (S[s], S[s + 1])
 *     d odd:  s = (d - 1) / 2, weights (0.75f, 0.25f)
 *     s < 0:      the value is S[0], copied (no multiply)
 *     s >= n - 1: the value is S[n - 1], copied (no multiply)
 *     D[dy][dx] = Hrow[j0][dx] * v0 + Hrow[j1][dx] * v1,
 *     Hrow[r][dx] = S[r][i0] * w0 + S[r][i1] * w1.
 * A 1 x 1 image gives four copies; a 1 x N or N x 1 image doubles both axes.
 * Denormal values are not flushed.  NaN and infinite inputs are unspecified
 * beyond "no byte outside dst's pixels is written".  rows or cols < 1, a NULL
 * buffer or context, or a stride too small for its rows: SIFT_E_INVALID; a
 * dimension above 2^30: SIFT_E_SIZE.  The context's creation limits do not
 * apply.  Under SIFT_FLAG_PROFILE the stage is "upsample2x" (20 algorithmic
 * bytes per source pixel).
 * Host buffers (synchronous): src rows are row_stride_bytes apart (0 = cols * 4;
 * a multiple of 4) and only the bytes a strided view owns are read; dst is
 * 2 rows x 2 cols floats, packed: */
int sift_upsample2x(sift_ctx* ctx, const float* src, int rows, int cols, size_t row_stride_bytes, float* dst);
/* Device buffers, a batch of images, enqueued on the context stream with no
 * synchronisation.  Strides in elements (floats), as sift_detect_compute_batch
 * takes them: out_row_stride >= 2 * cols, and for batch > 1 the image strides
 * cover an image.  Only the 2 rows x 2 cols pixels of each output image are
 * written -- row and image padding keep their bytes.  Rows of d_dst that are
 * 16-byte aligned (d_dst and out_row_stride, and out_img_stride for a batch,
 * multiples of 4 floats) are written with 16-byte stores. */
int sift_upsample2x_device(sift_ctx* ctx, const float* d_src, int batch, int rows, int cols, size_t row_stride,
                           size_t img_stride, float* d_dst, size_t out_row_stride, size_t out_img_stride);

/* ---- warpPerspective of a whole batch (the call after the homography) -------
 * dst = cv::warpPerspective(src, dst, H, Size(out_cols, out_rows),
 *                           INTER_LINEAR [| WARP_INVERSE_MAP], BORDER_CONSTANT, 0)
 * on CV_32FC1 (SIFT_PIXEL_F32, channels 1), CV_8UC1 and CV_8UC3 (SIFT_PIXEL_U8,
 * channels 1 or 3, interleaved), stated here as the library's own rule
 * (csrc/warp_math.hpp, which host and device both compile; restated in numpy in
 * tests/warp_inputs.py); parity against OpenCV itself is by construction and
 * unpinned, as for sift_upsample2x and the homography (no OpenCV here).
 * The matrix M, in double: with SIFT_WARP_INVERSE_MAP M = H; otherwise
 * M = adj(H) * (1 / det(H)) with
 *     c0 = h4 h8 - h5 h7,  c1 = h5 h6 - h3 h8,  c2 = h3 h7 - h4 h6,
 *     det = (h0 c0 + h1 c1) + h2 c2,  r = 1 / det,
 *     M0 = c0 r,  M1 = (h2 h7 - h1 h8) r,  M2 = (h1 h5 - h2 h4) r,
 *     M3 = c1 r,  M4 = (h0 h8 - h2 h6) r,  M5 = (h2 h3 - h0 h5) r,
 *     M6 = c2 r,  M7 = (h1 h6 - h0 h7) r,  M8 = (h0 h4 - h1 h3) r
 * (each product difference two multiplies and one subtract, never fused).
 * A segment warps to nothing -- every destination pixel is 0 -- when
 * d_found[b] == 0, when an entry of H or of M is not finite, or when det is 0
 * or not finite: sift_perspective_transform_segmented_device's convention.
 * The source position of destination pixel (x, y), in double:
 *     Wd = (M6 x + M7 y) + M8,  W = Wd != 0 ? 32.0 / Wd : 0.0,
 *     fX = ((M0 x + M1 y) + M2) W,  fY = ((M3 x + M4 y) + M5) W;
 * a NaN fX or fY makes the pixel 0; otherwise each is clamped to
 * [INT_MIN, INT_MAX], X = (int)rint(fX), Y = (int)rint(fY) (ties to even),
 * sx = X >> 5, ax = X & 31, sy = Y >> 5, ay = Y & 31 (arithmetic shifts).
 * The samples v00 = S[sy][sx], v01 = S[sy][sx + 1], v10 = S[sy + 1][sx],
 * v11 = S[sy + 1][sx + 1]; a sample outside [0, rows) x [0, cols) is the value
 * 0 and is never read, each sample on its own.
 * f32: fx = ax * 0.03125f, fy = ay * 0.03125f, w00 = (1 - fy) * (1 - fx),
 * w01 = (1 - fy) * fx, w10 = fy * (1 - fx), w11 = fy * fx (exact multiples of
 * 1/1024), out = ((v00 * w00 + v01 * w01) + v10 * w10) + v11 * w11: four
 * multiplies and three adds in that order, never fused.  Denormals are not
 * flushed; a NaN or infinite sample inside the image propagates, even at
 * weight 0.
 * u8, each channel alone: k00 = (32 - ay) * (32 - ax), k01 = (32 - ay) * ax,
 * k10 = ay * (32 - ax), k11 = ay * ax (sum 1024),
 * out = (v00 k00 + v01 k01 + v10 k10 + v11 k11 + 512) >> 10 -- OpenCV's 15-bit
 * coefficient table with the common factor 32 taken out.
 * Errors: a NULL context or buffer (d_found may be NULL: all found), a dimension
 * < 1, a pixel / channels pair other than the three above, an unknown flag, a
 * stride too small for its row or image, or an f32 stride or pointer that is not
 * a multiple of 4: SIFT_E_INVALID; a dimension above 2^30: SIFT_E_SIZE.  The
 * context's creation limits do not apply.  Under SIFT_FLAG_PROFILE the stage is
 * "warp" (8 algorithmic bytes per f32 destination pixel, 2 or 6 per u8 pixel). */
#define SIFT_WARP_INVERSE_MAP 0x1u
#define SIFT_PIXEL_F32 0
#define SIFT_PIXEL_U8 1
/* Device buffers, enqueued on the context stream with no synchronisation, one
 * launch, no scratch.  Image b is warped by H[b]: d_H is [n_segments][9]
 * doubles and d_found [n_segments] ints, exactly what
 * sift_find_homography_segmented_device leaves.  Strides in bytes, 0 = packed;
 * img_stride == 0 with n_segments > 1 is one source image warped by every H.
 * Only the out_rows x out_cols pixels of each destination image are written --
 * row and image padding keep their bytes.  Destination rows that are 16-byte
 * aligned (u8: 4-byte) are written with 16-byte (dword) stores.  n_segments
 * == 0: SIFT_OK, nothing enqueued. */
int sift_warp_perspective_segmented_device(sift_ctx* ctx, int pixel, int channels, const void* d_src, int rows,
                                           int cols, size_t row_stride, size_t img_stride, const double* d_H,
                                           const int* d_found /* may be NULL: all found */, int n_segments,
                                           unsigned flags, void* d_dst, int out_rows, int out_cols,
                                           size_t out_row_stride, size_t out_img_stride);
/* Host buffers (synchronous), one image: only the bytes a strided view owns
 * are read; dst is out_rows x out_cols pixels, packed.  SIFT_E_INVALID with dst
 * zeroed if H warps to nothing. */
int sift_warp_perspective(sift_ctx* ctx, int pixel, int channels, const void* src, int rows, int cols,
                          size_t row_stride, const double* H, unsigned flags, void* dst, int out_rows, int out_cols);

/* ---- matching ------------------------------------------ */
/* Replaces `BFMatcher(NORM_L1).knnMatch(query, train, matches, k)` of the
 * reference application (src/main.cpp:25-27; the 0.86 ratio test at :28-40
 * stays with the caller).  query [n_query][128], train [n_train][128] floats;
 * for each query the k (1 or 2) nearest train rows by float L1 distance
 * (OpenCV normL1_ summation order, see match.hip), ascending, an earlier train
 * index first at equal distance.  idx / dist are [n_query][k].  A train row
 * whose distance overflowed to +inf is never a neighbour: where fewer than k
 * train rows are at a finite distance (n_train < k included) the missing
 * entries are idx -1, dist +inf, and the ratio stage below skips such a query.
 * This is the library's own rule; descriptors that produce NaN distances (NaN
 * or infinite elements) are unspecified.  Denormal values are not flushed.
 * Host buffers (synchronous): */
int sift_knn_match_l1(sift_ctx* ctx, const float* query, int n_query, const float* train, int n_train, int k,
                      int* idx, float* dist);
/* Device buffers (16-byte aligned rows), enqueued on the context's stream: */
int sift_knn_match_l1_device(sift_ctx* ctx, const float* d_query, int n_query, const float* d_train,
                             int n_train, int k, int* d_idx, float* d_dist);

/* ---- matching a whole batch (segments given by device-resident offsets) ----- */
/* knnMatch (src/main.cpp:25-27) for every image of a batch in one enqueue.
 * Query rows [q_offsets[b], q_offsets[b+1]) of d_query are segment b,
 * b < n_segments; d_q_offsets is a device array of n_segments + 1 ints, exactly
 * what sift_detect_compute_batch writes to d_img_offsets.  The offsets are read
 * on the device only, and every bound is clamped to q_cap (t_cap), the row
 * capacity of the buffer, so the batch call's overflow convention (the last
 * offset holds the true total) never reads or writes past a buffer.
 * Train side: d_t_offsets == NULL -- every segment searches all t_cap rows of
 * d_train ("find this object in every frame"); otherwise segment b searches
 * rows [t_offsets[b], t_offsets[b+1]) ("frame b against frame b+1").  Result
 * indices are local to the train segment (global when the train set is shared).
 * Distance, order, tie rule and the -1 / +inf fill are sift_knn_match_l1's.
 * d_idx / d_dist are [q_cap][k]; rows before q_offsets[0] and rows at or past
 * min(q_offsets[n_segments], q_cap) are left untouched.
 * Consecutive frames of one batch need no host value: d_train = d_query,
 * d_t_offsets = d_q_offsets + 1, t_cap = q_cap, n_segments = batch - 1.
 * Enqueued on the context stream, no synchronisation (the scratch grows, with
 * a wait, only when a call needs more than any call before it).  n_segments
 * == 0 or q_cap == 0: SIFT_OK, nothing enqueued. */
int sift_knn_match_l1_segmented_device(sift_ctx* ctx, const float* d_query, const int* d_q_offsets,
                                       int n_segments, int q_cap, const float* d_train,
                                       const int* d_t_offsets /* NULL = shared */, int t_cap, int k, int* d_idx,
                                       float* d_dist);
/* Host buffers (synchronous); query has q_cap rows, train t_cap rows: */
int sift_knn_match_l1_segmented(sift_ctx* ctx, const float* query, const int* q_offsets, int n_segments,
                                int q_cap, const float* train, const int* t_offsets /* NULL = shared */,
                                int t_cap, int k, int* idx, float* dist);

/* ---- 8-bit descriptors and their matcher (opt-in; match_u8.hip) ------------- */
/* The byte form of a descriptor row, 128 uint8: out[i][e] =
 * saturate_cast<uchar>(desc[i][e] * 512.f) -- the float multiply (exact), then
 * cvRound (ties to even), then a clamp to 0..255; the form the reference leaves
 * commented out at src/sift.cpp:720 (SIFT_INT_DESCR_FCTR = 512).  -0.0 and
 * negatives give 0, +inf gives 255, NaN is unspecified.
 * Device buffers (16-byte aligned), enqueued on the context stream, no
 * synchronisation: rows [0, min(*d_n_rows, row_cap)) are converted, all row_cap
 * rows when d_n_rows is NULL; rows at or past that bound are not written.
 * d_n_rows = d_img_offsets + batch (the batch call's total) needs no host value
 * and, clamped to row_cap, follows its overflow convention. */
int sift_descriptors_to_u8_device(sift_ctx* ctx, const float* d_desc, const int* d_n_rows /* may be NULL */,
                                  int row_cap, uint8_t* d_out);
/* Host buffers (synchronous), n rows: */
int sift_descriptors_to_u8(sift_ctx* ctx, const float* desc, int n, uint8_t* out);

/* sift_knn_match_l1_segmented_device on byte rows ([q_cap][128] / [t_cap][128]
 * uint8, 16-byte aligned).  The distance is the integer sum of |a - b| over the
 * 128 bytes taken as unsigned, at most 32,640, exact in any order; d_dist stays
 * float and holds that integer, so sift_ratio_matches_device and everything
 * after it take the output unchanged.  Everything else is the float form's
 * contract word for word: segments from device offsets with every bound clamped
 * to q_cap / t_cap, d_t_offsets == NULL for a shared train set, indices local
 * to the train range, k of 1 or 2, ascending (distance, train index) with the
 * lower index first at equal distance, idx -1 / dist +inf where fewer than k
 * train rows exist, rows outside [clamp(q_offsets[0]), clamp(q_offsets[n]))
 * untouched, n_segments == 0 or q_cap == 0: SIFT_OK with nothing enqueued, a
 * NULL context or required buffer: SIFT_E_INVALID; enqueued on the context
 * stream with no synchronisation (the scratch grows, with a wait, only when a
 * call needs more than any call before it).  Consecutive frames: d_train =
 * d_query, d_t_offsets = d_q_offsets + 1. */
int sift_knn_match_l1_u8_segmented_device(sift_ctx* ctx, const uint8_t* d_query, const int* d_q_offsets,
                                          int n_segments, int q_cap, const uint8_t* d_train,
                                          const int* d_t_offsets /* NULL = shared */, int t_cap, int k, int* d_idx,
                                          float* d_dist);
/* Host buffers (synchronous); query has q_cap rows, train t_cap rows: */
int sift_knn_match_l1_u8_segmented(sift_ctx* ctx, const uint8_t* query, const int* q_offsets, int n_segments,
                                   int q_cap, const uint8_t* train, const int* t_offsets /* NULL = shared */,
                                   int t_cap, int k, int* idx, float* dist);
/* sift_knn_match_l1 on byte rows (host buffers, synchronous): one segment of
 * n_query rows over all n_train rows. */
int sift_knn_match_l1_u8(sift_ctx* ctx, const uint8_t* query, int n_query, const uint8_t* train, int n_train,
                         int k, int* idx, float* dist);

/* ---- squared L2 on 8-bit descriptors (opt-in; match_l2_u8.hip) --------------- */
/* sift_knn_match_l1_u8_segmented_device with the squared Euclidean distance:
 * d(q, t) = the integer sum of (q[e] - t[e])^2 over the 128 bytes taken as
 * unsigned, at most 128 * 255^2 = 8,323,200 < 2^24, formed from integer matrix
 * products and exact; d_dist stays float and holds that integer.  No square
 * root is taken: d_dist is the SQUARED distance (cv::NORM_L2SQR), and the order
 * of neighbours is NORM_L2's.  The ratio test on it is sift_ratio_matches[_device]
 * unchanged with ratio * ratio passed as its ratio (d1 <= r^2 d2 on squares is
 * sqrt(d1) <= r sqrt(d2)): 0.86 * 0.86 for the application's 0.86.  Everything
 * else is the L1 form's contract word for word: segments from device offsets
 * with every bound clamped to q_cap / t_cap, d_t_offsets == NULL for a shared
 * train set, indices local to the train range, k of 1 or 2, ascending
 * (distance, train index) with the lower index first at equal distance, idx -1
 * / dist +inf where fewer than k train rows exist, rows outside
 * [clamp(q_offsets[0]), clamp(q_offsets[n])) untouched, n_segments == 0 or
 * q_cap == 0: SIFT_OK with nothing enqueued, a NULL context or required buffer:
 * SIFT_E_INVALID; enqueued on the context stream with no synchronisation (the
 * scratch, sized from the capacities, grows, with a wait, only when a call
 * needs more than any call before it).  Consecutive frames: d_train = d_query,
 * d_t_offsets = d_q_offsets + 1. */
int sift_knn_match_l2sqr_u8_segmented_device(sift_ctx* ctx, const uint8_t* d_query, const int* d_q_offsets,
                                             int n_segments, int q_cap, const uint8_t* d_train,
                                             const int* d_t_offsets /* NULL = shared */, int t_cap, int k,
                                             int* d_idx, float* d_dist);
/* Host buffers (synchronous); query has q_cap rows, train t_cap rows: */
int sift_knn_match_l2sqr_u8_segmented(sift_ctx* ctx, const uint8_t* query, const int* q_offsets, int n_segments,
                                      int q_cap, const uint8_t* train, const int* t_offsets /* NULL = shared */,
                                      int t_cap, int k, int* idx, float* dist);
/* sift_knn_match_l1_u8 with the squared L2 distance (host buffers,
 * synchronous): one segment of n_query rows over all n_train rows. */
int sift_knn_match_l2sqr_u8(sift_ctx* ctx, const uint8_t* query, int n_query, const uint8_t* train, int n_train,
                            int k, int* idx, float* dist);

/* ---- squared L2 on float descriptors (opt-in; match_l2_f32.hip) --------------- */
/* sift_knn_match_l1_segmented_device with the squared Euclidean distance on the
 * float rows themselves (cv::BFMatcher's default NORM_L2 on SIFT descriptors,
 * less the square root), formed on the exact f32 matrix pipe by one rule that a
 * CPU restates bit for bit.  pi is one fixed permutation of 0..127, the same
 * for every call and shape (the order the 16-byte operand loads give):
 *   pi = 0 4 1 5 2 6 3 7,  8 12 9 13 10 14 11 15,  ...,
 *        120 124 121 125 122 126 123 127
 * i.e. pi[8 c + 2 j + h] = 8 c + 4 h + j for c < 16, j < 4, h < 2.  With
 *   chain(x, y) = fmaf(x[pi127], y[pi127], ... fmaf(x[pi0], y[pi0], 0.0f))
 * (one rounding per product, IEEE binary32, round to nearest even):
 *   dot = chain(q, t), nq = chain(q, q), nt = chain(t, t),
 *   s = nq + nt                      (one rounding),
 *   d = fmaf(-2.0f, dot, s),
 *   d = d < 0 ? 0 : d                (a comparison: NaN stays NaN).
 * d_dist holds d, the SQUARED distance (cv::NORM_L2SQR); no square root is
 * taken on the device, and the order of neighbours is NORM_L2's.  The ratio
 * test on it is sift_ratio_matches[_device] unchanged with ratio * ratio passed
 * as its ratio (0.86 * 0.86 for the application's 0.86); cross-check is two
 * calls, the second with the sides exchanged and k = 1, into
 * sift_cross_check_matches_device.  No host value is read in between.
 * Accuracy: the form nq + nt - 2 dot cancels, so against the real-number
 * sum (q[e] - t[e])^2 the absolute error is about 2 gamma_130 (nq + nt),
 * gamma_n = n 2^-24 / (1 - n 2^-24): about 1.6e-5 (nq + nt), whatever d is --
 * two nearly equal rows get a distance near 0 with that absolute, not
 * relative, error.  The exact-difference form does not map to the matrix pipe.
 * Denormal values are not flushed.  Every (q, t) distance is formed in one
 * tile over all 128 elements, so no capacity, offset, split or tile position
 * changes a value.
 * Order, tie rule (an earlier train index first at equal distance), local
 * indices, clamps and the -1 / +inf fill are sift_knn_match_l1_segmented's word
 * for word: a train row at d = +inf is never a neighbour; where fewer than k
 * train rows are at a finite distance the missing entries are idx -1, dist
 * +inf.  Finite elements can give d = +inf (s overflows) or d = NaN (nq or nt
 * and dot both overflow: inf - inf); a row at a NaN d is never a neighbour
 * either, exactly like one at +inf, because the order is a strict '<', which is
 * false on NaN: its place is filled as above, idx -1 / dist +inf, so no NaN
 * ever appears in d_dist.  Descriptors with NaN or infinite elements are
 * unspecified.
 * Which rows are touched is that contract too: d_idx / d_dist are [q_cap][k]; rows before
 * q_offsets[0] and rows at or past min(q_offsets[n_segments], q_cap) are left
 * untouched; every bound is clamped to q_cap / t_cap; d_t_offsets == NULL is a
 * shared train set; n_segments == 0 or q_cap == 0: SIFT_OK, nothing enqueued; a
 * NULL context or required buffer: SIFT_E_INVALID.  Rows 16-byte aligned.
 * Enqueued on the context stream with no synchronisation (the scratch, sized
 * from the capacities, grows, with a wait, only when a call needs more than any
 * call before it).  Consecutive frames: d_train = d_query, d_t_offsets =
 * d_q_offsets + 1. */
int sift_knn_match_l2sqr_f32_segmented_device(sift_ctx* ctx, const float* d_query, const int* d_q_offsets,
                                              int n_segments, int q_cap, const float* d_train,
                                              const int* d_t_offsets /* NULL = shared */, int t_cap, int k,
                                              int* d_idx, float* d_dist);
/* Host buffers (synchronous); query has q_cap rows, train t_cap rows: */
int sift_knn_match_l2sqr_f32_segmented(sift_ctx* ctx, const float* query, const int* q_offsets, int n_segments,
                                       int q_cap, const float* train, const int* t_offsets /* NULL = shared */,
                                       int t_cap, int k, int* idx, float* dist);
/* Host buffers (synchronous): one segment of n_query rows over all n_train rows. */
int sift_knn_match_l2sqr_f32(sift_ctx* ctx, const float* query, int n_query, const float* train, int n_train,
                             int k, int* idx, float* dist);

/* One kept match: cv::DMatch's queryIdx / trainIdx (local to their segments),
 * distance, and the segment in imgIdx's place.  16 bytes. */
typedef struct sift_match {
  int32_t query, train;
  float distance;
  int32_t segment;
} sift_match;

/* The ratio test and the point gather of the application (src/main.cpp:28-52)
 * on the k = 2 output of the segmented matcher, same offsets: query row i is
 * kept iff idx[i][1] >= 0 and (double)dist[i][0] <= ratio * (double)dist[i][1]
 * (:36-38).  Kept matches are written densely in query order within a segment
 * and in segment order overall (an ordered scan, no atomics), so segment b's
 * records are [m_offsets[b], m_offsets[b+1]); d_m_offsets is n_segments + 1 ints
 * and its last entry is the true total.  Only the first m_cap records are
 * written (m_cap = q_cap always suffices).  With d_q_kpts != NULL the point
 * pairs of :47-52 are gathered as interleaved (x, y) floats, the input of
 * sift_find_homography: src = the query keypoint (keypoints1[queryIdx].pt),
 * dst = the train keypoint (keypoints0[trainIdx].pt; d_t_kpts row
 * t_offsets[segment] + train, or train when d_t_offsets is NULL).  With
 * d_q_kpts == NULL d_t_kpts, d_src_xy and d_dst_xy are not used.
 * Enqueued on the context stream, no synchronisation. */
int sift_ratio_matches_device(sift_ctx* ctx, const int* d_idx, const float* d_dist, const int* d_q_offsets,
                              int n_segments, int q_cap, double ratio, const sift_keypoint* d_q_kpts /* may be NULL */,
                              const sift_keypoint* d_t_kpts, const int* d_t_offsets, sift_match* d_matches,
                              float* d_src_xy, float* d_dst_xy, int m_cap, int* d_m_offsets);
/* Host buffers (synchronous); q_kpts has q_cap rows and t_kpts t_cap rows
 * (t_cap is not used when q_kpts is NULL): */
int sift_ratio_matches(sift_ctx* ctx, const int* idx, const float* dist, const int* q_offsets, int n_segments,
                       int q_cap, double ratio, const sift_keypoint* q_kpts /* may be NULL */,
                       const sift_keypoint* t_kpts, int t_cap, const int* t_offsets, sift_match* matches,
                       float* src_xy, float* dst_xy, int m_cap, int* m_offsets);

/* ---- cross-check: mutual nearest neighbours of a whole batch (cross_check.hip) -- */
/* cv::BFMatcher(norm, crossCheck = true) on the device: (q, t) is kept only if
 * t is q's nearest train row and q is t's nearest query row.  The two
 * directions are two runs of a segmented matcher; this stage joins them.
 * d_idx / d_dist are [q_cap][fwd_k], the forward result (query -> train) of any
 * of the three segmented matchers; d_ridx is [t_cap][rev_k], the result of the
 * same matcher with the sides exchanged (d_query = train, q_offsets =
 * t_offsets, d_train = query, t_offsets = q_offsets), of which only column 0
 * is read.  fwd_k and rev_k are 1 or 2 and act as row strides, so a k = 2
 * result is passed unchanged.
 * With qlo = clamp(q_offsets[b], q_cap) and tlo = clamp(t_offsets[b], t_cap),
 * query row i of segment b is kept iff i is in [clamp(q_offsets[0]),
 * clamp(q_offsets[n_segments])), j = idx[i][0] >= 0, tlo + j <
 * clamp(t_offsets[b + 1], t_cap), ridx[tlo + j][0] == i - qlo and, when ratio >
 * 0, also idx[i][1] >= 0 and (double)dist[i][0] <= ratio * (double)dist[i][1]
 * (sift_ratio_matches_device's test; pass ratio * ratio with the squared L2
 * matcher).  ratio == 0 is cross-check only; ratio > 0 needs fwd_k == 2; a
 * negative or NaN ratio is SIFT_E_INVALID.  Ties follow the matchers' rule in
 * both directions (the lower index wins at equal distance), so the kept set is
 * a function of the two tables alone.  No value of a row outside the live range
 * is used, and the address of the one dependent load (ridx) is bounded by the
 * segment's train range before the load.
 * d_t_offsets is required: one train segment per query segment.  A shared train
 * set (NULL) is SIFT_E_INVALID -- its reverse result would be [n_segments][t_cap],
 * which no matcher produces.
 * The outputs are sift_ratio_matches_device's: dense records in query order
 * within a segment and in segment order overall (an ordered scan, no atomics),
 * segment b's records are [m_offsets[b], m_offsets[b+1]); d_m_offsets is
 * n_segments + 1 ints and its last entry is the true total; only the first
 * m_cap records are written; with d_q_kpts != NULL the interleaved point pairs
 * are gathered, src = d_q_kpts[i], dst = d_t_kpts[tlo + j] (d_t_kpts has t_cap
 * rows); with d_q_kpts == NULL d_t_kpts, d_src_xy and d_dst_xy are not used.
 * Nothing else is written.  Enqueued on the context stream, no synchronisation
 * and no host read of an offset (the scratch grows, with a wait, only when a
 * call needs more than any call before it).  n_segments == 0 or q_cap == 0:
 * SIFT_OK, nothing enqueued.  A NULL context or required buffer:
 * SIFT_E_INVALID. */
int sift_cross_check_matches_device(sift_ctx* ctx, const int* d_idx, const float* d_dist, int fwd_k,
                                    const int* d_q_offsets, int n_segments, int q_cap, const int* d_ridx, int rev_k,
                                    const int* d_t_offsets, int t_cap, double ratio,
                                    const sift_keypoint* d_q_kpts /* may be NULL */, const sift_keypoint* d_t_kpts,
                                    sift_match* d_matches, float* d_src_xy, float* d_dst_xy, int m_cap,
                                    int* d_m_offsets);
/* Host buffers (synchronous); idx / dist have q_cap rows, ridx t_cap rows,
 * q_kpts q_cap rows and t_kpts t_cap rows: */
int sift_cross_check_matches(sift_ctx* ctx, const int* idx, const float* dist, int fwd_k, const int* q_offsets,
                             int n_segments, int q_cap, const int* ridx, int rev_k, const int* t_offsets, int t_cap,
                             double ratio, const sift_keypoint* q_kpts /* may be NULL */, const sift_keypoint* t_kpts,
                             sift_match* matches, float* src_xy, float* dst_xy, int m_cap, int* m_offsets);

/* The distance of sift_cross_match_segmented_device and the type of its rows:
 * float rows under L1 (sift_knn_match_l1_segmented_device), byte rows under L1
 * (sift_knn_match_l1_u8_segmented_device), byte rows under squared L2
 * (sift_knn_match_l2sqr_u8_segmented_device). */
#define SIFT_METRIC_L1_F32 0
#define SIFT_METRIC_L1_U8 1
#define SIFT_METRIC_L2SQR_U8 2
/* Float rows under squared L2 (sift_knn_match_l2sqr_f32_segmented_device): a
 * name for documentation and the Python module.  The one-call cross-match and
 * the windowed matcher take the three metrics above only and reject this one
 * (SIFT_E_INVALID); cross-check with it is two matcher calls and
 * sift_cross_check_matches_device. */
#define SIFT_METRIC_L2SQR_F32 3
/* The whole job in one call: the forward pass of the metric's segmented matcher
 * (k = 2 when ratio > 0, else k = 1), the reverse pass (k = 1, the sides
 * exchanged -- derived from these arguments) and the stage above, all enqueued
 * on the context stream with the two intermediate tables in context scratch,
 * which is sized for all three before the first enqueue.  The result equals the
 * three separate calls bit for bit.  d_query is [q_cap][128] and d_train
 * [t_cap][128] rows of the metric's type, 16-byte aligned; d_t_offsets is
 * required (see above); with SIFT_METRIC_L2SQR_U8 pass ratio * ratio.
 * Consecutive frames of one batch need no host value: d_train = d_query,
 * d_t_offsets = d_q_offsets + 1, t_cap = q_cap, n_segments = batch - 1.
 * An unknown metric is SIFT_E_INVALID; everything else is the stage's
 * contract. */
int sift_cross_match_segmented_device(sift_ctx* ctx, int metric, const void* d_query, const int* d_q_offsets,
                                      int n_segments, int q_cap, const void* d_train, const int* d_t_offsets,
                                      int t_cap, double ratio, const sift_keypoint* d_q_kpts /* may be NULL */,
                                      const sift_keypoint* d_t_kpts, sift_match* d_matches, float* d_src_xy,
                                      float* d_dst_xy, int m_cap, int* d_m_offsets);

/* ---- matching within a search window (match_window.hip) --------------------- */
/* The segmented matcher of the given SIFT_METRIC_* (rows of the metric's type,
 * [q_cap][128] / [t_cap][128], 16-byte aligned) with one change: a train row is
 * a candidate for a query row only if it is admissible -- what OpenCV spells as
 * the mask argument of knnMatch, computed here from keypoint positions.
 * Everything else is the dense segmented matcher's contract word for word:
 * segments from device offsets with every bound clamped to q_cap / t_cap,
 * d_t_offsets == NULL for a shared train set, indices local to the train range,
 * k of 1 or 2, ascending (distance, local train index) with the lower index
 * first at equal distance, idx -1 / dist +inf where fewer than k admissible rows
 * at a finite distance exist, rows outside [clamp(q_offsets[0]),
 * clamp(q_offsets[n_segments])) untouched, n_segments == 0 or q_cap == 0 SIFT_OK
 * with nothing enqueued, enqueued on the context stream with no synchronisation
 * and no host read of an offset.  Distances are the dense matchers' own bit for
 * bit (float L1 in match.hip's summation order, the byte metrics exact
 * integers), so d_idx / d_dist [q_cap][k] go to sift_ratio_matches_device and
 * everything after it unchanged, and with radius = +inf, d_H = NULL and finite
 * coordinates the output equals the dense call of the same metric byte for byte.
 * Admissibility of train row t for query row q of segment b: the predicted
 * position (px, py) is d_q_kpts[q]'s (x, y) itself when d_H == NULL or when
 * d_found != NULL and d_found[b] == 0; otherwise it is sift_perspective_transform's
 * value of H = d_H + 9 b at that point, |w| <= FLT_EPSILON -> (0, 0) included.
 * d_H is [n_segments][9] doubles and d_found [n_segments] ints, exactly what
 * sift_find_homography_segmented_device writes (src = query, dst = train), so
 * pair b's model can gate pair b's next match with no host value.  t is
 * admissible iff fabsf(tx - px) <= radius && fabsf(ty - py) <= radius, in float,
 * (tx, ty) = d_t_kpts[t]'s (x, y) (d_t_kpts is indexed like d_train: row
 * t_offsets[b] + local index): a closed square window; a NaN anywhere makes the
 * row inadmissible; radius = +inf admits every row with comparable coordinates,
 * radius = 0 only exactly coincident points.
 * rows, cols: the train images' extent, a hint that shapes the search grid.  No
 * result depends on it: coordinates outside [0, cols) x [0, rows), negatives
 * and infinities included, are legal and get the rule's answer.
 * The clamped train offsets must not decrease (ranges that overlap are searched
 * memory-safely, but which of their rows are candidates is unspecified).
 * SIFT_E_INVALID: NULL context, NULL required buffer (both keypoint arrays are
 * required), unknown metric, k outside {1, 2}, radius negative or NaN, rows or
 * cols < 1, unaligned rows.
 * Out of scope: a gated reverse pass or a gated cross-check (they would need
 * the inverse prior); no existing entry point changes. */
int sift_knn_match_window_segmented_device(sift_ctx* ctx, int metric, const void* d_query,
                                           const sift_keypoint* d_q_kpts, const int* d_q_offsets, int n_segments,
                                           int q_cap, const void* d_train, const sift_keypoint* d_t_kpts,
                                           const int* d_t_offsets /* NULL = shared */, int t_cap,
                                           const double* d_H /* may be NULL */, const int* d_found /* may be NULL */,
                                           float radius, int rows, int cols, int k, int* d_idx, float* d_dist);
/* Host buffers (synchronous); query and q_kpts have q_cap rows, train and
 * t_kpts t_cap rows, H n_segments x 9 doubles, found n_segments ints: */
int sift_knn_match_window_segmented(sift_ctx* ctx, int metric, const void* query, const sift_keypoint* q_kpts,
                                    const int* q_offsets, int n_segments, int q_cap, const void* train,
                                    const sift_keypoint* t_kpts, const int* t_offsets /* NULL = shared */, int t_cap,
                                    const double* H /* may be NULL */, const int* found /* may be NULL */,
                                    float radius, int rows, int cols, int k, int* idx, float* dist);

/* ---- homography ---------------------------------------- */
/* Replaces `findHomography(obj, scene, RANSAC)` and `perspectiveTransform`
 * (src/main.cpp:54-62): n point pairs as interleaved (x, y) floats, OpenCV's
 * defaults are ransac_thresh 3, max_iters 2000, confidence 0.995.  H is a
 * row-major 3x3 with H[8] = 1; inlier_mask (n bytes, may be NULL) gets the
 * RANSAC inliers.  Host code, no context.  SIFT_E_INVALID (H zeroed) when no
 * model is found or n < 4 -- OpenCV's empty Mat.
 * Not bit-compatible with OpenCV: the final refinement is 10 steps of a plain
 * Levenberg-Marquardt on H[0..7] (normal equations, Gaussian elimination), not
 * OpenCV's LMSolver, so H can differ from cv::findHomography's in the last
 * digits (the RANSAC sampling and inlier mask follow OpenCV's order).  Parity
 * is pinned only against oracle/homography.py, which restates the same steps.
 * n == 4 is a direct fit with no subset check (OpenCV's rule): a degenerate
 * quadruple gives none where a coordinate has no spread (four identical pairs,
 * a common dst point, a common x), and otherwise a model that may be finite but
 * meaningless (four collinear pairs: entries near 1e15).
 * A pair is an inlier iff its float reprojection error is <= (float)(thr * thr):
 * thr = -3 behaves as 3, thr = 0 admits only an exact zero error, and a thr
 * whose square overflows float to +inf admits every pair with a finite or
 * infinite (not NaN) error, so the first hypothesis ends the loop.
 * Non-finite coordinates: the call terminates (every loop is bounded by a
 * count), a row with a NaN coordinate or an infinite src coordinate is never an
 * inlier, one with an infinite dst coordinate only under the +inf limit above;
 * what the pair set as a whole gives (found, H) is otherwise unspecified.  In
 * the segmented forms below the other segments are unaffected. */
int sift_find_homography(const float* src_xy, const float* dst_xy, int n, double ransac_thresh, int max_iters,
                         double confidence, double* H, unsigned char* inlier_mask);
int sift_perspective_transform(const double* H, const float* xy, int n, float* out_xy);

/* The same for every segment of a batch, on the device in stream order: the
 * last stage after sift_ratio_matches_device, whose outputs plug in unchanged.
 * Segment b's pairs are rows [clamp(m_offsets[b]), clamp(m_offsets[b+1])) of
 * d_src_xy / d_dst_xy, clamped to m_cap -- the ratio stage's convention
 * (m_offsets[n_segments] may exceed m_cap).  Each segment gets exactly what
 * sift_find_homography gives for its pairs, bit for bit: n < 4 none; n == 4 a
 * direct fit with a mask of ones; else RANSAC, the refit on the inliers, 10 LM
 * steps, normalisation.  d_H is [n_segments][9] row-major with H[8] = 1;
 * d_found[b] is 1 for a model, 0 for none, and then H[b] is nine zeros and the
 * segment's mask bytes are 0.  max_iters < 1 or confidence outside (0, 1) gives
 * every segment found = 0.  d_inlier_mask is [m_cap] bytes by pair row and may
 * be NULL; bytes outside [clamp(m_offsets[0]), clamp(m_offsets[n_segments]))
 * are never written.
 * Enqueued on the context stream, no synchronisation (the scratch grows, with
 * a wait, only when a call needs more than any call before it).  n_segments
 * == 0 or m_cap == 0: SIFT_OK, nothing enqueued.  A NULL context or a NULL
 * required buffer: SIFT_E_INVALID (sift_last_error names it). */
int sift_find_homography_segmented_device(sift_ctx* ctx, const float* d_src_xy, const float* d_dst_xy,
                                          const int* d_m_offsets, int n_segments, int m_cap, double ransac_thresh,
                                          int max_iters, double confidence, double* d_H, int* d_found,
                                          unsigned char* d_inlier_mask /* may be NULL */);
/* Host buffers (synchronous); src_xy / dst_xy have m_cap rows: */
int sift_find_homography_segmented(sift_ctx* ctx, const float* src_xy, const float* dst_xy, const int* m_offsets,
                                   int n_segments, int m_cap, double ransac_thresh, int max_iters, double confidence,
                                   double* H, int* found, unsigned char* inlier_mask /* may be NULL */);
/* d_out_xy[b][i] = perspectiveTransform(d_xy[i], H[b]) for the n_pts shared
 * points (the object's corners), [n_segments][n_pts][2] floats; a segment with
 * d_found[b] == 0 gets zeros.  Enqueued on the context stream, no
 * synchronisation; n_segments == 0 or n_pts == 0: SIFT_OK, nothing enqueued. */
int sift_perspective_transform_segmented_device(sift_ctx* ctx, const double* d_H, const int* d_found, int n_segments,
                                                const float* d_xy, int n_pts, float* d_out_xy);

/* ---- affine and similarity transforms ---------------------------------------- */
/* `estimateAffine2D` (SIFT_MODEL_AFFINE: rows (a b tx; c d ty), m = 3 model
 * points) and `estimateAffinePartial2D` (SIFT_MODEL_SIMILARITY: rotation,
 * uniform scale, translation, rows (a -b tx; b a ty), m = 2) by RANSAC, for
 * consecutive frames where a homography's two spare parameters only fit noise.
 * n point pairs as interleaved (x, y) floats; OpenCV's defaults are
 * ransac_thresh 3, max_iters 2000, confidence 0.99.  A is a row-major 2x3;
 * inlier_mask (n bytes, may be NULL) gets the RANSAC inliers.  Host code, no
 * context.  SIFT_E_INVALID (A and the mask zeroed) when no model is found,
 * n < m, max_iters < 1, confidence outside (0, 1) or model is unknown.
 * The rule (csrc/affine_math.hpp) is sift_find_homography's loop with m in
 * place of 4: n == m is a direct fit with no subset check and a mask of ones
 * (none when the solve is singular: three collinear or two identical source
 * points); otherwise subsets of m distinct rows from RNG(~0) -- affine: neither
 * the three src nor the three dst points collinear; similarity: the two src
 * points not identical --, a closed-form minimal solve in double (Cramer, or
 * the complex quotient), a hypothesis wins iff it has more than
 * max(best, m - 1) inliers, and max_iters shrinks after every win.  A pair is
 * an inlier iff, with the six coefficients cast to float and unfused float
 * arithmetic, (f0 x + f1 y + f2 - X)^2 + (f3 x + f4 y + f5 - Y)^2 <=
 * (float)(thr * thr).  The final model is the ordinary least-squares fit to the
 * best hypothesis's inliers (closed form over centred double sums in pair
 * order): the residual is linear in the parameters, so this is the minimum
 * OpenCV's refineIters = 10 LMSolver iterations look for, and there is no
 * refineIters argument.  A singular or non-finite refit leaves the RANSAC model;
 * the mask is the best hypothesis's, taken before the refit.
 * The library's own rule, not bit-compatible with OpenCV: parity is pinned only
 * against tests/affine_oracle.py, which restates the same steps.
 * thr = -3 behaves as 3, thr = 0 admits only an exact zero error, and a thr
 * whose square overflows float to +inf admits every pair with a finite or
 * infinite (not NaN) error, so the first hypothesis ends the loop.
 * Non-finite coordinates: the call terminates (every loop is bounded by a
 * count), a hypothesis with a non-finite coefficient is no model, a row with a
 * NaN coordinate is never an inlier, one with an infinite coordinate only under
 * the +inf limit above; what the pair set as a whole gives (found, A) is
 * otherwise unspecified, but A is always finite.  In the segmented forms below
 * the other segments are unaffected. */
#define SIFT_MODEL_AFFINE 0
#define SIFT_MODEL_SIMILARITY 1
int sift_estimate_affine(const float* src_xy, const float* dst_xy, int n, int model, double ransac_thresh,
                         int max_iters, double confidence, double* A, unsigned char* inlier_mask);

/* The same for every segment of a batch, on the device in stream order, with
 * the contract of sift_find_homography_segmented_device: segment b's pairs are
 * rows [clamp(m_offsets[b]), clamp(m_offsets[b+1])) of d_src_xy / d_dst_xy,
 * clamped to m_cap, and each segment gets exactly what sift_estimate_affine
 * gives for its pairs, bit for bit.  d_H is [n_segments][9] row-major: A's two
 * rows, then 0 0 1, so sift_warp_perspective_segmented_device,
 * sift_perspective_transform_segmented_device and the d_H / d_found prediction
 * of sift_knn_match_window_segmented_device take it as it is.  d_found[b] is 1
 * for a model, 0 for none, and then H[b] is nine zeros and the segment's mask
 * bytes are 0.  max_iters < 1 or confidence outside (0, 1) gives every segment
 * found = 0.  d_inlier_mask is [m_cap] bytes by pair row and may be NULL; bytes
 * outside [clamp(m_offsets[0]), clamp(m_offsets[n_segments])) and rows of d_H /
 * d_found past n_segments are never written.
 * Enqueued on the context stream, no synchronisation, no scratch.  A NULL
 * context, then an unknown model: SIFT_E_INVALID.  n_segments == 0 or m_cap ==
 * 0: SIFT_OK, nothing enqueued.  A NULL required buffer: SIFT_E_INVALID
 * (sift_last_error names it). */
int sift_estimate_affine_segmented_device(sift_ctx* ctx, const float* d_src_xy, const float* d_dst_xy,
                                          const int* d_m_offsets, int n_segments, int m_cap, int model,
                                          double ransac_thresh, int max_iters, double confidence, double* d_H,
                                          int* d_found, unsigned char* d_inlier_mask /* may be NULL */);
/* Host buffers (synchronous); src_xy / dst_xy have m_cap rows: */
int sift_estimate_affine_segmented(sift_ctx* ctx, const float* src_xy, const float* dst_xy, const int* m_offsets,
                                   int n_segments, int m_cap, int model, double ransac_thresh, int max_iters,
                                   double confidence, double* H, int* found, unsigned char* inlier_mask /* may be NULL */);

/* ---- fundamental matrix ----------------------------------------------------- */
/* `findFundamentalMat(points1, points2, FM_RANSAC)`: the third motion model, for
 * stereo pairs, structure from motion and video with parallax, where no planar
 * model fits.  n point pairs as interleaved (x, y) floats; OpenCV's defaults are
 * ransac_thresh 3, max_iters 1000, confidence 0.99.  F is a row-major 3x3 with
 * [dst; 1]^T F [src; 1] = 0 (OpenCV's convention), of rank 2; inlier_mask (n
 * bytes, may be NULL) gets the RANSAC inliers.  Host code, no context.
 * SIFT_E_INVALID (F and the mask zeroed) when no model is found, n < 8,
 * max_iters < 1 or confidence outside (0, 1).
 * The rule (csrc/fundamental_math.hpp) is sift_find_homography's loop with 8 in
 * place of 4: n == 8 is a direct fit with no subset check and a mask of ones
 * (none when the solve fails); otherwise subsets of 8 distinct rows from
 * RNG(~0), accepted when the last drawn point is collinear with no two earlier
 * ones in src and in dst (at most 10000 draws per hypothesis), a hypothesis wins
 * iff it has more than max(best, 7) inliers, and max_iters shrinks after every
 * win.
 * The solve, for a hypothesis and for the final model, is the normalised
 * 8-point algorithm in double, every sum in pair order: per image the centroid
 * (the float coordinates summed, divided by the count) and the scale sqrt(2) /
 * (mean of sqrt(dx^2 + dy^2)) -- a mean distance below DBL_EPSILON or a
 * non-finite one fails the solve --; the nine-term row [X x, X y, X, Y x, Y y,
 * Y, x, y, 1] over normalised coordinates (x, y src; X, Y dst); the 45 sums of
 * A^T A's upper triangle, mirrored; f = the eigenvector of its smallest
 * eigenvalue (the homography's cyclic Jacobi); rank 2 by F0 <- F0 - (F0 v) v^T
 * with v the eigenvector of the smallest eigenvalue of F0^T F0 (the same Jacobi
 * at 3x3: (F0 v) v^T is the sigma_3 u_3 v_3^T term of the SVD); F = T_dst^T F0
 * T_src, divided by F[8] when |F[8]| > FLT_EPSILON (OpenCV's rule; otherwise
 * left as it is); a non-finite entry fails the solve.
 * A pair is an inlier iff, with the nine coefficients cast to float and unfused
 * float arithmetic left to right, max(d_dst^2 s_dst, d_src^2 s_src) <=
 * (float)(thr * thr): the squared distances of each point to the other's
 * epipolar line, s = 1 / (a^2 + b^2) of that line.  A NaN error is never an
 * inlier.  The final model is the same solve over the best hypothesis's inliers
 * (a failed or non-finite refit leaves the RANSAC model); the mask is the best
 * hypothesis's, taken before the refit.  There is no Levenberg-Marquardt or
 * Sampson refinement and no 7-point solver (n == 7 gives none).
 * The library's own rule, not bit-compatible with OpenCV: parity is pinned only
 * against tests/fundamental_oracle.py, which restates the same steps.
 * thr = -3 behaves as 3, thr = 0 admits only an exact zero error, and a thr
 * whose square overflows float to +inf admits every pair with a finite or
 * infinite (not NaN) error, so the first hypothesis ends the loop.
 * Non-finite coordinates: the call terminates (every loop is bounded by a
 * count), a hypothesis with a non-finite coefficient is no model, a row with a
 * NaN coordinate is never an inlier, one with an infinite coordinate only under
 * the +inf limit above; what the pair set as a whole gives (found, F) is
 * otherwise unspecified, but F is always finite when found.  In the segmented
 * forms below the other segments are unaffected. */
int sift_find_fundamental(const float* src_xy, const float* dst_xy, int n, double ransac_thresh, int max_iters,
                          double confidence, double* F, unsigned char* inlier_mask);

/* The same for every segment of a batch, on the device in stream order, with
 * the contract of sift_estimate_affine_segmented_device: segment b's pairs are
 * rows [clamp(m_offsets[b]), clamp(m_offsets[b+1])) of d_src_xy / d_dst_xy,
 * clamped to m_cap, and each segment gets exactly what sift_find_fundamental
 * gives for its pairs, bit for bit.  d_F is [n_segments][9] row-major.
 * d_found[b] is 1 for a model, 0 for none, and then F[b] is nine zeros and the
 * segment's mask bytes are 0.  max_iters < 1 or confidence outside (0, 1) gives
 * every segment found = 0.  d_inlier_mask is [m_cap] bytes by pair row and may
 * be NULL; bytes outside [clamp(m_offsets[0]), clamp(m_offsets[n_segments])) and
 * rows of d_F / d_found past n_segments are never written.
 * Enqueued on the context stream, no synchronisation, no scratch, no host value
 * read.  A NULL context: SIFT_E_INVALID.  n_segments == 0 or m_cap == 0:
 * SIFT_OK, nothing enqueued.  A NULL required buffer: SIFT_E_INVALID
 * (sift_last_error names it). */
int sift_find_fundamental_segmented_device(sift_ctx* ctx, const float* d_src_xy, const float* d_dst_xy,
                                           const int* d_m_offsets, int n_segments, int m_cap, double ransac_thresh,
                                           int max_iters, double confidence, double* d_F, int* d_found,
                                           unsigned char* d_inlier_mask /* may be NULL */);
/* Host buffers (synchronous); src_xy / dst_xy have m_cap rows: */
int sift_find_fundamental_segmented(sift_ctx* ctx, const float* src_xy, const float* dst_xy, const int* m_offsets,
                                    int n_segments, int m_cap, double ransac_thresh, int max_iters, double confidence,
                                    double* F, int* found, unsigned char* inlier_mask /* may be NULL */);

/* ---- matching along epipolar lines (match_epipolar.hip) --------------------- */
/* Guided matching for the third model (Hartley & Zisserman, Algorithm 11.4):
 * the windowed matcher above, with its contract word for word -- segments and
 * clamping, d_t_offsets == NULL for a shared train set, local indices, k of 1
 * or 2, ascending (distance, local train index), idx -1 / dist +inf fill, rows
 * outside the query range untouched, n_segments == 0 or q_cap == 0 SIFT_OK with
 * nothing enqueued, SIFT_METRIC_L1_F32 / _L1_U8 / _L2SQR_U8 (SIFT_METRIC_L2SQR_F32
 * is rejected), distances the dense matchers' own bit for bit, context stream,
 * no synchronisation, no host read of an offset or a model -- and a second gate.
 * Train row t with keypoint (X, Y) is admissible for query row q with keypoint
 * (x, y) of segment b iff both tests hold:
 *   Window: fabsf(X - x) <= radius && fabsf(Y - y) <= radius, in float -- the
 *   windowed matcher's test around the query's OWN position, the disparity bound
 *   of a stereo search.  radius = +inf admits every row with comparable
 *   coordinates; a NaN coordinate on either side makes the row inadmissible,
 *   always.
 *   Band: skipped when d_F == NULL, or when d_found != NULL and d_found[b] == 0
 *   (the segment has no model: the window alone gates it).  Otherwise the pair
 *   must be an inlier of F = d_F + 9 b by sift_find_fundamental's own test at the
 *   limit t = (float)(band * band), the product formed in double: the nine
 *   coefficients cast to float, unfused float arithmetic left to right, both
 *   squared point-to-epipolar-line distances d_dst^2 s_dst and d_src^2 s_src
 *   <= t, with src = query and dst = train, the convention
 *   sift_find_fundamental* writes.  It is one function, compiled for the
 *   estimate and for this matcher (fmath::is_inlier, csrc/fundamental_math.hpp).
 *   A NaN error (a query at the epipole, a non-finite F) is inadmissible;
 *   band = +inf admits every pair whose two errors are not NaN, band = 0 only
 *   exact zeros.
 * d_F is [n_segments][9] doubles and d_found [n_segments] ints exactly as
 * sift_find_fundamental_segmented_device writes them, so pair b's model gates
 * pair b's next match in stream order with no host value, and d_idx / d_dist
 * [q_cap][k] go to sift_ratio_matches_device and the next estimate unchanged.
 * With d_F == NULL the output equals sift_knn_match_window_segmented_device(...,
 * d_H = NULL, ...) byte for byte at every radius; with radius = +inf as well and
 * finite coordinates it equals the dense call of the metric byte for byte.
 * rows, cols: the train images' extent, a hint that shapes the search grid; no
 * result depends on it.
 * SIFT_E_INVALID: the windowed matcher's list (NULL context, NULL required
 * buffer -- both keypoint arrays are required --, unknown metric, k outside
 * {1, 2}, radius negative or NaN, rows or cols < 1, unaligned rows), and band
 * negative or NaN.
 * Out of scope: a gated reverse pass or a gated cross-check (they would need
 * the transposed model and the inverse window), SIFT_METRIC_L2SQR_F32, and a
 * one-sided (train-image-only) distance. */
int sift_knn_match_epipolar_segmented_device(sift_ctx* ctx, int metric, const void* d_query,
                                             const sift_keypoint* d_q_kpts, const int* d_q_offsets, int n_segments,
                                             int q_cap, const void* d_train, const sift_keypoint* d_t_kpts,
                                             const int* d_t_offsets /* NULL = shared */, int t_cap,
                                             const double* d_F /* may be NULL */, const int* d_found /* may be NULL */,
                                             double band, float radius, int rows, int cols, int k, int* d_idx,
                                             float* d_dist);
/* Host buffers (synchronous); query and q_kpts have q_cap rows, train and
 * t_kpts t_cap rows, F n_segments x 9 doubles, found n_segments ints: */
int sift_knn_match_epipolar_segmented(sift_ctx* ctx, int metric, const void* query, const sift_keypoint* q_kpts,
                                      const int* q_offsets, int n_segments, int q_cap, const void* train,
                                      const sift_keypoint* t_kpts, const int* t_offsets /* NULL = shared */, int t_cap,
                                      const double* F /* may be NULL */, const int* found /* may be NULL */,
                                      double band, float radius, int rows, int cols, int k, int* idx, float* dist);

/* ---- relative pose and triangulation (pose.hip, pose_batch.hip) ------------- */
/* `recoverPose(E, points1, points2, K, R, t, distanceThresh, mask,
 * triangulatedPoints)` for a fundamental matrix and two calibrations: what a
 * calibrated stereo rig or a moving camera does with the third model.  The
 * convention is OpenCV's and sift_find_fundamental's: src is image 1, dst image
 * 2, [dst; 1]^T F [src; 1] = 0, X_dst = R X_src + t, E ~ [t]x R.  F, K_src, K_dst
 * are row-major 3x3 doubles; n point pairs as interleaved (x, y) floats in
 * pixels; mask_in (n bytes, may be NULL = every row) says which rows vote --
 * sift_find_fundamental's inlier mask --; distance_thresh is OpenCV's
 * distanceThresh (50 in its samples; +inf allowed).  pose gets the twelve
 * doubles of [R | t] row by row, the camera P_dst in normalised coordinates with
 * |t| = 1; E (9, may be NULL) the essential matrix; mask_out (n bytes, may be
 * NULL) the rows in front of both cameras; xyz (n x 3 doubles, may be NULL) their
 * 3-D points in the src camera's frame; *n_good their number.  Host code, no
 * context.  SIFT_E_INVALID with every output zeroed when there is no pose.
 * The rule (csrc/pose_math.hpp), in double + - * / and sqrt only, no libm:
 * 1. Calibration.  K may be any invertible matrix; K^-1 = adj(K) / det(K).  A
 *    zero or non-finite determinant or a non-finite entry of the inverse: no
 *    pose.  A pixel (x, y) becomes K^-1 (x, y, 1)^T divided by its third
 *    component.
 * 2. Essential matrix.  E0 = K_dst^T (F K_src).  The eigenpairs of E0^T E0 by
 *    the homography's cyclic Jacobi at 3x3, ordered sigma_1^2 >= sigma_2^2 >=
 *    sigma_3^2 (of equal values the one the Jacobi left first stays first).  A
 *    non-finite sigma^2 or sigma_2^2 <= 0 -- a zero F, an E0 of rank 1 or of a
 *    pure rotation where the arithmetic leaves an exact zero -- : no pose; one
 *    that is degenerate only up to rounding goes on to the vote.  u1 = E0 v1 / sigma_1, u2 = E0 v2 / sigma_2, u3 =
 *    u1 x u2; v3 is negated when det [v1 v2 v3] < 0.  The reported E is
 *    ((sigma_1 + sigma_2) / 2) (u1 v1^T + u2 v2^T), the nearest essential matrix
 *    (Hartley & Zisserman 9.6).
 * 3. Candidates.  With W = [0 -1 0; 1 0 0; 0 0 1]: R1 = U W V^T, R2 = U W^T V^T,
 *    t = u3, in cv::decomposeEssentialMat's order inside recoverPose: (R1, +t),
 *    (R2, +t), (R1, -t), (R2, -t).  A non-finite entry: no pose.
 * 4. Triangulation (cv::triangulatePoints, DLT).  For normalised points (x, y),
 *    (X, Y) and cameras P_src, P_dst (3x4) the four rows x P_src[2] - P_src[0],
 *    y P_src[2] - P_src[1], X P_dst[2] - P_dst[0], Y P_dst[2] - P_dst[1]; Q is the
 *    eigenvector of the smallest eigenvalue of A^T A (the same Jacobi at 4x4),
 *    the ten upper-triangle sums taken row 0 + row 1 + row 2 + row 3 and
 *    mirrored.  Inside pose recovery P_src = [I | 0], P_dst = [R | t].
 * 5. Cheirality.  A row is considered iff mask_in is NULL or its byte is
 *    non-zero.  A considered row is good for a candidate iff, with Q /= Q[3],
 *    0 < z < distance_thresh both for Q[2] and for (P_dst Q)[2], compared in
 *    double: a NaN is never good.  The winner is the first candidate with the
 *    largest count of good rows (OpenCV's >= chain); n_good is that count,
 *    mask_out[row] = considered and good under the winner, xyz[row] the winner's
 *    Q[0..2] for a good row and three zeros for any other.  There is a pose iff
 *    the decomposition succeeded and n_good >= 1.  distance_thresh <= 0 or NaN:
 *    no pose.
 * The library's own rule, pinned bit for bit against tests/pose_oracle.py; not
 * bit-compatible with OpenCV, which decomposes E by an SVD.  SIFT_E_INVALID also
 * for a NULL F, K, pose or n_good, NULL points with n > 0, and n < 0. */
int sift_recover_pose(const double* F, const double* K_src, const double* K_dst, const float* src_xy,
                      const float* dst_xy, int n, const unsigned char* mask_in /* may be NULL */,
                      double distance_thresh, double* pose /* [12], rows of [R | t] */, double* E /* [9], may be NULL */,
                      unsigned char* mask_out /* [n], may be NULL */, double* xyz /* [n][3], may be NULL */,
                      int* n_good);

/* The same for every segment of a batch, on the device in stream order, with
 * the contract of sift_find_fundamental_segmented_device: segment b's pairs are
 * rows [clamp(m_offsets[b]), clamp(m_offsets[b+1])) of d_src_xy / d_dst_xy,
 * clamped to m_cap, and each segment gets exactly what sift_recover_pose gives
 * for its rows, bit for bit.  d_F [n_segments][9], d_found [n_segments] and
 * d_mask_in [m_cap] (may be NULL) are taken exactly as
 * sift_find_fundamental_segmented_device leaves d_F / d_found / d_inlier_mask,
 * and are only read; d_found[b] == 0 means no pose.  k_per_segment 0: d_K_src
 * and d_K_dst are one 3x3 each for all segments; 1: [n_segments][9].  d_pose is
 * [n_segments][12], the camera P_dst that
 * sift_triangulate_points_segmented_device takes; d_E [n_segments][9] (may be
 * NULL); d_pose_found and d_n_good [n_segments] ints; d_mask_out [m_cap] bytes
 * and d_xyz [m_cap][3] doubles by pair row (each may be NULL).  A segment with
 * no pose gets pose and E of zeros, pose_found 0, n_good 0, and zero mask_out
 * bytes and xyz rows.  Bytes and rows outside [clamp(m_offsets[0]),
 * clamp(m_offsets[n_segments])) and rows of the per-segment outputs past
 * n_segments are never written.
 * Enqueued on the context stream, no synchronisation, no scratch, no host value
 * read.  A NULL context: SIFT_E_INVALID.  n_segments == 0 or m_cap == 0:
 * SIFT_OK, nothing enqueued.  A NULL required buffer, a negative count or
 * k_per_segment outside {0, 1}: SIFT_E_INVALID (sift_last_error names it). */
int sift_recover_pose_segmented_device(sift_ctx* ctx, const float* d_src_xy, const float* d_dst_xy,
                                       const int* d_m_offsets, int n_segments, int m_cap, const double* d_F,
                                       const int* d_found, const double* d_K_src, const double* d_K_dst,
                                       int k_per_segment, const unsigned char* d_mask_in /* may be NULL */,
                                       double distance_thresh, double* d_pose, double* d_E /* may be NULL */,
                                       int* d_pose_found, int* d_n_good, unsigned char* d_mask_out /* may be NULL */,
                                       double* d_xyz /* may be NULL */);
/* Host buffers (synchronous); src_xy / dst_xy / mask_in / mask_out / xyz have
 * m_cap rows: */
int sift_recover_pose_segmented(sift_ctx* ctx, const float* src_xy, const float* dst_xy, const int* m_offsets,
                                int n_segments, int m_cap, const double* F, const int* found, const double* K_src,
                                const double* K_dst, int k_per_segment, const unsigned char* mask_in /* may be NULL */,
                                double distance_thresh, double* pose, double* E /* may be NULL */, int* pose_found,
                                int* n_good, unsigned char* mask_out /* may be NULL */, double* xyz /* may be NULL */);

/* `triangulatePoints(projMatr1, projMatr2, projPoints1, projPoints2, points4D)`:
 * step 4 above alone, with the caller's cameras (row-major 3x4 doubles) and
 * points as given -- no normalisation, and xyzw (n x 4 doubles) is the
 * homogeneous eigenvector, not divided by w, as cv::triangulatePoints divides
 * nothing.  It is the per-pair function of pose recovery, compiled once.  Host
 * code, no context; SIFT_E_INVALID for a NULL buffer or n < 0. */
int sift_triangulate_points(const double* P_src, const double* P_dst, const float* src_xy, const float* dst_xy, int n,
                            double* xyzw);
/* The same for every segment, on the device in stream order: segment b's rows
 * (clamped as above) are solved under d_P_src + 12 b and d_P_dst + 12 b into
 * d_xyzw [m_cap][4] by pair row; rows outside the segments are never written.
 * Context stream, no synchronisation, no scratch, no host value read; the
 * entry-point rules of sift_recover_pose_segmented_device. */
int sift_triangulate_points_segmented_device(sift_ctx* ctx, const float* d_src_xy, const float* d_dst_xy,
                                             const int* d_m_offsets, int n_segments, int m_cap, const double* d_P_src,
                                             const double* d_P_dst, double* d_xyzw);

/* ---- absolute pose of a view against 3-D points (pnp.hip, pnp_batch.hip) ----- */
/* `solveP3P` and `solvePnPRansac` for a calibrated view: where is the next frame
 * relative to the points that sift_recover_pose* left?  Convention: X_cam = R X
 * + t; a pose is the twelve doubles of [R | t] row by row, what
 * sift_recover_pose* writes and sift_triangulate_points* takes as P_dst.  xyz is
 * n x 3 doubles by row, xy the view's n interleaved (x, y) float pixels, row i
 * belonging to 3-D row i; K a row-major 3x3 double matrix, any invertible one.
 * The rule (csrc/pnp_math.hpp), in double + - * / and sqrt only, every loop of a
 * fixed length, no libm outside RANSAC's iteration count:
 * 1. Calibration.  K^-1 = adj(K) / det(K) as in sift_recover_pose; a singular or
 *    non-finite K: no model.  A pixel's normalised point (u, v) is K^-1 (x, y,
 *    1)^T divided by its third component, its bearing (u, v, 1) / sqrt(u u + v v +
 *    1).
 * 2. P3P on three rows, the Lambda-Twist route (Persson & Nordberg 2018), which
 *    needs neither cbrt nor acos.  With a_ij = |x_i - x_j|^2, b_ij = y_i . y_j the
 *    depths L satisfy L^T M_ij L = a_ij.  D1 = a23 M12 - a12 M23, D2 = a23 M13 -
 *    a13 M23.  The cubic det(D1 + g D2) has the coefficients det D1, tr(adj(D1)
 *    D2), tr(adj(D2) D1), det D2; a leading coefficient of exactly zero (or NaN):
 *    no solution.  Divided by it, the cubic is bisected for 64 steps on [-B, B],
 *    B = 1 + max |coefficient| (a negative value moves the lower end), then takes
 *    2 Newton steps (one is skipped where the derivative is zero).  The
 *    eigenpairs of D0 = D1 + g D2 by the homography's cyclic Jacobi at 3x3; the
 *    first eigenvalue of smallest magnitude is the zero one, the other two must
 *    be s1 > 0 > s2, else no solution; s = sqrt(-s2 / s1).  For the line w = e1 +
 *    s e2, then w = e1 - s e2: l1 = p l2 + q l3 with p = -w1 / w0, q = -w2 / w0;
 *    L = (p + q tau, 1, tau) in L^T D1 L = 0 is a quadratic a tau^2 + b tau + c;
 *    none for a negative discriminant; roots (sqrt(disc) - b) / 2a, then
 *    (-sqrt(disc) - b) / 2a; a root is kept iff tau > 0, p + q tau > 0 and den = 1
 *    + tau^2 - 2 b23 tau > 0; l2 = sqrt(a23 / den), l3 = tau l2, l1 = (p + q tau)
 *    l2; five Gauss-Newton steps on the three constraints (3x3 solve by adjugate
 *    and determinant; a zero determinant ends them).  R = Y X^-1, X's columns x1
 *    - x2, x1 - x3 and their cross product, Y's the same of l_i y_i, the inverse
 *    by adjugate and determinant; t = l1 y1 - R x1.  A non-finite entry drops the
 *    solution.  At most four, in the order (line +, line -) x (root +, root -).
 *    sift_solve_p3p returns exactly this list: *n_solutions poses at the front of
 *    poses, the rest zeros.  SIFT_OK also for none (a singular K among them);
 *    SIFT_E_INVALID for a NULL argument.
 * 3. A hypothesis is 4 rows: P3P on the first three; of its solutions that put
 *    the fourth point at z > 0 the first with the smallest squared reprojection
 *    error of the fourth row in normalised coordinates (an error that is not
 *    below +inf is no candidate); none: no model.
 * 4. Inlier test, no division, in double: p = K (R x + t), ex = p0 - x_pix p2, ey =
 *    p1 - y_pix p2; a row is an inlier iff p2 > 0 && ex ex + ey ey <= (thr thr)(p2
 *    p2).  A NaN is never an inlier, nor a row whose row_mask byte is 0 (row_mask
 *    NULL: every row counts).  thr = -8 behaves as 8, thr = 0 admits only an exact
 *    zero error, thr = +inf every row in front of the camera.  The all-zero rows
 *    sift_recover_pose* writes for rejected pairs carry a zero byte in its
 *    mask_out, so with that mask as row_mask they act as outliers: no compaction.
 * 5. The loop is sift_find_fundamental's with m = 4: n < 4 none; n == 4 a direct
 *    fit from rows 0..3 with a mask of ones (none if the solve fails or a row is
 *    masked out); else Rng{~0}, subsets of 4 distinct rows; a subset holding a
 *    masked-out row, or one whose solve gives nothing, is a counted iteration
 *    with no model; a hypothesis wins iff good > max(max_good, 3); after a win
 *    niters = update_num_iters(confidence, (n - good) / n, 4, niters), n the row
 *    count.  max_iters < 1 or confidence outside (0, 1): none.
 * 6. Final model.  The mask is the best hypothesis's, taken before the refit.
 *    The refit minimises the reprojection error in normalised coordinates over
 *    those inliers: five Gauss-Newton steps on six parameters, R <- R C(d) with
 *    the Cayley transform C = ((1 - a.a) I + 2 a a^T + 2 [a]x) / (1 + a.a), a = d /
 *    2, t <- t + dt; Jacobian rows d(X/Z, Y/Z)/dp_c . [-R [x]x | I]; the 21 + 6
 *    normal-equation sums and the cost in row order; the 6x6 solve by Gaussian
 *    elimination with partial pivoting (a pivot below 1e-300 ends the loop); a
 *    step is kept iff the cost fell, else the loop ends; a non-finite result
 *    leaves the RANSAC model.  R is written as computed.
 * pose gets [R | t]; inlier_mask (n bytes, may be NULL) the mask; *n_inliers its
 * count.  SIFT_E_INVALID with every output zeroed when there is no model, and
 * for a NULL K, pose or n_inliers, NULL rows with n > 0, and n < 0.  Host code, no
 * context.  The library's own rule, pinned bit for bit against
 * tests/pnp_oracle.py; not bit-compatible with OpenCV. */
int sift_solve_p3p(const double* xyz /* [3][3] */, const float* xy /* [3][2] */, const double* K,
                   double* poses /* [4][12] */, int* n_solutions);
int sift_solve_pnp(const double* xyz /* [n][3] */, const float* xy /* [n][2] */, int n,
                   const unsigned char* row_mask /* may be NULL */, const double* K, double reproj_thresh,
                   int max_iters, double confidence, double* pose /* [12], rows of [R | t] */,
                   unsigned char* inlier_mask /* [n], may be NULL */, int* n_inliers);

/* The same for every segment of a batch, on the device in stream order, with
 * the contract of sift_find_fundamental_segmented_device: segment b's rows are
 * rows [clamp(m_offsets[b]), clamp(m_offsets[b+1])) of d_xyz / d_xy / d_row_mask,
 * clamped to m_cap (a backwards pair is an empty segment; segments may overlap),
 * and each segment gets exactly what sift_solve_pnp gives for its rows, bit for
 * bit.  d_xyz is [m_cap][3] doubles exactly as sift_recover_pose_segmented_device
 * leaves d_xyz, d_row_mask [m_cap] bytes (may be NULL) exactly as it leaves
 * d_mask_out; both are only read.  k_per_segment 0: d_K is one 3x3 for all
 * segments; 1: [n_segments][9].  d_pose is [n_segments][12], d_found and
 * d_n_inliers [n_segments] ints, d_inlier_mask [m_cap] bytes by row (may be
 * NULL).  A segment with no model gets a pose of zeros, found 0, n_inliers 0 and
 * zero mask bytes.  Bytes outside the segments and rows of the per-segment
 * outputs past n_segments are never written.
 * Enqueued on the context stream, no synchronisation, no scratch, no host value
 * read.  A NULL context: SIFT_E_INVALID.  n_segments == 0 or m_cap == 0:
 * SIFT_OK, nothing enqueued.  A NULL required buffer, a negative count or
 * k_per_segment outside {0, 1}: SIFT_E_INVALID (sift_last_error names it).
 * max_iters < 1 or confidence outside (0, 1): every segment found = 0. */
int sift_solve_pnp_segmented_device(sift_ctx* ctx, const double* d_xyz, const float* d_xy, const int* d_m_offsets,
                                    int n_segments, int m_cap, const unsigned char* d_row_mask /* may be NULL */,
                                    const double* d_K, int k_per_segment, double reproj_thresh, int max_iters,
                                    double confidence, double* d_pose /* [n_segments][12] */, int* d_found,
                                    int* d_n_inliers, unsigned char* d_inlier_mask /* [m_cap], may be NULL */);
/* Host buffers (synchronous); xyz / xy / row_mask / inlier_mask have m_cap rows: */
int sift_solve_pnp_segmented(sift_ctx* ctx, const double* xyz, const float* xy, const int* m_offsets, int n_segments,
                             int m_cap, const unsigned char* row_mask /* may be NULL */, const double* K,
                             int k_per_segment, double reproj_thresh, int max_iters, double confidence, double* pose,
                             int* found, int* n_inliers, unsigned char* inlier_mask /* may be NULL */);

/* ---- the join of two match tables on a shared keypoint: 2-D / 3-D rows (join.hip) ----
 * sift_solve_pnp* wants row i of xyz to belong to row i of xy.  sift_recover_pose*
 * leaves xyz by pair row of the table between views b and b + 1; the next view's
 * pixels sit in another table, between b + 1 and b + 2, with other rows in another
 * order.  The two tables share the keypoints of view b + 1, and this call joins
 * them on that keypoint's index.  The rule for one segment:
 * Table A is na records with a_xyz ([na][3] doubles) and a_mask (na bytes, may be
 * NULL), exactly as sift_recover_pose* leaves xyz and mask_out.  Table B is nb
 * records with b_mask (nb bytes, may be NULL) and b_xy ([nb][2] floats), the new
 * view's pixel per record: the src_xy or dst_xy the ratio stage gathered.
 * a_key_side and b_key_side say which index of a record names the shared view's
 * keypoint, its query (SIFT_JOIN_QUERY) or its train (SIFT_JOIN_TRAIN); n_keys is
 * the shared view's keypoint count.  A record's segment field is not read.
 * 1. An A row is a candidate iff its mask byte is non-zero (or the mask is NULL),
 *    its key lies in [0, n_keys) and distance >= 0 (false for NaN).
 * 2. Among the candidates of one key the winner has the smallest
 *    ((uint64)bits(distance + 0.0f) << 32) | row: the smallest distance (-0.0 counts
 *    as 0, +inf is the largest), then the lowest row.  A ratio table may name one
 *    train keypoint from several queries; this decides between them.
 * 3. A B row joins iff its mask byte is non-zero (or the mask is NULL), its key lies
 *    in [0, n_keys) and that key has a winner.  Several B rows may join one A row.
 * 4. Joined B rows are written densely in B's row order: xyz_out[j] = a_xyz[winner]
 *    (three doubles copied bit for bit), xy_out[j] = b_xy[row], a_row[j] = winner,
 *    b_row[j] = row -- row indices into the caller's arrays, with which a caller
 *    extends its tracks.  b_joined[row] is 1 iff B row `row` joined, else 0, for
 *    every B row: its complement is the set of pairs to triangulate once the new
 *    view's pose is known.  Every output may be NULL; xyz_out needs a_xyz and
 *    xy_out needs b_xy.
 * No floating arithmetic beyond the + 0.0f.  Returns the number of joined rows (at
 * most nb, the capacity the row outputs need), or SIFT_E_INVALID for NULL records
 * with a count > 0, a negative count or a side outside {0, 1}.  Host code, no
 * context; pinned bit for bit against tests/join_oracle.py. */
#define SIFT_JOIN_QUERY 0
#define SIFT_JOIN_TRAIN 1
int sift_join_matches(const sift_match* a, int na, int a_key_side, const unsigned char* a_mask /* may be NULL */,
                      const double* a_xyz /* [na][3] */, const sift_match* b, int nb, int b_key_side,
                      const unsigned char* b_mask /* may be NULL */, const float* b_xy /* [nb][2] */, int n_keys,
                      double* xyz_out, float* xy_out, int* a_row, int* b_row, unsigned char* b_joined);

/* The same for every segment of a batch, on the device in stream order, with the
 * row contract of sift_find_fundamental_segmented_device on each of three offset
 * arrays (n_segments + 1 ints each, read on the device, never by the host):
 * segment s takes A rows [clamp(a_offsets[s]), clamp(a_offsets[s+1])) of d_a /
 * d_a_mask / d_a_xyz clamped to a_cap, B rows from d_b_offsets in the same way
 * clamped to b_cap (a backwards pair is an empty segment), and n_keys =
 * clamp(key_offsets[s+1]) - clamp(key_offsets[s]) clamped to key_cap, the total
 * keypoint count of the shared views; its winners live in entries
 * [clamp(key_offsets[s]), + n_keys) of a lookup of key_cap entries.  Each segment
 * gets exactly what sift_join_matches gives for its rows, with a_row and b_row
 * absolute rows of d_a and d_b.  Segment s's joined rows are [j_offsets[s],
 * j_offsets[s+1]) of d_xyz_out ([j_cap][3]), d_xy_out ([j_cap][2]), d_a_row and
 * d_b_row ([j_cap]), in segment order (an ordered scan, no atomics); d_j_offsets is
 * n_segments + 1 ints and its last entry is the true total; only the first j_cap
 * rows are written (j_cap = b_cap always suffices).  d_b_joined is [b_cap] bytes by
 * B row; bytes outside the segments' B rows are never written.  d_xyz_out, d_xy_out,
 * d_a_row, d_b_row, d_b_joined, the masks, d_a_xyz and d_b_xy may be NULL as above.
 * The record tables must be 16-byte aligned.  The inputs are only read, and may
 * alias each other.
 * Consecutive frames, one table and no copy: with d_matches / d_dst_xy / d_m_offsets
 * from sift_ratio_matches_device over the batch - 1 pairs of a batch matched as
 * sift_knn_match_l1_segmented_device describes (pair b: query = view b, train =
 * view b + 1), d_xyz / d_mask_out from sift_recover_pose_segmented_device on them
 * and d_img_offsets the batch's keypoint offsets, pass d_a = d_b = d_matches,
 * d_a_offsets = d_m_offsets, d_b_offsets = d_m_offsets + 1, a_cap = b_cap = m_cap,
 * a_key_side = SIFT_JOIN_TRAIN (view b + 1 is pair b's train), b_key_side =
 * SIFT_JOIN_QUERY (and pair b + 1's query), d_a_mask = d_mask_out, d_a_xyz = d_xyz,
 * d_b_mask = NULL, d_b_xy = d_dst_xy (view b + 2 is pair b + 1's train),
 * d_key_offsets = d_img_offsets + 1, n_segments = batch - 2.  d_xyz_out, d_xy_out and
 * d_j_offsets then go straight into sift_solve_pnp_segmented_device as d_xyz, d_xy
 * and d_m_offsets with d_row_mask = NULL.
 * Enqueued on the context stream, no synchronisation and no host value read; the
 * scratch (the lookup, two tables of n_segments + 1 ints and one count per 256 B
 * rows) is the context's one block, which grows, with a wait, only when a call
 * needs more than any call before it.  A NULL context: SIFT_E_INVALID.  A negative
 * count or a side outside {0, 1}: SIFT_E_INVALID.  n_segments == 0: SIFT_OK, nothing
 * enqueued.  A NULL required buffer (the offsets, d_j_offsets, a table with a
 * capacity > 0): SIFT_E_INVALID, nothing enqueued.  b_cap == 0: d_j_offsets is all
 * zeros.  Key slices that overlap because key_offsets decreases give unspecified
 * rows, and row ranges of one table that overlap (offsets that fall and rise
 * again) are joined only as far as cap / 256 + n_segments blocks of 256 rows reach
 * (d_j_offsets counts what was joined); every access stays in bounds. */
int sift_join_matches_segmented_device(sift_ctx* ctx, const sift_match* d_a, const int* d_a_offsets, int a_cap,
                                       int a_key_side, const unsigned char* d_a_mask /* may be NULL */,
                                       const double* d_a_xyz, const sift_match* d_b, const int* d_b_offsets, int b_cap,
                                       int b_key_side, const unsigned char* d_b_mask /* may be NULL */,
                                       const float* d_b_xy, const int* d_key_offsets, int key_cap, int n_segments,
                                       double* d_xyz_out, float* d_xy_out, int* d_a_row, int* d_b_row,
                                       unsigned char* d_b_joined, int j_cap, int* d_j_offsets);
/* Host buffers (synchronous); the tables have a_cap / b_cap rows, the row outputs j_cap: */
int sift_join_matches_segmented(sift_ctx* ctx, const sift_match* a, const int* a_offsets, int a_cap, int a_key_side,
                                const unsigned char* a_mask /* may be NULL */, const double* a_xyz,
                                const sift_match* b, const int* b_offsets, int b_cap, int b_key_side,
                                const unsigned char* b_mask /* may be NULL */, const float* b_xy,
                                const int* key_offsets, int key_cap, int n_segments, double* xyz_out, float* xy_out,
                                int* a_row, int* b_row, unsigned char* b_joined, int j_cap, int* j_offsets);

/* ---- lens undistortion: images and point rows (the calls in front of the chain) ----
 * dst = cv::undistort(src, K, dist, newK) with INTER_LINEAR and BORDER_CONSTANT 0,
 * and cv::undistortPoints(src, dst, K, dist, noArray(), P), for OpenCV's
 * 8-coefficient rational model: dist is always eight doubles
 * (k1, k2, p1, p2, k3, k4, k5, k6), unused ones zero.  K, newK and P are
 * row-major 3x3 doubles and may be any invertible matrix (P any finite one).
 * Stated here as the library's own rule (csrc/undistort_math.hpp, which host and
 * device both compile with -ffp-contract=off; restated in numpy in
 * tests/undistort_oracle.py): double + - * /, rint and the float blend, no libm
 * call.  It is not bit-compatible with OpenCV (whose undistort goes through
 * float maps and whose undistortPoints stops on a criterion); parity is by
 * construction and unpinned -- no OpenCV here.
 * The inverse of a calibration is K^-1 = adj(K) / det(K) exactly as step 1 of
 * sift_recover_pose forms it (nine cofactors, det = K0 c0 + K1 c3 + K2 c6, each
 * entry one divide).  A camera has no rule -- an image undistorts to zeros, a
 * segment's rows are zeros and its flag 0 -- when an entry of K, newK, P or
 * dist is not finite, or det(K) or det(newK) is zero or not finite or an entry
 * of the inverse is not finite.
 * The model's terms at normalised (x, y), in double, every multiply and add on
 * its own:
 *     xx = x x,  yy = y y,  r2 = xx + yy,
 *     num = 1 + ((k3 r2 + k2) r2 + k1) r2,  den = 1 + ((k6 r2 + k5) r2 + k4) r2,
 *     dx = ((2 p1) x) y + p2 (r2 + 2 xx),   dy = p1 (r2 + 2 yy) + ((2 p2) x) y.
 * project(A, u, v): X = (A0 u + A1 v) + A2, Y = (A3 u + A4 v) + A5,
 * W = (A6 u + A7 v) + A8, the point (X / W, Y / W).
 * Images, per destination pixel (u, v): (x, y) = project(newK^-1, u, v);
 * s = num / den, xd = x s + dx, yd = y s + dy; Wd = (K6 xd + K7 yd) + K8,
 *     fX = (32 ((K0 xd + K1 yd) + K2)) / Wd,  fY = (32 ((K3 xd + K4 yd) + K5)) / Wd;
 * from there the statement of sift_warp_perspective takes over unchanged: a NaN
 * fX or fY makes the pixel 0, the clamp to the int range, rint (ties to even),
 * the split into sx, ax, sy, ay, samples outside the image are 0 and never
 * read, and the f32 / u8 blends.
 * Points, per row (u, v): (x0, y0) = project(K^-1, u, v), x = x0, y = y0;
 * iters times (OpenCV's count is 5; 0 .. 100), with the terms taken at (x, y):
 *     icd = den / num,  x = (x0 - dx) icd,  y = (y0 - dy) icd;
 * then (x, y) = project(P, x, y) where P is given (NULL is the identity and is
 * not multiplied by: normalised coordinates, as OpenCV gives them; P = K gives
 * ideal pixels under the same K, what sift_find_fundamental* and
 * sift_recover_pose* take); then one rounding of each to float.  A NaN row
 * gives a NaN row and harms no other. */
/* Images on the device, enqueued on the context stream: one launch, no scratch,
 * no host value read, no synchronisation.  d_K, d_dist, d_newK hold one camera
 * for the whole batch (k_per_segment 0: 9, 8, 9 doubles) or one per image
 * (k_per_segment 1: [n][9], [n][8], [n][9]); d_newK may be NULL: K.  Pixel types
 * and strides (bytes, 0 = packed; img_stride == 0 with n > 1 is one source image
 * for every camera) as sift_warp_perspective_segmented_device takes them;
 * out_rows x out_cols may differ from the source size.  Only the destination
 * pixels are written; destination rows that are 16-byte aligned (u8: 4-byte)
 * are written with 16-byte (dword) stores.  Under one shared camera a workgroup
 * forms its tile's source positions once and walks a group of images with
 * them.  Errors as the warp call's: a NULL context or buffer, a dimension < 1,
 * a pixel / channels pair other than F32 x 1, U8 x 1, U8 x 3, a stride too
 * small, an f32 stride or pointer not a multiple of 4, k_per_segment outside
 * {0, 1}: SIFT_E_INVALID; a dimension above 2^30: SIFT_E_SIZE; n == 0: SIFT_OK,
 * nothing enqueued.  Under SIFT_FLAG_PROFILE the stage is "undistort". */
int sift_undistort_batch_device(sift_ctx* ctx, int pixel, int channels, const void* d_src, int rows, int cols,
                                size_t row_stride, size_t img_stride, const double* d_K, const double* d_dist,
                                const double* d_newK /* may be NULL: K */, int k_per_segment, int n, void* d_dst,
                                int out_rows, int out_cols, size_t out_row_stride, size_t out_img_stride);
/* Host buffers (synchronous), one image: only the bytes a strided view owns are
 * read; dst is out_rows x out_cols pixels, packed.  SIFT_E_INVALID with dst
 * zeroed if the camera has no rule. */
int sift_undistort(sift_ctx* ctx, int pixel, int channels, const void* src, int rows, int cols, size_t row_stride,
                   const double* K, const double* dist, const double* newK /* may be NULL: K */, void* dst,
                   int out_rows, int out_cols);
/* Points.  A row is an (x, y) float pair; rows are xy_stride_bytes apart in src
 * and in dst alike (a multiple of 4, at least 8: 8 is a src_xy / dst_xy array,
 * sizeof(sift_keypoint) a keypoint array, whose other fields are not touched).
 * dst may be src.  Host code, no context, one camera: SIFT_E_INVALID for a NULL
 * buffer, n < 0, iters outside 0 .. 100 or a bad stride (nothing written), and
 * for a camera with no rule (the n rows zeroed). */
int sift_undistort_points(const double* K, const double* dist, const double* P /* may be NULL: identity */, int iters,
                          const void* src, void* dst, size_t xy_stride_bytes, int n);
/* The same for every segment, on the device in stream order: segment b's rows
 * [m_offsets[b], m_offsets[b + 1]), clamped to m_cap as in
 * sift_triangulate_points_segmented_device (segments may overlap or run
 * backwards; with dst == src, overlapping segments are unspecified), go through
 * camera b (k_per_segment 1: d_K [n][9], d_dist [n][8], d_P [n][9]) or the one
 * camera (k_per_segment 0); rows outside the segments are never written.
 * d_ok [n_segments]: 1, or 0 where the segment's camera has no rule (its rows
 * are zeros); written for every segment, also when m_cap == 0.  Context stream,
 * one launch, no synchronisation, no scratch, no host value read.  Rows must be
 * 4-byte aligned. */
int sift_undistort_points_segmented_device(sift_ctx* ctx, const void* d_src, void* d_dst, size_t xy_stride_bytes,
                                           const int* d_m_offsets, int n_segments, int m_cap, const double* d_K,
                                           const double* d_dist, const double* d_P /* may be NULL */,
                                           int k_per_segment, int iters, int* d_ok);
/* Host buffers (synchronous): only the rows between the smallest and the largest
 * clamped offset travel; rows outside the segments keep their bytes. */
int sift_undistort_points_segmented(sift_ctx* ctx, const void* src, void* dst, size_t xy_stride_bytes,
                                    const int* m_offsets, int n_segments, int m_cap, const double* K,
                                    const double* dist, const double* P /* may be NULL */, int k_per_segment,
                                    int iters, int* ok);

/* ---- self-test ------------------------------------------------------------ */
/* Evaluates one device arithmetic helper element-wise on host arrays (n
 * values), for bit-exact checks of the GPU math against the CPU oracle:
 * op 0 exp32f(a), 1 fastAtan2(a, b) (y = a, x = b, degrees), 2 magnitude(a, b),
 * 3 (float)cos((double)a), 4 (float)sin((double)a), 5 (float)exp2((double)a),
 * 6 cvRound(a) (as float), 7 cvFloor(a) (as float),
 * 8 the homography's RANSACUpdateNumIters(0.995, (double)(b - a) / b, 4, 2000)
 * for a = good inliers of b = n pairs (integers as floats, exact below 2^24; the
 * result as float), 9 the same with confidence 0.5: the one libm-dependent
 * site of sift_find_homography_segmented_device, evaluated on the device. */
int sift_selftest_math(sift_ctx* ctx, int op, const float* a, const float* b, float* out, int n);
/* The point evaluation of an octave's widest scale that batch SIFT_NCL uses
 * instead of blurring that plane: for each of n points (r, c) = rc[2i], rc[2i+1]
 * of a packed rows x cols plane, out[9i + 3(dy+1) + (dx+1)] =
 * Gaussian_Blur(plane, sig[4]) at (r + dy, c + dx), dy, dx in -1..1 -- the dense
 * blur's floats.  Points may lie anywhere with |r|, |c| < 2^20. */
int sift_selftest_g4_points(sift_ctx* ctx, const float* plane, int rows, int cols, const int* rc, int n, float* out);
/* Diagnostic of the same point evaluation in the last sift_detect_compute_batch
 * call of the context (synchronises its stream; zeros when that call blurred
 * every plane 4 densely): the slots the first fill served, the slots whose
 * refinement then waited for a further patch, and the most fills any one slot
 * took (at most 5, the reference's SIFT_MAX_INTERP_STEPS). */
int sift_g4_fill_stats(sift_ctx* ctx, int* first_slots, int* waiting, int* max_fills);

/* ---- profiling ------------------------------------------------------------ */
/* With SIFT_FLAG_PROFILE: per-stage device time accumulated since the last
 * reset (synchronises).  Writes up to cap entries, *n gets the count. */
int sift_get_stage_stats(sift_ctx* ctx, sift_stage_stat* out, int cap, int* n, int reset);

#ifdef __cplusplus
}
#endif
#endif /* SIFT_HIP_H_ */
