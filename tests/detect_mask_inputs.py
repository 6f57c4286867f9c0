"""The detection mask of SIFT_NCL (the *_masked entry points) written in numpy,
and the masks and inputs its CPU and GPU tests share.

The rule is cv::KeyPointsFilter::runByPixelsMask as include/sift_hip.h states it:
a keypoint with emitted coordinates (x, y) is dropped iff
mask[(int)(y + 0.5f)][(int)(x + 0.5f)] == 0, the sums formed in float32 and
truncated toward zero; an index outside the mask, or one formed from a NaN, drops
the keypoint.  The library keeps the survivors in the unmasked order, so the
expected output of an image is always `filter_keypoints(*unmasked, mask)`.
"""
import numpy as np

import adversarial_inputs as A

SHAPE = (203, 157)        # the one-image cases
BATCH_SHAPE = (160, 128)  # the batch cases
MARK_THREADS = 256        # threads of one workgroup of the mark kernel (detmask.hip, kDetMaskT)


def pixel_index(coord, size):
    """(index, valid) per coordinate: index = (int)(coord + 0.5f) where that lies in
    [0, size), formed in float32 and truncated toward zero.  The range test is
    made on the float sum -- it is in range iff -1 < sum < size -- so neither a
    NaN nor a value beyond int32 is ever converted."""
    s = np.asarray(coord, np.float32) + np.float32(0.5)
    assert s.dtype == np.float32
    with np.errstate(invalid="ignore"):
        valid = (s > np.float32(-1.0)) & (s < np.float32(size))   # NaN: False
    idx = np.where(valid, s, np.float32(0)).astype(np.int32)      # astype truncates toward zero
    return idx, valid


def keep_mask(x, y, mask):
    """Boolean array: which keypoints at (x, y) the mask keeps."""
    mask = np.asarray(mask)
    rows, cols = mask.shape
    c, cok = pixel_index(x, cols)
    r, rok = pixel_index(y, rows)
    ok = cok & rok
    keep = np.zeros(len(ok), bool)
    keep[ok] = mask[r[ok], c[ok]] != 0
    return keep


def filter_keypoints(kps, desc, mask):
    """(keypoints, descriptors) of one image under the mask, in their own order."""
    m = keep_mask(kps["x"], kps["y"], mask)
    return kps[m], desc[m]


# ---- masks ------------------------------------------------------------------------
def full(shape, value=1):
    return np.full(shape, value, np.uint8)


def zeros(shape):
    return np.zeros(shape, np.uint8)


def checkerboard(shape, keep_value=255):
    """1-pixel squares, (0, 0) kept: a keypoint's fate depends on the parity of both
    indices, so truncation instead of rounding, or x and y exchanged on a
    non-square mask, changes the kept set."""
    r, c = np.indices(shape)
    return np.where((r + c) % 2 == 0, keep_value, 0).astype(np.uint8)


def half_plane(shape, value=1):
    """The left half (columns below cols // 2) kept."""
    m = np.zeros(shape, np.uint8)
    m[:, :shape[1] // 2] = value
    return m


def window(shape, top, left, size=16, value=7):
    """A single kept size x size window."""
    m = np.zeros(shape, np.uint8)
    m[top:top + size, left:left + size] = value
    return m


def window_on_keypoints(shape, kps, size=16):
    """window() placed where it holds the most keypoints (by the rule above)."""
    best, arg = -1, (0, 0)
    for top in range(0, shape[0] - size + 1, 4):
        for left in range(0, shape[1] - size + 1, 4):
            n = int(keep_mask(kps["x"], kps["y"], window(shape, top, left, size)).sum())
            if n > best:
                best, arg = n, (top, left)
    return window(shape, *arg, size=size)


def batch_masks(shape, kps_of_window_image):
    """The five masks of the batch case: zeros, ones, checkerboard, half-plane, window."""
    return [zeros(shape), full(shape), checkerboard(shape), half_plane(shape),
            window_on_keypoints(shape, kps_of_window_image)]


def padded(mask, pad):
    """The mask in rows of cols + pad bytes whose padding holds the opposite of the
    row's last mask byte (255 after a zero, 0 after a non-zero): a kernel that took
    the packed stride would read shifted rows and padding."""
    rows, cols = mask.shape
    out = np.empty((rows, cols + pad), np.uint8)
    out[:, :cols] = mask
    out[:, cols:] = np.where(mask[:, -1:] == 0, 255, 0)
    return out


# ---- inputs -----------------------------------------------------------------------
def stars_blobs_image(rows=SHAPE[0], cols=SHAPE[1]):
    """adversarial_inputs.img_stars at 0.6 contrast plus seven smooth blobs (sigma 8,
    amplitude +-80): the stars' several hundred octave-0 extrema, and extrema in
    octaves 1 and 2 from the blobs.  Integer-valued in 0..255."""
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    bl = np.zeros_like(yy)
    for i, (cy, cx) in enumerate([(16, 16), (48, 80), (112, 48), (144, 112), (80, 144), (176, 16), (176, 80)]):
        bl += (1 if i % 2 else -1) * 80.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 8.0 * 8.0))
    return np.clip(np.round(A.img_stars(rows, cols) * 0.6 + 50 + bl), 0, 255).astype(np.float32)


def distinct_positions(kps):
    """Distinct (x, y, octave) triples: a lower bound on the live candidate slots."""
    if len(kps) == 0:
        return 0
    f = np.stack([kps["x"].view(np.int32), kps["y"].view(np.int32), kps["octave"] & 255], 1)
    return len(np.unique(f, axis=0))


def fractions(v):
    """(count with frac < 0.5, count with frac >= 0.5)"""
    f = np.asarray(v, np.float32) - np.floor(np.asarray(v, np.float32))
    return int((f < 0.5).sum()), int((f >= 0.5).sum())
