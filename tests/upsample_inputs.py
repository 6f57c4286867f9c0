"""The upsampled first octave (sift_set_upsample, sift_upsample2x) written in
numpy, and the inputs its CPU and GPU tests share.

The doubling rule is include/sift_hip.h's statement of
cv::resize(src, Size(2 * cols, 2 * rows), 0, 0, INTER_LINEAR) on CV_32F: a
horizontal pass, then a vertical pass, both in float32, every value formed as
a * w0 + b * w1 with two multiplies and one add.  For destination index d along
an axis of n source samples S:
    d even: s = d / 2 - 1,   weights (0.25, 0.75) on (S[s], S[s + 1])
    d odd:  s = (d - 1) / 2, weights (0.75, 0.25)
    s < 0:      S[0], copied;   s >= n - 1: S[n - 1], copied.

The expected output of an upsampled SIFT_NCL is the CPU oracle's output on the
doubled image with OpenCV's post-pass for firstOctave < 0 (half_scale): x, y
and size times 0.5, the low byte of octave decremented, descriptors unchanged.
"""
import numpy as np

# (rows, cols) and the synthetic image's seed; at 5 octaves they give 99 -> 257,
# 165 -> 414 and 19 -> 56 keypoints (plain -> upsampled)
IMAGES = {"128x160": (128, 160, 0), "157x203": (157, 203, 0), "96x64": (96, 64, 0)}
OCTAVES = (5, 6)
BATCH_SHAPE = (128, 160)
BATCH_SEEDS = (0, 1, 2)


def _double_axis0(S):
    n = S.shape[0]
    D = np.empty((2 * n,) + S.shape[1:], np.float32)
    for d in range(2 * n):
        s, w0, w1 = (d // 2 - 1, 0.25, 0.75) if d % 2 == 0 else ((d - 1) // 2, 0.75, 0.25)
        if s < 0:
            D[d] = S[0]
        elif s >= n - 1:
            D[d] = S[n - 1]
        else:
            a = S[s] * np.float32(w0)
            b = S[s + 1] * np.float32(w1)
            D[d] = a + b
    return D


def upsample2x_ref(img):
    """img [rows, cols] float32 -> [2 * rows, 2 * cols] float32 by the rule above."""
    img = np.ascontiguousarray(img, np.float32)
    assert img.ndim == 2 and img.size > 0
    with np.errstate(all="ignore"):
        h = _double_axis0(img.T).T      # the horizontal pass
        return np.ascontiguousarray(_double_axis0(np.ascontiguousarray(h)))


def half_scale(kps):
    """OpenCV's post-pass in SIFT::detectAndCompute for firstOctave < 0, on a copy."""
    out = np.array(kps, copy=True)
    for f in ("x", "y", "size"):
        out[f] = kps[f] * np.float32(0.5)
    out["octave"] = (kps["octave"] & ~255) | ((kps["octave"] - 1) & 255)
    return out


def double_scale(kps):
    """half_scale undone (exact: the factors are powers of two)."""
    out = np.array(kps, copy=True)
    for f in ("x", "y", "size"):
        out[f] = kps[f] * np.float32(2.0)
    out["octave"] = (kps["octave"] & ~255) | ((kps["octave"] + 1) & 255)
    return out


def image(name):
    import oracle as O
    O.build()
    rows, cols, seed = IMAGES[name]
    return O.synth_image(seed, rows, cols)


def batch_images():
    import oracle as O
    O.build()
    return [O.synth_image(s, *BATCH_SHAPE) for s in BATCH_SEEDS]


_expected = {}


def expected(img, n_oct=5):
    """(keypoints, descriptors) an upsampled SIFT_NCL of img must give:
    oracle.sift(upsample2x_ref(img), n_oct) with the half-scale post-pass.
    Computed once per (image, octave count) and never changed."""
    import oracle as O
    O.build()
    img = np.ascontiguousarray(img, np.float32)
    key = (img.shape, img.tobytes(), n_oct)
    if key not in _expected:
        kps, desc = O.sift(upsample2x_ref(img), n_oct)
        kps = half_scale(kps)
        kps.setflags(write=False)
        desc.setflags(write=False)
        _expected[key] = (kps, desc)
    return _expected[key]
