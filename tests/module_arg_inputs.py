"""Deterministic inputs over the arguments the module entry points accept.

Seeded generators only, shared by tests/test_module_args.py (CPU: the oracle
against the reference's own source), tests/test_gpu_module_args.py (GPU: the
library against both) and tests/golden/make_ref_golden.py (the recorded
family tests/golden/ref_args_*.npz).

* blur cases: (rows, cols, sigma) for Gaussian_Blur / Gaussian_Blur_1D, with
  w = floor(3 sigma) in {0, 1, 4, 6, 8, 12, 15, 18, 21, 36, 75, 300}: the single
  tap, every LDS-tile width {4, 8, 12, 18} at a sigma that is not the pyramid's
  own, generic widths beyond a tile and beyond the image, and planes with
  rows - 1 == 0 or cols - 1 == 0 (the getSubMatrix border rule zeroes them);
* octave cases: images with 6, 7 and 8 octaves (last planes 2 x 3 .. 1 x 1);
* degenerate images for the whole path, down to 1 x 1 with one octave;
* caller keypoints for calDescriptor at firstOctave in {-2 .. 2}: packed octave
  bytes covering oi = 0 .. 4 (bytes 254 and 255 are octaves -2 and -1), layers
  0 .. 4, angles outside [0, 360), window radii from 0 to beyond the row table
  and beyond the plane diagonal, positions inside, on and outside the plane;
  and the rows the CV_Assert analogue must refuse.
"""
import math

import numpy as np

K_BORDER = 5          # SIFT_IMG_BORDER
N_LAYERS = 2          # nOctaveLayers
MAX_WIN_ROWS = 81     # descriptor.hip: window rows with a row table (radius <= 40)
LDS_TILE_W = (4, 8, 12, 18)

# the pyramid's own blur sigmas (src/sift.cpp:237-244)
PYRAMID_SIGMAS = [math.sqrt(1.6 * 1.6 + 0.2 * 0.2)] + [
    float(np.float32(math.sqrt((2 ** (i / 2) * 1.6) ** 2 - 1.6 ** 2))) for i in range(1, 5)]


def kernel_half_width(sigma):
    """w of getGaussianKernel (float sigma) and getGaussianKernel1D (double sigma): the same for every sigma here."""
    w = int(math.floor(np.float32(3) * np.float32(sigma)))
    assert w == int(math.floor(3 * float(sigma))), sigma
    return w


# ---- blur cases ---------------------------------------------------------------------
BLUR_SIGMAS = [0.2, 0.34, 1.5, 2.0, 2.9, 4.2, 5.0, 6.1, 7.0, 12.0, 25.0]
BLUR_SHAPES = [(64, 96), (37, 300)]
BLUR_DEGENERATE_SHAPES = [(1, 1), (1, 40), (40, 1), (2, 2), (3, 70), (70, 3)]
BLUR_DEGENERATE_SIGMAS = [1.6, 2.0]


def blur_cases():
    """[(rows, cols, sigma)]"""
    cases = [(r, c, s) for (r, c) in BLUR_SHAPES for s in BLUR_SIGMAS]
    cases.append((8, 8, 100.0))
    cases += [(r, c, s) for (r, c) in BLUR_DEGENERATE_SHAPES for s in BLUR_DEGENERATE_SIGMAS]
    return cases


def blur_id(case):
    r, c, s = case
    return f"{r}x{c}-sigma{s:g}"


def blur_image(rows, cols, sigma):
    """Non-integer pixels of both signs off a 0 .. 255 ramp, seeded by the case."""
    rng = np.random.default_rng([rows, cols, int(round(sigma * 100))])
    return (rng.uniform(0, 255, (rows, cols)) - 16 * (rng.random((rows, cols)) < 0.1)).astype(np.float32)


def _check_blur_cases():
    cases = blur_cases()
    ws = {kernel_half_width(s) for (_, _, s) in cases}
    assert ws == {0, 1, 4, 6, 8, 12, 15, 18, 21, 36, 75, 300}, ws
    for w in LDS_TILE_W:   # each LDS-tile width with coefficients other than the pyramid's own
        assert any(kernel_half_width(s) == w and all(abs(s - p) > 0.02 for p in PYRAMID_SIGMAS)
                   for (r, c, s) in cases if min(r, c) > 1), w
    assert {kernel_half_width(p) for p in PYRAMID_SIGMAS} == set(LDS_TILE_W)
    assert any(kernel_half_width(s) > max(r, c) for (r, c, s) in cases)
    assert any(r == 1 for (r, c, s) in cases) and any(c == 1 for (r, c, s) in cases)


_check_blur_cases()


# ---- octave cases and degenerate images ---------------------------------------------------
# (seed of oracle.synth_image, rows, cols, octave count)
OCTAVE_CASES = [(21, 64, 96, 6), (21, 64, 96, 7), (22, 203, 157, 7), (22, 203, 157, 8), (23, 128, 192, 8),
                (24, 33, 1200, 6),
                (50, 384, 416, 6)]      # the one whose sixth octave (12 x 13) is wider than the border: 5 keypoints there
DEGENERATE_CASES = [(31, 1, 1, 1), (32, 2, 2, 2), (33, 11, 11, 1), (34, 12, 12, 1), (35, 16, 700, 5),
                    (36, 700, 16, 5), (37, 10, 300, 4), (38, 17, 31, 5)]
SCATTER_CASES = [OCTAVE_CASES[1], OCTAVE_CASES[3]]          # also run with the scatter blur forced
BATCH_CASE = (40, 64, 96, 7)                                # detect_compute_batch of three images: seeds 40, 41, 42


def image_id(case):
    b, r, c, n = case
    return f"{r}x{c}-{n}oct"


def max_octaves_for(rows, cols, limit=12):
    n = 0
    while n < limit and (rows >> n) >= 1 and (cols >> n) >= 1:
        n += 1
    return n


def octave_can_hold_a_keypoint(rows, cols, o):
    """The extrema scan covers rows / columns [kBorder, n - kBorder) of the octave's planes."""
    return (rows >> o) > 2 * K_BORDER and (cols >> o) > 2 * K_BORDER


for (_b, _r, _c, _n) in OCTAVE_CASES + DEGENERATE_CASES + [BATCH_CASE]:
    assert 1 <= _n <= max_octaves_for(_r, _c), (_r, _c, _n)
assert {n for (_, _, _, n) in OCTAVE_CASES} == {6, 7, 8}


# ---- caller keypoints ---------------------------------------------------------------------
CALLER_IMAGE = (11, 120, 160)       # oracle.synth_image(11, 120, 160), 5 octaves: planes 120 x 160 .. 7 x 10
CALLER_OCTAVES = 5
FIRST_OCTAVES = [-2, -1, 0, 1, 2]
ROWS_PER_FIRST_OCTAVE = 80
ANGLES = [-30.0, -0.0, 0.0, 360.0, 400.0, 720.0, float(np.nextafter(np.float32(360), np.float32(0)))]
# size in pixels of the keypoint's own octave: descriptor window radius = cvRound(size * 5.303...)
SIZES = [0.05, 0.2, None, None, 9.0, 11.5, 40.0]     # radius 0, 1, random 8 .. 37, 48, 61 (past the row table), 212


def pack_octave(octave, layer):
    """The KeyPoint::octave word: octave byte (two's complement) | layer << 8."""
    return (int(octave) & 255) | (int(layer) << 8)


def descriptor_radius(size_oct):
    return int(np.rint(np.float32(3 * size_oct * 0.5) * np.float32(1.4142135623730951) * 5 * np.float32(0.5)))


def caller_keypoints(first_octave, dtype, n=ROWS_PER_FIRST_OCTAVE):
    """n valid keypoints on the CALLER_IMAGE pyramid for calDescriptor(gpyr, kps, first_octave).
    Row i: oi = i % 5, layer = (i // 5) % 5, so every (oi, layer) pair occurs; angle, size and
    position classes cycle with co-prime periods."""
    _, rows, cols = CALLER_IMAGE
    rng = np.random.default_rng(1000 + first_octave)
    kps = np.zeros(n, dtype)
    for i in range(n):
        oi, layer = i % 5, (i // 5) % 5
        octave = first_octave + oi
        scale = 1.0 / (1 << octave) if octave >= 0 else float(1 << -octave)
        pr, pc = rows >> oi, cols >> oi
        a = ANGLES[i % 8] if i % 8 < len(ANGLES) else rng.uniform(0, 360)
        s = SIZES[i % 7]
        if s is None:
            s = rng.uniform(1.5, 7.0)
        pos = i % 9
        if pos < 4:                           # inside
            u, v = rng.uniform(0, pc - 1), rng.uniform(0, pr - 1)
        elif pos == 4:                        # on the border: first / last column, half-way cases of cvRound
            u, v = (0.0, pr - 1.0) if i % 2 else (pc - 1.0, 0.5)
        elif pos == 5:
            u, v = pc - 0.5, pr - 0.5
        else:                                 # outside, up to 3 pixels (and once far outside)
            u, v = rng.uniform(-3.0, pc + 3.0), rng.uniform(-3.0, pr + 3.0)
            if pos == 8:
                u, v = (-3.0 - pc, v) if i % 2 else (u, 2.0 * pr + 3.0)
        kps["x"][i] = np.float32(u / scale)
        kps["y"][i] = np.float32(v / scale)
        kps["size"][i] = np.float32(s / scale)
        kps["angle"][i] = np.float32(a)
        kps["response"][i] = np.float32(0.01 * i)
        kps["octave"][i] = pack_octave(octave, layer)
        kps["class_id"][i] = -1
    return kps


def angle_outside_contract(kps):
    """Rows whose angle is outside [0, 720].  calcSIFTDescriptor wraps the orientation bin once
    (src/sift.cpp: `if (o0 < 0) o0 += n; if (o0 >= n) o0 -= n;`), which is enough for ori = 360 - angle in
    [-360, 360].  Beyond that o0 stays at -1 (or n + ...) and the reference adds the sample one float below
    its cell of the histogram -- for the first cell, below the histogram itself, into the CBin array.  The
    oracle reproduces that layout (it equals the reference on these rows, test_module_args.py); the
    library's descriptor for such a row is unspecified (include/sift_hip.h)."""
    return (kps["angle"] < 0) | (kps["angle"] > 720)


OUTSIDE_ANGLES = [1000.0, -1000.0, -1.0, -30.0, 765.5, 12345.0, -720.5]


def outside_contract_keypoints(first_octave, dtype):
    """40 caller keypoints of which every second one has an angle outside [0, 720] (`OUTSIDE_ANGLES`: above
    765 the reference's single wrap leaves the bin at 9 or more, below -360 at -2 or less; -1 is
    cv::KeyPoint's "no orientation"), the others being valid rows of caller_keypoints."""
    kps = caller_keypoints(first_octave, dtype)
    kps = kps[~angle_outside_contract(kps)][:40].copy()
    for j in range(0, len(kps), 2):
        kps["angle"][j] = np.float32(OUTSIDE_ANGLES[(j // 2) % len(OUTSIDE_ANGLES)])
    assert angle_outside_contract(kps).sum() == 20
    return kps


def invalid_keypoints(first_octave, dtype):
    """[(name, one keypoint)] the CV_Assert analogue must refuse (src/sift.cpp:744 and the bounds of gpyr)."""
    good = caller_keypoints(first_octave, dtype, 10)[7:8]      # oi = 2, layer = 1
    out = []
    for name, octave, layer in [("oi=-1", first_octave - 1, 1), ("oi=n_oct", first_octave + CALLER_OCTAVES, 1),
                                ("layer=5", first_octave + 2, 5), ("layer=255", first_octave + 2, 255)]:
        k = good.copy()
        k["octave"][0] = pack_octave(octave, layer)
        out.append((name, k))
    return out


def _check_caller_keypoints():
    dt = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                   ("octave", "<i4"), ("class_id", "<i4")])
    bytes_seen = set()
    for fo in FIRST_OCTAVES:
        k = caller_keypoints(fo, dt)
        octave = (k["octave"] & 255).astype(np.int64)
        bytes_seen |= set(octave.tolist())
        octave = np.where(octave < 128, octave, octave - 256)
        pairs = set(zip((octave - fo).tolist(), ((k["octave"] >> 8) & 255).tolist()))
        assert pairs == {(o, l) for o in range(5) for l in range(5)}, fo
        assert set(np.float32(ANGLES).tolist()) <= set(k["angle"].tolist())
    assert {254, 255, 0, 1, 2, 3, 4, 5, 6} == bytes_seen
    radii = [descriptor_radius(s) for s in SIZES if s is not None]
    assert radii[:2] == [0, 1] and sum(2 * r + 1 > MAX_WIN_ROWS for r in radii) == 3
    assert radii[-1] > math.hypot(CALLER_IMAGE[1], CALLER_IMAGE[2])      # beyond the diagonal of every plane
    assert len(FIRST_OCTAVES) * ROWS_PER_FIRST_OCTAVE == 400


_check_caller_keypoints()
