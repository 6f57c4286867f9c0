"""Deterministic crafted inputs for the detect / describe kernels.

Two kinds, all seeded and all finite (NaN / Inf inputs stay unspecified: the
reference defines no ordering for them):

* pyramid families for findScaleSpaceExtrema / calDescriptor -- packed
  Gaussian (5 planes per octave) and DoG (4 planes per octave) arrays that are
  not real pyramids, so that refinement rejections, singular Hessians, ties and
  many-peaked orientation histograms are reached cheaply;
* image families for the full SIFT_NCL path.

tests/test_adversarial_inputs.py asserts, on the CPU oracle alone, which
branches each committed case reaches; tests/test_gpu_adversarial.py compares
the GPU with the oracle on the same inputs.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_OCTAVES = 5
PYRAMID_SHAPES = [(96, 128), (83, 117)]   # 83 x 117: every octave odd-sized in one dimension at least
IMAGE_SHAPES = [(240, 320), (203, 157)]
REGROW_SHAPE = (256, 320)


def octave_shapes(rows, cols, n_octaves=N_OCTAVES):
    out = []
    for _ in range(n_octaves):
        out.append((rows, cols))
        rows //= 2
        cols //= 2
    return out


def _pack(planes):
    return np.ascontiguousarray(np.concatenate([np.asarray(p, np.float32).reshape(-1) for p in planes]))


def _per_octave(rows, cols, per, make):
    """make(o, s, r, c) -> plane; packed over 5 octaves."""
    return _pack([make(o, s, r, c) for o, (r, c) in enumerate(octave_shapes(rows, cols)) for s in range(per)])


def _noise_gauss(rng, rows, cols):
    """White-noise u8 Gaussian planes."""
    return _per_octave(rows, cols, 5, lambda o, s, r, c: rng.integers(0, 256, (r, c)).astype(np.float32))


def _smooth121(a):
    p = np.pad(a, 1, mode="edge")
    a = (p[:-2, 1:-1] + 2 * p[1:-1, 1:-1] + p[2:, 1:-1]) / 4
    p = np.pad(a, 1, mode="edge")
    return (p[1:-1, :-2] + 2 * p[1:-1, 1:-1] + p[1:-1, 2:]) / 4


# ---- pyramid families ---------------------------------------------------------
def pyr_white(rows, cols, seed=1):
    """White-noise DoG (sigma 8) over white-noise u8 Gaussian planes."""
    rng = np.random.default_rng(seed)
    g = _noise_gauss(rng, rows, cols)
    d = _per_octave(rows, cols, 4, lambda o, s, r, c: rng.normal(0, 8, (r, c)).astype(np.float32))
    return g, d


def pyr_smooth(rows, cols, seed=2):
    """DoG noise smoothed in the plane ([1 2 1]^2 / 16) and across the scales of
    an octave, so that the quadratic fit is meaningful and refinement
    converges after moving."""
    rng = np.random.default_rng(seed)
    g = _noise_gauss(rng, rows, cols)
    planes = []
    for (r, c) in octave_shapes(rows, cols):
        raw = [_smooth121(rng.normal(0, 40, (r, c))) for _ in range(6)]
        planes += [(raw[s] + 2 * raw[s + 1] + raw[s + 2]) / 4 for s in range(4)]
    return g, _pack(planes)


def pyr_plateau(rows, cols, seed=3):
    """Integer-valued 2 x 2-block DoG: exact ties and singular Hessians."""
    rng = np.random.default_rng(seed)
    g = _noise_gauss(rng, rows, cols)

    def plane(o, s, r, c):
        b = rng.integers(-14, 15, ((r + 1) // 2, (c + 1) // 2))
        return np.kron(b, np.ones((2, 2)))[:r, :c]
    return g, _per_octave(rows, cols, 4, plane)


def pyr_flat(rows, cols, seed=4):
    """Flat Gaussian planes under a lively DoG: candidates are kept, every
    orientation histogram is zero, no keypoint comes out."""
    rng = np.random.default_rng(seed)
    g = _per_octave(rows, cols, 5, lambda o, s, r, c: np.full((r, c), 100.0 + s))
    d = _per_octave(rows, cols, 4, lambda o, s, r, c: rng.normal(0, 8, (r, c)).astype(np.float32))
    return g, d


def pyr_checker(rows, cols, seed=5):
    """A checkerboard Gaussian (3 x 3 cells of 0 / 255): gradients are 0 or
    +-255, so the orientation histograms are full of exact ties."""
    rng = np.random.default_rng(seed)

    def plane(o, s, r, c):
        yy, xx = np.mgrid[0:r, 0:c]
        return (((yy + s) // 3 + xx // 3) & 1) * 255.0
    g = _per_octave(rows, cols, 5, plane)
    d = _per_octave(rows, cols, 4, lambda o, s, r, c: rng.normal(0, 8, (r, c)).astype(np.float32))
    return g, d


# Hand-planted DoG neighbourhoods around a centre in layer 1 of octave 0;
# everything else in the DoG is zero.  Patches are [layer -1..+1][r -1..+1][c -2..+2].
def _nb(centre, **kw):
    """Centre value with every other entry 0, then named overrides 'lrc' ->
    value: l, r in {m, 0, p} (minus / same / plus), c in {M, m, 0, p, P} (-2 .. +2)."""
    a = np.zeros((3, 3, 5), np.float64)
    a[1, 1, 2] = centre
    ix = {"m": 0, "0": 1, "p": 2}
    cx = {"M": 0, "m": 1, "0": 2, "p": 3, "P": 4}
    for k, v in kw.items():
        a[ix[k[0]], ix[k[1]], cx[k[2]]] = v
    return a


def planted_neighbourhoods():
    """(name, patch) pairs.

    half_*: with v the centre, a = v in the next column and b = 0 in the
    previous one, g_c = (a - b) / 510 and d_cc = (a + b - 2 v) / 255 give the
    offset -g_c / d_cc = 0.5f: not < 0.5f, and cvRound(0.5f) = 0, so the
    candidate neither converges nor moves and is rejected after
    SIFT_MAX_INTERP_STEPS (the same along r and along the layer).

    huge: at an extremum the 1-D offset is bounded by 0.5, and a float 3 x 3
    solve's determinant cannot cancel below about 2^-24 of its terms (a random
    search over near-singular neighbourhoods reached 1.8e8 at most), so the
    INT_MAX / 3 rejection is reached in the SECOND step, where the point is no
    extremum and the gradient is unconstrained.  With v = 2^31 at the centre,
    -2 v on its left, -1 on its right, -7 v above and below it in scale and
    -13 v at (upper scale, left) and (lower scale, right), the first solve has
    g = (v, 0, 0) / 255, d_cc = -4 v / 255, d_ss = -16 v / 255 and
    d_cs = 6.5 v / 255: offsets (0.74, 0, 0.30), one column to the right.
    There the neighbours in the row are v and -v around -1, every cross
    derivative is 0, d_cc = 2 / 255 and g_c = -2 v / 510: offset v / 2 = 2^30,
    above INT_MAX / 3 = 7.2e8."""
    v = 2.0 ** 31
    huge = {"00m": -2 * v, "00p": -1.0, "00P": -v, "p00": -7 * v, "m00": -7 * v, "p0m": -13 * v, "m0p": -13 * v}
    return [
        ("half_c", _nb(16.0, **{"00p": 16.0})),
        ("half_r", _nb(16.0, **{"0p0": 16.0})),
        ("half_s", _nb(16.0, **{"p00": 16.0})),
        ("half_c_neg", _nb(-16.0, **{"00m": -16.0})),
        ("huge", _nb(v, **huge)),
        ("huge_neg", -_nb(v, **huge)),
        # finite pixels, non-finite arithmetic: the 3 x 3 determinant overflows to -inf and a
        # numerator to +inf, so the column offset is (-0) * inf = NaN: neither < 0.5f nor
        # > INT_MAX / 3, cvRound(NaN) moves nowhere, rejected after SIFT_MAX_INTERP_STEPS
        ("nan_offset", _nb(1e20, **{"00m": -1e20})),
        # isolated spike: diagonal Hessian, zero gradient, offset 0, kept
        ("spike", _nb(40.0)),
        # a constant block: every derivative 0, the 3 x 3 solve is singular (x = 0), then det <= 0
        ("flat_block", np.full((3, 3, 5), 12.0)),
    ]


def pyr_planted(rows, cols, seed=6):
    """Planted neighbourhoods on a 9-pixel grid in layers 0..2 of octave 0 of
    an otherwise zero DoG, over white-noise Gaussian planes."""
    rng = np.random.default_rng(seed)
    g = _noise_gauss(rng, rows, cols)
    shapes = octave_shapes(rows, cols)
    planes = [np.zeros(shapes[o], np.float32) for o in range(N_OCTAVES) for _ in range(4)]
    r0, c0 = 10, 10
    for _, nb in planted_neighbourhoods():
        for dl in range(3):
            planes[dl][r0 - 1:r0 + 2, c0 - 2:c0 + 3] = nb[dl]
        c0 += 9
        if c0 + 8 >= cols:
            r0, c0 = r0 + 9, 10
    return g, _pack(planes)


PYRAMID_FAMILIES = {"white": pyr_white, "smooth": pyr_smooth, "plateau": pyr_plateau, "flat": pyr_flat,
                    "checker": pyr_checker, "planted": pyr_planted}


def pyramid_cases():
    """Every committed (family, rows, cols)."""
    return [(f, r, c) for f in PYRAMID_FAMILIES for (r, c) in PYRAMID_SHAPES]


def regrow_pyramid():
    """The white-noise family at the size where the keypoints outgrow a fresh
    context's internal buffer while the raw extrema still fit its workspace."""
    return pyr_white(*REGROW_SHAPE, seed=7)


# ---- image families -----------------------------------------------------------
def img_noise_u8(rows, cols, seed=11):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols)).astype(np.float32)


def img_fractional(rows, cols, seed=12):
    return np.random.default_rng(seed).uniform(0, 255, (rows, cols)).astype(np.float32)


def img_u16_range(rows, cols, seed=13):
    return np.random.default_rng(seed).uniform(0, 65535, (rows, cols)).astype(np.float32)


def img_signed(rows, cols, seed=14):
    return np.random.default_rng(seed).normal(0, 80, (rows, cols)).astype(np.float32)


def img_stars(rows, cols, seed=None):
    """5-fold star discs, 128 + 127 sign(sin 5 theta) inside r < 14, centred on a
    32-pixel grid over a 128 background."""
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    dy, dx = (yy % 32) - 16, (xx % 32) - 16
    star = 128 + 127 * np.sign(np.sin(5 * np.arctan2(dy, dx)))
    return np.where(dy * dy + dx * dx < 14 * 14, star, 128.0).astype(np.float32)


def img_constant(rows, cols, seed=None):
    """Dark enough that the zero last row / column of the blurs (src/sift.cpp:116)
    stays under the DoG threshold: no keypoint at all."""
    return np.full((rows, cols), 32.0, np.float32)


def img_constant_bright(rows, cols, seed=None):
    """255 everywhere: the only structure is the blurs' zero last row / column,
    which yields a few keypoints in the coarse octaves of the larger shape."""
    return np.full((rows, cols), 255.0, np.float32)


IMAGE_FAMILIES = {"noise_u8": img_noise_u8, "fractional": img_fractional, "u16_range": img_u16_range,
                  "signed": img_signed, "stars": img_stars, "constant": img_constant,
                  "constant_bright": img_constant_bright}
BATCH_ORDER = ["constant", "noise_u8", "constant", "stars", "constant"]  # empty images first, between, last


# ---- the library's default capacities (read from its source, one truth) ---------
def default_candidate_capacity(max_rows, max_cols):
    """Candidate slots per image of a fresh context: max(FLOOR, px / DIV) as
    sift_ctx_create computes it from the named constants of
    sift-gpu_amd/csrc/ctx.hip."""
    return max(_ctx_constant("kCandidateFloor"), max_rows * max_cols // _ctx_constant("kPixelsPerCandidate"))


def keypoints_per_candidate_slot():
    """Initial internal keypoint buffer, in keypoints per candidate slot
    (alloc_candidates in ctx.hip)."""
    return _ctx_constant("kKeypointsPerCandidateSlot")


def _ctx_constant(name):
    src = open(os.path.join(ROOT, "sift-gpu_amd", "csrc", "ctx.hip")).read()
    m = re.search(r"constexpr\s+(?:long long|int)\s+" + name + r"\s*=\s*(\d+)\s*;", src)
    assert m, f"ctx.hip no longer defines {name} the way this helper reads"
    return int(m.group(1))
