"""The CPU oracle against the reference's own source over the arguments the
module entry points accept (inputs: tests/module_arg_inputs.py), bit for bit.

Covered values
  * blurs, 2-D and 1-D: w = floor(3 sigma) in {0, 1, 4, 6, 8, 12, 15, 18, 21, 36,
    75} on 64 x 96 and 37 x 300, w = 300 on 8 x 8, w in {4, 6} on 1 x 1, 1 x 40,
    40 x 1, 2 x 2, 3 x 70 and 70 x 3;
  * octave counts 6, 7, 8 (64 x 96, 203 x 157, 128 x 192, 33 x 1200, and 384 x 416
    whose sixth octave, 12 x 13, holds 5 keypoints) and the
    degenerate images 1 x 1 / 1, 2 x 2 / 2, 11 x 11 / 1, 12 x 12 / 1, 16 x 700 / 5,
    700 x 16 / 5, 10 x 300 / 4, 17 x 31 / 5 (shape / octaves): every DoG plane,
    keypoints, descriptors;
  * calDescriptor at firstOctave in {-2, -1, 0, 1, 2}: octave bytes 254, 255,
    0 .. 6, layers 0 .. 4, angles -30, -0.0, 0, 360, 400, 720 and the float below
    360, window radii 0 .. 212.

Inputs left to the oracle alone, and why
  * buildGaussianPyramid and SIFT_NCL with an octave count other than 5:
    src/sift.cpp:248 stores plane (o, i) at gpyr[o * nOctaves + i] and reads it at
    gpyr[o * nScales + i], so with 6 or more octaves it writes past the vector
    and with fewer it overwrites planes.  The reference's buildDoGPyramid,
    findScaleSpaceExtrema and calDescriptor index by nScales; they are compared
    on the oracle's Gaussian planes, and where the count is 5 the Gaussian
    planes and SIFT_NCL are compared too.
  * keypoints the CV_Assert of src/sift.cpp:744 refuses (or that index past
    gpyr, which it does not check): the reference aborts inside an OpenMP
    region.  The library returns SIFT_E_INVALID for them
    (test_gpu_module_args.py); the oracle is never given one.
  * caller keypoints with an angle outside [0, 720], here -30 (10 of the 80 rows
    at each firstOctave).  calcSIFTDescriptor wraps the orientation bin once, so
    with ori = 360 - angle = 390 the bin stays at -1 and the sample is added one
    float below its histogram cell; for the first cell that is below the
    histogram, in the CBin array of the same AutoBuffer.  No throw, but the bytes
    follow the reference's memory layout, so these rows are left out of the
    comparison with the reference and of the fixtures.  The library wraps the
    bin modulo 8 there (include/sift_hip.h), and test_gpu_module_args.py pins it
    against the oracle's test-only statement of that (oracle.circular_bins()),
    which test_circular_bins_is_the_reference_inside_the_contract pins here.
  Nothing else: w = 0 and 1-pixel-high or -wide planes run through the
  reference's own code without a throw or a read outside a Mat (w = 0: the 2-D
  kernel is the single tap 8192 / (2 pi sigma^2), the image times 3.98 at sigma
  0.2, and the 1-D loop `k = -ksize/2; k < ksize/2` has no iteration, all
  zeros; rows - 1 == 0 or cols - 1 == 0: getSubMatrix (:116) zeroes every
  element, all zeros).

A note on the border: the extrema scan covers [kBorder, n - kBorder) in both
directions, one pixel when a side is 2 kBorder + 1 = 11.  The reference and the
oracle both return two keypoints for the 11 x 11 image (one extremum, two
orientation peaks), so "no keypoint" is asserted where a side is at most
2 kBorder, and for 11 x 11 that every keypoint comes from the one scanned pixel.
"""
import functools
import os

import numpy as np
import pytest

import module_arg_inputs as M
from conftest import GOLDEN, assert_bits_equal, kp_bytes, load_golden, sha
from reference_inputs import args_image_fixture, check_fixture_descriptors, expected_device_descriptors, libm_rows

import refsrc as R

HAVE_REF = os.path.isdir(R.ref_build.reference_dir()) or os.path.exists(R.LIB_PATH)
needs_ref = pytest.mark.skipif(not HAVE_REF, reason=f"no reference directory {R.ref_build.reference_dir()} "
                               f"(SIFT_REFERENCE_DIR) and no built {os.path.relpath(R.LIB_PATH, os.path.dirname(GOLDEN))}")

BLUR_CASES = M.blur_cases()
IMAGE_CASES = M.OCTAVE_CASES + M.DEGENERATE_CASES


@pytest.fixture(scope="module")
def ref():
    R.lib()      # builds when stale; fails here if the reference is present but does not compile or load
    return R


@functools.lru_cache(maxsize=None)
def _oracle_image(oracle, case):
    """(img, packed Gaussian, packed DoG, keypoints, descriptors, branch counters) of the oracle."""
    b, r, c, n = case
    img = oracle.synth_image(b, r, c)
    g = oracle.build_gaussian_pyramid(img, n)
    d = oracle.build_dog_pyramid(g, r, c, n)
    oracle.extrema_stats_reset()
    kps = oracle.find_scale_space_extrema(g, d, r, c, n)
    stats = oracle.extrema_stats()
    return img, g, d, kps, oracle.calc_descriptors(g, r, c, kps, n), stats


@functools.lru_cache(maxsize=None)
def _caller(oracle):
    b, r, c = M.CALLER_IMAGE
    return r, c, oracle.build_gaussian_pyramid(oracle.synth_image(b, r, c), M.CALLER_OCTAVES)


# ---- (a) the oracle against the reference's source ---------------------------------------
@needs_ref
@pytest.mark.parametrize("case", BLUR_CASES, ids=M.blur_id)
def test_blurs(ref, oracle, case):
    r, c, sigma = case
    img = M.blur_image(r, c, sigma)
    assert_bits_equal(ref.gaussian_blur(img, sigma), oracle.gaussian_blur(img, sigma), f"blur {case}")
    assert_bits_equal(ref.gaussian_blur_1d(img, sigma), oracle.gaussian_blur_1d(img, sigma), f"blur1d {case}")


@needs_ref
@pytest.mark.parametrize("case", IMAGE_CASES, ids=M.image_id)
def test_images(ref, oracle, case):
    b, r, c, n = case
    img, g, d, ko, do, _ = _oracle_image(oracle, case)
    assert np.isfinite(g).all()
    if n == 5:
        assert_bits_equal(ref.build_gaussian_pyramid(img), g, "Gaussian planes")
    for i, (p, q) in enumerate(zip(ref.split_planes(ref.build_dog_pyramid(g, r, c, n), r, c, n, 4),
                                   oracle.split_planes(d, r, c, n, 4))):
        assert_bits_equal(p, q, f"DoG plane {i}")
    kr = ref.find_scale_space_extrema(g, d, r, c, n)
    dr = ref.calc_descriptors(g, r, c, kr, n)
    with oracle.libm_mode():
        k1 = oracle.find_scale_space_extrema(g, d, r, c, n)
        d1 = oracle.calc_descriptors(g, r, c, kr, n)
    assert len(kr) == len(k1)
    assert_bits_equal(kp_bytes(kr), kp_bytes(k1), "keypoints")
    assert_bits_equal(dr, d1, "descriptors")
    if n == 5:
        ks, ds = ref.sift(img)
        assert_bits_equal(kp_bytes(ks), kp_bytes(kr), "SIFT_NCL keypoints")
        assert_bits_equal(ds, dr, "SIFT_NCL descriptors")


@needs_ref
@pytest.mark.parametrize("fo", M.FIRST_OCTAVES)
def test_caller_keypoints(ref, oracle, fo):
    r, c, g = _caller(oracle)
    kps = M.caller_keypoints(fo, oracle.KEYPOINT_DTYPE)
    kps = kps[~M.angle_outside_contract(kps)]
    assert len(kps) == 70
    with oracle.libm_mode():
        do = oracle.calc_descriptors(g, r, c, kps, M.CALLER_OCTAVES, fo)
    assert_bits_equal(ref.calc_descriptors(g, r, c, kps, M.CALLER_OCTAVES, fo), do, f"firstOctave {fo}")


# ---- (b) the oracle alone ----------------------------------------------------------------
def test_w0_and_one_pixel_planes(oracle):
    img = M.blur_image(64, 96, 0.2)
    k = oracle.gaussian_kernel(0.2)
    assert k.shape == (1, 1) and 3.97 < float(k[0, 0]) / 8192 < 3.99
    ref = (img * k[0, 0]) / np.float32(8192)
    ref[-1, :] = 0          # the last row and column are never read (getSubMatrix)
    ref[:, -1] = 0
    assert_bits_equal(oracle.gaussian_blur(img, 0.2), ref + np.float32(0), "w = 0: the single tap")
    assert not oracle.gaussian_blur_1d(img, 0.2).any(), "w = 0: the 1-D tap loop is empty"
    for (r, c, s) in BLUR_CASES:
        if r == 1 or c == 1:
            img = M.blur_image(r, c, s)
            assert not oracle.gaussian_blur(img, s).any() and not oracle.gaussian_blur_1d(img, s).any()


@pytest.mark.parametrize("case", M.OCTAVE_CASES, ids=M.image_id)
def test_octave_cases_keypoints(oracle, case):
    """384 x 416 has keypoints in its sixth octave (index 5).  No octave of index 5 or higher of the other
    images can hold one: its planes are at most 37 columns by 1 row (33 x 1200) or 6 x 4 (203 x 157),
    inside the 5-pixel border."""
    b, r, c, n = case
    _, g, _, kps, _, stats = _oracle_image(oracle, case)
    assert np.isfinite(g).all()
    assert len(kps) > 20 and stats["keypoints"][:n].sum() == len(kps)
    high = (kps["octave"] & 255) >= 5
    if (r, c) == (384, 416):
        assert M.octave_can_hold_a_keypoint(r, c, 5)
        assert stats["keypoints"][5].sum() == high.sum() == 5
    else:
        assert not any(M.octave_can_hold_a_keypoint(r, c, o) for o in range(5, n))
        assert stats["keypoints"][5:].sum() == 0 and not high.any()
    # and the octaves beyond the fifth change nothing in the first five
    _, _, _, k5, d5, _ = _oracle_image(oracle, (b, r, c, 5))
    assert_bits_equal(kp_bytes(kps[~high]), kp_bytes(k5), "octave prefix")


def test_circular_bins_is_the_reference_inside_the_contract(oracle):
    """oracle.circular_bins() (the orientation bin modulo 8, the library's definition outside the
    reference's contract) changes no byte for an angle in [0, 720], and does change the rows at -30."""
    r, c, g = _caller(oracle)
    for fo in M.FIRST_OCTAVES:
        kps = M.caller_keypoints(fo, oracle.KEYPOINT_DTYPE)
        out = M.angle_outside_contract(kps)
        d0 = oracle.calc_descriptors(g, r, c, kps, M.CALLER_OCTAVES, fo)
        with oracle.circular_bins():
            d1 = oracle.calc_descriptors(g, r, c, kps, M.CALLER_OCTAVES, fo)
        assert_bits_equal(d0[~out], d1[~out], f"firstOctave {fo}")
        assert (d0[out] != d1[out]).any()
        assert np.isfinite(d1).all()


@pytest.mark.parametrize("case", M.DEGENERATE_CASES, ids=M.image_id)
def test_degenerate_images_keypoints(oracle, case):
    b, r, c, n = case
    _, g, _, kps, _, stats = _oracle_image(oracle, case)
    assert np.isfinite(g).all()
    if min(r, c) <= 2 * M.K_BORDER:
        assert stats["raw_extrema"] == 0 and len(kps) == 0
    if max(r, c) <= 2 * M.K_BORDER + 1:
        assert stats["raw_extrema"] <= 1      # the scan is one pixel, or empty


# ---- (c) the recorded fixtures ------------------------------------------------------------------
def test_fixture_blurs_equal_oracle(oracle):
    g = load_golden("ref_args_blur")
    assert list(g["ids"]) == [M.blur_id(c) for c in BLUR_CASES]
    for i, case in enumerate(BLUR_CASES):
        img = M.blur_image(*case)
        assert sha(oracle.gaussian_blur(img, case[2])) == str(g["blur_sha"][i]), case
        assert sha(oracle.gaussian_blur_1d(img, case[2])) == str(g["blur1d_sha"][i]), case


@pytest.mark.parametrize("case", IMAGE_CASES, ids=M.image_id)
def test_fixture_images_equal_oracle(oracle, case):
    b, r, c, n = case
    g, k = args_image_fixture(M.image_id(case))
    assert (int(g["seed"]), int(g["rows"]), int(g["cols"]), int(g["n_octaves"])) == case
    assert str(g["gpyr_from"]) == ("reference" if n == 5 else "oracle")
    _, gp, d, kps, desc, _ = _oracle_image(oracle, case)
    assert [sha(p) for p in oracle.split_planes(gp, r, c, n, 5)] == list(g["gpyr_sha"])
    assert [sha(p) for p in oracle.split_planes(d, r, c, n, 4)] == list(g["dog_sha"])
    assert len(kps) == int(g["n"])
    assert_bits_equal(kp_bytes(kps), k["kps"], "keypoints")
    # the reference's bytes, except that rows at libm-dependent angles are `desc_def` (reference_inputs.py)
    check_fixture_descriptors(desc, k, "descriptors")


@pytest.mark.parametrize("fo", M.FIRST_OCTAVES)
def test_fixture_caller_equals_oracle(oracle, fo):
    g = load_golden(f"ref_args_caller_fo{fo}")
    r, c, gp = _caller(oracle)
    kps = M.caller_keypoints(fo, oracle.KEYPOINT_DTYPE)
    assert_bits_equal(np.flatnonzero(~M.angle_outside_contract(kps)).astype(np.int32), g["rows"], "rows")
    kps = kps[g["rows"]]
    assert sha(kps) == str(g["kp_sha"]) and int(g["first_octave"]) == fo
    assert_bits_equal(oracle.calc_descriptors(gp, r, c, kps, M.CALLER_OCTAVES, fo), expected_device_descriptors(g),
                      f"firstOctave {fo}")


@needs_ref
def test_fixtures_are_the_live_reference(ref, oracle):
    """What make_ref_golden.py --args records, recomputed: digests and bytes off the libm-dependent rows."""
    g = load_golden("ref_args_blur")
    for i, case in enumerate(BLUR_CASES):
        img = M.blur_image(*case)
        assert sha(ref.gaussian_blur(img, case[2])) == str(g["blur_sha"][i])
        assert sha(ref.gaussian_blur_1d(img, case[2])) == str(g["blur1d_sha"][i])
    r, c, gp = _caller(oracle)
    for fo in M.FIRST_OCTAVES:
        g = load_golden(f"ref_args_caller_fo{fo}")
        kps = M.caller_keypoints(fo, oracle.KEYPOINT_DTYPE)[g["rows"]]
        keep = ~libm_rows(oracle, ref, kps)
        keep[g["libm_rows"]] = False
        assert_bits_equal(ref.calc_descriptors(gp, r, c, kps, M.CALLER_OCTAVES, fo)[keep], g["desc"][keep], f"fo {fo}")
