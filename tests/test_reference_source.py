"""The CPU oracle against the reference's own source.

oracle/_ref/libsift_ref.so is the reference's src/sift.cpp, compiled unmodified
with its makefile's flags over the stand-in OpenCV headers of oracle/cvmini/
(oracle/ref_build.py, bound by oracle/refsrc.py).  Every comparison here is
total and bit for bit, reference source against oracle/sift_oracle.c: single
blurs, every Gaussian and DoG plane, extrema, descriptors, the crafted inputs
of adversarial_inputs.py, and the header's primitives against the oracle's (the
third statement of each, next to the numpy ones in test_oracle.py).

Outcome.  The oracle departs from the reference's text in
one respect, on purpose: src/sift.cpp calls libm's cosf / sinf (:583-584) and
powf (:384), the oracle and the device take (float)f((double)x).  Under
"glibc 2.35" cosf differs from that on 27165 and sinf on 27147 of 2^21
descriptor angles (1.3 % each, always by one ulp, the oracle's value being the
correctly rounded one), powf(2, y) on 1279 of 2^21 (test_libm_against_oracle_
definition pins these counts).  At that rate no choice of seeds keeps the
keypoint angles of these inputs clear of such values -- the white-noise
pyramid alone has 6201 keypoints, of which 173 sit on one -- so the check that
no keypoint angle of the inputs is libm-dependent cannot be had.  Instead the
oracle has a test-only switch, off by default (oracle.libm_mode()), that takes
libm at exactly those three call sites; with it every keypoint and descriptor
byte of every input below equals the reference's, on any libm.  So the three
calls are the whole difference, and nothing is excluded from a comparison.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import adversarial_inputs as A
from conftest import GOLDEN, assert_bits_equal, book_image, kp_bytes, load_golden, sha
from reference_inputs import REF_FIXTURES, descriptor_angles, expected_device_descriptors, libm_rows, ref_input
from test_gpu_parity import _helper_inputs
from test_oracle import GOLDEN_CASES, PYR_SIGMAS

import refsrc as R

if not os.path.isdir(R.ref_build.reference_dir()) and not os.path.exists(R.LIB_PATH):
    pytest.skip(f"no reference directory {R.ref_build.reference_dir()} (SIFT_REFERENCE_DIR) and no built "
                f"{os.path.relpath(R.LIB_PATH, os.path.dirname(GOLDEN))}", allow_module_level=True)

# The libm under which the counts below and the bytes of tests/golden/ref_*.npz that follow libm were recorded.
LIBM = "glibc 2.35"
LIBM_COUNTS = {3: 27165, 4: 27147, 5: 1279}    # cosf, sinf, powf(2, .): differing values of 2^21


def _libm_here():
    f = ctypes.CDLL(None).gnu_get_libc_version
    f.restype = ctypes.c_char_p
    return "glibc " + f().decode()


LIBM_MATCHES = _libm_here() == LIBM


@pytest.fixture(scope="module")
def ref():
    R.lib()      # builds when stale; fails here if the reference is present but does not compile or load
    return R


def _ulps(a, b):
    """Distance in representable floats (finite, same-sign values)."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_equal(kr, dr, ko, do, what):
    """Reference (kr, dr) against the oracle with libm at the three call sites (ko, do): every byte."""
    assert len(kr) == len(ko), f"{what}: {len(kr)} reference keypoints, {len(ko)} oracle keypoints"
    assert_bits_equal(kp_bytes(kr), kp_bytes(ko), f"{what} keypoints")
    assert_bits_equal(dr, do, f"{what} descriptors")


# ---- (a) stage by stage -------------------------------------------------------------
@pytest.mark.parametrize("sigma", PYR_SIGMAS + [0.7, 1.0, 3.3])
def test_gaussian_blur(ref, oracle, sigma):
    img = oracle.synth_image(3, 97, 131)
    assert_bits_equal(ref.gaussian_blur(img, sigma), oracle.gaussian_blur(img, sigma), f"blur {sigma}")


@pytest.mark.parametrize("sigma", [1.6, 2.5, 4.0])
def test_gaussian_blur_1d(ref, oracle, sigma):
    """Includes the reference's `omp parallel num_threads(16)` row partition."""
    img = oracle.synth_image(5, 97, 131)
    assert_bits_equal(ref.gaussian_blur_1d(img, sigma), oracle.gaussian_blur_1d(img, sigma), f"blur1d {sigma}")


def golden_input(name, oracle):
    if name == "book":
        return book_image()
    g = load_golden(name)
    return oracle.synth_image(int(name[5]), int(g["rows"]), int(g["cols"]))


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_planes(ref, oracle, name):
    img = golden_input(name, oracle)
    r, c = img.shape
    assert max(r, c) <= 420 and min(r, c) <= 300
    g_ref, g_orc = ref.build_gaussian_pyramid(img), oracle.build_gaussian_pyramid(img)
    for i, (p, q) in enumerate(zip(ref.split_planes(g_ref, r, c, 5, 5), oracle.split_planes(g_orc, r, c, 5, 5))):
        assert_bits_equal(p, q, f"{name} Gaussian plane {i}")
    d_ref, d_orc = ref.build_dog_pyramid(g_ref, r, c), oracle.build_dog_pyramid(g_orc, r, c)
    for i, (p, q) in enumerate(zip(ref.split_planes(d_ref, r, c, 5, 4), oracle.split_planes(d_orc, r, c, 5, 4))):
        assert_bits_equal(p, q, f"{name} DoG plane {i}")


@functools.lru_cache(maxsize=None)
def _stages(oracle, name):
    """findScaleSpaceExtrema and calDescriptor of both sides on the same (oracle-built) pyramid."""
    img = golden_input(name, oracle)
    r, c = img.shape
    g = oracle.build_gaussian_pyramid(img)
    d = oracle.build_dog_pyramid(g, r, c)
    kr = R.find_scale_space_extrema(g, d, r, c)
    with oracle.libm_mode():
        ko, do = oracle.find_scale_space_extrema(g, d, r, c), oracle.calc_descriptors(g, r, c, kr)
    return kr, R.calc_descriptors(g, r, c, kr), ko, do


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_extrema_descriptors(ref, oracle, name):
    kr, dr, ko, do = _stages(oracle, name)
    assert len(kr) > 50
    check_equal(kr, dr, ko, do, name)


# ---- (b) primitives, three ways ----------------------------------------------------
@pytest.mark.parametrize("op", [0, 1, 2, 6, 7])
def test_header_primitives(ref, oracle, op):
    """exp32f, fastAtan2, magnitude32f, cvRound, cvFloor of oracle/cvmini against the oracle's."""
    a, b = _helper_inputs(op, np.random.default_rng(100 + op), 1 << 18)
    assert_bits_equal(ref.helper(op, a, b), oracle.helper(op, a, b), f"op {op}")


def test_header_rounding_edges(ref, oracle):
    x = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 2.4999, 2.5001, -0.0, 0.0, 254.5, 255.5, 256.0, -3.0, 1e6, -1e6,
                  np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(-0.5), np.float32(0))],
                 np.float32)
    for op in (6, 7):
        assert_bits_equal(ref.helper(op, x), oracle.helper(op, x), f"op {op}")
    assert_bits_equal(ref.saturate_u8(x), np.clip(np.rint(x), 0, 255).astype(np.float32) + np.float32(0), "saturate_cast<uchar>")


def test_header_solve3(ref, oracle):
    rng = np.random.default_rng(3)
    mats = []
    for k in range(4000):
        a = rng.normal(size=(3, 3)).astype(np.float32)
        if k % 2:
            a = a + a.T     # symmetric, like the Hessian of adjustLocalExtrema
        if k % 5 == 0:
            a = a * np.float32(10.0 ** rng.integers(-12, 12))
        mats.append((a, rng.normal(size=3).astype(np.float32)))
    one = np.ones((3, 3), np.float32)
    mats += [(one, np.ones(3, np.float32)), (np.zeros((3, 3), np.float32), np.ones(3, np.float32)),
             (np.diag(np.float32([1, 2, 0])), np.ones(3, np.float32)), (one * np.float32(12), np.zeros(3, np.float32))]
    for a, b in mats:
        x, ok = oracle.solve3(a, b)
        assert_bits_equal(ref.solve3(a, b), x, "solve3")
        assert ok or not x.any()


@pytest.mark.parametrize("shape", [(300, 210), (203, 157), (75, 52), (41, 29)])
def test_header_resize_nn(ref, oracle, shape):
    r, c = shape
    src = np.arange(r * c, dtype=np.float32).reshape(r, c)
    assert_bits_equal(ref.resize_nn(src, r // 2, c // 2), oracle.resize_nn(src, r // 2, c // 2), "resize")


# ---- (c) libm's cosf / sinf / powf against the oracle's definition --------------------
def _all_keypoint_angles(oracle):
    ks = [_stages(oracle, n)[0] for n in GOLDEN_CASES] + [_image(oracle, i)[0] for i in IMAGE_IDS]
    ks += [_pyramid(oracle, i)[0] for i in PYRAMID_IDS] + [_caller(oracle)[0]]
    return np.concatenate([descriptor_angles(k) for k in ks])


@pytest.mark.parametrize("op", [3, 4, 5])
def test_libm_against_oracle_definition(ref, oracle, op):
    """libm does not agree with (float)f((double)x) everywhere, so the oracle's definition stays and the
    count under LIBM is pinned.  Wherever the two differ they are neighbouring
    floats and the oracle's is the correctly rounded one."""
    n = 1 << 21
    if op == 5:
        x, _ = _helper_inputs(5, np.random.default_rng(105), n)
        exact = np.exp2(x.astype(np.float64))
    else:
        ori = (np.random.default_rng(100 + op).random(n) * 360).astype(np.float32)
        ori[ori >= 360] = 0
        x = ori * np.float32(np.pi / 180)
        x = np.concatenate([x, _all_keypoint_angles(oracle)])
        exact = (np.cos if op == 3 else np.sin)(x.astype(np.float64))
    lib, orc = ref.helper(op, x), oracle.helper(op, x)
    assert_bits_equal(orc, exact.astype(np.float32), f"op {op}: the oracle's value is the rounded double")
    bad = lib.view(np.uint32) != orc.view(np.uint32)
    print(f"op {op}: libm differs on {int(bad[:n].sum())} of {n} sampled values, {int(bad[n:].sum())} of {x.size - n} "
          f"keypoint angles ({_libm_here()})")
    assert np.array_equal(np.signbit(lib), np.signbit(orc))
    assert _ulps(np.abs(lib[bad]), np.abs(orc[bad])).max(initial=0) <= 1
    if LIBM_MATCHES:
        assert int(bad[:n].sum()) == LIBM_COUNTS[op]


# ---- (d) crafted inputs -------------------------------------------------------------------
IMAGE_IDS = [f"{f}-{r}x{c}" for f in A.IMAGE_FAMILIES for (r, c) in A.IMAGE_SHAPES]
PYRAMID_IDS = [f"{f}-{r}x{c}" for (f, r, c) in A.pyramid_cases()]


def _parse(case):
    fam, shape = case.rsplit("-", 1)
    r, c = shape.split("x")
    return fam, int(r), int(c)


@functools.lru_cache(maxsize=None)
def _image(oracle, case):
    fam, r, c = _parse(case)
    img = A.IMAGE_FAMILIES[fam](r, c)
    with oracle.libm_mode():
        return R.sift(img) + oracle.sift(img)


@functools.lru_cache(maxsize=None)
def _pyramid(oracle, case):
    fam, r, c = _parse(case)
    g, d = A.PYRAMID_FAMILIES[fam](r, c)
    kr = R.find_scale_space_extrema(g, d, r, c)
    with oracle.libm_mode():
        ko, do = oracle.find_scale_space_extrema(g, d, r, c), oracle.calc_descriptors(g, r, c, kr)
    return kr, R.calc_descriptors(g, r, c, kr), ko, do


@functools.lru_cache(maxsize=None)
def _caller(oracle):
    """The 600 caller-supplied keypoints of test_gpu_parity.test_descriptors_caller_keypoints_bitexact."""
    img = oracle.synth_image(11, 240, 320)
    r, c = img.shape
    g = oracle.build_gaussian_pyramid(img)
    rng = np.random.default_rng(5)
    n = 600
    kps = np.zeros(n, oracle.KEYPOINT_DTYPE)
    o = rng.integers(0, 5, n)
    layer = rng.integers(1, 3, n)
    size_oct = np.where(rng.random(n) < 0.25, rng.uniform(7.6, 12.0, n), rng.uniform(1.5, 7.0, n))
    kps["x"] = rng.uniform(-3.0, c + 3.0, n).astype(np.float32)
    kps["y"] = rng.uniform(-3.0, r + 3.0, n).astype(np.float32)
    kps["size"] = (size_oct * (1 << o)).astype(np.float32)
    ang = rng.uniform(0, 360, n).astype(np.float32)
    ang[:40] = 0.0
    ang[40:80] = np.nextafter(np.float32(360), np.float32(0))
    kps["angle"] = ang
    kps["octave"] = (o + (layer << 8)).astype(np.int32)
    with oracle.libm_mode():
        do = oracle.calc_descriptors(g, r, c, kps)
    return kps, R.calc_descriptors(g, r, c, kps), kps, do


@pytest.mark.parametrize("case", IMAGE_IDS)
def test_crafted_images(ref, oracle, case):
    check_equal(*_image(oracle, case), case)


@pytest.mark.parametrize("case", PYRAMID_IDS)
def test_crafted_pyramids(ref, oracle, case):
    check_equal(*_pyramid(oracle, case), case)


def test_caller_keypoints(ref, oracle):
    check_equal(*_caller(oracle), "caller keypoints")


def test_libm_mode_is_off_by_default_and_restored(oracle):
    """The switch is test-only: the oracle's definition is what every other test and the device use."""
    assert oracle.lib().so_get_libm() == 0
    with oracle.libm_mode():
        assert oracle.lib().so_get_libm() == 1
    assert oracle.lib().so_get_libm() == 0


# ---- (e) committed fixtures ------------------------------------------------------------------
# descriptor rows of each fixture whose bytes under the oracle's definition (`desc_def`) are not the reference's
ROWS_THAT_FOLLOW_LIBM = {"ref_book": 1, "ref_synth_160x128": 0, "ref_synth_203x157": 0, "ref_synth_240x320": 0,
                         "ref_fractional_203x157": 0, "ref_stars_203x157": 0}


@pytest.mark.parametrize("name", REF_FIXTURES)
def test_fixture_is_the_live_reference(ref, oracle, name):
    g = load_golden(name)
    img = ref_input(name, oracle)
    r, c = img.shape
    assert (r, c) == (int(g["rows"]), int(g["cols"])) and max(r, c) <= 420 and min(r, c) <= 300
    gp = ref.build_gaussian_pyramid(img)
    assert [sha(p) for p in ref.split_planes(gp, r, c, 5, 5)] == list(g["gpyr_sha"])
    assert [sha(p) for p in ref.split_planes(ref.build_dog_pyramid(gp, r, c), r, c, 5, 4)] == list(g["dog_sha"])
    kps, desc = ref.sift(img)
    assert len(kps) == int(g["n"]) > 0
    # no recorded keypoint byte depends on libm (make_ref_golden.py asserts it), so this holds on any libm
    assert_bits_equal(kp_bytes(kps), g["kps"], f"{name} keypoints")
    live = libm_rows(oracle, ref, kps)
    if LIBM_MATCHES:
        assert str(g["libm"]) == LIBM
        assert_bits_equal(np.flatnonzero(live).astype(np.int32), g["libm_rows"], "libm_rows")
        assert_bits_equal(desc, g["desc"], f"{name} descriptors")
    # rows that neither the recording libm nor this one decides
    keep = ~live
    keep[g["libm_rows"]] = False
    assert_bits_equal(desc[keep], g["desc"][keep], f"{name} descriptors off the libm rows")


@pytest.mark.parametrize("name", REF_FIXTURES)
def test_fixture_equals_oracle(oracle, name):
    """Needs no reference library: the recorded reference outputs against the oracle, every byte -- the
    reference's own, except that the rows at libm-dependent angles are `desc_def`."""
    g = load_golden(name)
    img = ref_input(name, oracle)
    r, c = img.shape
    gp = oracle.build_gaussian_pyramid(img)
    assert [sha(p) for p in oracle.split_planes(gp, r, c, 5, 5)] == list(g["gpyr_sha"])
    assert [sha(p) for p in oracle.split_planes(oracle.build_dog_pyramid(gp, r, c), r, c, 5, 4)] == list(g["dog_sha"])
    kps, desc = oracle.sift(img)
    assert_bits_equal(kp_bytes(kps), g["kps"], f"{name} keypoints")
    assert_bits_equal(desc, expected_device_descriptors(g), f"{name} descriptors")
    differ = (g["desc_def"].view(np.uint32) != g["desc"][g["libm_rows"]].view(np.uint32)).any(axis=1)
    assert int(differ.sum()) == ROWS_THAT_FOLLOW_LIBM[name]
    if LIBM_MATCHES:
        with oracle.libm_mode():
            kps, desc = oracle.sift(img)
        assert_bits_equal(kp_bytes(kps), g["kps"], f"{name} keypoints, libm at the three call sites")
        assert_bits_equal(desc, g["desc"], f"{name} descriptors, libm at the three call sites")


def test_1080p_golden_is_the_references(oracle):
    """The headline workload's golden against the one-off run of the reference's source at 1080p
    (make_ref_golden.py --1080p).  Planes and count by digest, nothing run; keypoints and descriptors by
    running the oracle once with each definition (about 15 s): the default gives the golden's digests, libm
    at the three call sites gives the reference's, and the two differ in exactly the recorded 14 `size`
    fields and 140 descriptor rows."""
    a, b = load_golden("synth0_1080x1920"), load_golden("ref_synth0_1080x1920")
    assert (int(a["rows"]), int(a["cols"])) == (int(b["rows"]), int(b["cols"])) == (1080, 1920)
    assert list(a["gpyr_sha"]) == list(b["gpyr_sha"])
    assert list(a["dog_sha"]) == list(b["dog_sha"])
    assert int(a["n"]) == int(b["n"]) == 12932
    assert len(b["libm_size_rows"]) == 14 and len(b["libm_desc_rows"]) == 140
    g = oracle.build_gaussian_pyramid(oracle.synth_image(0, 1080, 1920))
    d = oracle.build_dog_pyramid(g, 1080, 1920)
    oracle.set_threads(16)
    try:
        k0 = oracle.find_scale_space_extrema(g, d, 1080, 1920)
        e0 = oracle.calc_descriptors(g, 1080, 1920, k0)
        with oracle.libm_mode():
            k1 = oracle.find_scale_space_extrema(g, d, 1080, 1920)
            e1 = oracle.calc_descriptors(g, 1080, 1920, k1)
    finally:
        oracle.set_threads(1)
    assert sha(k0) == str(a["kp_sha"]) and sha(e0) == str(a["desc_sha"])
    nosize = k0.copy()
    nosize["size"] = 0
    assert sha(nosize) == str(b["kp_nosize_sha"])       # every keypoint field but `size` is the reference's
    if LIBM_MATCHES:
        assert str(b["libm"]) == LIBM
        assert sha(k1) == str(b["kp_sha"]) and sha(e1) == str(b["desc_sha"])
        assert_bits_equal(np.flatnonzero(k0["size"].view(np.uint32) != k1["size"].view(np.uint32)).astype(np.int32),
                          b["libm_size_rows"], "sizes that follow powf")
        # one ulp of powf(2, y) in [1, 2), times 1.6f, is up to 1.6 ulps of the product: two floats at most
        assert _ulps(k0["size"], k1["size"]).max() <= 2
        assert_bits_equal(np.flatnonzero((e0.view(np.uint32) != e1.view(np.uint32)).any(axis=1)).astype(np.int32),
                          b["libm_desc_rows"], "descriptor rows that follow cosf / sinf")
