"""GPU: the module entry points over the arguments they accept, against the CPU
oracle live and against the outputs recorded from the reference's own source
(tests/golden/ref_args_*.npz), byte for byte.  Inputs: tests/module_arg_inputs.py;
the oracle itself is pinned to the reference on the same inputs by
tests/test_module_args.py.

Covered values
  * Gaussian_Blur / Gaussian_Blur_1D: w = floor(3 sigma) in {0, 1, 4, 6, 8, 12, 15,
    18, 21, 36, 75, 300}: the LDS-tile kernels (w in {4, 8, 12, 18}) with
    coefficients other than the pyramid's, blur_generic_kernel wider than a tile
    and than the image, planes with rows - 1 == 0 or cols - 1 == 0; the sigma
    contract (0, negative, NaN, 100.5 refused, 100 accepted);
  * octave counts 6, 7, 8 through buildGaussianPyramid, buildDoGPyramid,
    findScaleSpaceExtrema, calDescriptor, SIFT_NCL after set_octaves(n) (384 x 416: 5 keypoints in the
    sixth octave, oi = 5 in the extrema and descriptor kernels) and one
    detect_compute_batch of three images, in exact mode, with SIFT_FLAG_FAST
    (planes against oracle.fast_pyramid) and with the scatter blur forced; counts
    the image or the context cannot hold;
  * degenerate images from 1 x 1 with one octave to 700 x 16 with five, with
    graph replay and with SIFT_FLAG_NO_GRAPH;
  * calDescriptor at firstOctave in {-2 .. 2} (octave bytes 254, 255, 0 .. 6,
    layers 0 .. 4), n = 0, n = 1, n above the context's initial keypoint
    capacity, and the rows the CV_Assert analogue refuses: oi = -1, oi = n_oct,
    layer 5, layer 255, alone and among valid rows.

Outside the reference's contract: caller keypoints with an angle outside
[0, 720].  The reference wraps the orientation bin once and then adds such a
keypoint's samples outside their histogram cell, by its memory layout.  The
library wraps the bin modulo 8 (include/sift_hip.h); the oracle states that in
oracle.circular_bins(), identical inside the contract, and
test_caller_keypoints (-30) and test_angles_outside_the_contract (1000, -1000,
-1, 765.5, 12345, -720.5 among valid rows) compare every byte with it.

Left to the oracle alone (test_module_args.py says why): Gaussian planes and
SIFT_NCL at an octave count other than 5 (the fixtures' `gpyr_sha` are then the
planes the reference's other functions were given), and the refused keypoints,
which the reference aborts on.
"""
import numpy as np
import pytest

import adversarial_inputs as A
import module_arg_inputs as M
from conftest import assert_bits_equal, kp_bytes, load_golden, sha
from reference_inputs import args_image_fixture, check_fixture_descriptors, expected_device_descriptors
from test_gpu_adversarial import _check, _check_batch, _run_batch

pytestmark = pytest.mark.gpu

FAST = 0x1
BLUR_CASES = M.blur_cases()
IMAGE_CASES = M.OCTAVE_CASES + M.DEGENERATE_CASES
_cache = {}


def _ref(oracle, case):
    """(img, Gaussian planes, DoG planes, keypoints, descriptors) of the oracle, computed once."""
    if case not in _cache:
        b, r, c, n = case
        img = oracle.synth_image(b, r, c)
        g = oracle.build_gaussian_pyramid(img, n)
        d = oracle.build_dog_pyramid(g, r, c, n)
        kps = oracle.find_scale_space_extrema(g, d, r, c, n)
        _cache[case] = (img, oracle.split_planes(g, r, c, n, 5), oracle.split_planes(d, r, c, n, 4), kps,
                        oracle.calc_descriptors(g, r, c, kps, n))
    return _cache[case]


def _caller_planes(oracle):
    if "caller" not in _cache:
        b, r, c = M.CALLER_IMAGE
        g = oracle.build_gaussian_pyramid(oracle.synth_image(b, r, c), M.CALLER_OCTAVES)
        _cache["caller"] = (r, c, g, oracle.split_planes(g, r, c, M.CALLER_OCTAVES, 5))
    return _cache["caller"]


def _planes_equal(got, ref, what):
    assert len(got) == len(ref), what
    for i, (p, q) in enumerate(zip(got, ref)):
        assert_bits_equal(p, q, f"{what} plane {i} {q.shape}")


@pytest.fixture(scope="module")
def fctx(siftgpu):
    c = siftgpu.Context(700, 1200, 3, device=0, flags=FAST)
    yield c
    c.close()


@pytest.fixture
def octaves():
    """set_octaves(n) on a shared context; 5 octaves and the context's own flags restored afterwards."""
    used = []

    def set_(ctx, n, flags=0):
        used.append((ctx, flags))
        ctx.set_octaves(n)
    yield set_
    for c, flags in used:
        c.set_flags(flags)
        c.set_octaves(5)


# ---- blurs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BLUR_CASES, ids=M.blur_id)
def test_blurs(ctx, oracle, case):
    r, c, sigma = case
    img = M.blur_image(r, c, sigma)
    g = load_golden("ref_args_blur")
    i = list(g["ids"]).index(M.blur_id(case))
    out = ctx.Gaussian_Blur(img, sigma)
    assert_bits_equal(out, oracle.gaussian_blur(img, sigma), "Gaussian_Blur")
    assert sha(out) == str(g["blur_sha"][i]), "Gaussian_Blur against the reference's recorded digest"
    out = ctx.Gaussian_Blur_1D(img, sigma)
    assert_bits_equal(out, oracle.gaussian_blur_1d(img, sigma), "Gaussian_Blur_1D")
    assert sha(out) == str(g["blur1d_sha"][i]), "Gaussian_Blur_1D against the reference's recorded digest"


def test_blur_w0_is_the_single_tap(ctx, oracle):
    img = M.blur_image(64, 96, 0.2)
    k = oracle.gaussian_kernel(0.2)
    assert k.shape == (1, 1)
    ref = (img * k[0, 0]) / np.float32(8192)
    ref[-1, :] = 0
    ref[:, -1] = 0
    assert_bits_equal(ctx.Gaussian_Blur(img, 0.2), ref + np.float32(0), "w = 0")
    assert not ctx.Gaussian_Blur_1D(img, 0.2).any(), "w = 0: the reference's asymmetric tap loop is empty"


def test_blur_one_pixel_planes_are_zero(ctx):
    for (r, c, s) in BLUR_CASES:
        if r == 1 or c == 1:
            img = M.blur_image(r, c, s)
            assert not ctx.Gaussian_Blur(img, s).any() and not ctx.Gaussian_Blur_1D(img, s).any(), (r, c, s)


def test_blur_sigma_contract(ctx, siftgpu, oracle):
    img = M.blur_image(8, 8, 100.0)
    for fn in (ctx.Gaussian_Blur, ctx.Gaussian_Blur_1D):
        for sigma in (0.0, -1.6, float("nan"), 100.5):
            with pytest.raises(siftgpu.SiftError) as e:
                fn(img, sigma)
            assert e.value.code == siftgpu.SIFT_E_INVALID, (fn.__name__, sigma)
    assert_bits_equal(ctx.Gaussian_Blur(img, 100.0), oracle.gaussian_blur(img, 100.0), "sigma 100")
    assert_bits_equal(ctx.Gaussian_Blur_1D(img, 100.0), oracle.gaussian_blur_1d(img, 100.0), "sigma 100, 1-D")
    ctx.sync()


# ---- octave counts 6 .. 8 and degenerate images: the module chain -------------------------------------
@pytest.mark.parametrize("case", IMAGE_CASES, ids=M.image_id)
def test_module_chain(ctx, oracle, case):
    b, r, c, n = case
    img, gr, dr, kr, er = _ref(oracle, case)
    g, k = args_image_fixture(M.image_id(case))
    gp = ctx.buildGaussianPyramid(img, n)
    _planes_equal(gp, gr, "Gaussian")
    # not independent evidence unless n == 5: for another count `gpyr_sha` are the oracle's planes, the ones
    # the reference's DoG / extrema / descriptor functions were given (`gpyr_from`, make_ref_golden.py)
    assert [sha(p) for p in gp] == list(g["gpyr_sha"]), f"Gaussian planes recorded from the {g['gpyr_from']}"
    dp = ctx.buildDoGPyramid(gp, n)
    _planes_equal(dp, dr, "DoG")
    assert [sha(p) for p in dp] == list(g["dog_sha"])
    kps = ctx.findScaleSpaceExtrema(gp, dp, n)
    _check(kps, None, kr, None, "findScaleSpaceExtrema")
    assert_bits_equal(kp_bytes(kps), k["kps"], "keypoints against the reference's recorded ones")
    desc = ctx.calDescriptor(gp, kr, 0)
    assert_bits_equal(desc, er, "calDescriptor")
    check_fixture_descriptors(desc, k, "descriptors against the reference's recorded ones")


@pytest.mark.parametrize("case", IMAGE_CASES, ids=M.image_id)
def test_sift_ncl(ctx, siftgpu, oracle, octaves, case):
    """SIFT_NCL after set_octaves(n): captured, replayed, and with SIFT_FLAG_NO_GRAPH."""
    b, r, c, n = case
    img, _, _, kr, er = _ref(oracle, case)
    _, k = args_image_fixture(M.image_id(case))
    octaves(ctx, n)
    _check(*ctx.SIFT_NCL(img), kr, er, "SIFT_NCL")
    kps, desc = ctx.SIFT_NCL(img)
    _check(kps, desc, kr, er, "SIFT_NCL, graph replay")
    assert_bits_equal(kp_bytes(kps), k["kps"], "keypoints against the reference's recorded ones")
    check_fixture_descriptors(desc, k, "descriptors against the reference's recorded ones")
    ctx.set_flags(siftgpu.SIFT_FLAG_NO_GRAPH)
    _check(*ctx.SIFT_NCL(img), kr, er, "SIFT_NCL, no graph")
    ctx.sync()


def test_batch_of_three(ctx, oracle, octaves):
    b, r, c, n = M.BATCH_CASE
    imgs = [oracle.synth_image(b + i, r, c) for i in range(3)]
    refs = [oracle.sift(im, n) for im in imgs]
    assert sum(len(k) for k, _ in refs) > 30
    octaves(ctx, n)
    _check_batch(_run_batch(ctx, imgs), refs, f"{n} octaves")


@pytest.mark.parametrize("case", IMAGE_CASES, ids=M.image_id)
def test_fast_mode(fctx, oracle, octaves, case):
    """SIFT_FLAG_FAST: every plane equals oracle.fast_pyramid(img, n) bit for bit, and a batch of three
    equals three single-image calls."""
    b, r, c, n = case
    img = oracle.synth_image(b, r, c)
    _planes_equal(fctx.buildGaussianPyramid(img, n), oracle.split_planes(oracle.fast_pyramid(img, n), r, c, n, 5),
                  "fast Gaussian")
    imgs = [img, oracle.synth_image(b + 50, r, c), img]
    octaves(fctx, n, FAST)
    refs = [fctx.SIFT_NCL(im) for im in imgs]
    assert refs[0][0].tobytes() == refs[2][0].tobytes() and refs[0][1].tobytes() == refs[2][1].tobytes()
    _check_batch(_run_batch(fctx, imgs), refs, "fast batch against single")


@pytest.mark.parametrize("case", M.SCATTER_CASES, ids=M.image_id)
def test_scatter_blur(siftgpu, oracle, monkeypatch, case):
    b, r, c, n = case
    img, gr, _, kr, er = _ref(oracle, case)
    monkeypatch.setenv("SIFT_HIP_SYM_MIN", "0")          # read at context creation
    monkeypatch.setenv("SIFT_HIP_SYM_ROWS_MIN", "0")
    with siftgpu.Context(r, c, 1, device=0) as sc:
        _planes_equal(sc.buildGaussianPyramid(img, n), gr, "scatter-blur Gaussian")
        sc.set_octaves(n)
        _check(*sc.SIFT_NCL(img), kr, er, "scatter-blur SIFT_NCL")


def test_octave_count_limits(ctx, siftgpu, oracle):
    img = oracle.synth_image(21, 64, 96)
    gp = ctx.buildGaussianPyramid(img, 7)
    assert [p.shape for p in gp[-5:]] == [(1, 1)] * 5
    for n in (8, 13):       # above the image's own limit (7), above kMaxOctaves
        out = np.empty(siftgpu.lib().sift_packed_size(64, 96, 7, 5) + 64, np.float32)
        rc = siftgpu.lib().sift_build_gaussian_pyramid(ctx.h, siftgpu._fp(img), 64, 96, n, siftgpu._fp(out))
        assert rc == siftgpu.SIFT_E_INVALID, n
    big = oracle.synth_image(23, 128, 192)
    out = np.empty(siftgpu.lib().sift_packed_size(128, 192, 8, 5), np.float32)
    rc = siftgpu.lib().sift_build_gaussian_pyramid(ctx.h, siftgpu._fp(big), 128, 192, 13, siftgpu._fp(out))
    assert rc == siftgpu.SIFT_E_INVALID
    with siftgpu.Context(64, 96, 1, device=0) as small:      # max_oct = 7
        for n in (8, 13):
            with pytest.raises(siftgpu.SiftError) as e:
                small.set_octaves(n)
            assert e.value.code == siftgpu.SIFT_E_INVALID
        small.set_octaves(7)
        # 8 octaves fit the image but not the context (an image can only have more octaves than the
        # context when it is larger than the context)
        rc = siftgpu.lib().sift_build_gaussian_pyramid(small.h, siftgpu._fp(big), 128, 192, 8, siftgpu._fp(out))
        assert rc == siftgpu.SIFT_E_SIZE
        img7, _, _, kr, er = _ref(oracle, M.OCTAVE_CASES[1])
        _check(*small.SIFT_NCL(img7), kr, er, "after the errors")
        small.sync()
    _planes_equal(ctx.buildGaussianPyramid(img, 7), gp, "after the errors")
    ctx.sync()


# ---- caller keypoints ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fo", M.FIRST_OCTAVES)
def test_caller_keypoints(ctx, oracle, fo):
    r, c, g, gpl = _caller_planes(oracle)
    kps = M.caller_keypoints(fo, oracle.KEYPOINT_DTYPE)
    fx = load_golden(f"ref_args_caller_fo{fo}")
    out = M.angle_outside_contract(kps)
    assert out.sum() == 10 and (kps["angle"][out] == -30).all()
    assert sha(kps[~out]) == str(fx["kp_sha"])
    desc = ctx.calDescriptor(gpl, kps, fo)
    ref = oracle.calc_descriptors(g, r, c, kps, M.CALLER_OCTAVES, fo)
    assert_bits_equal(desc[~out], ref[~out], f"firstOctave {fo}")
    assert_bits_equal(desc[~out], expected_device_descriptors(fx), f"firstOctave {fo} against the reference's recorded ones")
    # angle -30 is outside the reference's contract (M.angle_outside_contract): the library wraps the
    # orientation bin modulo 8 there (sift_hip.h), which oracle.circular_bins() states on the CPU
    with oracle.circular_bins():
        circ = oracle.calc_descriptors(g, r, c, kps, M.CALLER_OCTAVES, fo)
    assert_bits_equal(desc, circ, f"firstOctave {fo}, every row, bins modulo 8")
    assert_bits_equal(ctx.calDescriptor(gpl, kps[~out], fo), ref[~out], "the same rows without the others")
    one = ctx.calDescriptor(gpl, kps[33:34], fo)
    assert_bits_equal(one, ref[33:34], "n = 1")
    assert ctx.calDescriptor(gpl, kps[:0], fo).shape == (0, 128)


@pytest.mark.parametrize("fo", M.FIRST_OCTAVES)
def test_angles_outside_the_contract(ctx, oracle, fo):
    """Angles 1000, -1000, -1, -30, 765.5, 12345, -720.5 on every second row: where the reference's single
    wrap would leave the orientation bin at 9 .. 15 or below -1.  The call succeeds, those rows are the
    circular histogram's (oracle.circular_bins()), byte for byte, and the valid rows between them are the
    reference's, as they are in a call without the others and in the call after."""
    r, c, g, gpl = _caller_planes(oracle)
    kps = M.outside_contract_keypoints(fo, oracle.KEYPOINT_DTYPE)
    out = M.angle_outside_contract(kps)
    ref = oracle.calc_descriptors(g, r, c, kps[~out], M.CALLER_OCTAVES, fo)
    with oracle.circular_bins():
        circ = oracle.calc_descriptors(g, r, c, kps, M.CALLER_OCTAVES, fo)
    assert_bits_equal(circ[~out], ref, "the oracle's two statements agree inside the contract")
    assert circ[out].any(axis=1).sum() >= 10
    desc = ctx.calDescriptor(gpl, kps, fo)
    assert_bits_equal(desc[~out], ref, "valid rows among the others")
    assert_bits_equal(desc, circ, "every row, bins modulo 8")
    assert_bits_equal(ctx.calDescriptor(gpl, kps[~out], fo), ref, "the call after")
    ctx.sync()


def test_caller_keypoints_above_the_initial_capacity(siftgpu, oracle):
    r, c, g, gpl = _caller_planes(oracle)
    cap = A.default_candidate_capacity(r, c) * A.keypoints_per_candidate_slot()
    fo = -1
    kps = M.caller_keypoints(fo, oracle.KEYPOINT_DTYPE)
    kps = kps[~M.angle_outside_contract(kps)]
    octave = (kps["octave"] & 255).astype(np.int64)
    octave = np.where(octave < 128, octave, octave - 256)
    radius = np.array([M.descriptor_radius(s) for s in kps["size"] * 2.0 ** -octave])
    kps = kps[2 * radius + 1 <= M.MAX_WIN_ROWS]           # the cheap windows only
    n = cap + 77
    kps = np.tile(kps, n // len(kps) + 1)[:n].copy()
    kps["x"] += (np.arange(n) % 7).astype(np.float32) * np.float32(0.25)
    oracle.set_threads(16)
    try:
        ref = oracle.calc_descriptors(g, r, c, kps, M.CALLER_OCTAVES, fo)
    finally:
        oracle.set_threads(1)
    with siftgpu.Context(r, c, 1, device=0) as small:
        assert_bits_equal(small.calDescriptor(gpl, kps, fo), ref, f"{n} keypoints, initial capacity {cap}")
        assert_bits_equal(small.calDescriptor(gpl, kps[:5], fo), ref[:5], "and a small call after the growth")
        small.sync()


@pytest.mark.parametrize("fo", [-2, 0, 2])
def test_refused_keypoints(ctx, siftgpu, oracle, fo):
    """The CV_Assert analogue: each refused row alone and in the middle of valid rows returns
    SIFT_E_INVALID; the next valid call is correct and sync() reports nothing stale."""
    r, c, g, gpl = _caller_planes(oracle)
    good = M.caller_keypoints(fo, oracle.KEYPOINT_DTYPE)
    good = good[~M.angle_outside_contract(good)][:20]
    ref = oracle.calc_descriptors(g, r, c, good, M.CALLER_OCTAVES, fo)
    for name, bad in M.invalid_keypoints(fo, oracle.KEYPOINT_DTYPE):
        for rows in (bad, np.concatenate([good[:9], bad, good[9:]])):
            with pytest.raises(siftgpu.SiftError) as e:
                ctx.calDescriptor(gpl, rows, fo)
            assert e.value.code == siftgpu.SIFT_E_INVALID, (name, len(rows))
            assert_bits_equal(ctx.calDescriptor(gpl, good, fo), ref, f"after {name}")
            ctx.sync()
