"""GPU tests on the crafted inputs of tests/adversarial_inputs.py, on strided and
misaligned input layouts, and at octave counts 1-3.  Everything is compared
bit for bit with the CPU oracle (no tolerance, nothing sampled);
tests/test_adversarial_inputs.py asserts on the oracle alone which branches the
crafted inputs reach.

* crafted pyramids through findScaleSpaceExtrema / calDescriptor: every
  refinement rejection, singular Hessians, ties, up to 9 orientation peaks per
  extremum, zero-norm descriptors;
* the internal keypoint buffer regrow (more than 2 keypoints per candidate slot);
* crafted images (fractional, 0..65535, signed, stars, constant) through the
  one-image kernels, the batch kernels with empty images first / between /
  last, direct launches, and the module chain against the fused path;
* row strides cols + k, image strides with a remainder, a base pointer aligned
  to 4 bytes only, NaN in all padding -- exact and SIFT_FLAG_FAST;
* octave counts 1, 2, 3.
"""
import ctypes

import numpy as np
import pytest

import adversarial_inputs as A
from conftest import assert_bits_equal, kp_bytes

pytestmark = pytest.mark.gpu

FAST = 0x1
STRIDE_PADS = (1, 3, 13, 32)      # row_stride = cols + k
IMG_REMAINDERS = (0, 5)           # img_stride = rows * row_stride + j
_cache = {}


def _ref_image(oracle, fam, shape):
    """(image, oracle keypoints, oracle descriptors), computed once per module run."""
    key = ("img", fam, shape)
    if key not in _cache:
        img = A.IMAGE_FAMILIES[fam](*shape) if fam in A.IMAGE_FAMILIES else oracle.synth_image(int(fam), *shape)
        _cache[key] = (img,) + oracle.sift(img)
    return _cache[key]


def _ref_pyramid(oracle, fam, shape):
    """(packed g, packed d, plane lists, oracle keypoints, oracle descriptors)."""
    key = ("pyr", fam, shape)
    if key not in _cache:
        r, c = shape
        g, d = A.PYRAMID_FAMILIES[fam](r, c)
        kps = oracle.find_scale_space_extrema(g, d, r, c)
        _cache[key] = (g, d, oracle.split_planes(g, r, c, 5, 5), oracle.split_planes(d, r, c, 5, 4), kps,
                       oracle.calc_descriptors(g, r, c, kps))
    return _cache[key]


def _check(kps, desc, kr, dr, what):
    assert len(kps) == len(kr), f"{what}: {len(kps)} keypoints, the CPU path has {len(kr)}"
    assert_bits_equal(kp_bytes(kps), kp_bytes(kr), f"{what} keypoints")
    if desc is not None:
        assert_bits_equal(desc, dr, f"{what} descriptors")


def _run_batch(ctx, imgs, row_stride=None, img_stride=None, lead=0):
    """One sift_detect_compute_batch call on host images laid out on the device
    with the given strides (elements), `lead` floats after the allocation's
    start, every other float of the buffer NaN; outputs pre-filled with -1.
    Returns (offsets, keypoint bytes [cap, 28], descriptors [cap, 128], cap)."""
    import torch
    B = len(imgs)
    R, C = imgs[0].shape
    rs = row_stride or C
    ist = img_stride or R * rs
    assert rs >= C and ist >= R * rs
    buf = torch.full((lead + B * ist + rs + 64,), float("nan"), dtype=torch.float32, device="cuda")
    for b, im in enumerate(imgs):
        s = lead + b * ist
        buf[s:s + R * rs].view(R, rs)[:, :C] = torch.from_numpy(np.ascontiguousarray(im, np.float32)).cuda()
    return _run_batch_on(ctx, buf, B, R, C, rs, ist, lead)


def _run_batch_on(ctx, buf, B, R, C, rs, ist, lead, cap=20000):
    import torch
    kpts = torch.full((cap, 7), -1, dtype=torch.int32, device="cuda")
    desc = torch.full((cap, 128), -1.0, dtype=torch.float32, device="cuda")
    offs = torch.full((B + 1,), -1, dtype=torch.int32, device="cuda")
    ctx.detect_compute_batch(buf.data_ptr() + 4 * lead, B, R, C, rs, ist, kpts.data_ptr(), desc.data_ptr(), cap,
                             offs.data_ptr())
    ctx.sync()
    return offs.cpu().numpy(), kpts.cpu().numpy().view(np.uint8).reshape(cap, 28), desc.cpu().numpy(), cap


def _check_batch(out, refs, what):
    """Every image against its (keypoints, descriptors) reference; the total;
    nothing written past the total."""
    o, k, d, cap = out
    B = len(refs)
    assert o[0] == 0
    for b, (kr, dr) in enumerate(refs):
        assert o[b + 1] - o[b] == len(kr), f"{what} image {b}: {o[b + 1] - o[b]} keypoints, expected {len(kr)}"
        assert_bits_equal(k[o[b]:o[b + 1]], kp_bytes(kr), f"{what} image {b} keypoints")
        assert_bits_equal(d[o[b]:o[b + 1]], dr, f"{what} image {b} descriptors")
    assert o[B] == sum(len(kr) for kr, _ in refs) <= cap
    assert np.all(k[o[B]:].view(np.int32) == -1), f"{what}: keypoint writes past the total"
    assert np.all(d[o[B]:] == -1.0), f"{what}: descriptor writes past the total"


# ---- a. crafted pyramids ----------------------------------------------------------
@pytest.mark.parametrize("shape", A.PYRAMID_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fam", list(A.PYRAMID_FAMILIES))
def test_crafted_pyramid_extrema_and_descriptors(ctx, oracle, fam, shape):
    g, d, gpl, dpl, kr, dr = _ref_pyramid(oracle, fam, shape)
    kps = ctx.findScaleSpaceExtrema(gpl, dpl, 5)
    _check(kps, None, kr, None, f"{fam} {shape}")
    assert_bits_equal(ctx.calDescriptor(gpl, kr, 0), dr, f"{fam} {shape} descriptors")


@pytest.mark.parametrize("shape", A.PYRAMID_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_zero_norm_descriptors(ctx, oracle, shape):
    """Caller keypoints on flat Gaussian planes: every gradient is 0, the
    descriptor norm is below FLT_EPSILON (src/sift.cpp:702-712), and the CPU
    path emits finite zeros -- so must the GPU (no NaN from 0 / 0)."""
    r, c = shape
    g, _, gpl, _, kr_flat, _ = _ref_pyramid(oracle, "flat", shape)
    assert len(kr_flat) == 0
    kps = _ref_pyramid(oracle, "white", shape)[4]       # keypoints of every octave, layer and angle
    ref = oracle.calc_descriptors(g, r, c, kps)
    assert len(kps) > 1000 and not ref.any() and np.isfinite(ref).all()
    assert_bits_equal(ctx.calDescriptor(gpl, kps, 0), ref, "zero-norm descriptors")


# ---- b. internal keypoint buffer regrow ---------------------------------------------
def test_keypoint_buffer_regrow(siftgpu, oracle):
    """More than 2 keypoints per candidate slot on a fresh context: the first
    findScaleSpaceExtrema call grows the internal buffer and runs again; a
    second call, a later SIFT_NCL (reallocated buffers, dropped graphs) and
    the raw two-call sizing all return the CPU path's list."""
    r, c = A.REGROW_SHAPE
    g, d = A.regrow_pyramid()
    gpl, dpl = oracle.split_planes(g, r, c, 5, 5), oracle.split_planes(d, r, c, 5, 4)
    kr = oracle.find_scale_space_extrema(g, d, r, c)
    assert len(kr) > A.keypoints_per_candidate_slot() * A.default_candidate_capacity(r, c)
    img, ki, di = _ref_image(oracle, "1", (240, 320))
    with siftgpu.Context(r, c, 1, device=0) as ctx:
        _check(ctx.SIFT_NCL(img)[0], None, ki, None, "synth before the regrow")   # a graph is cached
        _check(ctx.findScaleSpaceExtrema(gpl, dpl, 5), None, kr, None, "first call (grows, runs again)")
        _check(ctx.findScaleSpaceExtrema(gpl, dpl, 5), None, kr, None, "second call")
        _check(*ctx.SIFT_NCL(img), ki, di, "synth after the regrow")
    # the two-call sizing through the raw ABI, the regrow inside the first call
    L = siftgpu.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    with siftgpu.Context(r, c, 1, device=0) as ctx:
        n = ctypes.c_int(0)
        rc = L.sift_find_scale_space_extrema(ctx.h, g.ctypes.data_as(fp), d.ctypes.data_as(fp), r, c, 5, None, 0,
                                             ctypes.byref(n))
        assert rc == siftgpu.SIFT_E_CAPACITY and n.value == len(kr)
        out = np.zeros(n.value, siftgpu.KEYPOINT_DTYPE)
        m = ctypes.c_int(0)
        assert L.sift_copy_results(ctx.h, out.ctypes.data, None, n.value, ctypes.byref(m)) == siftgpu.SIFT_OK
        assert m.value == len(kr)
        _check(out, None, kr, None, "two-call sizing")


# ---- c. crafted images ------------------------------------------------------------
@pytest.mark.parametrize("shape", A.IMAGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fam", list(A.IMAGE_FAMILIES))
def test_crafted_image_one_image_kernels(siftgpu, oracle, fam, shape):
    img, kr, dr = _ref_image(oracle, fam, shape)
    with siftgpu.Context(*shape, 1, device=0) as ctx:
        _check(*ctx.SIFT_NCL(img), kr, dr, f"{fam} {shape}")


@pytest.mark.parametrize("no_graph", [False, True], ids=["graph", "direct"])
@pytest.mark.parametrize("shape", A.IMAGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_with_empty_images(siftgpu, oracle, shape, no_graph):
    """B = 5: constant, noise, constant, stars, constant -- empty images first,
    between dense ones and last; twice (the second call replays the graph)."""
    refs = [_ref_image(oracle, f, shape) for f in A.BATCH_ORDER]
    assert [len(kr) == 0 for _, kr, _ in refs] == [True, False, True, False, True]
    with siftgpu.Context(*shape, 5, device=0) as ctx:
        if no_graph:
            ctx.set_flags(siftgpu.SIFT_FLAG_NO_GRAPH)
        for rep in range(2):
            out = _run_batch(ctx, [im for im, _, _ in refs])
            o = out[0]
            for b in (0, 2, 4):
                assert o[b + 1] == o[b], f"empty image {b}: offsets {o.tolist()}"
            _check_batch(out, [(kr, dr) for _, kr, dr in refs], f"{shape} call {rep}")


@pytest.mark.parametrize("fam", ["fractional", "u16_range", "signed"])
@pytest.mark.parametrize("shape", A.IMAGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_of_non_integer_images(siftgpu, oracle, shape, fam):
    """The batch kernels on non-integer / out-of-range pixels (B = 2, the image
    and its vertical flip)."""
    img, kr, dr = _ref_image(oracle, fam, shape)
    flip = np.ascontiguousarray(img[::-1])
    kf, df = oracle.sift(flip)
    with siftgpu.Context(*shape, 2, device=0) as ctx:
        _check_batch(_run_batch(ctx, [img, flip]), [(kr, dr), (kf, df)], f"{fam} {shape}")


@pytest.mark.parametrize("shape", A.IMAGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fam", ["fractional", "signed"])
def test_module_chain_equals_fused_path(ctx, oracle, fam, shape):
    """buildGaussianPyramid -> buildDoGPyramid -> findScaleSpaceExtrema ->
    calDescriptor equals SIFT_NCL: the stored DoG planes against the DoG the
    fused extrema pass forms on the fly, on non-integer data."""
    img, kr, dr = _ref_image(oracle, fam, shape)
    gp = ctx.buildGaussianPyramid(img, 5)
    dp = ctx.buildDoGPyramid(gp, 5)
    g = oracle.build_gaussian_pyramid(img)
    for i, (p, q) in enumerate(zip(gp, oracle.split_planes(g, *shape, 5, 5))):
        assert_bits_equal(p, q, f"{fam} gaussian plane {i}")
    for i, (p, q) in enumerate(zip(dp, oracle.split_planes(oracle.build_dog_pyramid(g, *shape), *shape, 5, 4))):
        assert_bits_equal(p, q, f"{fam} dog plane {i}")
    kps = ctx.findScaleSpaceExtrema(gp, dp, 5)
    _check(kps, ctx.calDescriptor(gp, kps, 0), kr, dr, f"{fam} module chain")
    _check(*ctx.SIFT_NCL(img), kr, dr, f"{fam} fused")


# ---- d. strides, exact mode ---------------------------------------------------------
STRIDE_IMAGES = ["21", "fractional", "stars"]    # a synth image, fractional noise, the stars


@pytest.mark.parametrize("shape", A.IMAGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_row_stride(siftgpu, oracle, shape):
    """sift_detect_compute on a view of a wider NaN-filled host array, and
    row_stride_bytes = 0 (the documented default, cols * 4)."""
    R, C = shape
    img, kr, dr = _ref_image(oracle, "21", shape)
    assert len(kr) > 50
    with siftgpu.Context(R, C, 1, device=0) as ctx:
        for k in STRIDE_PADS:
            wide = np.full((R, C + k), np.nan, np.float32)
            wide[:, :C] = img
            _check(*ctx.SIFT_NCL(wide[:, :C], row_stride_bytes=(C + k) * 4), kr, dr, f"row stride cols + {k}")
        _check(*ctx.SIFT_NCL(img, row_stride_bytes=0), kr, dr, "row_stride_bytes = 0")


@pytest.mark.parametrize("flags", [0, FAST], ids=["exact", "fast"])
@pytest.mark.parametrize("shape", A.IMAGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_device_strides_and_alignment(siftgpu, oracle, shape, flags):
    """sift_detect_compute_batch, B = 3, row_stride = cols + k, img_stride =
    rows * row_stride + j, the base pointer 4 bytes past a device allocation
    and NaN in every float that is no pixel.  Exact mode: every image equals
    the CPU path.  SIFT_FLAG_FAST: every image equals the fast single-image
    path on the contiguous copy (test_fast_pyramid_equals_its_oracle pins
    that one to its own oracle)."""
    R, C = shape
    imgs = [_ref_image(oracle, f, shape)[0] for f in STRIDE_IMAGES]
    with siftgpu.Context(R, C, 3, device=0, flags=flags) as ctx:
        if flags & FAST:
            refs = [ctx.SIFT_NCL(im) for im in imgs]
        else:
            refs = [_ref_image(oracle, f, shape)[1:] for f in STRIDE_IMAGES]
        assert min(len(kr) for kr, _ in refs) > 20
        _check_batch(_run_batch(ctx, imgs), refs, "contiguous")
        for k in STRIDE_PADS:
            for j in IMG_REMAINDERS:
                rs = C + k
                out = _run_batch(ctx, imgs, row_stride=rs, img_stride=R * rs + j, lead=1)
                _check_batch(out, refs, f"row_stride cols + {k}, img_stride + {j}, base + 4 bytes")


def test_graph_cache_keys_on_strides(siftgpu, oracle):
    """Two consecutive calls on the same buffers with different strides (the
    images rewritten in between), then the first layout again: each result is
    the CPU path's, because the strides are part of the graph key."""
    import torch
    R, C = 203, 157
    fams = ["21", "stars"]
    refs = [_ref_image(oracle, f, (R, C))[1:] for f in fams]
    imgs = [torch.from_numpy(_ref_image(oracle, f, (R, C))[0]).cuda() for f in fams]
    layouts = [(C + 3, R * (C + 3) + 5), (C + 32, R * (C + 32)), (C + 3, R * (C + 3) + 5)]
    with siftgpu.Context(R, C, 2, device=0) as ctx:
        buf = torch.empty((8 + 2 * max(i for _, i in layouts) + 256,), dtype=torch.float32, device="cuda")
        caps0 = ctx.graph_stats()[0]
        for rs, ist in layouts:
            buf.fill_(float("nan"))
            for b, im in enumerate(imgs):
                buf[1 + b * ist:1 + b * ist + R * rs].view(R, rs)[:, :C] = im
            _check_batch(_run_batch_on(ctx, buf, 2, R, C, rs, ist, 1), refs, f"strides {rs}, {ist}")
        assert ctx.graph_stats()[0] - caps0 >= 2      # two shapes: at least two captures


@pytest.mark.parametrize("shape", [(203, 157), (48, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_synth_images_strided(siftgpu, oracle, shape):
    """sift_synth_images with row_stride > cols and img_stride > rows *
    row_stride: the pixels are oracle.synth_image's, the padding is untouched."""
    import torch
    R, C = shape
    B, rs = 3, C + 13
    ist = R * rs + 5
    with siftgpu.Context(R, C, B, device=0) as ctx:
        buf = torch.full((1 + B * ist + 7,), -3.0, dtype=torch.float32, device="cuda")
        ctx.synth_images(buf.data_ptr() + 4, B, R, C, rs, ist, seed_base=90)
        ctx.sync()
        h = buf.cpu().numpy()
    pixel = np.zeros(h.shape, bool)
    for b in range(B):
        v = h[1 + b * ist:1 + b * ist + R * rs].reshape(R, rs)
        assert_bits_equal(v[:, :C], oracle.synth_image(90 + b, R, C), f"image {b}")
        pixel[1 + b * ist:1 + b * ist + R * rs].reshape(R, rs)[:, :C] = True
    assert np.all(h[~pixel] == -3.0), "sift_synth_images wrote into the padding"


# ---- f. octave counts ----------------------------------------------------------------
@pytest.mark.parametrize("n_oct", [1, 2, 3])
def test_octave_counts(siftgpu, oracle, n_oct):
    """set_octaves(n): SIFT_NCL and a B = 2 batch equal oracle.sift(img, n),
    which is the octave prefix of the 5-octave result."""
    shape = (300, 420)
    img, k5, d5 = _ref_image(oracle, "8", shape)
    img2, k25, d25 = _ref_image(oracle, "9", shape)
    kr, dr = oracle.sift(img, n_oct)
    keep = (k5["octave"] & 255) < n_oct
    _check(kr, dr, k5[keep], d5[keep], "the oracle's own prefix property")
    keep2 = (k25["octave"] & 255) < n_oct
    with siftgpu.Context(*shape, 2, device=0) as ctx:
        ctx.set_octaves(n_oct)
        try:
            _check(*ctx.SIFT_NCL(img), kr, dr, f"{n_oct} octaves")
            _check_batch(_run_batch(ctx, [img, img2]), [(kr, dr), (k25[keep2], d25[keep2])], f"{n_oct} octaves batch")
        finally:
            ctx.set_octaves(5)
        _check(*ctx.SIFT_NCL(img), k5, d5, "5 octaves restored")


def test_module_entry_points_three_octaves(ctx, oracle):
    """buildGaussianPyramid / buildDoGPyramid / findScaleSpaceExtrema /
    calDescriptor with nOctaves = 3."""
    shape = (300, 420)
    img = _ref_image(oracle, "8", shape)[0]
    g = oracle.build_gaussian_pyramid(img, 3)
    d = oracle.build_dog_pyramid(g, *shape, 3)
    gp = ctx.buildGaussianPyramid(img, 3)
    assert len(gp) == 15
    for i, (p, q) in enumerate(zip(gp, oracle.split_planes(g, *shape, 3, 5))):
        assert_bits_equal(p, q, f"gaussian plane {i}")
    dp = ctx.buildDoGPyramid(gp, 3)
    assert len(dp) == 12
    for i, (p, q) in enumerate(zip(dp, oracle.split_planes(d, *shape, 3, 4))):
        assert_bits_equal(p, q, f"dog plane {i}")
    kr = oracle.find_scale_space_extrema(g, d, *shape, 3)
    assert len(kr) > 100
    _check(ctx.findScaleSpaceExtrema(gp, dp, 3), None, kr, None, "3 octaves")
    assert_bits_equal(ctx.calDescriptor(gp, kr, 0), oracle.calc_descriptors(g, *shape, kr, 3), "3-octave descriptors")
