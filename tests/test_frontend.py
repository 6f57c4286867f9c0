"""Image front end: readImage's conversion,
src/main.cpp:79-87 -- INTER_LINEAR resize of the 8-bit BGR image (scene:
960 x 960), COLOR_RGB2GRAY on BGR bytes, CV_32F.

CPU: the restatement oracle/frontend.py against the committed fixture
(book_bgr.npz -> book_gray.pgm, the gray conversion) and resize properties.
GPU (-m gpu): frontend.hip through the C ABI, bit-exact against the fixture
and the oracle (up- and down-scaling, odd sizes with a scalar row tail,
batched device API).  Resize parity against OpenCV itself is unpinned.

The vertical pass has two forms, switched at element `vtail` of an output row
(frontend.vertical_tail).  Output widths 1, 2 (3 and 6 elements: all scalar),
3, 5 (9 and 15: one 8-lane step), 6, 8 (18 and 24: the 16-lane loop only), 11
(33) and 21 (63: 16-lane loop and an 8-lane step) cover every class; the CPU
test test_vertical_forms_disagree_around_vtail shows for every noise case with
a source other than 1 x 1 that the two forms differ on each non-empty side of
`vtail`, so a kernel that used the wrong form there would fail (the older
5 x 3 -> 2 x 9 case is the exception, noted in the test).
Sources of 1 x 1, 1 x 40 and 40 x 1, 400 x 300 -> 3 x 4 and 3 x 4 -> 300 x 401,
all-0, all-255 and 0 / 255 checkerboard sources, and padded source strides on
the host entry point (a buffer of exactly the bytes the image owns) and on the
device entry point."""
import numpy as np
import pytest

from conftest import GOLDEN, assert_bits_equal, load_golden, read_pgm

import frontend as F


def _book_bgr():
    return load_golden("book_bgr")["bgr"]


def _book_gray():
    import os
    return read_pgm(os.path.join(GOLDEN, "book_gray.pgm"))


# ---- CPU ---------------------------------------------------------------------
def test_oracle_gray_matches_fixture():
    assert_bits_equal(F.rgb2gray_on_bgr(_book_bgr()), _book_gray(), "gray")
    assert F.read_image_gray(_book_bgr(), False).dtype == np.float32


def test_oracle_resize_properties():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (41, 67, 3), dtype=np.uint8)
    assert_bits_equal(F.resize_linear_u8(img, 41, 67), img, "identity")
    const = np.full((23, 31, 3), 201, np.uint8)
    assert (F.resize_linear_u8(const, 60, 17) == 201).all()
    # within one LSB of a float bilinear with the same pixel-centre mapping
    out = F.resize_linear_u8(img, 97, 29).astype(np.float64)
    ys = np.clip((np.arange(97) + 0.5) * 41 / 97 - 0.5, 0, 40)
    xs = np.clip((np.arange(29) + 0.5) * 67 / 29 - 0.5, 0, 66)
    y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
    y1, x1 = np.minimum(y0 + 1, 40), np.minimum(x0 + 1, 66)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    f = img.astype(np.float64)
    ref = (f[y0][:, x0] * (1 - fy) * (1 - fx) + f[y0][:, x1] * (1 - fy) * fx +
           f[y1][:, x0] * fy * (1 - fx) + f[y1][:, x1] * fy * fx)
    assert np.abs(out - ref).max() <= 1.01


WIDTHS = [1, 2, 3, 5, 6, 8, 11, 21]
OLD_NOISE_CASES = [((97, 131), (960, 960)), ((123, 77), (50, 31)), ((64, 64), (17, 200)), ((5, 3), (2, 9))]
NEW_NOISE_CASES = ([((37, 53), (61, w)) for w in WIDTHS] +
                   [((1, 1), (7, 5)), ((1, 40), (9, 21)), ((40, 1), (90, 5)), ((400, 300), (3, 4)),
                    ((3, 4), (300, 401))])


def _noise(shape, out):
    return np.random.default_rng(shape[0] * 7 + out[1]).integers(0, 256, shape + (3,), dtype=np.uint8)


def _case_id(v):
    return f"{v[0]}x{v[1]}"


def test_vertical_tail_classes():
    assert [F.vertical_tail(w) for w in WIDTHS] == [0, 0, 8, 8, 16, 16, 32, 56]
    assert [3 * w - F.vertical_tail(w) for w in WIDTHS] == [3, 6, 1, 7, 2, 8, 1, 7]


@pytest.mark.parametrize("shape,out", OLD_NOISE_CASES + NEW_NOISE_CASES, ids=_case_id)
def test_vertical_forms_disagree_around_vtail(shape, out):
    """Otherwise a bit-exact GPU result would not say which form the kernel used on that side."""
    simd, scal, vtail = F.vertical_forms(_noise(shape, out), *out)
    differ = (simd != scal).reshape(out[0], -1)
    below, above = int(differ[:, :vtail].sum()), int(differ[:, vtail:].sum())
    print(f"{shape} -> {out}: vtail {vtail} of {3 * out[1]}, forms differ on {below} elements below, {above} at or above")
    if shape == (1, 1):
        assert below == above == 0       # a constant image: both forms return the constant
        return
    if (shape, out) == ((5, 3), (2, 9)):
        # an older case whose 2 x 3 tail elements happen to agree: it cannot tell the forms apart at
        # or above vtail; widths 3 and 11 (the same class, one element past an 8-lane step) can
        assert below > 0 and above == 0
        return
    assert vtail == 0 or below > 0
    assert vtail == 3 * out[1] or above > 0


# ---- GPU ---------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_gray_matches_fixture(ctx):
    g = ctx.bgr8_to_gray(_book_bgr())
    assert_bits_equal(g, _book_gray().astype(np.float32), "gray")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,out", [((300, 210), (960, 960)), ((97, 131), (960, 960)),
                                       ((123, 77), (50, 31)), ((64, 64), (17, 200)), ((5, 3), (2, 9))])
def test_gpu_resize_gray_vs_oracle(ctx, shape, out):
    rng = np.random.default_rng(shape[0] * 7 + out[1])
    bgr = _book_bgr() if shape == (300, 210) else rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    g = ctx.bgr8_to_gray(bgr, *out)
    ref = F.rgb2gray_on_bgr(F.resize_linear_u8(bgr, *out)).astype(np.float32)
    assert_bits_equal(g, ref, f"{shape}->{out}")


@pytest.mark.gpu
def test_gpu_read_image_then_sift(siftgpu):
    """readImage(scene, resized=1) then SIFT_NCL: the GPU gray equals the oracle's
    and feeds the detector (src/main.cpp:19-23)."""
    _, gray = siftgpu.readImage(_book_bgr(), True)
    assert gray.shape == (960, 960)
    assert_bits_equal(gray, F.read_image_gray(_book_bgr(), True), "gray")
    kps, desc = siftgpu.SIFT_NCL(gray)
    assert len(kps) > 100 and desc.shape == (len(kps), 128)


@pytest.mark.gpu
def test_gpu_device_batch(siftgpu, ctx):
    import torch
    rng = np.random.default_rng(5)
    B, H, W, OH, OW = 3, 45, 70, 32, 100
    bgr = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    d_src = torch.from_numpy(bgr).cuda()
    d_out = torch.empty((B, OH, OW + 12), dtype=torch.float32, device="cuda")  # padded rows
    ctx.bgr8_to_gray_device(d_src.data_ptr(), B, H, W, W * 3, H * W * 3, OH, OW, d_out.data_ptr(),
                            (OW + 12) * 4, OH * (OW + 12) * 4)
    ctx.sync()
    out = d_out.cpu().numpy()[:, :, :OW]
    for b in range(B):
        ref = F.rgb2gray_on_bgr(F.resize_linear_u8(bgr[b], OH, OW)).astype(np.float32)
        assert_bits_equal(out[b], ref, f"image {b}")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,out", NEW_NOISE_CASES, ids=_case_id)
def test_gpu_resize_widths_and_degenerate_sources(ctx, shape, out):
    bgr = _noise(shape, out)
    ref = F.rgb2gray_on_bgr(F.resize_linear_u8(bgr, *out)).astype(np.float32)
    assert_bits_equal(ctx.bgr8_to_gray(bgr, *out), ref, f"{shape}->{out}")


def _checker(rows, cols):
    yy, xx = np.mgrid[0:rows, 0:cols]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["zeros", "full", "checker"])
def test_gpu_saturated_sources(ctx, name):
    src = {"zeros": np.zeros((37, 53, 3), np.uint8), "full": np.full((37, 53, 3), 255, np.uint8),
           "checker": _checker(37, 53)}[name]
    for out in [(37, 53), (61, 21), (61, 5), (20, 90), (3, 4)]:
        ref = F.rgb2gray_on_bgr(F.resize_linear_u8(src, *out)).astype(np.float32)
        assert_bits_equal(ctx.bgr8_to_gray(src, *out), ref, f"{name} -> {out}")
    if name == "full":
        assert (ref == 255).all()


@pytest.mark.gpu
@pytest.mark.parametrize("out", [(37, 53), (61, 21)], ids=_case_id)
def test_gpu_host_row_stride(ctx, siftgpu, out):
    """sift_bgr8_to_gray on a strided view (an ROI): a buffer of exactly (rows - 1) * row_stride + 3 * cols
    bytes, through the raw ABI and through Context.bgr8_to_gray(row_stride=...)."""
    import ctypes
    rows, cols = 37, 53
    stride = 3 * cols + 5
    bgr = _noise((rows, cols), out)
    owned = (rows - 1) * stride + 3 * cols
    buf = np.full(owned, 0xA5, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (rows, cols, 3), (stride, 3, 1))
    view[...] = bgr
    packed = ctx.bgr8_to_gray(bgr, *out)
    gray = np.full(out, -1, np.float32)
    rc = siftgpu.lib().sift_bgr8_to_gray(ctx.h, buf.ctypes.data, rows, cols, stride, out[0], out[1],
                                         gray.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    assert rc == siftgpu.SIFT_OK
    assert_bits_equal(gray, packed, "strided against packed")
    assert_bits_equal(gray, F.rgb2gray_on_bgr(F.resize_linear_u8(bgr, *out)).astype(np.float32), "strided")
    assert_bits_equal(ctx.bgr8_to_gray(view, *out, row_stride=stride), packed, "Context.bgr8_to_gray(row_stride)")
    rc = siftgpu.lib().sift_bgr8_to_gray(ctx.h, buf.ctypes.data, rows, cols, 3 * cols - 1, out[0], out[1],
                                         gray.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    assert rc == siftgpu.SIFT_E_INVALID
    assert_bits_equal(ctx.bgr8_to_gray(bgr, *out), packed, "after the error")
    ctx.sync()


@pytest.mark.gpu
@pytest.mark.parametrize("out", [(45, 70), (32, 100), (90, 7)], ids=_case_id)
def test_gpu_device_padded_source(ctx, out):
    """The device entry point with a padded source row_stride and img_stride (padding 0xFF), without
    and with resize."""
    import torch
    B, H, W = 2, 45, 70
    OH, OW = out
    rs, ist = 3 * W + 7, (3 * W + 7) * H + 11
    bgr = np.random.default_rng(17).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    host = np.full(B * ist, 0xFF, np.uint8)
    for b in range(B):
        np.lib.stride_tricks.as_strided(host[b * ist:], (H, W, 3), (rs, 3, 1))[...] = bgr[b]
    d_src = torch.from_numpy(host).cuda()
    d_out = torch.full((B, OH + 1, OW + 3), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()      # the fill runs on torch's stream, the kernel on the context's
    ctx.bgr8_to_gray_device(d_src.data_ptr(), B, H, W, rs, ist, OH, OW, d_out.data_ptr(), (OW + 3) * 4,
                            (OH + 1) * (OW + 3) * 4)
    ctx.sync()
    res = d_out.cpu().numpy()
    for b in range(B):
        ref = F.rgb2gray_on_bgr(F.resize_linear_u8(bgr[b], OH, OW)).astype(np.float32)
        assert_bits_equal(res[b, :OH, :OW], ref, f"image {b}")
    assert (res[:, OH, :] == -1).all() and (res[:, :, OW:] == -1).all(), "writes into the output padding"
