"""GPU tests of the upsampled first octave (sift_set_upsample, sift_upsample2x,
sift_upsample2x_device).  The doubling kernel is compared bit for bit with the
numpy rule of tests/upsample_inputs.py; every detect / compute output is
compared byte for byte -- keypoint bytes, descriptor bits, offsets, nothing
written past the total -- with upsample_inputs.expected(): the CPU oracle on
the doubled image with OpenCV's half-scale post-pass.  SIFT_FLAG_FAST has no CPU
oracle of its own, so there the upsampled call is compared with the fast
pipeline run on the host-doubled image (GPU against GPU)."""
import numpy as np
import pytest

import detect_mask_inputs as M
import retain_best_inputs as R
import upsample_inputs as U
from conftest import assert_bits_equal, kp_bytes

pytestmark = pytest.mark.gpu

CAP = 2000
MAX_SHAPE = (2 * 157, 2 * 203)   # the largest doubled image here


@pytest.fixture(scope="module")
def uctx(siftgpu):
    """One context for the doubled shapes, batch 3; each test leaves the setting off."""
    c = siftgpu.Context(*MAX_SHAPE, 3, device=0)
    yield c
    c.close()


class Bufs:
    def __init__(self, batch, cap=CAP):
        import torch
        self.cap, self.batch = cap, batch
        self.k = torch.empty((cap, 7), dtype=torch.int32, device="cuda")
        self.d = torch.empty((cap, 128), dtype=torch.float32, device="cuda")
        self.o = torch.empty((batch + 1,), dtype=torch.int32, device="cuda")

    def clear(self):
        import torch
        self.k.fill_(-1)
        self.d.fill_(-1.0)
        self.o.fill_(-1)
        torch.cuda.synchronize()  # the fills ran on torch's stream, the call runs on the context's

    def host(self):
        return (self.o.cpu().numpy(), self.k.cpu().numpy().view(np.uint8).reshape(self.cap, 28), self.d.cpu().numpy())


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _enqueue(ctx, imgs_t, bufs, masks_t=None):
    B, R_, C_ = imgs_t.shape
    bufs.clear()
    kw = {} if masks_t is None else dict(masks_ptr=masks_t.data_ptr(), mask_row_stride=masks_t.shape[-1],
                                         mask_img_stride=R_ * masks_t.shape[-1] if masks_t.dim() == 3 else 0)
    ctx.detect_compute_batch(imgs_t.data_ptr(), B, R_, C_, C_, R_ * C_, bufs.k.data_ptr(), bufs.d.data_ptr(),
                             bufs.cap, bufs.o.data_ptr(), **kw)


def _run(ctx, imgs_t, bufs, masks_t=None):
    _enqueue(ctx, imgs_t, bufs, masks_t)
    ctx.sync()
    return bufs.host()


def _check(out, want, what):
    o, k, d = out
    assert o[0] == 0
    for b, (kr, dr) in enumerate(want):
        assert o[b + 1] - o[b] == len(kr), f"{what} image {b}: {o[b + 1] - o[b]} keypoints, expected {len(kr)}"
        assert_bits_equal(k[o[b]:o[b + 1]], kp_bytes(kr), f"{what} image {b} keypoints")
        assert_bits_equal(d[o[b]:o[b + 1]], dr, f"{what} image {b} descriptors")
    assert np.all(k[o[len(want)]:].view(np.int32) == -1), f"{what}: keypoint writes past the total"
    assert np.all(d[o[len(want)]:] == -1.0), f"{what}: descriptor writes past the total"


def _same(got, want, what):
    gk, gd = got
    assert len(gk) == len(want[0]), f"{what}: {len(gk)} keypoints, expected {len(want[0])}"
    assert_bits_equal(kp_bytes(gk), kp_bytes(want[0]), f"{what} keypoints")
    assert_bits_equal(gd, want[1], f"{what} descriptors")


def _values(shape, seed):
    """Negatives, large and small magnitudes, denormals and zeros."""
    r = np.random.default_rng(seed)
    v = (r.standard_normal(shape) * 100).astype(np.float32)
    flat = v.reshape(-1)
    n = flat.size
    flat[r.integers(0, n, max(1, n // 7))] = np.float32(2.0 ** -140) * r.integers(-9, 10, max(1, n // 7)).astype(np.float32)
    flat[r.integers(0, n, max(1, n // 11))] = np.float32(1.0) + np.float32(2.0 ** -23)
    return v


# ---- the doubling kernel -----------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (33, 65), (64, 63), (64, 64), (65, 129)])
def test_upsample2x_host(uctx, shape):
    img = _values(shape, 3)
    if img.size >= 100:
        assert (img < 0).any() and (np.abs(img[img != 0]) < np.float32(2.0 ** -126)).any()   # negatives, denormals
    got = uctx.upsample2x(img)
    assert got.shape == (2 * shape[0], 2 * shape[1])
    assert_bits_equal(got, U.upsample2x_ref(img), f"sift_upsample2x {shape}")


@pytest.mark.parametrize("pad_in,pad_out", [(5, 3), (0, 6)], ids=["unaligned_rows", "aligned_rows"])
def test_upsample2x_device_padded_batch(uctx, pad_in, pad_out):
    """Batch 3 with padded input and output strides: the pixels equal the rule, the output's row
    and image padding keeps its sentinel.  (33, 65): more than one strip of rows, a last 4-column
    group of 2; output rows of 133 floats take the scalar stores, rows of 136 the 16-byte ones."""
    import torch
    B, R_, C_ = 3, 33, 65
    rs, ors = C_ + pad_in, 2 * C_ + pad_out
    ims, oims = R_ * rs + 8, 2 * R_ * ors + 12
    assert (ors % 4 == 0 and oims % 4 == 0) == (pad_out == 6)
    imgs = [_values((R_, C_), 10 + b) for b in range(B)]
    src = np.full(B * ims, np.float32(12345.0), np.float32)
    for b in range(B):
        src[b * ims:b * ims + R_ * rs].reshape(R_, rs)[:, :C_] = imgs[b]
    sentinel = np.int32(-0x12345678)
    dst = torch.full((B * oims,), int(sentinel), dtype=torch.int32, device="cuda")
    src_t = _dev(src)
    uctx.upsample2x_device(src_t.data_ptr(), B, R_, C_, rs, ims, dst.data_ptr(), ors, oims)
    uctx.sync()
    out = dst.cpu().numpy()
    written = np.zeros(B * oims, bool)
    for b in range(B):
        blk = out[b * oims:b * oims + 2 * R_ * ors].reshape(2 * R_, ors)
        assert_bits_equal(blk[:, :2 * C_].view(np.float32), U.upsample2x_ref(imgs[b]), f"image {b}")
        written[b * oims:b * oims + 2 * R_ * ors].reshape(2 * R_, ors)[:, :2 * C_] = True
    assert np.all(out[~written] == sentinel), "padding bytes were written"


# ---- the upsampled SIFT_NCL, the host call ---------------------------------------------
@pytest.mark.parametrize("n_oct", U.OCTAVES)
@pytest.mark.parametrize("name", list(U.IMAGES))
def test_sift_ncl_upsampled(uctx, oracle, name, n_oct):
    img = U.image(name)
    want = U.expected(img, n_oct)
    assert ((want[0]["octave"] & 255) == 255).any()
    uctx.set_octaves(n_oct)
    try:
        for rep in range(2):   # the second call replays the captured sequence
            _same(uctx.SIFT_NCL_upsampled(img), want, f"{name}, {n_oct} octaves, call {rep}")
    finally:
        uctx.set_octaves(5)


def test_module_level_call(siftgpu, oracle):
    img = U.image("96x64")
    _same(siftgpu.SIFT_NCL_upsampled(img), U.expected(img, 5), "module SIFT_NCL_upsampled(image)")
    k, d = U.expected(img, 5)
    assert_bits_equal(siftgpu.compute(img, k, upsample=True), d, "module compute(image, keypoints, upsample=True)")
    _same(siftgpu.SIFT_NCL(img), oracle.sift(img), "module SIFT_NCL(image) afterwards")


# ---- a batch ------------------------------------------------------------------------------
def _batch():
    imgs = U.batch_images()
    return imgs, [U.expected(i, 5) for i in imgs]


def test_batch_graph_and_no_graph(siftgpu, uctx, oracle):
    imgs, want = _batch()
    imgs_t, bufs = _dev(np.stack(imgs)), Bufs(3)
    uctx.set_upsample(True)
    try:
        g0 = uctx.graph_stats()
        first = _run(uctx, imgs_t, bufs)
        _check(first, want, "captured")
        g1 = uctx.graph_stats()
        assert (g1[0] - g0[0], g1[2] - g0[2]) == (1, 1)
        _check(_run(uctx, imgs_t, bufs), want, "replayed")
        assert uctx.graph_stats() == g1
        uctx.set_flags(siftgpu.SIFT_FLAG_NO_GRAPH)
        _check(_run(uctx, imgs_t, bufs), want, "SIFT_FLAG_NO_GRAPH")
        assert uctx.graph_stats() == g1
    finally:
        uctx.set_flags(0)
        uctx.set_upsample(False)


def test_batch_capacity_below_the_total(siftgpu, uctx, oracle):
    imgs, want = _batch()
    total = sum(len(w[0]) for w in want)
    cap = total - 100
    imgs_t, bufs = _dev(np.stack(imgs)), Bufs(3, cap)
    uctx.set_upsample(True)
    try:
        _enqueue(uctx, imgs_t, bufs)
        with pytest.raises(siftgpu.SiftError) as e:
            uctx.sync()
        assert e.value.code == siftgpu.SIFT_E_CAPACITY
    finally:
        uctx.set_upsample(False)
    o, k, d = bufs.host()
    assert o.tolist() == np.concatenate([[0], np.cumsum([len(w[0]) for w in want])]).tolist()   # the true total
    assert_bits_equal(k, np.concatenate([kp_bytes(w[0]) for w in want])[:cap], "first kp_cap keypoints")
    assert_bits_equal(d, np.concatenate([w[1] for w in want])[:cap], "first kp_cap descriptors")


# ---- with the other detector options ---------------------------------------------------
def test_with_a_keypoint_budget(uctx, oracle):
    imgs, want = _batch()
    kept = [R.filter_keypoints(k, d, 20) for k, d in want]
    assert all(20 <= len(k[0]) < len(w[0]) for k, w in zip(kept, want))
    imgs_t, bufs = _dev(np.stack(imgs)), Bufs(3)
    uctx.set_upsample(True)
    uctx.set_max_features(20)
    try:
        _check(_run(uctx, imgs_t, bufs), kept, "set_max_features(20)")
        _same(uctx.SIFT_NCL(imgs[0]), kept[0], "the host call")
    finally:
        uctx.set_max_features(0)
        uctx.set_upsample(False)


def test_with_a_half_zero_mask_of_the_original_size(uctx, oracle):
    imgs, want = _batch()
    mask = M.half_plane(U.BATCH_SHAPE)
    assert mask.shape == imgs[0].shape
    kept = [M.filter_keypoints(k, d, mask) for k, d in want]
    assert all(0 < len(k[0]) < len(w[0]) for k, w in zip(kept, want))
    # some kept keypoint lies right of where the mask would end were it read at doubled coordinates
    assert any((k[0]["x"] >= U.BATCH_SHAPE[1] // 4).any() for k in kept)
    imgs_t, bufs = _dev(np.stack(imgs)), Bufs(3)
    uctx.set_upsample(True)
    try:
        _check(_run(uctx, imgs_t, bufs, _dev(mask)), kept, "one shared mask")
        _check(_run(uctx, imgs_t, bufs, _dev(np.stack([mask] * 3))), kept, "a mask per image")
        _same(uctx.SIFT_NCL(imgs[1], mask=mask), kept[1], "the host call")
    finally:
        uctx.set_upsample(False)


def test_compute_batch_on_the_emitted_keypoints(siftgpu, uctx, oracle):
    import torch
    imgs, want = _batch()
    imgs_t, bufs = _dev(np.stack(imgs)), Bufs(3)
    B, (R_, C_) = 3, U.BATCH_SHAPE
    d2 = torch.full((CAP, 128), -1.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def compute():
        uctx.compute_batch(imgs_t.data_ptr(), B, R_, C_, C_, R_ * C_, bufs.k.data_ptr(), bufs.o.data_ptr(), CAP,
                           d2.data_ptr(), 3)

    uctx.set_upsample(True)
    try:
        o, k, d = _run(uctx, imgs_t, bufs)
        _check((o, k, d), want, "detect")
        total = int(o[-1])
        assert (k.view(np.int32).reshape(-1, 7)[:total, 5] & 255 == 255).any()   # rows with octave -1
        compute()
        uctx.sync()   # no row is invalid
        got = d2.cpu().numpy()
        assert_bits_equal(got[:total], d[:total], "compute_batch on the upsampled call's keypoints")
        assert np.all(got[total:] == -1.0)
        # the host form, image 1
        assert_bits_equal(uctx.compute(imgs[1], want[1][0]), want[1][1], "compute(image, keypoints)")
    finally:
        uctx.set_upsample(False)
    # the setting off: a row with octave 255 is an invalid row, as before -- zeros and SIFT_E_INVALID
    compute()
    with pytest.raises(siftgpu.SiftError) as e:
        uctx.sync()
    assert e.value.code == siftgpu.SIFT_E_INVALID
    got = d2.cpu().numpy()
    kk = np.concatenate([w[0] for w in want])
    minus1 = (kk["octave"] & 255) == 255
    assert minus1.any() and not minus1.all()
    assert np.all(got[:total][minus1] == 0.0)
    assert np.all(np.any(got[:total][~minus1] != 0.0, axis=1))


def test_fast_mode_equals_the_fast_pipeline_on_the_doubled_image(siftgpu, oracle):
    img = U.image("128x160")
    big = U.upsample2x_ref(img)
    with siftgpu.Context(*big.shape, 1, device=0, flags=siftgpu.SIFT_FLAG_FAST) as ctx:
        bk, bd = ctx.SIFT_NCL(big)
        assert len(bk) > 100
        _same(ctx.SIFT_NCL_upsampled(img), (U.half_scale(bk), bd), "SIFT_FLAG_FAST")
        _same(ctx.SIFT_NCL(big), (bk, bd), "the doubled image again, the setting off")


def test_setting_off_after_on(siftgpu, oracle):
    """The plain result is the reference's again (the CPU oracle's, which the goldens record),
    and the two settings are two entries of the graph cache."""
    img = U.image("128x160")
    plain = oracle.sift(img)
    with siftgpu.Context(2 * img.shape[0], 2 * img.shape[1], 1, device=0) as ctx:
        s0 = ctx.graph_stats()
        _same(ctx.SIFT_NCL(img), plain, "before")
        s1 = ctx.graph_stats()
        ctx.set_upsample(True)
        _same(ctx.SIFT_NCL(img), U.expected(img, 5), "on")
        s2 = ctx.graph_stats()
        ctx.set_upsample(False)
        _same(ctx.SIFT_NCL(img), plain, "off again")
        s3 = ctx.graph_stats()
        ctx.set_upsample(True)
        _same(ctx.SIFT_NCL(img), U.expected(img, 5), "on again")
        s4 = ctx.graph_stats()
        ctx.set_upsample(False)
    assert (s1[0] - s0[0], s1[2] - s0[2]) == (1, 1)   # off: a new executable
    assert (s2[0] - s1[0], s2[2] - s1[2]) == (1, 1)   # on: a second entry, not an update of the first
    assert s3 == s2 and s4 == s2                      # both replayed from the cache


def test_errors(siftgpu, oracle):
    import ctypes
    img = U.image("96x64")
    fp = ctypes.POINTER(ctypes.c_float)
    n = ctypes.c_int(0)
    with siftgpu.Context(2 * 96 - 1, 2 * 64, 1, device=0) as ctx:   # one row short of the doubled shape
        k, d = ctx.SIFT_NCL(img)
        with pytest.raises(siftgpu.SiftError) as e:
            ctx.SIFT_NCL_upsampled(img)
        assert e.value.code == siftgpu.SIFT_E_SIZE
        with pytest.raises(siftgpu.SiftError) as e:
            ctx.compute(img, k, upsample=True)
        assert e.value.code == siftgpu.SIFT_E_SIZE
        _same(ctx.SIFT_NCL(img), (k, d), "after the errors")
        # the doubling alone is not bound by the context's limits
        assert_bits_equal(ctx.upsample2x(img), U.upsample2x_ref(img), "upsample2x")
        out = np.zeros((2, 2), np.float32)
        for rows, cols in ((0, 1), (1, 0), (-1, 4)):
            assert ctx._L.sift_upsample2x(ctx.h, img.ctypes.data_as(fp), rows, cols, 0,
                                          out.ctypes.data_as(fp)) == siftgpu.SIFT_E_INVALID
    L = siftgpu.lib()
    assert L.sift_set_upsample(None, 1) == siftgpu.SIFT_E_INVALID
    assert L.sift_upsample2x(None, img.ctypes.data_as(fp), 96, 64, 0, None) == siftgpu.SIFT_E_INVALID
    assert L.sift_detect_compute(None, img.ctypes.data_as(fp), 96, 64, 0, None, None, 0,
                                 ctypes.byref(n)) == siftgpu.SIFT_E_INVALID
