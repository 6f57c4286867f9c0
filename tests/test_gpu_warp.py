"""GPU tests of the perspective warp (sift_warp_perspective_segmented_device,
sift_warp_perspective, csrc/warp.hip): the kernel against the numpy restatement
of tests/warp_inputs.py over the shared case table, bit for bit, on packed,
padded and unaligned buffers whose padding must keep its sentinel bytes; the
inverse flag, a batch with an absent segment, one source for every H, the
homography stage feeding the warp in stream order, the front ends and the
argument errors.  (A NaN pixel, reached only from NaN or infinite samples, is
compared as "a NaN, here": warp_inputs.canonical.)"""
import ctypes

import numpy as np
import pytest

import warp_inputs as W
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
LAYOUTS = ("packed", "padded", "unaligned")


@pytest.fixture(scope="module")
def wctx(siftgpu):
    """The context's creation limits do not apply to the warp: 8 x 8 serves every shape here."""
    c = siftgpu.Context(8, 8, 1, device=0)
    yield c
    c.close()


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _layout(kind, cols, ocols, layout):
    """(source pitch, destination base offset, destination pitch) in bytes."""
    bpp = W.pixel_args(kind)[2]
    row, orow = cols * bpp, ocols * bpp
    if layout == "packed":
        return row, 0, orow
    if layout == "padded":      # rows on 16-byte boundaries: the wide stores, with padding after each row
        return row + 3 * bpp, 0, (orow + 15) // 16 * 16 + 16
    if kind == "f32":           # base and pitch multiples of 4 only
        return row + 4, 4, orow + 4
    return row + 5, 1, orow + (1 if orow % 2 == 0 else 2)   # an odd pitch from an odd base


def run_device(ctx, kind, srcs, Hs, found, inverse, out_shape, layout, shared_src=False):
    """srcs: one array per segment (or one in all with shared_src); Hs [n, 3, 3]; found: None or
    n ints.  Returns the n warped images; asserts that no byte outside their pixels was written."""
    import torch
    pixel, ch, bpp = W.pixel_args(kind)
    n = len(Hs)
    rows, cols = srcs[0].shape[:2]
    orows, ocols = out_shape
    spitch, doff, dpitch = _layout(kind, cols, ocols, layout)
    simg = 0 if shared_src else rows * spitch + (0 if layout == "packed" else 16)
    dimg = orows * dpitch + (0 if layout == "packed" else 32 if layout == "padded" else 4 if kind == "f32" else 7)
    src = np.full(max(simg, rows * spitch) * (1 if shared_src else n), 0x5A, np.uint8)
    for b, s in enumerate(srcs):
        blk = src[b * simg:b * simg + rows * spitch].reshape(rows, spitch)
        blk[:, :cols * bpp] = np.ascontiguousarray(s).view(np.uint8).reshape(rows, cols * bpp)
    dst = torch.full((doff + n * dimg + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    src_t, H_t = _dev(src), _dev(np.ascontiguousarray(Hs, np.float64).reshape(n, 9))
    found_t = None if found is None else _dev(np.asarray(found, np.int32))
    packed = layout == "packed"
    ctx.warp_perspective_segmented_device(
        pixel, ch, src_t.data_ptr(), rows, cols, 0 if packed else spitch, simg, H_t.data_ptr(),
        0 if found_t is None else found_t.data_ptr(), n, W_FLAG if inverse else 0, dst.data_ptr() + doff, orows, ocols,
        0 if packed else dpitch, 0 if packed and n == 1 else dimg)
    ctx.sync()
    out = dst.cpu().numpy()
    written = np.zeros(out.size, bool)
    imgs = []
    for b in range(n):
        at = doff + b * dimg
        blk = out[at:at + orows * dpitch].reshape(orows, dpitch)[:, :ocols * bpp]
        written[at:at + orows * dpitch].reshape(orows, dpitch)[:, :ocols * bpp] = True
        img = np.ascontiguousarray(blk)
        imgs.append(img.view(np.float32).reshape(orows, ocols) if kind == "f32" else
                    img.reshape((orows, ocols) + ((3,) if ch == 3 else ())))
    assert np.all(out[~written] == SENTINEL), f"{layout}: bytes outside the destination pixels were written"
    return imgs


W_FLAG = 0x1   # SIFT_WARP_INVERSE_MAP


def _same(got, want, what):
    assert_bits_equal(W.canonical(got), W.canonical(want), what)


# ---- the case table -------------------------------------------------------------------------
@pytest.mark.parametrize("case", W.CASES, ids=[c["name"] for c in W.CASES])
def test_case_table(wctx, case):
    want = W.expected(case)
    for layout in LAYOUTS:
        # d_found: NULL (all found) on the packed layout, the array otherwise; found = 0 always the array
        found = None if case["found"] and layout == "packed" else [case["found"]]
        got, = run_device(wctx, case["kind"], [case["src"]], [case["H"]], found, case["inverse"], case["out_shape"],
                          layout)
        _same(got, want, f"{case['name']} ({layout})")


@pytest.mark.parametrize("kind", W.PIXELS)
@pytest.mark.parametrize("name", ["rotation_30", "projective", "scale_0.5", "shift_x-1"])
def test_inverse_flag(wctx, kind, name):
    """warp(H) equals warp(inverse_rule(H), SIFT_WARP_INVERSE_MAP) byte for byte."""
    src = W.pixels(kind, (67, 131), 5)
    H = W.homographies(67, 131, 70, 259)[name][0]
    a, = run_device(wctx, kind, [src], [H], None, False, (70, 259), "packed")
    b, = run_device(wctx, kind, [src], [W.inverse_rule(H)], None, True, (70, 259), "packed")
    assert a.view(np.uint8).any()
    assert_bits_equal(a, b, f"{kind} {name}")
    _same(a, W.warp_ref(src, H, (70, 259)), f"{kind} {name} against the rule")


# ---- a batch ----------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", W.PIXELS)
def test_batch_of_three_with_an_absent_segment(wctx, kind, layout):
    hs = W.homographies(67, 131, 70, 259)
    Hs = [hs["rotation_30"][0], hs["projective"][0], hs["shift_5/32_-11/32"][0]]
    srcs = [W.pixels(kind, (67, 131), 20 + b) for b in range(3)]
    got = run_device(wctx, kind, srcs, Hs, [1, 0, 1], False, (70, 259), layout)
    for b in range(3):
        _same(got[b], W.warp_ref(srcs[b], Hs[b], (70, 259), found=[1, 0, 1][b]), f"image {b}")
    assert not got[1].view(np.uint8).any() and got[0].view(np.uint8).any() and got[2].view(np.uint8).any()
    # img_stride = 0: one source image warped by every H
    got = run_device(wctx, kind, srcs[:1], Hs, [1, 0, 1], False, (70, 259), layout, shared_src=True)
    for b in range(3):
        _same(got[b], W.warp_ref(srcs[0], Hs[b], (70, 259), found=[1, 0, 1][b]), f"shared source, H {b}")


# ---- stream order -----------------------------------------------------------------------------
def test_homography_stage_feeds_the_warp_in_stream_order(wctx):
    """Crafted point pairs through sift_find_homography_segmented_device, then the warp on the same
    stream with no synchronisation in between; checked against the rule applied with the H and
    found copied back afterwards.  Segment 1 has three pairs: no model, zeros."""
    import torch
    true_H = [np.array([[0.98, 0.05, 3.0], [-0.04, 1.02, -2.0], [1e-4, -5e-5, 1.0]]),
              np.eye(3),
              np.array([[1.0, 0.0, 7.25], [0.0, 1.0, -3.5], [0.0, 0.0, 1.0]])]
    r = np.random.default_rng(9)
    counts = [40, 3, 25]
    src_xy, dst_xy = [], []
    for H, n in zip(true_H, counts):
        p = (r.random((n, 2)) * [130, 66]).astype(np.float32)
        q = np.c_[p.astype(np.float64), np.ones(n)] @ H.T
        src_xy.append(p)
        dst_xy.append((q[:, :2] / q[:, 2:]).astype(np.float32))
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    s_t, d_t, o_t = _dev(np.concatenate(src_xy)), _dev(np.concatenate(dst_xy)), _dev(offs)
    H_t = torch.full((3, 9), 7.0, dtype=torch.float64, device="cuda")
    f_t = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    imgs = np.stack([W.pixels("f32", (67, 131), 30 + b) for b in range(3)])
    img_t = _dev(imgs)
    out_t = torch.full((3, 70, 259), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    wctx.find_homography_segmented_device(s_t.data_ptr(), d_t.data_ptr(), o_t.data_ptr(), 3, int(offs[-1]),
                                          H_t.data_ptr(), f_t.data_ptr())
    wctx.warp_perspective_segmented_device(0, 1, img_t.data_ptr(), 67, 131, 0, 67 * 131 * 4, H_t.data_ptr(),
                                           f_t.data_ptr(), 3, 0, out_t.data_ptr(), 70, 259, 0, 0)
    wctx.sync()
    H, found, out = H_t.cpu().numpy(), f_t.cpu().numpy(), out_t.cpu().numpy()
    assert found.tolist() == [1, 0, 1] and not H[1].any()
    for b in range(3):
        _same(out[b], W.warp_ref(imgs[b], H[b].reshape(3, 3), (70, 259), found=int(found[b])), f"pair {b}")
    assert out[0].any() and not out[1].any() and out[2].any()


# ---- the front ends ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", W.PIXELS)
def test_host_call_and_python_front_ends(siftgpu, wctx, kind):
    src = W.pixels(kind, (17, 31), 6)
    hs = W.homographies(17, 31, 31, 17)
    for name in ("rotation_30", "projective"):
        H = hs[name][0]
        want = W.warp_ref(src, H, (31, 17))
        got = wctx.warpPerspective(src, H, (17, 31))          # dsize = (width, height)
        assert got.dtype == src.dtype and got.shape == want.shape
        _same(got, want, f"Context.warpPerspective {name}")
        _same(siftgpu.warpPerspective(src, H, (17, 31)), want, f"module warpPerspective {name}")
        _same(siftgpu.warpPerspective(src, W.inverse_rule(H), (17, 31), flags=siftgpu.WARP_INVERSE_MAP | 1), want,
              f"module warpPerspective {name}, WARP_INVERSE_MAP")
        _same(wctx.warpPerspective(src, W.inverse_rule(H), (17, 31), inverse=True), want, f"inverse=True {name}")


def test_host_call_reads_a_strided_view_and_zeroes_dst_for_an_absent_segment(siftgpu, wctx):
    L = siftgpu.lib()
    big = W.pixels("f32", (20, 40), 8)
    view = big[2:19, 5:36]                                    # 17 x 31, rows 160 bytes apart, ends inside the buffer
    H = np.ascontiguousarray(W.homographies(17, 31, 31, 17)["projective"][0])
    out = np.full((31, 17), 9.0, np.float32)
    dp = ctypes.POINTER(ctypes.c_double)
    rc = L.sift_warp_perspective(wctx.h, 0, 1, view.ctypes.data, 17, 31, 160, H.ctypes.data_as(dp), 0,
                                 out.ctypes.data, 31, 17)
    assert rc == siftgpu.SIFT_OK
    _same(out, W.warp_ref(np.ascontiguousarray(view), H, (31, 17)), "strided source view")
    for name in ("singular", "nan_entry", "overflowing_inverse"):
        bad = np.ascontiguousarray(W.homographies(17, 31, 31, 17)[name][0])
        out[:] = 9.0
        rc = L.sift_warp_perspective(wctx.h, 0, 1, view.ctypes.data, 17, 31, 160, bad.ctypes.data_as(dp), 0,
                                     out.ctypes.data, 31, 17)
        assert rc == siftgpu.SIFT_E_INVALID and not out.any(), name
        with pytest.raises(siftgpu.SiftError) as e:
            wctx.warpPerspective(np.ascontiguousarray(view), bad, (17, 31))
        assert e.value.code == siftgpu.SIFT_E_INVALID


def test_errors_and_the_profile_stage(siftgpu):
    import torch
    L = siftgpu.lib()
    INV, SIZE = siftgpu.SIFT_E_INVALID, siftgpu.SIFT_E_SIZE
    src = _dev(np.zeros((4, 8), np.float32))
    dst = torch.full((4 * 8 * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    H = _dev(np.eye(3).reshape(1, 9))
    torch.cuda.synchronize()
    with siftgpu.Context(8, 8, 1, device=0, flags=siftgpu.SIFT_FLAG_PROFILE) as ctx:
        def call(pixel=0, ch=1, s=src.data_ptr(), rows=4, cols=8, rs=0, ims=0, h=H.data_ptr(), n=1, flags=0,
                 d=dst.data_ptr(), orows=4, ocols=8, ors=0, oims=0):
            vp = ctypes.c_void_p
            return L.sift_warp_perspective_segmented_device(ctx.h, pixel, ch, vp(s), rows, cols, rs, ims, vp(h), None,
                                                            n, flags, vp(d), orows, ocols, ors, oims)
        for kw in (dict(s=None), dict(h=None), dict(d=None), dict(rows=0), dict(cols=-1), dict(orows=0),
                   dict(ocols=0), dict(pixel=2), dict(pixel=0, ch=3), dict(pixel=1, ch=2), dict(pixel=1, ch=4),
                   dict(n=-1), dict(flags=2), dict(rs=31), dict(rs=34), dict(ors=28), dict(ors=33),
                   dict(n=2, oims=100), dict(n=2, ims=100), dict(n=2, oims=130)):
            assert call(**kw) == INV, kw
        for kw in (dict(rows=(1 << 30) + 1), dict(cols=(1 << 30) + 1), dict(orows=(1 << 30) + 1),
                   dict(ocols=(1 << 30) + 1)):
            assert call(**kw) == SIZE, kw
        ctx.sync()
        ctx.stage_stats()
        assert call(n=0) == siftgpu.SIFT_OK and call(n=0, s=None, d=None, h=None) == siftgpu.SIFT_OK
        ctx.sync()
        assert "warp" not in ctx.stage_stats() and (dst.cpu().numpy() == SENTINEL).all()   # nothing enqueued
        assert call() == siftgpu.SIFT_OK
        ctx.sync()
        st = ctx.stage_stats()
        assert st["warp"]["launches"] == 1 and st["warp"]["bytes"] == 8.0 * 4 * 8
        assert not dst.cpu().numpy().any()      # the identity of a zero image, every pixel written
        # the host form's own checks
        a, o = np.zeros((4, 8), np.float32), np.zeros((4, 8), np.float32)
        Hh = np.eye(3)
        dp = ctypes.POINTER(ctypes.c_double)
        for rows, cols, rs in ((0, 8, 0), (4, 0, 0), (4, 8, 31), (4, 8, 34)):
            assert L.sift_warp_perspective(ctx.h, 0, 1, a.ctypes.data, rows, cols, rs, Hh.ctypes.data_as(dp), 0,
                                           o.ctypes.data, 4, 8) == INV
        assert L.sift_warp_perspective(ctx.h, 0, 1, a.ctypes.data, 4, 8, 0, Hh.ctypes.data_as(dp), 0, None, 4, 8) == INV
        assert L.sift_warp_perspective(ctx.h, 1, 3, a.ctypes.data, 4, 8, 23, Hh.ctypes.data_as(dp), 0,
                                       o.ctypes.data, 1, 1) == INV
