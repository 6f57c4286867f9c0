"""The segmented affine / similarity estimate on the GPU (-m gpu): every H
double, every found flag and every mask byte equals affine_oracle.py run per
segment, and the host sift_estimate_affine run per segment, bit for bit.  Inputs
and expected values are affine_inputs.py's (one call per model, computed once
per process); the outputs are sentinel-filled, so a write outside the segments'
range shows."""
import numpy as np
import pytest

from conftest import assert_bits_equal

import affine_inputs as I
import affine_oracle as AO
import homography_batch_inputs as HI

pytestmark = pytest.mark.gpu
H_SENT, F_SENT, M_SENT = -7.0, -77, 0xEE
MODEL_IDS = [I.NAMES[m] for m in I.MODELS]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _affine_device(ctx, src, dst, moff, m_cap, model, thr=3.0, max_iters=2000, confidence=0.99, with_mask=True,
                   extra=64):
    """Device form into sentinel-filled outputs: H [n_seg + 2, 9], found [n_seg + 2], mask [rows + extra]."""
    import torch
    rows = len(src)
    nseg = len(moff) - 1
    ds, dd, dmo = _dev(np.asarray(src, np.float32).reshape(-1, 2)), _dev(np.asarray(dst, np.float32).reshape(-1, 2)), \
        _dev(np.asarray(moff, np.int32))
    dH = torch.full((nseg + 2, 9), H_SENT, dtype=torch.float64, device="cuda")
    df = torch.full((nseg + 2,), F_SENT, dtype=torch.int32, device="cuda")
    dm = torch.full((rows + extra,), M_SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                  # the context's stream does not wait for torch's
    ctx.estimate_affine_segmented_device(ds.data_ptr(), dd.data_ptr(), dmo.data_ptr(), nseg, m_cap, model,
                                         dH.data_ptr(), df.data_ptr(), dm.data_ptr() if with_mask else None, thr,
                                         max_iters, confidence)
    ctx.sync()
    return dH.cpu().numpy(), df.cpu().numpy(), dm.cpu().numpy()


def _check(out, exp, moff, m_cap, what):
    """Segments equal the expected values; H / found rows past n_seg and mask bytes outside
    [clamp(moff[0]), clamp(moff[-1])) still hold their sentinels."""
    H, found, mask = out
    eH, ef, em = exp
    nseg = len(moff) - 1
    assert_bits_equal(found[:nseg], ef, what + " found")
    for b in range(nseg):
        assert H[b].tobytes() == eH[b].tobytes(), f"{what}: H of segment {b}: {H[b]} != {eH[b]}"
    lo, hi = (int(v) for v in np.clip([moff[0], moff[-1]], 0, m_cap))
    assert_bits_equal(mask[lo:hi], em[lo:hi], what + " mask")
    assert (H[nseg:] == H_SENT).all() and (found[nseg:] == F_SENT).all(), what + ": rows past n_segments written"
    dead = np.r_[0:lo, hi:len(mask)]
    assert (mask[dead] == M_SENT).all(), what + ": mask bytes outside the segments' range written"


def _host_per_segment(siftgpu, c):
    nseg = len(c.labels)
    H = np.zeros((nseg, 9), np.float64)
    found = np.zeros(nseg, np.int32)
    mask = np.zeros(c.m_cap, np.uint8)
    fn = siftgpu.estimateAffine2D if c.model == AO.AFFINE else siftgpu.estimateAffinePartial2D
    for b in range(nseg):
        lo, hi = c.bounds(b)
        A, m = fn(c.src[lo:hi], c.dst[lo:hi], c.thr, c.max_iters, c.confidence)
        H[b], found[b] = AO.as_h(None if A is None else A.reshape(6)), A is not None
        mask[lo:hi] = m
    return H, found, mask


@pytest.mark.parametrize("model", I.MODELS, ids=MODEL_IDS)
def test_gpu_bitexact_per_segment(ctx, siftgpu, model):
    """The one call of affine_inputs.gpu_call(model), with and without a mask buffer, against the
    oracle and the host path; then the host-buffer form against the device form."""
    c = I.gpu_call(model)
    eH, ef, em, _ = I.expected(model)
    out = _affine_device(ctx, c.src, c.dst, c.moff, c.m_cap, model, c.thr, c.max_iters, c.confidence)
    for b, label in enumerate(c.labels):
        print(f"{I.NAMES[model]} {label}: n={c.size(b)} found={out[1][b]} (oracle {ef[b]})")
    _check(out, (eH, ef, em), c.moff, c.m_cap, I.NAMES[model])
    _check(out, _host_per_segment(siftgpu, c), c.moff, c.m_cap, I.NAMES[model] + " against the host path")
    assert (out[2][c.m_cap:] == M_SENT).all()
    assert ef[c.index("nan") - 1] == ef[c.index("nan") + 1] == 1       # the poisoned segment's neighbours
    # without a mask buffer: the same H and found
    H2, f2, m2 = _affine_device(ctx, c.src, c.dst, c.moff, c.m_cap, model, c.thr, c.max_iters, c.confidence,
                                with_mask=False)
    assert H2.tobytes() == out[0].tobytes() and f2.tobytes() == out[1].tobytes() and (m2 == M_SENT).all()
    # the host-buffer form: rows up to m_cap
    res = ctx.estimateAffineBatch(c.src[:c.m_cap], c.dst[:c.m_cap], c.moff, model, c.thr, c.max_iters, c.confidence)
    assert len(res) == len(c.labels)
    for b, (A, m) in enumerate(res):
        lo, hi = c.bounds(b)
        assert (A is None) == (out[1][b] == 0), b
        if A is not None:
            assert A.tobytes() == out[0][b, :6].tobytes(), f"host form A of segment {b}"
        assert_bits_equal(m, out[2][lo:hi], f"host form mask of segment {b}")


@pytest.mark.parametrize("model", I.MODELS, ids=MODEL_IDS)
def test_gpu_invalid_parameters_give_none(ctx, model):
    c = I.gpu_call(model)
    n = len(c.labels)
    for max_iters, conf in ((0, 0.99), (2000, 0.0), (2000, 1.0), (-3, 0.5)):
        H, found, mask = _affine_device(ctx, c.src, c.dst, c.moff, c.m_cap, model, 3.0, max_iters, conf)
        assert (found[:n] == 0).all() and (H[:n] == 0).all() and (mask[:c.m_cap] == 0).all()
        assert (H[n:] == H_SENT).all() and (mask[c.m_cap:] == M_SENT).all()


def test_gpu_entry_point_rules(ctx, siftgpu):
    """With a live context: nothing to do returns SIFT_OK whatever the buffers;
    a null required buffer or an unknown model is SIFT_E_INVALID with a message."""
    L, h = siftgpu.lib(), ctx.h
    E = siftgpu.SIFT_E_INVALID
    t = _dev(np.zeros(64, np.float64))
    p = t.data_ptr()
    for model in I.MODELS:
        dev = lambda *a: L.sift_estimate_affine_segmented_device(h, *a[:5], model, 3.0, 2000, 0.99, *a[5:])  # noqa: E731
        assert dev(None, None, None, 0, 5, None, None, None) == 0
        assert dev(None, None, None, 3, 0, None, None, None) == 0
        assert L.sift_estimate_affine_segmented(h, None, None, None, 0, 0, model, 3.0, 2000, 0.99, None, None,
                                                None) == 0
        for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p),
                     (p, p, p, p, None)):
            s, d, o, H, f = args
            assert dev(s, d, o, 1, 4, H, f, None) == E
            assert b"null" in L.sift_last_error(h)
        assert dev(p, p, p, -1, 4, p, p, None) == E
    assert L.sift_estimate_affine_segmented_device(h, p, p, p, 1, 4, 2, 3.0, 2000, 0.99, p, p, None) == E
    assert b"model" in L.sift_last_error(h)


def test_gpu_similarity_feeds_the_warp_and_the_corner_transform(ctx, siftgpu):
    """d_H / d_found of a similarity estimate go straight into the warp and the
    corner transform on the same stream; the results equal those calls on the
    same nine doubles uploaded from the host, and the found = 0 segment warps to
    zeros."""
    import torch
    R, C = 48, 64
    ramp = (np.arange(R, dtype=np.float32)[:, None] * 2 + np.arange(C, dtype=np.float32)[None, :] * 3)
    ang = np.deg2rad(7.0)
    A = np.array([[np.cos(ang), -np.sin(ang), 5.5], [np.sin(ang), np.cos(ang), -3.25]])
    gy, gx = np.mgrid[4:R:8, 4:C:8]
    p = np.c_[gx.ravel(), gy.ravel()].astype(np.float32)
    src = np.concatenate([p, p[:1]])
    dst = np.concatenate([I.apply(A, p), p[:1]])
    moff = np.array([0, len(p), len(p) + 1], np.int32)          # segment 1: one pair, no model
    corners = np.array([[0, 0], [C, 0], [C, R], [0, R]], np.float32)
    ds, dd, dmo, dimg, dc = _dev(src), _dev(dst), _dev(moff), _dev(ramp), _dev(corners)

    def outputs():
        return (torch.full((2, R, C), -7.0, dtype=torch.float32, device="cuda"),
                torch.full((2, 4, 2), -5.0, dtype=torch.float32, device="cuda"))

    def warp_and_transform(H_t, f_t, w_t, c_t):
        ctx.warp_perspective_segmented_device(siftgpu.SIFT_PIXEL_F32, 1, dimg.data_ptr(), R, C, 0, 0, H_t.data_ptr(),
                                              f_t.data_ptr(), 2, 0, w_t.data_ptr(), R, C)
        ctx.perspective_transform_segmented_device(H_t.data_ptr(), f_t.data_ptr(), 2, dc.data_ptr(), 4,
                                                   c_t.data_ptr())

    dH = torch.full((2, 9), H_SENT, dtype=torch.float64, device="cuda")
    df = torch.full((2,), F_SENT, dtype=torch.int32, device="cuda")
    w1, c1 = outputs()
    torch.cuda.synchronize()
    ctx.estimate_affine_segmented_device(ds.data_ptr(), dd.data_ptr(), dmo.data_ptr(), 2, len(src),
                                         siftgpu.SIFT_MODEL_SIMILARITY, dH.data_ptr(), df.data_ptr())
    warp_and_transform(dH, df, w1, c1)
    ctx.sync()
    H, found = dH.cpu().numpy(), df.cpu().numpy()
    assert found.tolist() == [1, 0] and not H[1].any() and H[0, 6:].tolist() == [0.0, 0.0, 1.0]
    np.testing.assert_allclose(H[0, :6].reshape(2, 3), A, atol=1e-4)     # float32 destinations of an exact transform
    uH, uf = _dev(H), _dev(found)
    w2, c2 = outputs()
    torch.cuda.synchronize()
    warp_and_transform(uH, uf, w2, c2)
    ctx.sync()
    w1, c1, w2, c2 = (t.cpu().numpy() for t in (w1, c1, w2, c2))
    assert_bits_equal(w1, w2, "warp by the estimate's own d_H")
    assert_bits_equal(c1, c2, "corners by the estimate's own d_H")
    assert w1[0].any() and not w1[1].any() and not c1[1].any()
    np.testing.assert_allclose(c1[0], I.apply(A, corners), atol=1e-2)


def test_gpu_homography_unchanged_by_an_affine_call(ctx):
    """The bytes of sift_find_homography_segmented_device on one input of
    homography_batch_inputs.py are the same before and after affine calls (device
    and host form) on the same context: the shared scratch block is not
    corrupted."""
    import torch
    hc = HI.calls()[1]

    def homog():
        ds, dd, dmo = _dev(hc.src), _dev(hc.dst), _dev(hc.moff)
        n = len(hc.sizes)
        dH = torch.full((n, 9), H_SENT, dtype=torch.float64, device="cuda")
        df = torch.full((n,), F_SENT, dtype=torch.int32, device="cuda")
        dm = torch.full((len(hc.src),), M_SENT, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.find_homography_segmented_device(ds.data_ptr(), dd.data_ptr(), dmo.data_ptr(), n, len(hc.src),
                                             dH.data_ptr(), df.data_ptr(), dm.data_ptr(), hc.thr, hc.max_iters,
                                             hc.confidence)
        ctx.sync()
        return dH.cpu().numpy().tobytes(), df.cpu().numpy().tobytes(), dm.cpu().numpy().tobytes()

    before = homog()
    eH, ef, em, _ = HI.expected()[hc.name]
    assert before == (eH.tobytes(), ef.tobytes(), em.tobytes())
    for model in I.MODELS:
        c = I.gpu_call(model)
        _affine_device(ctx, c.src, c.dst, c.moff, c.m_cap, model, c.thr, c.max_iters, c.confidence)
        ctx.estimateAffineBatch(c.src[:c.m_cap], c.dst[:c.m_cap], c.moff, model, c.thr, c.max_iters, c.confidence)
    assert homog() == before
