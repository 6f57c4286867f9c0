"""The segmented homography on the GPU (-m gpu): every H double, every found
flag and every mask byte equals oracle/homography.py run per segment, and the
host sift_find_homography run per segment, bit for bit.  Inputs and expected
values are homography_batch_inputs.py's (computed once per process); the
outputs are sentinel-filled, so a write outside the segments' range shows."""
import ctypes
import functools

import numpy as np
import pytest

from conftest import assert_bits_equal, book_image

import homography as HO
import homography_batch_inputs as I
import match as M

pytestmark = pytest.mark.gpu
H_SENT, F_SENT, M_SENT = -7.0, -77, 0xEE
CORNERS = np.array([[0, 0], [640, 0], [640, 480], [0, 480]], np.float32)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _homog_device(ctx, src, dst, moff, m_cap=None, thr=3.0, max_iters=2000, confidence=0.995, with_mask=True,
                  extra=64):
    """Device form into sentinel-filled outputs: H [n_seg + 2, 9], found [n_seg + 2], mask [rows + extra]."""
    import torch
    rows = len(src)
    m_cap = rows if m_cap is None else m_cap
    nseg = len(moff) - 1
    ds, dd, dmo = _dev(np.asarray(src, np.float32).reshape(-1, 2)), _dev(np.asarray(dst, np.float32).reshape(-1, 2)), \
        _dev(np.asarray(moff, np.int32))
    dH = torch.full((nseg + 2, 9), H_SENT, dtype=torch.float64, device="cuda")
    df = torch.full((nseg + 2,), F_SENT, dtype=torch.int32, device="cuda")
    dm = torch.full((rows + extra,), M_SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                  # the context's stream does not wait for torch's
    ctx.find_homography_segmented_device(ds.data_ptr() if rows else 0, dd.data_ptr() if rows else 0, dmo.data_ptr(),
                                         nseg, m_cap, dH.data_ptr(), df.data_ptr(),
                                         dm.data_ptr() if with_mask else None, thr, max_iters, confidence)
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


def _host_per_segment(siftgpu, src, dst, moff, m_cap, thr, max_iters, confidence):
    o = np.clip(np.asarray(moff, np.int64), 0, m_cap)
    H = np.zeros((len(o) - 1, 9), np.float64)
    found = np.zeros(len(o) - 1, np.int32)
    mask = np.zeros(m_cap, np.uint8)
    for b in range(len(o) - 1):
        lo, hi = int(o[b]), int(max(o[b], o[b + 1]))
        h, m = siftgpu.findHomography(src[lo:hi], dst[lo:hi], siftgpu.RANSAC, thr, None, max_iters, confidence)
        if h is not None:
            H[b], found[b] = h.reshape(9), 1
            mask[lo:hi] = m
    return H, found, mask


@pytest.mark.parametrize("which", [0, 1, 2], ids=["main", "capped", "none"])
def test_gpu_bitexact_per_segment(ctx, siftgpu, which):
    c = I.calls()[which]
    eH, ef, em, _ = I.expected()[c.name]
    out = _homog_device(ctx, c.src, c.dst, c.moff, None, c.thr, c.max_iters, c.confidence)
    for b, label in enumerate(c.labels):
        print(f"{c.name} {label}: n={c.sizes[b]} found={out[1][b]} (oracle {ef[b]})")
    _check(out, (eH, ef, em), c.moff, len(c.src), c.name)
    _check(out, _host_per_segment(siftgpu, c.src, c.dst, c.moff, len(c.src), c.thr, c.max_iters, c.confidence),
           c.moff, len(c.src), c.name + " against the host path")
    # without a mask buffer: the same H and found
    H2, f2, m2 = _homog_device(ctx, c.src, c.dst, c.moff, None, c.thr, c.max_iters, c.confidence, with_mask=False)
    assert H2.tobytes() == out[0].tobytes() and f2.tobytes() == out[1].tobytes() and (m2 == M_SENT).all()


@functools.lru_cache(maxsize=None)
def _small_sets():
    """Eight distinct 5- to 40-pair sets and their oracle results, reused by the many-segment cases."""
    sets = []
    for k, (n, f, nz) in enumerate([(5, 0.0, 0.2), (9, 0.1, 0.3), (17, 0.2, 0.0), (23, 0.1, 0.5), (31, 0.2, 0.4),
                                    (40, 0.15, 0.3), (12, 0.0, 0.0), (6, 0.0, 0.1)]):
        s, d = I.data(50 + k, n, f, nz)
        sets.append((s, d, HO.find_homography(s, d)))
    return sets


def _many(nseg):
    """nseg segments drawn round-robin from _small_sets(), with empty segments first, between and last."""
    sets = _small_sets()
    src, dst, sizes, eH, ef, em = [], [], [], [], [], []
    for b in range(nseg):
        if b in (0, nseg // 2, nseg - 1) and nseg > 2:
            sizes.append(0)
            eH.append(np.zeros(9))
            ef.append(0)
            continue
        s, d, (h, m) = sets[b % len(sets)]
        src.append(s)
        dst.append(d)
        sizes.append(len(s))
        eH.append(np.zeros(9) if h is None else np.array(h, np.float64))
        ef.append(0 if h is None else 1)
        em.append(m)
    moff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return np.concatenate(src), np.concatenate(dst), moff, (np.array(eH), np.array(ef, np.int32), np.concatenate(em))


@pytest.mark.parametrize("nseg", [1, 63, 300])
def test_gpu_segment_counts(ctx, nseg):
    if nseg == 1:
        c = I.calls()[0]
        b = c.index("n300")
        lo, hi = int(c.moff[b]), int(c.moff[b + 1])
        eH, ef, em, _ = I.expected()["MAIN"]
        src, dst, moff = c.src[lo:hi], c.dst[lo:hi], np.array([0, hi - lo], np.int32)
        exp = (eH[b:b + 1], ef[b:b + 1], em[lo:hi])
    else:
        src, dst, moff, exp = _many(nseg)
        assert moff[1] == 0 and moff[-1] == moff[-2] and (np.diff(moff) <= 40).all()
    _check(_homog_device(ctx, src, dst, moff), exp, moff, len(src), f"{nseg} segments")


def test_gpu_clamps(ctx):
    """m_offsets[n] above m_cap: the straddling segment is estimated from its
    in-range rows only, the segment wholly past m_cap gives none, and no mask
    byte at or past m_cap is written."""
    c = I.calls()[0]
    parts = [c.index("set10"), c.index("set12"), c.index("five")]
    src = np.concatenate([c.src[c.moff[b]:c.moff[b + 1]] for b in parts])
    dst = np.concatenate([c.dst[c.moff[b]:c.moff[b + 1]] for b in parts])
    moff = np.concatenate([[0], np.cumsum([c.sizes[b] for b in parts])]).astype(np.int32)
    m_cap = int(moff[1]) + 17
    assert moff[1] < m_cap < moff[2] and moff[-1] > m_cap
    exp = I.expect_segments(src, dst, moff, m_cap, 3.0, 2000, 0.995)
    assert exp[1].tolist() == [1, 1, 0]
    out = _homog_device(ctx, src, dst, moff, m_cap=m_cap)
    _check(out, exp, moff, m_cap, "m_cap clamp")
    assert (out[2][m_cap:] == M_SENT).all()
    # a first offset above 0: the rows before it are untouched too
    moff2 = moff.copy()
    moff2[0] = 7
    exp2 = I.expect_segments(src, dst, moff2, m_cap, 3.0, 2000, 0.995)
    _check(_homog_device(ctx, src, dst, moff2, m_cap=m_cap), exp2, moff2, m_cap, "moff[0] > 0")


def test_gpu_invalid_parameters_give_none(ctx):
    c = I.calls()[1]
    for max_iters, conf in ((0, 0.995), (2000, 0.0), (2000, 1.0), (-3, 0.5)):
        H, found, mask = _homog_device(ctx, c.src, c.dst, c.moff, None, 3.0, max_iters, conf)
        n = len(c.sizes)
        assert (found[:n] == 0).all() and (H[:n] == 0).all() and (mask[:len(c.src)] == 0).all()
        assert (H[n:] == H_SENT).all() and (mask[len(c.src):] == M_SENT).all()


def test_gpu_entry_point_rules(ctx, siftgpu):
    """With a live context: nothing to do returns SIFT_OK whatever the buffers;
    a null required buffer is SIFT_E_INVALID with a message."""
    L, h = siftgpu.lib(), ctx.h
    assert L.sift_find_homography_segmented_device(h, None, None, None, 0, 5, 3.0, 2000, 0.995, None, None, None) == 0
    assert L.sift_find_homography_segmented_device(h, None, None, None, 3, 0, 3.0, 2000, 0.995, None, None, None) == 0
    assert L.sift_find_homography_segmented(h, None, None, None, 0, 0, 3.0, 2000, 0.995, None, None, None) == 0
    assert L.sift_perspective_transform_segmented_device(h, None, None, 0, None, 4, None) == 0
    assert L.sift_perspective_transform_segmented_device(h, None, None, 2, None, 0, None) == 0
    E = siftgpu.SIFT_E_INVALID
    t = _dev(np.zeros(64, np.float64))
    p = t.data_ptr()
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        s, d, o, H, f = args
        assert L.sift_find_homography_segmented_device(h, s, d, o, 1, 4, 3.0, 2000, 0.995, H, f, None) == E
        assert b"null" in L.sift_last_error(h)
    assert L.sift_perspective_transform_segmented_device(h, p, p, 1, None, 4, p) == E
    assert L.sift_find_homography_segmented_device(h, p, p, p, -1, 4, 3.0, 2000, 0.995, p, p, None) == E


def _transform_device(ctx, H, found, pts):
    import torch
    dH, df, dp = _dev(np.asarray(H, np.float64)), _dev(np.asarray(found, np.int32)), _dev(pts)
    out = torch.full((len(found) + 1, len(pts), 2), -5.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.perspective_transform_segmented_device(dH.data_ptr(), df.data_ptr(), len(found), dp.data_ptr(), len(pts),
                                               out.data_ptr())
    ctx.sync()
    return out.cpu().numpy()


def test_gpu_forms_and_determinism(ctx):
    c = I.calls()[0]
    eH, ef, em, _ = I.expected()["MAIN"]
    a = _homog_device(ctx, c.src, c.dst, c.moff)
    b = _homog_device(ctx, c.src, c.dst, c.moff)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), "two calls differ"
    res = ctx.findHomographyBatch(c.src, c.dst, c.moff)
    assert len(res) == len(c.sizes)
    for i, (H, m) in enumerate(res):
        lo, hi = int(c.moff[i]), int(c.moff[i + 1])
        assert (H is None) == (a[1][i] == 0), i
        if H is not None:
            assert H.reshape(9).tobytes() == a[0][i].tobytes(), f"host form H of segment {i}"
        assert_bits_equal(m, a[2][lo:hi], f"host form mask of segment {i}")
    # the segmented transform, a found == 0 segment included
    out = _transform_device(ctx, a[0][:len(ef)], a[1][:len(ef)], CORNERS)
    assert 0 in ef and 1 in ef
    for i in range(len(ef)):
        ref = HO.perspective_transform(list(eH[i]), CORNERS) if ef[i] else np.zeros_like(CORNERS)
        assert_bits_equal(out[i], ref, f"corners of segment {i}")
    assert (out[len(ef)] == -5.0).all()


CROPS = [(0, 0), (7, 11), (3, 5)]   # (dy, dx) of the book_image() crops: frame b against frame b + 1


def test_gpu_flow_in_stream_order(ctx, siftgpu):
    """detect_compute_batch -> segmented kNN -> ratio with keypoints -> segmented
    homography -> segmented transform of the crop's corners, enqueued with no
    host read in between; one sync, then download.  H equals the host
    sift_find_homography on the downloaded pairs bit for bit, and the corners
    land within 1 px of the crops' relative shifts."""
    import torch
    img = book_image()
    R, C = img.shape[0] - 16, img.shape[1] - 16
    B = len(CROPS)
    imgs = torch.from_numpy(np.stack([img[dy:dy + R, dx:dx + C] for dy, dx in CROPS])).contiguous().cuda()
    cap = 1024
    kpts = torch.zeros((cap, 7), dtype=torch.int32, device="cuda")
    desc = torch.zeros((cap, 128), dtype=torch.float32, device="cuda")
    offs = torch.zeros((B + 1,), dtype=torch.int32, device="cuda")
    idx = torch.full((cap, 2), -77, dtype=torch.int32, device="cuda")
    dist = torch.full((cap, 2), -5.0, dtype=torch.float32, device="cuda")
    mt = torch.full((cap, 4), -77, dtype=torch.int32, device="cuda")
    src = torch.full((cap, 2), -5.0, dtype=torch.float32, device="cuda")
    dst = torch.full((cap, 2), -5.0, dtype=torch.float32, device="cuda")
    moff = torch.zeros((B,), dtype=torch.int32, device="cuda")
    dH = torch.full((B - 1, 9), H_SENT, dtype=torch.float64, device="cuda")
    df = torch.full((B - 1,), F_SENT, dtype=torch.int32, device="cuda")
    dm = torch.full((cap,), M_SENT, dtype=torch.uint8, device="cuda")
    corners = np.array([[0, 0], [C, 0], [C, R], [0, R]], np.float32)
    dc = _dev(corners)
    dout = torch.full((B - 1, 4, 2), -5.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def match_and_estimate():
        ctx.knn_match_segmented_device(desc.data_ptr(), offs.data_ptr(), B - 1, cap, desc.data_ptr(),
                                       offs.data_ptr() + 4, cap, 2, idx.data_ptr(), dist.data_ptr())
        ctx.ratio_matches_device(idx.data_ptr(), dist.data_ptr(), offs.data_ptr(), B - 1, cap, M.RATIO,
                                 kpts.data_ptr(), kpts.data_ptr(), offs.data_ptr() + 4, mt.data_ptr(),
                                 src.data_ptr(), dst.data_ptr(), cap, moff.data_ptr())
        ctx.find_homography_segmented_device(src.data_ptr(), dst.data_ptr(), moff.data_ptr(), B - 1, cap,
                                             dH.data_ptr(), df.data_ptr(), dm.data_ptr())
        ctx.perspective_transform_segmented_device(dH.data_ptr(), df.data_ptr(), B - 1, dc.data_ptr(), 4,
                                                   dout.data_ptr())

    match_and_estimate()      # on empty offsets: grows every stage's scratch, so the run below enqueues without a wait
    ctx.sync()
    dm.fill_(M_SENT)
    torch.cuda.synchronize()
    ctx.detect_compute_batch(imgs.data_ptr(), B, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                             offs.data_ptr())
    match_and_estimate()
    ctx.sync()
    mo = moff.cpu().numpy()
    s, d = src.cpu().numpy(), dst.cpu().numpy()
    H, found, mask, out = dH.cpu().numpy(), df.cpu().numpy(), dm.cpu().numpy(), dout.cpu().numpy()
    assert 0 == mo[0] < mo[1] < mo[2] <= cap
    for b in range(B - 1):
        lo, hi = int(mo[b]), int(mo[b + 1])
        h, m = siftgpu.findHomography(s[lo:hi], d[lo:hi], siftgpu.RANSAC)
        assert h is not None and found[b] == 1
        assert H[b].tobytes() == h.reshape(9).tobytes(), f"segment {b}: {H[b]} != {h.reshape(9)}"
        assert_bits_equal(mask[lo:hi], m, f"mask of segment {b}")
        assert_bits_equal(out[b], siftgpu.perspectiveTransform(corners, h), f"corners of segment {b}")
        shift = np.array([CROPS[b][1] - CROPS[b + 1][1], CROPS[b][0] - CROPS[b + 1][0]], np.float32)
        np.testing.assert_allclose(out[b], corners + shift, atol=1.0)
    assert (mask[mo[-1]:] == M_SENT).all()
