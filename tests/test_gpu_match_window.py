"""The windowed (spatially gated) matcher on the device.

Expected values come from match_window_inputs.py alone -- admissibility in
float32 loops, oracle/homography.py's perspective_transform, the dense
references' distances, a stable sort -- and every comparison is exact: idx and
dist as bytes, and the sentinel fill in the rows of no segment and in the spare
rows after every output.
The edges case (empty sides, one train row, one crowded cell, points at exactly
radius and one ulp beyond, cell boundaries, border clamping, NaN and infinite
coordinates, ties), clamped offsets over garbage, many small segments,
radius = +inf against the dense matcher byte for byte, radius = 0, homography
priors, the chain from the dense match to the gated ratio stage in stream
order, consecutive frames by aliasing, the host form and window_match, calls
that enqueue nothing, the argument checks on a live context."""
import numpy as np
import pytest

from conftest import assert_bits_equal

import match_window_inputs as W

pytestmark = pytest.mark.gpu

EXTRA = 16      # sentinel rows after every output


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()      # a copy: the shared inputs are read-only


def _dev_kpts(k):
    return _dev(np.array(k).view(np.int32).reshape(len(k), 7))


class Out:
    """Sentinel-filled idx / dist of q_cap + EXTRA rows."""

    def __init__(self, q_cap, k):
        import torch
        self.idx = torch.full((q_cap + EXTRA, k), W.SENT_I, dtype=torch.int32, device="cuda")
        self.dist = torch.full((q_cap + EXTRA, k), W.SENT_F, dtype=torch.float32, device="cuda")

    def host(self):
        return self.idx.cpu().numpy(), self.dist.cpu().numpy()


def _expect(c, k):
    """The reference with the sentinel in every row outside the live range."""
    idx = np.full((c.q_cap + EXTRA, k), W.SENT_I, np.int32)
    dist = np.full((c.q_cap + EXTRA, k), W.SENT_F, np.float32)
    live = c.live()
    ri, rd = c.ref(k)
    idx[live], dist[live] = ri[live], rd[live]
    return idx, dist


def _run(ctx, c, k, radius=None, H="case", found="case", rows=None, cols=None):
    """One device call on fresh buffers; returns the downloaded (idx, dist)."""
    import torch
    H = c.H if isinstance(H, str) else H
    found = c.found if isinstance(found, str) else found
    dq, dt, dqk, dtk = _dev(c.q), _dev(c.t), _dev_kpts(c.qk), _dev_kpts(c.tk)
    qo = _dev(c.qoff)
    to = None if c.toff is None else _dev(c.toff)
    dH = None if H is None else _dev(np.ascontiguousarray(H, np.float64))
    df = None if found is None else _dev(np.ascontiguousarray(found, np.int32))
    o = Out(c.q_cap, k)
    torch.cuda.synchronize()
    ctx.knn_match_window_segmented_device(
        c.metric, dq.data_ptr(), dqk.data_ptr(), qo.data_ptr(), len(c.qoff) - 1, c.q_cap, dt.data_ptr(), dtk.data_ptr(),
        None if to is None else to.data_ptr(), c.t_cap, None if dH is None else dH.data_ptr(),
        None if df is None else df.data_ptr(), c.radius if radius is None else radius, rows or c.rows, cols or c.cols, k,
        o.idx.data_ptr(), o.dist.data_ptr())
    ctx.sync()
    return o.host()


def _check(ctx, c, k, **kw):
    idx, dist = _run(ctx, c, k, **kw)
    ri, rd = _expect(c, k)
    assert_bits_equal(idx, ri, f"{c.name} k={k} idx")
    assert_bits_equal(dist, rd, f"{c.name} k={k} dist")


# ---- the edges case ------------------------------------------------------------------------
@pytest.mark.parametrize("seg_train", [True, False], ids=["segmented", "shared"])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_edges(ctx, metric, k, seg_train):
    c = W.edges_case(metric, seg_train)
    s = W.census(c)
    assert s["zero"] and s["one"] and s["two"] and 2 * s["two_or_more"] >= s["live"] and s["differs"]
    _check(ctx, c, k)


@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_result_does_not_depend_on_the_extent_hint(ctx, metric):
    """rows, cols only shape the grid: one cell, the case's small extent, 1080p, the largest ints."""
    c = W.edges_case(metric, True)
    for rows, cols in ((1, 1), (1080, 1920), (7, 3000), (2**31 - 1, 2**31 - 1)):
        _check(ctx, c, 2, rows=rows, cols=cols)


# ---- clamps, many segments -------------------------------------------------------------------
@pytest.mark.parametrize("seg_train", [True, False], ids=["segmented", "shared"])
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_clamped_offsets_over_garbage(ctx, metric, seg_train):
    c = W.clamp_case(metric, seg_train)
    assert c.qoff[0] == 3 and c.qoff[-1] > c.q_cap
    for k in (1, 2):
        _check(ctx, c, k)


@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_many_small_segments(ctx, metric):
    _check(ctx, W.many_segments_case(metric), 2)


# ---- radius = +inf and radius = 0 ------------------------------------------------------------
@pytest.mark.parametrize("seg_train", [True, False], ids=["segmented", "shared"])
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_infinite_radius_equals_the_dense_matcher(ctx, metric, seg_train):
    """On the edges case without its NaN and infinite coordinates: byte for byte the dense
    sift_knn_match_*_segmented_device output of the same metric."""
    import torch
    c = W.edges_case(metric, seg_train, True, float("inf"))
    dense = [ctx.knn_match_segmented_device, ctx.knn_match_u8_segmented_device,
             ctx.knn_match_l2sqr_u8_segmented_device][metric]
    dq, dt, qo = _dev(c.q), _dev(c.t), _dev(c.qoff)
    to = None if c.toff is None else _dev(c.toff)
    for k in (1, 2):
        o = Out(c.q_cap, k)
        torch.cuda.synchronize()
        dense(dq.data_ptr(), qo.data_ptr(), len(c.qoff) - 1, c.q_cap, dt.data_ptr(),
              None if to is None else to.data_ptr(), c.t_cap, k, o.idx.data_ptr(), o.dist.data_ptr())
        ctx.sync()
        di, dd = o.host()
        wi, wd = _run(ctx, c, k)
        assert_bits_equal(wi, di, f"{c.name} k={k} idx against the dense call")
        assert_bits_equal(wd, dd, f"{c.name} k={k} dist against the dense call")
        _check(ctx, c, k)


@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_radius_zero_matches_coincident_points_only(ctx, metric):
    c = W.coincident_case(metric)
    assert (c.n_adm == 0).any() and (c.n_adm >= 2).any()
    for k in (1, 2):
        _check(ctx, c, k)


# ---- priors --------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_found", [True, False], ids=["found", "found-null"])
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_priors(ctx, metric, use_found):
    """A translation, a projective H with |w| <= FLT_EPSILON at some queries, a NaN H behind
    found == 0 (the identity) or used as given (found NULL), 2 I."""
    c = W.prior_case(metric, use_found)
    for k in (1, 2):
        _check(ctx, c, k)


# ---- stream order ------------------------------------------------------------------------------------
def test_gpu_chain_in_stream_order(ctx, siftgpu):
    """Two synthetic frames: the second holds the first's keypoints moved by a known
    homography, with slightly changed descriptors, plus distractors that repeat descriptors
    far away.  Dense match, ratio stage, segmented homography, the windowed match reading
    that d_H / d_found, ratio stage: all enqueued, one sync.  The final records equal the
    same sequence through the host forms, with the windowed step taken from the reference."""
    import torch
    rng = np.random.default_rng(5)
    n, nd = 200, 120
    Ht = np.array([1.02, 0.03, 14.0, -0.02, 0.99, -9.0, 1e-5, -2e-5, 1.0])
    axy = np.stack([rng.random(n) * 300, rng.random(n) * 200], 1).astype(np.float32)
    bxy = siftgpu.perspectiveTransform(axy, Ht.reshape(3, 3)).astype(np.float32)
    bxy += (rng.random((n, 2)).astype(np.float32) - np.float32(0.5))
    ad = W.rows_of(rng, n, W.L1_F32)
    bd = (ad + rng.random((n, 128)).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    dd = (ad[:nd] + rng.random((nd, 128)).astype(np.float32) * np.float32(0.0095)).astype(np.float32)  # as near, elsewhere
    dxy = np.stack([rng.random(nd) * 300, rng.random(nd) * 200], 1).astype(np.float32)
    q, qk = ad, W.kpts_at(axy)
    t, tk = np.concatenate([bd, dd]), W.kpts_at(np.concatenate([bxy, dxy]))
    qoff, toff = np.array([0, n], np.int32), np.array([0, n + nd], np.int32)
    cap, radius, R, C = n, 40.0, 200, 300       # about 30 candidates per window: a second neighbour for the ratio test
    dq, dt, dqk, dtk, dqo, dto = _dev(q), _dev(t), _dev_kpts(qk), _dev_kpts(tk), _dev(qoff), _dev(toff)
    o1, o2 = Out(cap, 2), Out(cap, 2)

    def records():
        return (torch.full((cap + EXTRA, 4), W.SENT_I, dtype=torch.int32, device="cuda"),
                torch.full((cap + EXTRA, 2), W.SENT_F, dtype=torch.float32, device="cuda"),
                torch.full((cap + EXTRA, 2), W.SENT_F, dtype=torch.float32, device="cuda"),
                torch.full((2 + EXTRA,), W.SENT_I, dtype=torch.int32, device="cuda"))

    m1, s1, d1, mo1 = records()
    m2, s2, d2, mo2 = records()
    dH = torch.full((1, 9), -5.0, dtype=torch.float64, device="cuda")
    df = torch.full((1,), W.SENT_I, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.knn_match_segmented_device(dq.data_ptr(), dqo.data_ptr(), 1, cap, dt.data_ptr(), dto.data_ptr(), n + nd, 2,
                                   o1.idx.data_ptr(), o1.dist.data_ptr())
    ctx.ratio_matches_device(o1.idx.data_ptr(), o1.dist.data_ptr(), dqo.data_ptr(), 1, cap, 0.86, dqk.data_ptr(),
                             dtk.data_ptr(), dto.data_ptr(), m1.data_ptr(), s1.data_ptr(), d1.data_ptr(), cap,
                             mo1.data_ptr())
    ctx.find_homography_segmented_device(s1.data_ptr(), d1.data_ptr(), mo1.data_ptr(), 1, cap, dH.data_ptr(),
                                         df.data_ptr(), None)
    ctx.knn_match_window_segmented_device(W.L1_F32, dq.data_ptr(), dqk.data_ptr(), dqo.data_ptr(), 1, cap,
                                          dt.data_ptr(), dtk.data_ptr(), dto.data_ptr(), n + nd, dH.data_ptr(),
                                          df.data_ptr(), radius, R, C, 2, o2.idx.data_ptr(), o2.dist.data_ptr())
    ctx.ratio_matches_device(o2.idx.data_ptr(), o2.dist.data_ptr(), dqo.data_ptr(), 1, cap, 0.86, dqk.data_ptr(),
                             dtk.data_ptr(), dto.data_ptr(), m2.data_ptr(), s2.data_ptr(), d2.data_ptr(), cap,
                             mo2.data_ptr())
    ctx.sync()
    # the same sequence, step by step on the host
    hi, hd = ctx.knnMatchSegmented(q, qoff, t, toff, 2)
    hm, hmo, hs, hdst = ctx.ratioMatches(hi, hd, qoff, 0.86, qk, tk, toff)
    (h, _), = ctx.findHomographyBatch(hs, hdst, hmo)
    assert h is not None and len(hm) < n // 2            # the distractors cost the dense ratio test most pairs
    assert dH.cpu().numpy().tobytes() == np.asarray(h, np.float64).tobytes() and df.cpu().numpy().tolist() == [1]
    wi, wd, n_adm = W.window_ref(W.L1_F32, q, qk, qoff, t, tk, toff, radius, H=np.asarray(h).reshape(1, 9),
                                 found=np.array([1]))
    gi, gd = o2.host()
    assert_bits_equal(gi[:cap], wi, "windowed idx")
    assert_bits_equal(gd[:cap], wd, "windowed dist")
    wm, wmo, ws, wdst = ctx.ratioMatches(wi, wd, qoff, 0.86, qk, tk, toff)
    assert len(wm) > len(hm) + 50 and (wm["train"] == wm["query"]).all()   # the gate removes most distractors
    k = len(wm)
    got = m2.cpu().numpy().view(siftgpu.MATCH_DTYPE).reshape(-1)
    assert_bits_equal(mo2.cpu().numpy()[:2], wmo, "m_offsets")
    assert_bits_equal(got[:k], wm, "records")
    assert (got[k:].view(np.int32) == W.SENT_I).all()
    assert_bits_equal(s2.cpu().numpy()[:k], ws, "src_xy")
    assert_bits_equal(d2.cpu().numpy()[:k], wdst, "dst_xy")


@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_consecutive_frames_aliased(ctx, metric):
    """d_train = d_query, d_t_offsets = d_q_offsets + 1, the keypoints aliased likewise."""
    import torch
    c = W.frames_case(metric)
    d, dk, off = _dev(c.q), _dev_kpts(c.qk), _dev(c.off)
    for k in (1, 2):
        o = Out(c.q_cap, k)
        torch.cuda.synchronize()
        ctx.knn_match_window_segmented_device(metric, d.data_ptr(), dk.data_ptr(), off.data_ptr(), 3, c.q_cap,
                                              d.data_ptr(), dk.data_ptr(), off.data_ptr() + 4, c.q_cap, None, None,
                                              c.radius, c.rows, c.cols, k, o.idx.data_ptr(), o.dist.data_ptr())
        ctx.sync()
        ri, rd = _expect(c, k)
        idx, dist = o.host()
        assert_bits_equal(idx, ri, f"{c.name} k={k} idx")
        assert_bits_equal(dist, rd, f"{c.name} k={k} dist")


# ---- the host form and Python ----------------------------------------------------------------------
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_host_form_and_window_match(ctx, siftgpu, metric):
    c = W.prior_case(metric, True)
    for k in (1, 2):
        gi, gd = _run(ctx, c, k)
        hi, hd = ctx.knnMatchWindowSegmented(metric, c.q, c.qk, c.qoff, c.t, c.tk, c.toff, c.radius, c.H, c.found,
                                             (c.rows, c.cols), k)
        assert_bits_equal(hi, gi[:c.q_cap], "host form idx")
        assert_bits_equal(hd, gd[:c.q_cap], "host form dist")
    # the host form leaves the rows of no segment as it found them (idx -1 / dist +inf in the binding)
    c = W.clamp_case(metric, True)
    hi, hd = ctx.knnMatchWindowSegmented(metric, c.q[:c.q_cap], c.qk[:c.q_cap], c.qoff, c.t[:c.t_cap], c.tk[:c.t_cap],
                                         c.toff, c.radius, None, None, (c.rows, c.cols), 2)
    assert_bits_equal(hi, c.idx, "host form over clamped offsets, idx")
    assert_bits_equal(hd, c.dist, "host form over clamped offsets, dist")
    # window_match: one pair, with and without a prior, equal to the device form's segment
    c = W.prior_case(metric, True)
    norm = siftgpu.NORM_L2SQR if metric == W.L2SQR_U8 else siftgpu.NORM_L1
    for b, H in ((0, c.H[0]), (2, None)):
        ql, qh, tl, th = int(c.qoff[b]), int(c.qoff[b + 1]), int(c.toff[b]), int(c.toff[b + 1])
        for size in (None, (c.rows, c.cols)):
            got = siftgpu.window_match(c.q[ql:qh], c.qk[ql:qh], c.t[tl:th], c.tk[tl:th], c.radius, H, norm, 2, size,
                                       ctx=ctx)
            want = [[(i, int(c.idx[ql + i, j]), 0, float(c.dist[ql + i, j])) for j in range(2) if c.idx[ql + i, j] >= 0]
                    for i in range(qh - ql)]
            assert [[(m.queryIdx, m.trainIdx, m.imgIdx, m.distance) for m in row] for row in got] == want
    assert siftgpu.window_match(c.q[:0], c.qk[:0], c.t, c.tk, 4.0, None, norm, ctx=ctx) == []
    assert siftgpu.window_match(c.q[:3], c.qk[:3], c.t[:0], c.tk[:0], 4.0, None, norm, ctx=ctx) == [[], [], []]


# ---- calls that enqueue nothing, and the argument checks on a live context -------------------
def test_gpu_calls_that_enqueue_nothing(ctx, siftgpu):
    L, h = siftgpu.lib(), ctx.h
    o = Out(8, 2)
    p = o.idx.data_ptr()
    for nseg, q_cap in ((0, 8), (3, 0)):
        for metric in range(3):
            assert L.sift_knn_match_window_segmented_device(h, metric, p, p, p, nseg, q_cap, p, p, p, 8, None, None,
                                                            4.0, 10, 10, 2, o.idx.data_ptr(), o.dist.data_ptr()) == 0
            # whatever the buffers
            assert L.sift_knn_match_window_segmented_device(h, metric, None, None, None, nseg, q_cap, None, None, None,
                                                            0, None, None, 4.0, 10, 10, 2, None, None) == 0
    ctx.sync()
    idx, dist = o.host()
    assert (idx == W.SENT_I).all() and (dist == W.SENT_F).all()


def test_gpu_argument_checks_on_a_live_context(ctx, siftgpu):
    """Each call has exactly one fault; every one is SIFT_E_INVALID with a message."""
    import torch
    L, h, E = siftgpu.lib(), ctx.h, siftgpu.SIFT_E_INVALID
    t = torch.zeros(1024, dtype=torch.int32, device="cuda")
    p = t.data_ptr()

    def call(metric=1, q=p, qk=p, qo=p, nseg=1, q_cap=1, tr=p, tk=p, to=p, t_cap=1, H=None, found=None, radius=4.0,
             rows=10, cols=10, k=2, idx=p, dist=p):
        return L.sift_knn_match_window_segmented_device(h, metric, q, qk, qo, nseg, q_cap, tr, tk, to, t_cap, H, found,
                                                        radius, rows, cols, k, idx, dist)

    assert call() == 0 and call(to=None) == 0 and call(H=p, found=p) == 0 and call(radius=0.0) == 0
    assert call(radius=float("inf")) == 0 and call(tr=None, t_cap=0) == 0
    ctx.sync()
    bad = [dict(metric=-1), dict(metric=3), dict(q=None), dict(qk=None), dict(qo=None), dict(tr=None), dict(tk=None),
           dict(idx=None), dict(dist=None), dict(k=0), dict(k=3), dict(radius=-1.0), dict(radius=float("nan")),
           dict(radius=float("-inf")), dict(rows=0), dict(cols=0), dict(rows=-5), dict(nseg=-1), dict(q_cap=-1),
           dict(t_cap=-1), dict(q=p + 4), dict(tk=None, t_cap=0, tr=None)]
    for kw in bad:
        assert call(**kw) == E and L.sift_last_error(h), kw
    assert b"radius" in (call(radius=-1.0), L.sift_last_error(h))[1]
    assert b"metric" in (call(metric=7), L.sift_last_error(h))[1]
    assert b"keypoint" in (call(qk=None), L.sift_last_error(h))[1]
    assert L.sift_knn_match_window_segmented_device(None, 1, p, p, p, 1, 1, p, p, p, 1, None, None, 4.0, 10, 10, 2, p,
                                                    p) == E
    # the host form shares the checks
    z = np.zeros(128, np.uint8)
    zk = np.zeros(1, siftgpu.KEYPOINT_DTYPE)
    for kw in (dict(radius=-1.0), dict(image_size=(0, 5))):
        with pytest.raises(siftgpu.SiftError):
            ctx.knnMatchWindowSegmented(1, z, zk, [0, 1], z, zk, **kw)
