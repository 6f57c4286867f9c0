"""The epipolar matcher on the device.

Expected values come from match_epipolar_inputs.epipolar_ref alone -- the window
test of match_window_inputs, fmath::is_inlier restated in float32 numpy, the
dense references' distances, a stable sort -- and every comparison is exact: idx
and dist as bytes over sentinel-filled outputs, the rows of no segment and the
spare rows after every output included.
The edge case (horizontal, vertical and oblique models, a segment without one;
window-only, dst-only, src-only and NaN rejections, the band's boundary, a point
outside the extent, a crowded cell, one and no admissible row), the equalities
with the windowed and the dense matchers, the extent hint, clamped offsets over
garbage, a non-monotone query offset, 200 small segments, found NULL against
found given, a NaN model beside clean ones, the chain from the ratio stage
through the fundamental estimate in stream order, the host form and
epipolar_match, calls that enqueue nothing, the argument checks on a live
context, and the neighbours' outputs around the new call."""
import numpy as np
import pytest

from conftest import assert_bits_equal

import fundamental_inputs as FI
import match_epipolar_inputs as E
import match_window_inputs as W

pytestmark = pytest.mark.gpu

EXTRA = 16      # sentinel rows after every output
INF = float("inf")


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


def _expect(c, k, ref=None):
    """The reference with the sentinel in every row outside the live range."""
    idx = np.full((c.q_cap + EXTRA, k), W.SENT_I, np.int32)
    dist = np.full((c.q_cap + EXTRA, k), W.SENT_F, np.float32)
    live = c.live()
    ri, rd = c.ref(k) if ref is None else (ref[0][:, :k], ref[1][:, :k])
    idx[live], dist[live] = ri[live], rd[live]
    return idx, dist


def _args(c):
    dq, dt, dqk, dtk, qo = _dev(c.q), _dev(c.t), _dev_kpts(c.qk), _dev_kpts(c.tk), _dev(c.qoff)
    to = None if c.toff is None else _dev(c.toff)
    return dq, dt, dqk, dtk, qo, to


def _run(ctx, c, k, F="case", found="case", band=None, radius=None, rows=None, cols=None):
    """One device call on fresh buffers; returns the downloaded (idx, dist)."""
    import torch
    F = c.F if isinstance(F, str) else F
    found = c.found if isinstance(found, str) else found
    dq, dt, dqk, dtk, qo, to = _args(c)
    dF = None if F is None else _dev(np.ascontiguousarray(F, np.float64))
    df = None if found is None else _dev(np.ascontiguousarray(found, np.int32))
    o = Out(c.q_cap, k)
    torch.cuda.synchronize()
    ctx.knn_match_epipolar_segmented_device(
        c.metric, dq.data_ptr(), dqk.data_ptr(), qo.data_ptr(), len(c.qoff) - 1, c.q_cap, dt.data_ptr(), dtk.data_ptr(),
        None if to is None else to.data_ptr(), c.t_cap, None if dF is None else dF.data_ptr(),
        None if df is None else df.data_ptr(), c.band if band is None else band, c.radius if radius is None else radius,
        rows or c.rows, cols or c.cols, k, o.idx.data_ptr(), o.dist.data_ptr())
    ctx.sync()
    return o.host()


def _run_window(ctx, c, k, radius):
    import torch
    dq, dt, dqk, dtk, qo, to = _args(c)
    o = Out(c.q_cap, k)
    torch.cuda.synchronize()
    ctx.knn_match_window_segmented_device(
        c.metric, dq.data_ptr(), dqk.data_ptr(), qo.data_ptr(), len(c.qoff) - 1, c.q_cap, dt.data_ptr(), dtk.data_ptr(),
        None if to is None else to.data_ptr(), c.t_cap, None, None, radius, c.rows, c.cols, k, o.idx.data_ptr(),
        o.dist.data_ptr())
    ctx.sync()
    return o.host()


def _run_dense(ctx, c, k):
    import torch
    dense = [ctx.knn_match_segmented_device, ctx.knn_match_u8_segmented_device,
             ctx.knn_match_l2sqr_u8_segmented_device][c.metric]
    dq, dt, _, _, qo, to = _args(c)
    o = Out(c.q_cap, k)
    torch.cuda.synchronize()
    dense(dq.data_ptr(), qo.data_ptr(), len(c.qoff) - 1, c.q_cap, dt.data_ptr(), None if to is None else to.data_ptr(),
          c.t_cap, k, o.idx.data_ptr(), o.dist.data_ptr())
    ctx.sync()
    return o.host()


def _same(got, want, what):
    assert_bits_equal(got[0], want[0], what + " idx")
    assert_bits_equal(got[1], want[1], what + " dist")


def _check(ctx, c, k, **kw):
    _same(_run(ctx, c, k, **kw), _expect(c, k), f"{c.name} k={k}")


# ---- the edge case ---------------------------------------------------------------------------
@pytest.mark.parametrize("seg_train", [True, False], ids=["segmented", "shared"])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_edges(ctx, metric, k, seg_train):
    c = E.edges_case(metric, seg_train)
    down = E.edges_case(metric, seg_train, float(W.down(E.BAND)))
    assert all(n >= 1 for n in E.census(c, down).values())
    _check(ctx, c, k)
    _check(ctx, down, k)            # one float32 ulp below the band: the boundary rows are out


# ---- equalities with the other matchers -----------------------------------------------------------
@pytest.mark.parametrize("seg_train", [True, False], ids=["segmented", "shared"])
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_without_a_model_equals_the_windowed_and_the_dense_matcher(ctx, metric, seg_train):
    """d_F = NULL at radius 4 and +inf against the windowed call; at +inf (the window case's
    finite coordinates only) against the dense call as well."""
    c = W.edges_case(metric, seg_train, True, INF)
    for k in (1, 2):
        for radius in (4.0, INF):
            got = _run(ctx, c, k, F=None, found=None, band=3.0, radius=radius)
            _same(got, _run_window(ctx, c, k, radius), f"{c.name} k={k} radius={radius} against the windowed call")
        _same(got, _run_dense(ctx, c, k), f"{c.name} k={k} against the dense call")
        _same(got, _expect(c, k), f"{c.name} k={k} against the reference")


@pytest.mark.parametrize("seg_train", [True, False], ids=["segmented", "shared"])
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_infinite_band_and_radius_equal_the_dense_matcher(ctx, metric, seg_train):
    """The edge case's points under one regular F whose epipoles lie far from every keypoint: no
    error is NaN (checked on the restatement), so band = +inf and radius = +inf admit every row."""
    c = E.edges_case(metric, seg_train)
    n = len(c.qoff) - 1
    F = np.tile(E.pencil_F((1234.5, -777.25), [[1.01, 0.02, 3.5], [-0.03, 0.98, -2.25], [0, 0, 1]]), (n, 1))
    for i in c.live():
        e_dst, e_src = E.errors(F[0], c.qk["x"][i], c.qk["y"][i], c.tk["x"], c.tk["y"])
        assert not (np.isnan(e_dst) | np.isnan(e_src)).any()
    for k in (1, 2):
        got = _run(ctx, c, k, F=F, found=None, band=INF, radius=INF)
        _same(got, _run_dense(ctx, c, k), f"{c.name} k={k} against the dense call")
        _same(got, _expect(c, k, E.epipolar_ref(metric, c.q, c.qk, c.qoff, c.t, c.tk, c.toff, F, None, INF, INF)),
              f"{c.name} k={k} against the reference")


# ---- contract cases -------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_result_does_not_depend_on_the_extent_hint(ctx, metric):
    c = E.edges_case(metric, True)
    for rows, cols in ((E.ROWS, E.COLS), (1, 1), (4096, 4096)):
        _check(ctx, c, 2, rows=rows, cols=cols)


@pytest.mark.parametrize("seg_train", [True, False], ids=["segmented", "shared"])
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_clamped_offsets_over_garbage(ctx, metric, seg_train):
    c = E.clamp_case(metric, seg_train)
    assert c.qoff[0] == 3 and c.qoff[-1] > c.q_cap
    for k in (1, 2):
        _check(ctx, c, k)


@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_non_monotone_query_offset_and_many_small_segments(ctx, metric):
    _check(ctx, E.nonmonotone_case(metric), 2)
    c = E.many_segments_case(metric)
    assert len(c.qoff) == 201
    _check(ctx, c, 2)


@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_found_null_against_found_given_and_a_nan_model(ctx, metric):
    c = E.edges_case(metric, True)
    F = c.F.copy()
    F[3] = E.pencil_F((10.0, 70.0), np.eye(3))         # a regular model in the segment that had none
    with_found = E.epipolar_ref(metric, c.q, c.qk, c.qoff, c.t, c.tk, c.toff, F, c.found, c.band, c.radius)
    without = E.epipolar_ref(metric, c.q, c.qk, c.qoff, c.t, c.tk, c.toff, F, None, c.band, c.radius)
    q3 = int(c.seg_qoff[3])
    assert (with_found[0][q3:] != without[0][q3:]).any()
    _same(_run(ctx, c, 2, F=F), _expect(c, 2, with_found), "found given")
    _same(_run(ctx, c, 2, F=F, found=None), _expect(c, 2, without), "found NULL")
    # a NaN-poisoned model in segment 1, used as given: its rows find nothing, the others' bytes stay
    P = F.copy()
    P[1, 4] = np.nan
    clean, bad = _run(ctx, c, 2, F=F, found=None), _run(ctx, c, 2, F=P, found=None)
    q1, q2 = int(c.seg_qoff[1]), int(c.seg_qoff[2])
    keep = np.r_[0:q1, q2:c.q_cap + EXTRA]
    _same((bad[0][keep], bad[1][keep]), (clean[0][keep], clean[1][keep]), "the other segments")
    assert (bad[0][q1:q2] == -1).all() and (bad[1][q1:q2] == np.inf).all() and (clean[0][q1:q2, 0] >= 0).any()
    _same(bad, _expect(c, 2, E.epipolar_ref(metric, c.q, c.qk, c.qoff, c.t, c.tk, c.toff, P, None, c.band, c.radius)),
          "the poisoned call against the reference")


# ---- the chain ----------------------------------------------------------------------------------------
def test_gpu_chain_in_stream_order(ctx, siftgpu):
    """Two planted two-view pairs (fundamental_inputs.data: 0.25 px noise, a quarter of the
    pairs moved off their lines) with matching descriptors: dense match, ratio stage,
    find_fundamental_segmented_device, the epipolar matcher at band 3 reading that d_F / d_found,
    ratio stage -- all enqueued on one stream, one sync, no host value in between."""
    import torch
    rng = np.random.default_rng(9)
    n, nseg = 150, 2
    src, dst, good = zip(*(FI.data(700 + b, n, 0.25, 0.25) for b in range(nseg)))
    qk, tk = W.kpts_at(np.concatenate(src)), W.kpts_at(np.concatenate(dst))
    q = W.rows_of(rng, n * nseg, W.L1_F32)
    t = (q + rng.random((n * nseg, 128)).astype(np.float32) * np.float32(0.01)).astype(np.float32)
    perm = np.concatenate([b * n + rng.permutation(n) for b in range(nseg)])      # the true pair of query i is train inv[i]
    t, tk = t[perm], tk[perm]
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    off = np.array([0, n, 2 * n], np.int32)
    cap = n * nseg
    dq, dt, dqk, dtk, do = _dev(q), _dev(t), _dev_kpts(qk), _dev_kpts(tk), _dev(off)
    o1, o2 = Out(cap, 2), Out(cap, 2)

    def records():
        return (torch.full((cap + EXTRA, 4), W.SENT_I, dtype=torch.int32, device="cuda"),
                torch.full((cap + EXTRA, 2), W.SENT_F, dtype=torch.float32, device="cuda"),
                torch.full((cap + EXTRA, 2), W.SENT_F, dtype=torch.float32, device="cuda"),
                torch.full((nseg + 1 + EXTRA,), W.SENT_I, dtype=torch.int32, device="cuda"))

    m1, s1, d1, mo1 = records()
    m2, s2, d2, mo2 = records()
    dF = torch.full((nseg, 9), -5.0, dtype=torch.float64, device="cuda")
    df = torch.full((nseg,), W.SENT_I, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.knn_match_segmented_device(dq.data_ptr(), do.data_ptr(), nseg, cap, dt.data_ptr(), do.data_ptr(), cap, 2,
                                   o1.idx.data_ptr(), o1.dist.data_ptr())
    ctx.ratio_matches_device(o1.idx.data_ptr(), o1.dist.data_ptr(), do.data_ptr(), nseg, cap, 0.8, dqk.data_ptr(),
                             dtk.data_ptr(), do.data_ptr(), m1.data_ptr(), s1.data_ptr(), d1.data_ptr(), cap,
                             mo1.data_ptr())
    ctx.find_fundamental_segmented_device(s1.data_ptr(), d1.data_ptr(), mo1.data_ptr(), nseg, cap, dF.data_ptr(),
                                          df.data_ptr(), None)
    ctx.knn_match_epipolar_segmented_device(W.L1_F32, dq.data_ptr(), dqk.data_ptr(), do.data_ptr(), nseg, cap,
                                            dt.data_ptr(), dtk.data_ptr(), do.data_ptr(), cap, dF.data_ptr(),
                                            df.data_ptr(), 3.0, INF, 480, 640, 2, o2.idx.data_ptr(), o2.dist.data_ptr())
    ctx.ratio_matches_device(o2.idx.data_ptr(), o2.dist.data_ptr(), do.data_ptr(), nseg, cap, 0.8, dqk.data_ptr(),
                             dtk.data_ptr(), do.data_ptr(), m2.data_ptr(), s2.data_ptr(), d2.data_ptr(), cap,
                             mo2.data_ptr())
    ctx.sync()
    F, found = dF.cpu().numpy(), df.cpu().numpy()
    assert found.tolist() == [1, 1] and np.isfinite(F).all()
    ri, rd, adm = E.epipolar_ref(W.L1_F32, q, qk, off, t, tk, off, F, found, 3.0, INF)
    gi, gd = o2.host()
    assert_bits_equal(gi[:cap], ri, "epipolar idx against the restatement fed the F read back")
    assert_bits_equal(gd[:cap], rd, "epipolar dist")
    assert (gi[cap:] == W.SENT_I).all() and (gd[cap:] == W.SENT_F).all()
    # every planted true pair within the band under that F is a candidate
    within = 0
    for b in range(nseg):
        for i in range(b * n, (b + 1) * n):
            j = int(inv[i])
            e_dst, e_src = E.errors(F[b], qk["x"][i], qk["y"][i], tk["x"][j:j + 1], tk["y"][j:j + 1])
            if e_dst[0] <= np.float32(9) and e_src[0] <= np.float32(9):
                within += 1
                assert j - b * n in adm[i], (b, i, j)
    assert within > 0.7 * np.concatenate(good).sum()
    # the second ratio stage reads the new call's output unchanged
    wm, wmo, _, _ = ctx.ratioMatches(ri, rd, off, 0.8, qk, tk, off)
    got = m2.cpu().numpy().view(siftgpu.MATCH_DTYPE).reshape(-1)
    assert_bits_equal(mo2.cpu().numpy()[:nseg + 1], wmo, "m_offsets")
    assert_bits_equal(got[:len(wm)], wm, "records")


# ---- the host form and Python -----------------------------------------------------------------------
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_gpu_host_form_and_epipolar_match(ctx, siftgpu, metric):
    c = E.edges_case(metric, True)
    for k in (1, 2):
        gi, gd = _run(ctx, c, k)
        hi, hd = ctx.knnMatchEpipolarSegmented(metric, c.q, c.qk, c.qoff, c.t, c.tk, c.toff, c.F, c.found, c.band,
                                               c.radius, (c.rows, c.cols), k)
        assert_bits_equal(hi, gi[:c.q_cap], "host form idx")
        assert_bits_equal(hd, gd[:c.q_cap], "host form dist")
    # the host form leaves the rows of no segment as it found them (idx -1 / dist +inf in the binding)
    cc = E.clamp_case(metric, True)
    hi, hd = ctx.knnMatchEpipolarSegmented(metric, cc.q[:cc.q_cap], cc.qk[:cc.q_cap], cc.qoff, cc.t[:cc.t_cap],
                                           cc.tk[:cc.t_cap], cc.toff, cc.F, None, cc.band, cc.radius, (cc.rows, cc.cols), 2)
    assert_bits_equal(hi, cc.idx, "host form over clamped offsets, idx")
    assert_bits_equal(hd, cc.dist, "host form over clamped offsets, dist")
    # epipolar_match: one pair, equal to the device form's segment
    norm = siftgpu.NORM_L2SQR if metric == W.L2SQR_U8 else siftgpu.NORM_L1
    for b in (0, 2):
        ql, qh, tl, th = int(c.qoff[b]), int(c.qoff[b + 1]), int(c.toff[b]), int(c.toff[b + 1])
        for size in (None, (c.rows, c.cols)):
            got = siftgpu.epipolar_match(c.q[ql:qh], c.qk[ql:qh], c.t[tl:th], c.tk[tl:th], c.F[b].reshape(3, 3), c.band,
                                         c.radius, norm, 2, size, ctx=ctx)
            want = [[(i, int(c.idx[ql + i, j]), 0, float(c.dist[ql + i, j])) for j in range(2) if c.idx[ql + i, j] >= 0]
                    for i in range(qh - ql)]
            assert [[(m.queryIdx, m.trainIdx, m.imgIdx, m.distance) for m in row] for row in got] == want
    assert siftgpu.epipolar_match(c.q[:0], c.qk[:0], c.t, c.tk, np.eye(3), normType=norm, ctx=ctx) == []
    assert siftgpu.epipolar_match(c.q[:3], c.qk[:3], c.t[:0], c.tk[:0], np.eye(3), normType=norm, ctx=ctx) == [[], [], []]


# ---- calls that enqueue nothing, and the argument checks on a live context -------------------
def test_gpu_calls_that_enqueue_nothing(ctx, siftgpu):
    L, h = siftgpu.lib(), ctx.h
    o = Out(8, 2)
    p = o.idx.data_ptr()
    for nseg, q_cap in ((0, 8), (3, 0)):
        for metric in range(3):
            assert L.sift_knn_match_epipolar_segmented_device(h, metric, p, p, p, nseg, q_cap, p, p, p, 8, None, None,
                                                              3.0, 4.0, 10, 10, 2, o.idx.data_ptr(),
                                                              o.dist.data_ptr()) == 0
            assert L.sift_knn_match_epipolar_segmented_device(h, metric, None, None, None, nseg, q_cap, None, None,
                                                              None, 0, None, None, 3.0, 4.0, 10, 10, 2, None, None) == 0
    ctx.sync()
    idx, dist = o.host()
    assert (idx == W.SENT_I).all() and (dist == W.SENT_F).all()


def test_gpu_argument_checks_on_a_live_context(ctx, siftgpu):
    """Each call has exactly one fault; every one is SIFT_E_INVALID with a message."""
    import torch
    L, h, Einv = siftgpu.lib(), ctx.h, siftgpu.SIFT_E_INVALID
    t = torch.zeros(1024, dtype=torch.int32, device="cuda")
    p = t.data_ptr()

    def call(metric=1, q=p, qk=p, qo=p, nseg=1, q_cap=1, tr=p, tk=p, to=p, t_cap=1, F=None, found=None, band=3.0,
             radius=4.0, rows=10, cols=10, k=2, idx=p, dist=p):
        return L.sift_knn_match_epipolar_segmented_device(h, metric, q, qk, qo, nseg, q_cap, tr, tk, to, t_cap, F, found,
                                                          band, radius, rows, cols, k, idx, dist)

    assert call() == 0 and call(to=None) == 0 and call(F=p, found=p) == 0 and call(F=p) == 0 and call(band=0.0) == 0
    assert call(band=INF, radius=INF) == 0 and call(radius=0.0) == 0 and call(tr=None, t_cap=0) == 0
    ctx.sync()
    bad = [dict(metric=-1), dict(metric=3), dict(q=None), dict(qk=None), dict(qo=None), dict(tr=None), dict(tk=None),
           dict(idx=None), dict(dist=None), dict(k=0), dict(k=3), dict(radius=-1.0), dict(radius=float("nan")),
           dict(radius=-INF), dict(band=-1.0), dict(band=float("nan")), dict(band=-INF), dict(rows=0), dict(cols=0),
           dict(rows=-5), dict(nseg=-1), dict(q_cap=-1), dict(t_cap=-1), dict(q=p + 4), dict(tk=None, t_cap=0, tr=None)]
    for kw in bad:
        assert call(**kw) == Einv and L.sift_last_error(h), kw
    assert b"band" in (call(band=-1.0), L.sift_last_error(h))[1]
    assert b"radius" in (call(radius=-1.0), L.sift_last_error(h))[1]
    assert b"metric" in (call(metric=3), L.sift_last_error(h))[1]
    assert b"keypoint" in (call(qk=None), L.sift_last_error(h))[1]
    assert L.sift_knn_match_epipolar_segmented_device(None, 1, p, p, p, 1, 1, p, p, p, 1, None, None, 3.0, 4.0, 10, 10,
                                                      2, p, p) == Einv
    z = np.zeros(128, np.uint8)
    zk = np.zeros(1, siftgpu.KEYPOINT_DTYPE)
    for kw in (dict(band=-1.0), dict(radius=-1.0), dict(image_size=(0, 5))):
        with pytest.raises(siftgpu.SiftError):
            ctx.knnMatchEpipolarSegmented(1, z, zk, [0, 1], z, zk, **kw)


# ---- the neighbours around the new call -----------------------------------------------------------------
def test_gpu_neighbours_are_unchanged_around_the_new_call(ctx, siftgpu):
    """The windowed matcher and the fundamental estimate give the same bytes before and after
    an epipolar call on the same context (they share its scratch block and the binning)."""
    import torch
    c = E.edges_case(W.L1_U8, True)
    s, d, _ = FI.data(31, 120, 0.3, 0.25)
    ds, dd, mo = _dev(s.astype(np.float32)), _dev(d.astype(np.float32)), _dev(np.array([0, 120], np.int32))

    def estimate():
        dF = torch.full((1, 9), -5.0, dtype=torch.float64, device="cuda")
        df = torch.full((1,), W.SENT_I, dtype=torch.int32, device="cuda")
        ctx.find_fundamental_segmented_device(ds.data_ptr(), dd.data_ptr(), mo.data_ptr(), 1, 120, dF.data_ptr(),
                                              df.data_ptr(), None)
        ctx.sync()
        return dF.cpu().numpy(), df.cpu().numpy()

    w0, f0 = _run_window(ctx, c, 2, 16.0), estimate()
    _check(ctx, c, 2)
    w1, f1 = _run_window(ctx, c, 2, 16.0), estimate()
    _same(w1, w0, "the windowed matcher")
    assert f0[1].tolist() == [1] and f1[0].tobytes() == f0[0].tobytes() and f1[1].tolist() == [1]
    wi, wd, _ = W.window_ref(c.metric, c.q, c.qk, c.qoff, c.t, c.tk, c.toff, 16.0)
    idx, dist = _expect(c, 2, (wi, wd))
    _same(w1, (idx, dist), "the windowed matcher against its reference")
