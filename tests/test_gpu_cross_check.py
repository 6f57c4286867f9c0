"""Cross-check (mutual nearest neighbour) matching for a whole batch on the device.

Expected values come from cross_check_inputs.py alone -- the keep rule restated
in loops and a brute-force matcher per metric -- and every comparison is exact:
records, m_offsets, point pairs as bytes, and the sentinel fill past
min(total, m_cap) and in the rows after every output.
The stage on crafted tables (block edges, many small segments, overflowed
offsets, garbage in the rows of no segment, strides, distance pairs exactly at
each ratio's boundary in double and one float32 ulp above it, m_cap); the one call per metric against the reference and, bit for bit, against
the three separate calls; consecutive frames by aliased offsets; the chain from
the quantiser to the corner transform in stream order; calls that enqueue
nothing; the argument checks on a live context; cross_check_match."""
import numpy as np
import pytest

from conftest import assert_bits_equal

import cross_check_inputs as X

pytestmark = pytest.mark.gpu

EXTRA = 16      # sentinel rows after every output


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()      # a copy: the shared inputs are read-only


def _dev_kpts(k):
    return _dev(np.array(k).view(np.int32).reshape(len(k), 7))


class Out:
    """Sentinel-filled outputs of m_cap + EXTRA rows (m_offsets: n_segments + 1 + EXTRA)."""

    def __init__(self, n_segments, m_cap):
        import torch
        self.m_cap = m_cap
        self.m = torch.full((m_cap + EXTRA, 4), X.SENT_I, dtype=torch.int32, device="cuda")
        self.src = torch.full((m_cap + EXTRA, 2), X.SENT_F, dtype=torch.float32, device="cuda")
        self.dst = torch.full((m_cap + EXTRA, 2), X.SENT_F, dtype=torch.float32, device="cuda")
        self.moff = torch.full((n_segments + 1 + EXTRA,), X.SENT_I, dtype=torch.int32, device="cuda")

    def host(self):
        return (self.m.cpu().numpy().view(X.MATCH_DTYPE).reshape(-1), self.moff.cpu().numpy(), self.src.cpu().numpy(),
                self.dst.cpu().numpy())


def _check(out, ref, n_segments, pairs, what):
    """Exact equality with the reference on the written part, the sentinel everywhere else."""
    m, moff, src, dst = out.host()
    rec, rmoff, rsrc, rdst = ref[:4]
    n = min(len(rec), out.m_cap)
    assert_bits_equal(moff[:n_segments + 1], rmoff, what + " m_offsets")
    assert (moff[n_segments + 1:] == X.SENT_I).all(), what + ": written past m_offsets"
    assert_bits_equal(m[:n], rec[:n], what + " records")
    assert (m[n:].view(np.int32) == X.SENT_I).all(), what + ": records past min(total, m_cap) written"
    if pairs:
        assert_bits_equal(src[:n], rsrc[:n], what + " src_xy")
        assert_bits_equal(dst[:n], rdst[:n], what + " dst_xy")
        n_xy = n
    else:
        n_xy = 0
    assert (src[n_xy:] == X.SENT_F).all() and (dst[n_xy:] == X.SENT_F).all(), what + ": xy rows written"


# ---- the stage on crafted tables -------------------------------------------------------------
STAGE_PARAMS = [(fk, rk, r) for fk in (1, 2) for rk in (1, 2) for r in range(3) if r == 0 or fk == 2]


@pytest.mark.parametrize("variant", ["overflow", "slack"])
@pytest.mark.parametrize("fk,rk,r", STAGE_PARAMS, ids=[f"fk{a}-rk{b}-ratio{c}" for a, b, c in STAGE_PARAMS])
def test_gpu_stage_crafted_tables(ctx, variant, fk, rk, r):
    """Every m_cap of {0, total - 1, total}, with and without point pairs, on tables of
    fk / rk columns (the columns the stage must not read are poisoned)."""
    import torch
    ratio = X.RATIOS[r]
    c = X.crafted(variant)
    ref = X.crafted_ref(variant, ratio)
    total, nseg = len(ref[0]), len(c.qoff) - 1
    assert total > 300 and (c.qoff[-1] > c.q_cap) == (variant == "overflow") == (c.toff[-1] > c.t_cap)
    idx, dist, ridx = (_dev(a) for a in X.tables(c, fk, rk, ratio))
    qo, to, qk, tk = _dev(c.qoff), _dev(c.toff), _dev_kpts(c.q_kpts), _dev_kpts(c.t_kpts)
    for m_cap in (0, total - 1, total):
        for pairs in (True, False):
            o = Out(nseg, m_cap)
            torch.cuda.synchronize()
            ctx.cross_check_matches_device(idx.data_ptr(), dist.data_ptr(), fk, qo.data_ptr(), nseg, c.q_cap,
                                           ridx.data_ptr(), rk, to.data_ptr(), c.t_cap, ratio,
                                           qk.data_ptr() if pairs else None, tk.data_ptr() if pairs else None,
                                           o.m.data_ptr(), o.src.data_ptr(), o.dst.data_ptr(), m_cap,
                                           o.moff.data_ptr())
            ctx.sync()
            _check(o, ref, nseg, pairs, f"{variant} fk={fk} rk={rk} ratio={ratio} m_cap={m_cap} pairs={pairs}")


def test_gpu_stage_host_form_equals_reference(ctx):
    c = X.crafted("overflow")
    for fk, rk, ratio in ((1, 1, 0.0), (2, 2, X.RATIO)):
        ref = X.crafted_ref("overflow", ratio)
        idx, dist, ridx = X.tables(c, fk, rk, ratio)
        m, moff, src, dst = ctx.crossCheckMatches(idx[:c.q_cap], ridx[:c.t_cap], c.qoff, c.toff, dist[:c.q_cap], ratio,
                                                  c.q_kpts[:c.q_cap], c.t_kpts[:c.t_cap])
        assert_bits_equal(m, ref[0], "host records")
        assert_bits_equal(moff, ref[1], "host m_offsets")
        assert_bits_equal(src, ref[2], "host src_xy")
        assert_bits_equal(dst, ref[3], "host dst_xy")
    m, moff, src, dst = ctx.crossCheckMatches(idx[:c.q_cap], ridx[:c.t_cap], c.qoff, c.toff, dist[:c.q_cap], X.RATIO)
    assert src is None and dst is None
    assert_bits_equal(m, ref[0], "host records, no keypoints")


# ---- the one call, per metric ------------------------------------------------------------------
def _knn_device(ctx, metric):
    return [ctx.knn_match_segmented_device, ctx.knn_match_u8_segmented_device,
            ctx.knn_match_l2sqr_u8_segmented_device][metric]


def _one_call_and_three(ctx, c, metric, ratio, aliased):
    """(one call's outputs, the three separate calls' outputs), both on sentinel-filled buffers."""
    import torch
    nseg, fk = len(c.qoff) - 1, 2 if ratio > 0 else 1
    dq, dqk = _dev(c.q), _dev_kpts(c.q_kpts)
    if aliased:     # one buffer, one offsets array: the train side is the same memory one offset on
        off = _dev(c.off)
        dt, dtk, qo_ptr, to_ptr = dq, dqk, off.data_ptr(), off.data_ptr() + 4
    else:
        dt, dtk, qo, to = _dev(c.t), _dev_kpts(c.t_kpts), _dev(c.qoff), _dev(c.toff)
        qo_ptr, to_ptr = qo.data_ptr(), to.data_ptr()
    a, b = Out(nseg, c.q_cap), Out(nseg, c.q_cap)
    idx = torch.full((c.q_cap, fk), X.SENT_I, dtype=torch.int32, device="cuda")
    dist = torch.full((c.q_cap, fk), X.SENT_F, dtype=torch.float32, device="cuda")
    ridx = torch.full((c.t_cap, 1), X.SENT_I, dtype=torch.int32, device="cuda")
    rdist = torch.full((c.t_cap, 1), X.SENT_F, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.cross_match_segmented_device(metric, dq.data_ptr(), qo_ptr, nseg, c.q_cap, dt.data_ptr(), to_ptr, c.t_cap,
                                     ratio, dqk.data_ptr(), dtk.data_ptr(), a.m.data_ptr(), a.src.data_ptr(),
                                     a.dst.data_ptr(), c.q_cap, a.moff.data_ptr())
    knn = _knn_device(ctx, metric)
    knn(dq.data_ptr(), qo_ptr, nseg, c.q_cap, dt.data_ptr(), to_ptr, c.t_cap, fk, idx.data_ptr(), dist.data_ptr())
    knn(dt.data_ptr(), to_ptr, nseg, c.t_cap, dq.data_ptr(), qo_ptr, c.q_cap, 1, ridx.data_ptr(), rdist.data_ptr())
    ctx.cross_check_matches_device(idx.data_ptr(), dist.data_ptr(), fk, qo_ptr, nseg, c.q_cap, ridx.data_ptr(), 1,
                                   to_ptr, c.t_cap, ratio, dqk.data_ptr(), dtk.data_ptr(), b.m.data_ptr(),
                                   b.src.data_ptr(), b.dst.data_ptr(), c.q_cap, b.moff.data_ptr())
    ctx.sync()
    return a, b


def _check_one_call(ctx, c, metric, aliased):
    nseg = len(c.qoff) - 1
    for ratio in (0.0, X.ratio_of(metric)):
        fk = 2 if ratio > 0 else 1
        ref = X.stage_ref(c.idx[:, :fk], c.dist[:, :fk], c.ridx, c.qoff, c.toff, c.q_cap, c.t_cap, ratio, c.q_kpts,
                          c.t_kpts)
        seg, rev_ok, ratio_ok = ref[4]
        assert len(ref[0]) > 0
        if ratio > 0:   # on the reference: each filter drops something the other keeps
            assert (rev_ok & ~ratio_ok).any() and (~rev_ok & ratio_ok).any()
        a, b = _one_call_and_three(ctx, c, metric, ratio, aliased)
        what = f"{X.METRIC_IDS[metric]} ratio={ratio}"
        _check(a, ref, nseg, True, what + " one call")
        for x, y, name in zip(a.host(), b.host(), ("records", "m_offsets", "src_xy", "dst_xy")):
            assert_bits_equal(x, y, f"{what}: {name} of the one call and of the three separate calls")


@pytest.mark.parametrize("metric", range(3), ids=X.METRIC_IDS)
def test_gpu_one_call_against_reference_and_three_calls(ctx, metric):
    c = X.descriptors(metric)
    # the planted duplicates tie in both directions and the lower index wins
    for b in range(3):
        ql, tl = int(c.qoff[b]), int(c.toff[b])
        assert c.idx[ql + 3, 0] == c.idx[ql + 40, 0] == 7 and c.ridx[tl + 7, 0] == 3
        assert c.idx[ql + 20].tolist() == [11, 50] and c.dist[ql + 20].tolist() == [0.0, 0.0]
    _check_one_call(ctx, c, metric, aliased=False)


@pytest.mark.parametrize("metric", range(3), ids=X.METRIC_IDS)
def test_gpu_one_call_consecutive_frames_aliased(ctx, metric):
    """d_train = d_query, d_t_offsets = d_q_offsets + 1, t_cap = q_cap, n_segments = batch - 1."""
    c = X.frames(metric)
    assert c.idx[10].tolist() == [5, 60] and c.idx[33, 0] == c.idx[44, 0] == 100 and c.ridx[90 + 100, 0] == 33
    assert (c.idx[90:] == -1).all()        # frame 1 searches the empty frame 2, frame 2 is empty
    _check_one_call(ctx, c, metric, aliased=True)


# ---- stream order ------------------------------------------------------------------------------------
def test_gpu_chain_in_stream_order(ctx, siftgpu):
    """synth_images (4 x 160x128), detect_compute_batch, the quantiser, the one call
    (squared L2, cross-check only, consecutive frames), the segmented homography and
    the corner transform: all enqueued, one sync.  Equal to the same chain step by
    step through the host forms on the downloaded descriptors."""
    import torch
    Bn, R, C, cap = 4, 160, 128, 2048
    imgs = torch.empty((Bn, R, C), dtype=torch.float32, device="cuda")
    kpts = torch.zeros((cap, 7), dtype=torch.int32, device="cuda")
    desc = torch.zeros((cap, 128), dtype=torch.float32, device="cuda")
    d8 = torch.full((cap, 128), 0xEE, dtype=torch.uint8, device="cuda")
    offs = torch.zeros((Bn + 1,), dtype=torch.int32, device="cuda")
    o = Out(Bn - 1, cap)
    dH = torch.full((Bn - 1, 9), -5.0, dtype=torch.float64, device="cuda")
    df = torch.full((Bn - 1,), X.SENT_I, dtype=torch.int32, device="cuda")
    corners = np.array([[0, 0], [C, 0], [C, R], [0, R]], np.float32)
    dc = _dev(corners)
    dout = torch.full((Bn - 1, 4, 2), -5.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.synth_images(imgs.data_ptr(), Bn, R, C, C, R * C, 0)
    ctx.detect_compute_batch(imgs.data_ptr(), Bn, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                             offs.data_ptr())
    ctx.descriptors_to_u8_device(desc.data_ptr(), offs.data_ptr() + 4 * Bn, cap, d8.data_ptr())
    ctx.cross_match_segmented_device(siftgpu.SIFT_METRIC_L2SQR_U8, d8.data_ptr(), offs.data_ptr(), Bn - 1, cap,
                                     d8.data_ptr(), offs.data_ptr() + 4, cap, 0.0, kpts.data_ptr(), kpts.data_ptr(),
                                     o.m.data_ptr(), o.src.data_ptr(), o.dst.data_ptr(), cap, o.moff.data_ptr())
    ctx.find_homography_segmented_device(o.src.data_ptr(), o.dst.data_ptr(), o.moff.data_ptr(), Bn - 1, cap,
                                         dH.data_ptr(), df.data_ptr(), None)
    ctx.perspective_transform_segmented_device(dH.data_ptr(), df.data_ptr(), Bn - 1, dc.data_ptr(), 4,
                                               dout.data_ptr())
    ctx.sync()
    off = offs.cpu().numpy()
    n = int(off[-1])
    assert 0 < n <= cap and (np.diff(off) > 0).all()
    kp = kpts.cpu().numpy().view(siftgpu.KEYPOINT_DTYPE).reshape(-1)
    # step by step, host forms
    q8 = ctx.descriptorsToU8(desc.cpu().numpy()[:n])
    fi, fd = ctx.knnMatchL2SqrU8Segmented(q8, off[:-1], q8, off[1:], 1)
    ri, _ = ctx.knnMatchL2SqrU8Segmented(q8, off[1:], q8, off[:-1], 1)
    hm, hmoff, hsrc, hdst = ctx.crossCheckMatches(fi, ri, off[:-1], off[1:], fd, 0.0, kp[:n], kp[:n])
    res = ctx.findHomographyBatch(hsrc, hdst, hmoff)
    m, moff, src, dst = o.host()
    k = len(hm)
    assert k >= 3 * 4 and (np.diff(hmoff) >= 4).all()
    assert_bits_equal(moff[:Bn], hmoff, "m_offsets")
    assert_bits_equal(m[:k], hm, "records")
    assert_bits_equal(src[:k], hsrc, "src_xy")
    assert_bits_equal(dst[:k], hdst, "dst_xy")
    assert (m[k:].view(np.int32) == X.SENT_I).all()
    # and the host chain is the brute-force reference's
    ref = X.stage_ref(*X.seg_knn(q8, off[:-1], q8, off[1:], 1, X.L2SQR_U8), X.seg_knn(q8, off[1:], q8, off[:-1], 1,
                      X.L2SQR_U8)[0], off[:-1], off[1:], n, n, 0.0, kp[:n], kp[:n])
    assert_bits_equal(hm, ref[0], "records against the reference")
    H, found, out = dH.cpu().numpy(), df.cpu().numpy(), dout.cpu().numpy()
    for b in range(Bn - 1):
        h, _ = res[b]
        assert found[b] == (h is not None)
        assert H[b].tobytes() == (np.zeros(9) if h is None else h.reshape(9)).tobytes(), f"H of segment {b}"
        want = np.zeros((4, 2), np.float32) if h is None else siftgpu.perspectiveTransform(corners, h)
        assert_bits_equal(out[b], want, f"corners of segment {b}")


# ---- calls that enqueue nothing, and the argument checks on a live context -------------------
def test_gpu_calls_that_enqueue_nothing(ctx, siftgpu):
    L, h = siftgpu.lib(), ctx.h
    o = Out(3, 8)
    p = o.m.data_ptr()
    for nseg, q_cap in ((0, 8), (3, 0)):
        assert L.sift_cross_check_matches_device(h, p, p, 1, p, nseg, q_cap, p, 1, p, 8, 0.0, p, p, o.m.data_ptr(),
                                                 o.src.data_ptr(), o.dst.data_ptr(), 8, o.moff.data_ptr()) == 0
        assert L.sift_cross_match_segmented_device(h, 0, p, p, nseg, q_cap, p, p, 8, 0.0, p, p, o.m.data_ptr(),
                                                   o.src.data_ptr(), o.dst.data_ptr(), 8, o.moff.data_ptr()) == 0
        # whatever the buffers
        assert L.sift_cross_check_matches_device(h, None, None, 1, None, nseg, q_cap, None, 1, None, 0, 0.0, None,
                                                 None, None, None, None, 0, None) == 0
        assert L.sift_cross_match_segmented_device(h, 2, None, None, nseg, q_cap, None, None, 0, 0.0, None, None,
                                                   None, None, None, 0, None) == 0
    ctx.sync()
    m, moff, src, dst = o.host()
    assert (m.view(np.int32) == X.SENT_I).all() and (moff == X.SENT_I).all()
    assert (src == X.SENT_F).all() and (dst == X.SENT_F).all()


def test_gpu_argument_checks_on_a_live_context(ctx, siftgpu):
    """Each call has exactly one fault; every one is SIFT_E_INVALID with a message."""
    import torch
    L, h, E = siftgpu.lib(), ctx.h, siftgpu.SIFT_E_INVALID
    t = torch.zeros(1024, dtype=torch.int32, device="cuda")
    p = t.data_ptr()

    def stage(idx=p, dist=p, fk=2, qo=p, ridx=p, rk=1, to=p, ratio=0.0, qk=None, tk=None, m=p, s=None, d=None, mo=p):
        return L.sift_cross_check_matches_device(h, idx, dist, fk, qo, 1, 1, ridx, rk, to, 1, ratio, qk, tk, m, s, d,
                                                 1, mo)

    def one(metric=1, q=p, qo=p, tr=p, to=p, ratio=0.0, qk=None, tk=None, m=p, s=None, d=None, mo=p, nseg=1):
        return L.sift_cross_match_segmented_device(h, metric, q, qo, nseg, 1, tr, to, 1, ratio, qk, tk, m, s, d, 1, mo)

    assert stage() == 0 and one() == 0
    ctx.sync()
    bad_stage = [dict(idx=None), dict(dist=None), dict(qo=None), dict(ridx=None), dict(to=None), dict(m=None),
                 dict(mo=None), dict(fk=0), dict(fk=3), dict(rk=0), dict(rk=3), dict(fk=1, ratio=0.86),
                 dict(ratio=-1.0), dict(ratio=float("nan")), dict(qk=p), dict(qk=p, tk=p), dict(qk=p, tk=p, s=p)]
    for kw in bad_stage:
        assert stage(**kw) == E and L.sift_last_error(h), kw
    assert b"train offsets" in (stage(to=None), L.sift_last_error(h))[1]
    bad_one = [dict(metric=-1), dict(metric=3), dict(q=None), dict(qo=None), dict(tr=None), dict(to=None),
               dict(m=None), dict(mo=None), dict(ratio=-0.5), dict(qk=p), dict(qk=p, tk=p, d=p), dict(nseg=-1),
               dict(q=p + 4)]
    for kw in bad_one:
        assert one(**kw) == E and L.sift_last_error(h), kw


# ---- Python: one pair ------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", range(3), ids=X.METRIC_IDS)
def test_gpu_cross_check_match_one_pair(ctx, siftgpu, metric):
    c = X.descriptors(metric)
    q, t = c.q[c.qoff[1]:c.qoff[2]], c.t[c.toff[1]:c.toff[2]]       # 129 x 300
    norm = siftgpu.NORM_L2SQR if metric == X.L2SQR_U8 else siftgpu.NORM_L1
    got = siftgpu.cross_check_match(q, t, norm, ctx=ctx)
    idx, dist = X.seg_knn(q, [0, len(q)], t, [0, len(t)], 1, metric)
    ridx, _ = X.seg_knn(t, [0, len(t)], q, [0, len(q)], 1, metric)
    rec = X.stage_ref(idx, dist, ridx, [0, len(q)], [0, len(t)], len(q), len(t), 0.0)[0]
    assert 0 < len(rec) < len(q)
    assert [(m.queryIdx, m.trainIdx, m.imgIdx, m.distance) for m in got] == \
        [(int(r["query"]), int(r["train"]), 0, float(r["distance"])) for r in rec]
    assert siftgpu.cross_check_match(q[:0], t, norm, ctx=ctx) == []
    assert siftgpu.cross_check_match(q, t[:0], norm, ctx=ctx) == []
