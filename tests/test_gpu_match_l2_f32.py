"""The squared-L2 kNN matcher on float descriptors (f32 MFMA) on the GPU.

Every expected value is match_l2_f32_inputs' oracle -- the rule of sift_hip.h walked
with a correctly rounded float32 fma -- compared bit for bit (indices and the float
distances), into sentinel-filled outputs with extra rows.  On dyadic rows (u / 512)
the result is also the byte squared-L2 matcher's, scaled by 2^-18.  The value
cases (signed rows, near-copies around the clamp, subnormals, +inf and NaN
distances of finite rows) pin the lines of the rule that depend on values."""
import numpy as np
import pytest

from conftest import assert_bits_equal

import cross_check_inputs as X
import match_l2_f32_inputs as F
import match_u8_inputs as U
import test_match_batch as B

pytestmark = pytest.mark.gpu

RATIO2 = 0.86 * 0.86    # the application's 0.86 on squared distances


def _f32_device(ctx, c, k, extra=64, train_is_query=False, toff_ptr_from_q=False, fn=None):
    """Device form into sentinel-filled outputs of q_cap + extra rows -> (idx, dist) numpy."""
    import torch
    dq, dqo = B._dev(c.q), B._dev(c.qoff)
    dt = dq if train_is_query else B._dev(c.t)
    dto = None if c.toff is None else B._dev(c.toff)
    to_ptr = None if dto is None else dto.data_ptr()
    if toff_ptr_from_q:
        to_ptr = dqo.data_ptr() + 4
    di = torch.full((c.q_cap + extra, k), U.SENT_I, dtype=torch.int32, device="cuda")
    dd = torch.full((c.q_cap + extra, k), U.SENT_D, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    (fn or ctx.knn_match_l2sqr_f32_segmented_device)(
        dq.data_ptr(), dqo.data_ptr(), len(c.qoff) - 1 - toff_ptr_from_q, c.q_cap, dt.data_ptr(), to_ptr, c.t_cap, k,
        di.data_ptr(), dd.data_ptr())
    ctx.sync()
    return di.cpu().numpy(), dd.cpu().numpy()


def _check_case(ctx, c, k):
    """The device form equals the oracle on the live rows and writes no other."""
    ridx, rdist = c.ref(k)
    idx, dist = _f32_device(ctx, c, k)
    B._check_live(idx, dist, ridx, rdist, c.qoff, c.q_cap, f"{c.name} k={k}")


# ---- bit equality with the oracle ----------------------------------------------------------
@pytest.mark.parametrize("k", [2, 1])
@pytest.mark.parametrize("seg_train", [False, True], ids=["shared", "segmented"])
def test_gpu_l2_f32_random_rows_tile_edges(ctx, k, seg_train):
    """Query segments of 0 / 1 / 31 / 32 / 33 / 63 / 64 / 65 / 255 / 256 / 257 rows; train
    ranges of 0 / 1 / 2 / 3 / 9 / 63 / 64 / 65 / 127 / 128 / 129 / 193 rows in one split
    (segmented) or 130 shared rows in three; ties planted across the half-wave, tile,
    step and split seams."""
    c = F.edges_case(seg_train)
    assert len(c.planted) >= 10
    _check_case(ctx, c, k)
    if seg_train:   # local indices; -1 / +inf where the range has fewer than k rows
        idx, dist = c.ref(k)
        for b, nt in enumerate(F.T_SIZES):
            seg = idx[c.qoff[b]:c.qoff[b + 1]]
            assert (seg < max(nt, 1)).all()
            if nt < k and len(seg):
                assert (seg[:, nt:] == -1).all() and np.isposinf(dist[c.qoff[b]:c.qoff[b + 1], nt:]).all()


@pytest.mark.parametrize("k", [2, 1])
def test_gpu_l2_f32_splits_with_an_empty_one(ctx, k):
    _check_case(ctx, F.splits_case(), k)


@pytest.mark.parametrize("k", [2, 1])
def test_gpu_l2_f32_operand_map_distinct_weights(ctx, k):
    _check_case(ctx, F.weights_case(), k)


def test_gpu_l2_f32_many_segments(ctx):
    c = F.many_segments_case()
    assert len(c.qoff) - 1 == 257
    _check_case(ctx, c, 2)


@pytest.mark.parametrize("n", range(5), ids=["q_cap", "q_cap-shared", "t_cap", "t_cap-shared", "first-offset"])
def test_gpu_l2_f32_capacity_clamps(ctx, n):
    c = F.clamp_cases()[n]
    assert c.name == ["q_cap", "q_cap-shared", "t_cap", "t_cap-shared", "first-offset"][n]
    _check_case(ctx, c, 2)


def test_gpu_l2_f32_short_train_sets(ctx, siftgpu):
    """n_train of 0 and 1 with k = 2: -1 / +inf, and the ratio stage skips those rows."""
    rng = np.random.default_rng(146)
    q, t = F.rows(rng, 70), F.rows(rng, 1)
    qoff = U.offsets([5, 65])
    c = F.Case("short", q, qoff, t, U.offsets([0, 1]))
    _check_case(ctx, c, 2)
    idx, dist = _f32_device(ctx, c, 2, extra=0)
    assert (idx[:5] == -1).all() and np.isposinf(dist[:5]).all()
    assert (idx[5:] == [0, -1]).all() and np.isposinf(dist[5:, 1]).all() and np.isfinite(dist[5:, 0]).all()
    m, moff, _, _ = B._ratio_device(ctx, siftgpu, idx, dist, qoff, len(q), 1.0, extra=8)
    assert moff.tolist() == [0, 0, 0] and (m.view(np.int32) == -77).all()
    for nt in (0, 1):
        hi, hd = ctx.knnMatchL2SqrF32(q, t[:nt], 2)
        assert (hi[:, nt:] == -1).all() and np.isposinf(hd[:, nt:]).all() and (hi[:, :nt] == 0).all()


def test_gpu_l2_f32_consecutive_frames_aliased(ctx):
    """d_train = d_query, d_t_offsets = d_q_offsets + 1: frame b against frame b + 1."""
    rng = np.random.default_rng(147)
    off = U.offsets([130, 0, 65, 257, 3])
    d = F.rows(rng, int(off[-1]))
    c = F.Case("aliased", d, off[:-1], d, off[1:])
    assert (c.idx[:130] == -1).all()          # frame 0 searches the empty frame 1
    a = F.Case("aliased", d, off, d, None)    # the device reads both offset arrays from `off`
    idx, dist = _f32_device(ctx, a, 2, train_is_query=True, toff_ptr_from_q=True)
    B._check_live(idx, dist, c.idx, c.dist, c.qoff, c.q_cap, "aliased")


# ---- dyadic rows: the byte matcher's result ------------------------------------------------
@pytest.mark.parametrize("n", range(4 + len(U.TIE_IDS)),
                         ids=["edges-shared", "edges-segmented", "extremes", "ties-segmented"] + U.TIE_IDS)
def test_gpu_l2_f32_dyadic_rows_equal_the_byte_matcher(ctx, n):
    """On rows u / 512 every product, sum and norm is an integer below 2^24 in units of
    2^-18: indices equal the byte squared-L2 matcher's on u and dist * 2^18 its dist."""
    u = F.dyadic_sources()[n]

    class C:    # the same call on the float form of the rows
        name, qoff, toff, q_cap, t_cap = u.name, u.qoff, u.toff, u.q_cap, u.t_cap
        q, t = F.dyadic(u.q), F.dyadic(u.t)

    for k in (2, 1):
        fi, fd = _f32_device(ctx, C, k)
        bi, bd = _f32_device(ctx, u, k, fn=ctx.knn_match_l2sqr_u8_segmented_device)
        lo, hi = (int(v) for v in U.clamped([u.qoff[0], u.qoff[-1]], u.q_cap))
        assert_bits_equal(fi, bi, f"{u.name} idx k={k}")
        assert_bits_equal(fd[lo:hi] * F.SCALE, bd[lo:hi], f"{u.name} dist * 2^18 k={k}")
        fs = fd.copy()
        fs[lo:hi] *= F.SCALE
        B._check_live(fi, fs, *u.ref(k), u.qoff, u.q_cap, f"{u.name} against the integer reference k={k}")


# ---- host forms and l2_match ---------------------------------------------------------------
def test_gpu_l2_f32_host_forms_equal_device_forms(ctx, siftgpu):
    for c in (F.edges_case(True), F.edges_case(False)):
        for k in (2, 1):
            di, dd = _f32_device(ctx, c, k, extra=0)
            hi, hd = ctx.knnMatchL2SqrF32Segmented(c.q, c.qoff, c.t, c.toff, k)
            assert_bits_equal(hi, c.ref(k)[0], f"{c.name} host idx k={k}")
            assert_bits_equal(hd, c.ref(k)[1], f"{c.name} host dist k={k}")
            lo, hi_ = int(c.qoff[0]), int(c.qoff[-1])
            assert_bits_equal(hi[lo:hi_], di[lo:hi_], f"{c.name} host idx equals device k={k}")
            assert_bits_equal(hd[lo:hi_], dd[lo:hi_], f"{c.name} host dist equals device k={k}")
    c = F.edges_case(False)
    q = c.q[c.qoff[11]:c.qoff[12]]          # 257 rows with the planted ties, unsegmented
    ridx, rdist = F.knn_ref(q, c.t, 2)
    for k in (2, 1):
        hi, hd = ctx.knnMatchL2SqrF32(q, c.t, k)
        assert_bits_equal(hi, ridx[:, :k], f"knnMatchL2SqrF32 idx k={k}")
        assert_bits_equal(hd, rdist[:, :k], f"knnMatchL2SqrF32 dist k={k}")
    for squared in (True, False):
        lists = siftgpu.l2_match(q, c.t, 2, squared=squared, ctx=ctx)
        want = rdist if squared else np.sqrt(rdist)
        assert [[m.trainIdx for m in row] for row in lists] == ridx.tolist()
        assert [[m.distance for m in row] for row in lists] == want.astype(np.float32).tolist()
        assert [m.queryIdx for row in lists for m in row] == np.repeat(np.arange(len(q)), 2).tolist()
    assert [len(r) for r in siftgpu.l2_match(q[:3], c.t[:1], 2, ctx=ctx)] == [1, 1, 1]


# ---- the flow in stream order --------------------------------------------------------------
def test_gpu_l2_f32_batch_flow_in_stream_order(ctx, siftgpu):
    """synth_images (4 x 240x320), detect_compute_batch, the float squared-L2 matcher on
    consecutive frames, the ratio stage at 0.86^2 with keypoints and the segmented
    homography, then the reverse pass and the cross-check stage: all enqueued, one
    sync.  The matcher tables equal the oracle's on the copied-back descriptors, and
    everything after them equals the same stages fed the oracle's tables."""
    import torch
    Bn, R, C, cap = 4, 240, 320, 2048
    i32, f32_ = torch.int32, torch.float32
    imgs = torch.empty((Bn, R, C), dtype=f32_, device="cuda")
    kpts = torch.zeros((cap, 7), dtype=i32, device="cuda")
    desc = torch.zeros((cap, 128), dtype=f32_, device="cuda")
    offs = torch.zeros((Bn + 1,), dtype=i32, device="cuda")
    idx = torch.full((cap, 2), -77, dtype=i32, device="cuda")
    dist = torch.full((cap, 2), -5.0, dtype=f32_, device="cuda")
    ridx = torch.full((cap, 1), -77, dtype=i32, device="cuda")
    rdist = torch.full((cap, 1), -5.0, dtype=f32_, device="cuda")
    mt = torch.full((cap, 4), -77, dtype=i32, device="cuda")
    src = torch.full((cap, 2), -5.0, dtype=f32_, device="cuda")
    dst = torch.full((cap, 2), -5.0, dtype=f32_, device="cuda")
    moff = torch.full((Bn,), -77, dtype=i32, device="cuda")
    dH = torch.full((Bn - 1, 9), -5.0, dtype=torch.float64, device="cuda")
    df = torch.full((Bn - 1,), -77, dtype=i32, device="cuda")
    xm = torch.full((cap, 4), -77, dtype=i32, device="cuda")
    xmoff = torch.full((Bn,), -77, dtype=i32, device="cuda")
    torch.cuda.synchronize()
    o0, o1 = offs.data_ptr(), offs.data_ptr() + 4
    ctx.synth_images(imgs.data_ptr(), Bn, R, C, C, R * C, 0)
    ctx.detect_compute_batch(imgs.data_ptr(), Bn, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap, o0)
    ctx.knn_match_l2sqr_f32_segmented_device(desc.data_ptr(), o0, Bn - 1, cap, desc.data_ptr(), o1, cap, 2,
                                             idx.data_ptr(), dist.data_ptr())
    ctx.ratio_matches_device(idx.data_ptr(), dist.data_ptr(), o0, Bn - 1, cap, RATIO2, kpts.data_ptr(),
                             kpts.data_ptr(), o1, mt.data_ptr(), src.data_ptr(), dst.data_ptr(), cap, moff.data_ptr())
    ctx.find_homography_segmented_device(src.data_ptr(), dst.data_ptr(), moff.data_ptr(), Bn - 1, cap, dH.data_ptr(),
                                         df.data_ptr(), None)
    ctx.knn_match_l2sqr_f32_segmented_device(desc.data_ptr(), o1, Bn - 1, cap, desc.data_ptr(), o0, cap, 1,
                                             ridx.data_ptr(), rdist.data_ptr())
    ctx.cross_check_matches_device(idx.data_ptr(), dist.data_ptr(), 2, o0, Bn - 1, cap, ridx.data_ptr(), 1, o1, cap,
                                   0.0, None, None, xm.data_ptr(), None, None, cap, xmoff.data_ptr())
    ctx.sync()
    o = offs.cpu().numpy()
    n = int(o[-1])
    assert 0 < n <= cap and (np.diff(o) > 0).all()
    kp = kpts.cpu().numpy().view(siftgpu.KEYPOINT_DTYPE).reshape(-1)
    d = desc.cpu().numpy()
    oi, od = F.seg_ref(d, o[:-1], d, o[1:], 2, q_cap=cap, t_cap=cap)
    B._check_live(idx.cpu().numpy(), dist.cpu().numpy(), oi, od, o[:-1], cap, "consecutive frames")
    ori, ord_ = F.seg_ref(d, o[1:], d, o[:-1], 1, q_cap=cap, t_cap=cap)
    B._check_live(ridx.cpu().numpy(), rdist.cpu().numpy(), ori, ord_, o[1:], cap, "reverse pass")
    # the ratio stage and the homography, fed the oracle's table
    rec, rmoff, rsrc, rdst = B._ref_ratio(oi, od, o[:-1], cap, RATIO2, kp, kp, o[1:])
    m = mt.cpu().numpy().view(siftgpu.MATCH_DTYPE).reshape(-1)
    k = len(rec)
    assert k >= 3 * 4
    assert_bits_equal(moff.cpu().numpy(), rmoff, "moff")
    assert_bits_equal(m[:k], B._rec_array(siftgpu, rec), "records")
    assert_bits_equal(src.cpu().numpy()[:k], rsrc, "src_xy")
    assert_bits_equal(dst.cpu().numpy()[:k], rdst, "dst_xy")
    assert (m[k:].view(np.int32) == -77).all()
    res = ctx.findHomographyBatch(rsrc, rdst, rmoff)
    H, found = dH.cpu().numpy(), df.cpu().numpy()
    for b in range(Bn - 1):
        h, _ = res[b]
        assert found[b] == (h is not None)
        assert H[b].tobytes() == (np.zeros(9) if h is None else h.reshape(9)).tobytes(), f"H of segment {b}"
    # the cross-check leg against the join of the oracle's two tables
    ref = X.stage_ref(oi, od, ori, o[:-1], o[1:], cap, cap, 0.0)
    xr = xm.cpu().numpy().view(siftgpu.MATCH_DTYPE).reshape(-1)
    kx = len(ref[0])
    assert kx > 0
    assert_bits_equal(xmoff.cpu().numpy(), ref[1], "cross-check m_offsets")
    assert_bits_equal(xr[:kx], ref[0], "cross-check records")
    assert (xr[kx:].view(np.int32) == -77).all()


# ---- sanity of the rule itself -------------------------------------------------------------
def test_gpu_l2_f32_rule_against_float64_on_real_descriptors(ctx):
    """Real descriptors of the golden images against a float64 sum (q - t)^2:
    |d - d64| <= B = 2 gamma_130 (nq + nt), and the indices are the float64 ranking's on
    every row whose 1st-2nd and 2nd-3rd gaps exceed 2 B; at most 1 % of rows exempt."""
    import test_match_l2_f32 as T
    for name, q, t in T.real_pairs():
        idx, dist = ctx.knnMatchL2SqrF32(q, t, 2)
        exempt = T.check_against_float64(name, q, t, idx, dist)
        assert exempt <= 0.01 * len(q), (name, exempt, len(q))


# ---- values: signs, cancellation, subnormals, overflow -------------------------------------
VALUE_CASES = {"signed": F.signed_case, "cancel": F.cancel_case, "subnormal": F.subnormal_case,
               "overflow": F.overflow_case}


@pytest.mark.parametrize("k", [2, 1])
@pytest.mark.parametrize("seg_train", [False, True], ids=["shared", "segmented"])
@pytest.mark.parametrize("name", list(VALUE_CASES))
def test_gpu_l2_f32_value_cases(ctx, name, seg_train, k):
    """Signed rows with negated and zero rows; near-copies whose fmaf(-2, dot, s) is rounding
    noise either side of 0; subnormal elements, products, norms and distances; finite rows
    whose distances are +inf and NaN.  The special rows sit either side of the half-wave,
    tile, step and split seams, on the last row of a tail step and on the last query of
    segments of 33 and 65.  No NaN reaches the result; idx and dist equal the oracle's bit
    for bit; rows outside the live range are untouched."""
    c = VALUE_CASES[name](seg_train)
    ridx, rdist = c.ref(k)
    assert not np.isnan(rdist).any()
    idx, dist = _f32_device(ctx, c, k)
    live = slice(int(c.qoff[0]), int(c.qoff[-1]))
    bad = np.nonzero(((idx[live] != ridx[live]) | (dist[live].view(np.int32) != rdist[live].view(np.int32))).any(axis=1))[0]
    for r in bad[:8]:
        print(f"{c.name} k={k} row {r}: idx {idx[r].tolist()} dist {dist[r].tolist()}, "
              f"oracle {ridx[r].tolist()} {rdist[r].tolist()}")
    print(f"{c.name} k={k}: {len(bad)} of {live.stop - live.start} rows differ from the oracle")
    assert not np.isnan(dist[live]).any(), c.name
    B._check_live(idx, dist, ridx, rdist, c.qoff, c.q_cap, f"{c.name} k={k}")


@pytest.mark.parametrize("name", ["cancel", "overflow"])
def test_gpu_l2_f32_value_cases_host_forms_and_roots(ctx, siftgpu, name):
    """The host segmented form and the one-segment form equal the device form, and
    l2_match(squared=False) returns the float32 square roots of the oracle's distances: 0
    stays 0, an entry at -1 / +inf is no match and its root in the table stays +inf."""
    for seg_train in (False, True):
        c = VALUE_CASES[name](seg_train)
        for k in (2, 1):
            di, dd = _f32_device(ctx, c, k, extra=0)
            hi, hd = ctx.knnMatchL2SqrF32Segmented(c.q, c.qoff, c.t, c.toff, k)
            assert_bits_equal(hi, di, f"{c.name} host idx equals device k={k}")
            assert_bits_equal(hd, dd, f"{c.name} host dist equals device k={k}")
            assert_bits_equal(hi, c.ref(k)[0], f"{c.name} host idx k={k}")
            assert_bits_equal(hd, c.ref(k)[1], f"{c.name} host dist k={k}")
        zeros = missing = 0
        for b, q0, qs, ts in F.seg_tables(c):
            ridx, rdist = c.idx[q0:q0 + len(qs)], c.dist[q0:q0 + len(qs)]
            oi, od = ctx.knnMatchL2SqrF32(qs, ts, 2)
            assert_bits_equal(oi, ridx, f"{c.name}[{b}] one-segment idx")
            assert_bits_equal(od, rdist, f"{c.name}[{b}] one-segment dist")
            root = np.sqrt(rdist)
            assert root.dtype == np.float32 and (root[rdist == 0].view(np.int32) == 0).all()
            assert np.isposinf(root[ridx < 0]).all() and np.isfinite(root[ridx >= 0]).all()
            lists = siftgpu.l2_match(qs, ts, 2, squared=False, ctx=ctx)
            assert [[m.trainIdx for m in row] for row in lists] == [[int(i) for i in r if i >= 0] for r in ridx]
            assert [[m.distance for m in row] for row in lists] == \
                [[float(d) for i, d in zip(ri, rd) if i >= 0] for ri, rd in zip(ridx, root)]
            assert [[m.queryIdx for m in row] for row in lists] == [[n] * int((r >= 0).sum()) for n, r in enumerate(ridx)]
            zeros, missing = zeros + int((rdist == 0).sum()), missing + int((ridx < 0).sum())
        assert zeros >= 1 and (name == "cancel" or not seg_train or missing >= 8)


def test_gpu_l2_f32_overflow_ratio_stage_in_stream_order(ctx, siftgpu):
    """The matcher on overflow_case and the ratio stage at 0.86^2 on its tables, enqueued one
    behind the other with one sync: no query whose second neighbour is -1 is kept (its d1 <=
    ratio * +inf holds as numbers), and the records are those of the oracle's tables."""
    import torch
    c = F.overflow_case(True)
    n = c.q_cap
    dq, dqo, dt, dto = B._dev(c.q), B._dev(c.qoff), B._dev(c.t), B._dev(c.toff)
    di = torch.full((n, 2), U.SENT_I, dtype=torch.int32, device="cuda")
    dd = torch.full((n, 2), U.SENT_D, dtype=torch.float32, device="cuda")
    dm = torch.full((n + 8, 4), -77, dtype=torch.int32, device="cuda")
    ds = torch.full((n + 8, 2), -5.0, dtype=torch.float32, device="cuda")
    dst = torch.full((n + 8, 2), -5.0, dtype=torch.float32, device="cuda")
    dmo = torch.full((len(c.qoff),), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nseg = len(c.qoff) - 1
    ctx.knn_match_l2sqr_f32_segmented_device(dq.data_ptr(), dqo.data_ptr(), nseg, n, dt.data_ptr(), dto.data_ptr(),
                                             c.t_cap, 2, di.data_ptr(), dd.data_ptr())
    ctx.ratio_matches_device(di.data_ptr(), dd.data_ptr(), dqo.data_ptr(), nseg, n, RATIO2, None, None, None,
                             dm.data_ptr(), ds.data_ptr(), dst.data_ptr(), n, dmo.data_ptr())
    ctx.sync()
    idx, dist = di.cpu().numpy(), dd.cpu().numpy()
    assert not np.isnan(dist).any()
    assert_bits_equal(idx, c.idx, "idx")
    assert_bits_equal(dist, c.dist, "dist")
    rec, rmoff, _, _ = B._ref_ratio(c.idx, c.dist, c.qoff, n, RATIO2)
    m = dm.cpu().numpy().view(siftgpu.MATCH_DTYPE).reshape(-1)
    kept = len(rec)
    one = (c.idx[:, 0] >= 0) & (c.idx[:, 1] < 0)
    assert kept >= 1 and one.sum() >= 8
    assert_bits_equal(dmo.cpu().numpy(), rmoff, "m_offsets")
    assert_bits_equal(m[:kept], B._rec_array(siftgpu, rec), "records")
    assert (m[kept:].view(np.int32) == -77).all()
    for r in m[:kept]:
        row = int(c.qoff[r["segment"]]) + int(r["query"])
        assert c.idx[row, 1] >= 0 and not one[row]
