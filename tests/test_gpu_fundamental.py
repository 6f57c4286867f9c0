"""The segmented fundamental-matrix estimate on the GPU (-m gpu): every F double,
every found flag and every mask byte equals fundamental_oracle.py run per
segment, and the host sift_find_fundamental run per segment, bit for bit.
Inputs and expected values are fundamental_inputs.py's (one call, computed once
per process); the outputs are sentinel-filled, so a write outside the segments'
range shows."""
import numpy as np
import pytest

from conftest import assert_bits_equal

import affine_inputs as AI
import fundamental_inputs as I
import fundamental_oracle as FO
import homography_batch_inputs as HI

pytestmark = pytest.mark.gpu
F_SENT, FOUND_SENT, M_SENT = -7.0, -77, 0xEE


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fund_device(ctx, src, dst, moff, m_cap, thr=3.0, max_iters=1000, confidence=0.99, with_mask=True, extra=64):
    """Device form into sentinel-filled outputs: F [n_seg + 2, 9], found [n_seg + 2], mask [rows + extra]."""
    import torch
    rows = len(src)
    nseg = len(moff) - 1
    ds, dd, dmo = _dev(np.asarray(src, np.float32).reshape(-1, 2)), _dev(np.asarray(dst, np.float32).reshape(-1, 2)), \
        _dev(np.asarray(moff, np.int32))
    dF = torch.full((nseg + 2, 9), F_SENT, dtype=torch.float64, device="cuda")
    df = torch.full((nseg + 2,), FOUND_SENT, dtype=torch.int32, device="cuda")
    dm = torch.full((rows + extra,), M_SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                  # the context's stream does not wait for torch's
    ctx.find_fundamental_segmented_device(ds.data_ptr(), dd.data_ptr(), dmo.data_ptr(), nseg, m_cap, dF.data_ptr(),
                                          df.data_ptr(), dm.data_ptr() if with_mask else None, thr, max_iters,
                                          confidence)
    ctx.sync()
    return dF.cpu().numpy(), df.cpu().numpy(), dm.cpu().numpy()


def _check(out, exp, moff, m_cap, what):
    """Segments equal the expected values; F / found rows past n_seg and mask bytes outside
    [clamp(moff[0]), clamp(moff[-1])) still hold their sentinels."""
    F, found, mask = out
    eF, ef, em = exp
    nseg = len(moff) - 1
    assert_bits_equal(found[:nseg], ef, what + " found")
    for b in range(nseg):
        assert F[b].tobytes() == eF[b].tobytes(), f"{what}: F of segment {b}: {F[b]} != {eF[b]}"
    lo, hi = (int(v) for v in np.clip([moff[0], moff[-1]], 0, m_cap))
    assert_bits_equal(mask[lo:hi], em[lo:hi], what + " mask")
    assert (F[nseg:] == F_SENT).all() and (found[nseg:] == FOUND_SENT).all(), what + ": rows past n_segments written"
    dead = np.r_[0:lo, hi:len(mask)]
    assert (mask[dead] == M_SENT).all(), what + ": mask bytes outside the segments' range written"


def _host_per_segment(siftgpu, c):
    nseg = len(c.labels)
    F = np.zeros((nseg, 9), np.float64)
    found = np.zeros(nseg, np.int32)
    mask = np.zeros(c.m_cap, np.uint8)
    for b in range(nseg):
        lo, hi = c.bounds(b)
        f, m = siftgpu.findFundamentalMat(c.src[lo:hi], c.dst[lo:hi], c.thr, c.max_iters, c.confidence)
        F[b], found[b] = FO.as_f(None if f is None else f.reshape(9)), f is not None
        mask[lo:hi] = m
    return F, found, mask


def test_gpu_bitexact_per_segment(ctx, siftgpu):
    """The one call of fundamental_inputs.gpu_call(), with and without a mask buffer, against the
    oracle and the host path; then the host-buffer form against the device form."""
    c = I.gpu_call()
    eF, ef, em, _ = I.expected()
    out = _fund_device(ctx, c.src, c.dst, c.moff, c.m_cap, c.thr, c.max_iters, c.confidence)
    for b, label in enumerate(c.labels):
        print(f"{label}: n={c.size(b)} found={out[1][b]} (oracle {ef[b]})")
    _check(out, (eF, ef, em), c.moff, c.m_cap, "fundamental")
    _check(out, _host_per_segment(siftgpu, c), c.moff, c.m_cap, "fundamental against the host path")
    assert (out[2][c.m_cap:] == M_SENT).all()
    assert ef[c.index("nan") - 1] == ef[c.index("nan") + 1] == 1       # the poisoned segment's neighbours
    found = out[1][:len(c.labels)].astype(bool)
    assert np.isfinite(out[0][:len(c.labels)][found]).all()
    # without a mask buffer: the same F and found
    F2, f2, m2 = _fund_device(ctx, c.src, c.dst, c.moff, c.m_cap, c.thr, c.max_iters, c.confidence, with_mask=False)
    assert F2.tobytes() == out[0].tobytes() and f2.tobytes() == out[1].tobytes() and (m2 == M_SENT).all()
    # the host-buffer form: rows up to m_cap
    res = ctx.findFundamentalBatch(c.src[:c.m_cap], c.dst[:c.m_cap], c.moff, c.thr, c.max_iters, c.confidence)
    assert len(res) == len(c.labels)
    for b, (f, m) in enumerate(res):
        lo, hi = c.bounds(b)
        assert (f is None) == (out[1][b] == 0), b
        if f is not None:
            assert f.tobytes() == out[0][b].tobytes(), f"host form F of segment {b}"
        assert_bits_equal(m, out[2][lo:hi], f"host form mask of segment {b}")


def test_gpu_invalid_parameters_give_none(ctx):
    c = I.gpu_call()
    n = len(c.labels)
    for max_iters, conf in ((0, 0.99), (1000, 0.0), (1000, 1.0), (-3, 0.5)):
        F, found, mask = _fund_device(ctx, c.src, c.dst, c.moff, c.m_cap, 3.0, max_iters, conf)
        assert (found[:n] == 0).all() and (F[:n] == 0).all() and (mask[:c.m_cap] == 0).all()
        assert (F[n:] == F_SENT).all() and (found[n:] == FOUND_SENT).all() and (mask[c.m_cap:] == M_SENT).all()


def test_gpu_entry_point_rules(ctx, siftgpu):
    """With a live context: nothing to do returns SIFT_OK whatever the buffers;
    a null required buffer is SIFT_E_INVALID with a message naming it."""
    L, h = siftgpu.lib(), ctx.h
    E = siftgpu.SIFT_E_INVALID
    t = _dev(np.zeros(64, np.float64))
    p = t.data_ptr()
    dev = lambda *a: L.sift_find_fundamental_segmented_device(h, *a[:5], 3.0, 1000, 0.99, *a[5:])  # noqa: E731
    assert dev(None, None, None, 0, 5, None, None, None) == 0
    assert dev(None, None, None, 3, 0, None, None, None) == 0
    assert L.sift_find_fundamental_segmented(h, None, None, None, 0, 0, 3.0, 1000, 0.99, None, None, None) == 0
    for s, d, o, F, f in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p),
                          (p, p, p, p, None)):
        assert dev(s, d, o, 1, 4, F, f, None) == E
        assert b"null" in L.sift_last_error(h)
    assert dev(p, p, p, -1, 4, p, p, None) == E


def test_gpu_homography_and_affine_unchanged_by_fundamental_calls(ctx):
    """The bytes of one homography_batch_inputs call and one affine call on the
    same context are the same before and after fundamental calls (device and host
    form): the shared scratch block is not corrupted, and the Jacobi they share
    gives the homography the bits it gave."""
    import torch
    hc = HI.calls()[1]
    ac = AI.gpu_call(0)

    def homog():
        ds, dd, dmo = _dev(hc.src), _dev(hc.dst), _dev(hc.moff)
        n = len(hc.sizes)
        dH = torch.full((n, 9), F_SENT, dtype=torch.float64, device="cuda")
        df = torch.full((n,), FOUND_SENT, dtype=torch.int32, device="cuda")
        dm = torch.full((len(hc.src),), M_SENT, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.find_homography_segmented_device(ds.data_ptr(), dd.data_ptr(), dmo.data_ptr(), n, len(hc.src),
                                             dH.data_ptr(), df.data_ptr(), dm.data_ptr(), hc.thr, hc.max_iters,
                                             hc.confidence)
        ctx.sync()
        return dH.cpu().numpy().tobytes(), df.cpu().numpy().tobytes(), dm.cpu().numpy().tobytes()

    def affine():
        ds, dd, dmo = _dev(ac.src), _dev(ac.dst), _dev(ac.moff)
        n = len(ac.labels)
        dH = torch.full((n, 9), F_SENT, dtype=torch.float64, device="cuda")
        df = torch.full((n,), FOUND_SENT, dtype=torch.int32, device="cuda")
        dm = torch.full((len(ac.src),), M_SENT, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.estimate_affine_segmented_device(ds.data_ptr(), dd.data_ptr(), dmo.data_ptr(), n, ac.m_cap, 0,
                                             dH.data_ptr(), df.data_ptr(), dm.data_ptr(), ac.thr, ac.max_iters,
                                             ac.confidence)
        ctx.sync()
        return dH.cpu().numpy().tobytes(), df.cpu().numpy().tobytes(), dm.cpu().numpy().tobytes()

    before_h, before_a = homog(), affine()
    eH, ef, em, _ = HI.expected()[hc.name]
    assert before_h == (eH.tobytes(), ef.tobytes(), em.tobytes())
    c = I.gpu_call()
    _fund_device(ctx, c.src, c.dst, c.moff, c.m_cap, c.thr, c.max_iters, c.confidence)
    ctx.findFundamentalBatch(c.src[:c.m_cap], c.dst[:c.m_cap], c.moff, c.thr, c.max_iters, c.confidence)
    assert homog() == before_h and affine() == before_a


def test_gpu_ratio_stage_feeds_the_fundamental_estimate(ctx, siftgpu):
    """A chain on one stream with no host value between the two calls: the outputs
    of ratio_matches_device (d_src_xy, d_dst_xy, d_m_offsets) go straight into
    find_fundamental_segmented_device.  Two segments of synthetic descriptors
    whose keypoints are the two views of fundamental_inputs.py: every query has
    its own train row as its nearest neighbour by a wide margin, so the ratio
    stage keeps every pair and the estimate finds the planted geometry."""
    import torch
    n_seg, per = 2, 40
    rng = np.random.default_rng(11)
    q_desc = rng.uniform(0, 1, (n_seg * per, 128)).astype(np.float32)
    t_desc = np.empty_like(q_desc)
    q_k = np.zeros(n_seg * per, siftgpu.KEYPOINT_DTYPE)
    t_k = np.zeros(n_seg * per, siftgpu.KEYPOINT_DTYPE)
    for b in range(n_seg):
        s, d, _ = I.data(900 + b, per, 0.0, 0.25)
        perm = rng.permutation(per)
        rows = slice(b * per, (b + 1) * per)
        td, tx, ty = np.empty((per, 128), np.float32), np.empty(per, np.float32), np.empty(per, np.float32)
        td[perm], tx[perm], ty[perm] = q_desc[rows], d[:, 0], d[:, 1]      # train row perm[i] is query i's twin
        t_desc[rows] = td
        q_k["x"][rows], q_k["y"][rows] = s[:, 0], s[:, 1]
        t_k["x"][rows], t_k["y"][rows] = tx, ty
    offs = np.arange(n_seg + 1, dtype=np.int32) * per
    cap = n_seg * per
    dq, dt, dqk, dtk, do = _dev(q_desc), _dev(t_desc), _dev(q_k.view(np.uint8)), _dev(t_k.view(np.uint8)), _dev(offs)
    idx = torch.empty((cap, 2), dtype=torch.int32, device="cuda")
    dist = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
    mt = torch.empty((cap, 4), dtype=torch.int32, device="cuda")
    sxy = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
    dxy = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
    moff = torch.empty((n_seg + 1,), dtype=torch.int32, device="cuda")
    dF = torch.full((n_seg, 9), F_SENT, dtype=torch.float64, device="cuda")
    df = torch.full((n_seg,), FOUND_SENT, dtype=torch.int32, device="cuda")
    dm = torch.full((cap,), M_SENT, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.knn_match_segmented_device(dq.data_ptr(), do.data_ptr(), n_seg, cap, dt.data_ptr(), do.data_ptr(), cap, 2,
                                   idx.data_ptr(), dist.data_ptr())
    ctx.ratio_matches_device(idx.data_ptr(), dist.data_ptr(), do.data_ptr(), n_seg, cap, 0.5, dqk.data_ptr(),
                             dtk.data_ptr(), do.data_ptr(), mt.data_ptr(), sxy.data_ptr(), dxy.data_ptr(), cap,
                             moff.data_ptr())
    ctx.find_fundamental_segmented_device(sxy.data_ptr(), dxy.data_ptr(), moff.data_ptr(), n_seg, cap, dF.data_ptr(),
                                          df.data_ptr(), dm.data_ptr())
    ctx.sync()
    mo, F, found, mask = moff.cpu().numpy(), dF.cpu().numpy(), df.cpu().numpy(), dm.cpu().numpy()
    src, dst = sxy.cpu().numpy(), dxy.cpu().numpy()
    assert mo.tolist() == offs.tolist(), "the ratio stage did not keep every planted pair"
    assert found.tolist() == [1] * n_seg
    for b in range(n_seg):
        lo, hi = int(mo[b]), int(mo[b + 1])
        hF, hm = siftgpu.findFundamentalMat(src[lo:hi], dst[lo:hi])
        assert hF.tobytes() == F[b].tobytes() and hm.tobytes() == mask[lo:hi].tobytes()
        d2, d1 = I.epipolar_distances(F[b], src[lo:hi], dst[lo:hi])
        assert mask[lo:hi].all() and max(d1.max(), d2.max()) < 3.0
