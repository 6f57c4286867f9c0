"""Relative pose and triangulation on the GPU (-m gpu): every pose, E, found flag,
count, mask byte and xyz double of the segmented device call equals
pose_oracle.py run per segment, and the host sift_recover_pose run per segment,
bit for bit.  Inputs and expected values are pose_inputs.py's (one call, computed
once per process); every output is sentinel-filled with two spare rows and 64
spare bytes, so a write outside the segments' range shows."""
import numpy as np
import pytest

from conftest import assert_bits_equal

import fundamental_inputs as FI
import pose_inputs as I
import pose_oracle as PO

pytestmark = pytest.mark.gpu
D_SENT, I_SENT, M_SENT = -7.0, -77, 0xEE


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pose_device(ctx, c, with_mask=True, k_per_segment=1, with_E=True, with_mask_out=True, with_xyz=True, thresh=None,
                 found=None):
    """Device form into sentinel-filled outputs -> dict of numpy arrays."""
    import torch
    rows, nseg = len(c.src), len(c.labels)
    ins = [_dev(c.src.reshape(-1, 2)), _dev(c.dst.reshape(-1, 2)), _dev(c.moff), _dev(c.F),
           _dev(c.found if found is None else found), _dev(c.K_src if k_per_segment else c.K_src[0]),
           _dev(c.K_dst if k_per_segment else c.K_dst[0]), _dev(c.mask)]
    keep = [t.clone() for t in (ins[3], ins[4], ins[7])]
    f64 = lambda *shape: torch.full(shape, D_SENT, dtype=torch.float64, device="cuda")  # noqa: E731
    i32 = lambda *shape: torch.full(shape, I_SENT, dtype=torch.int32, device="cuda")  # noqa: E731
    o = {"pose": f64(nseg + 2, 12), "E": f64(nseg + 2, 9), "found": i32(nseg + 2), "n_good": i32(nseg + 2),
         "mask": torch.full((rows + 64,), M_SENT, dtype=torch.uint8, device="cuda"), "xyz": f64(rows + 2, 3)}
    torch.cuda.synchronize()                  # the context's stream does not wait for torch's
    ctx.recover_pose_segmented_device(
        ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), nseg, c.m_cap, ins[3].data_ptr(), ins[4].data_ptr(),
        ins[5].data_ptr(), ins[6].data_ptr(), o["pose"].data_ptr(), o["found"].data_ptr(), o["n_good"].data_ptr(),
        k_per_segment, ins[7].data_ptr() if with_mask else None, c.thresh if thresh is None else thresh,
        o["E"].data_ptr() if with_E else None, o["mask"].data_ptr() if with_mask_out else None,
        o["xyz"].data_ptr() if with_xyz else None)
    ctx.sync()
    for t, k in zip((ins[3], ins[4], ins[7]), keep):     # F, found and the mask read are only read
        assert torch.equal(t.view(torch.uint8), k.view(torch.uint8))
    return {k: v.cpu().numpy() for k, v in o.items()}


def _check(out, exp, c, what, skip=()):
    """Segments equal the expected values; per-segment rows past n_seg and per-pair rows outside
    [clamp(moff[0]), clamp(moff[-1])) still hold their sentinels.  skip: outputs passed as NULL."""
    nseg = len(c.labels)
    lo, hi = (int(v) for v in np.clip([c.moff[0], c.moff[-1]], 0, c.m_cap))
    assert_bits_equal(out["found"][:nseg], exp["found"], what + " found")
    assert_bits_equal(out["n_good"][:nseg], exp["n_good"], what + " n_good")
    for b in range(nseg):
        assert out["pose"][b].tobytes() == exp["pose"][b].tobytes(), f"{what}: pose of segment {b} ({c.labels[b]})"
        if "E" not in skip:
            assert out["E"][b].tobytes() == exp["E"][b].tobytes(), f"{what}: E of segment {b} ({c.labels[b]})"
    for k, sent in (("pose", D_SENT), ("E", D_SENT), ("found", I_SENT), ("n_good", I_SENT)):
        assert (out[k][0 if k in skip else nseg:] == sent).all(), f"{what}: {k} rows past n_segments written"
    if "mask" in skip:
        assert (out["mask"] == M_SENT).all()
    else:
        assert_bits_equal(out["mask"][lo:hi], exp["mask"][lo:hi], what + " mask")
        assert (out["mask"][np.r_[0:lo, hi:len(out["mask"])]] == M_SENT).all(), what + ": mask bytes outside written"
    if "xyz" in skip:
        assert (out["xyz"] == D_SENT).all()
    else:
        assert out["xyz"][lo:hi].tobytes() == exp["xyz"][lo:hi].tobytes(), what + " xyz"
        assert (out["xyz"][np.r_[0:lo, hi:len(out["xyz"])]] == D_SENT).all(), what + ": xyz rows outside written"


def _host_per_segment(siftgpu, c):
    nseg = len(c.labels)
    e = {"pose": np.zeros((nseg, 12)), "E": np.zeros((nseg, 9)), "found": np.zeros(nseg, np.int32),
         "n_good": np.zeros(nseg, np.int32), "mask": np.zeros(c.m_cap, np.uint8), "xyz": np.zeros((c.m_cap, 3))}
    for b in range(nseg):
        lo, hi = c.bounds(b)
        if not c.found[b]:
            continue
        R, t, E, m, xyz, ng = siftgpu.recoverPose(c.F[b], c.K_src[b], c.K_dst[b], c.src[lo:hi], c.dst[lo:hi],
                                                  c.mask[lo:hi], c.thresh)
        if R is not None:
            e["pose"][b], e["E"][b], e["found"][b], e["n_good"][b] = np.c_[R, t].reshape(12), E.reshape(9), 1, ng
        e["mask"][lo:hi], e["xyz"][lo:hi] = m, xyz
    return e


@pytest.fixture(params=["default", "no_graph"])
def any_ctx(request, ctx, siftgpu):
    """The session context (default flags), and one created with SIFT_FLAG_NO_GRAPH."""
    if request.param == "default":
        yield ctx
        return
    c = siftgpu.Context(64, 64, 1, device=0, flags=siftgpu.SIFT_FLAG_NO_GRAPH)
    yield c
    c.close()


def test_gpu_bitexact_per_segment(any_ctx, siftgpu):
    """The one call of pose_inputs.gpu_call() against the oracle and the host path; then with the
    optional buffers NULL and with one calibration for all segments; then the host-buffer form."""
    ctx, c = any_ctx, I.gpu_call()
    exp = I.expected()
    out = _pose_device(ctx, c)
    for b, label in enumerate(c.labels):
        print(f"{label}: n={c.size(b)} found={out['found'][b]} n_good={out['n_good'][b]} (oracle slot {exp['slot'][b]})")
    _check(out, exp, c, "pose")
    _check(out, _host_per_segment(siftgpu, c), c, "pose against the host path")
    found = out["found"][:len(c.labels)].astype(bool)
    assert np.isfinite(out["pose"][:len(c.labels)][found]).all()
    # mask_in / mask_out / xyz / E as NULL: the remaining outputs keep the same bytes
    bare = _pose_device(ctx, c, with_E=False, with_mask_out=False, with_xyz=False)
    _check(bare, exp, c, "pose, optional outputs NULL", skip=("E", "mask", "xyz"))
    _check(_pose_device(ctx, c, with_mask=False), I.expected(False, 1), c, "pose, mask_in NULL")
    _check(_pose_device(ctx, c, k_per_segment=0), I.expected(True, 0), c, "pose, one K for all segments")
    # an invalid threshold: every segment no pose
    for thr in (0.0, -2.0, float("nan")):
        z = _pose_device(ctx, c, thresh=thr)
        n = len(c.labels)
        assert not z["found"][:n].any() and not z["pose"][:n].any() and not z["mask"][:c.m_cap].any()
    # the host-buffer form: rows up to m_cap
    res = ctx.recoverPoseBatch(c.F, c.found, c.K_src, c.K_dst, c.src[:c.m_cap], c.dst[:c.m_cap], c.moff,
                               c.mask[:c.m_cap], c.thresh)
    assert len(res) == len(c.labels)
    for b, (R, t, E, m, xyz, ng) in enumerate(res):
        lo, hi = c.bounds(b)
        assert (R is None) == (out["found"][b] == 0) and ng == out["n_good"][b], b
        if R is not None:
            assert np.c_[R, t].tobytes() == out["pose"][b].tobytes() and E.tobytes() == out["E"][b].tobytes(), b
        assert_bits_equal(m, out["mask"][lo:hi], f"host form mask of segment {b}")
        assert xyz.tobytes() == out["xyz"][lo:hi].tobytes(), f"host form xyz of segment {b}"


def test_gpu_triangulation(any_ctx):
    """The triangulation call over the same offsets, a camera pair per segment, against the oracle."""
    import torch
    ctx, c = any_ctx, I.gpu_call()
    exp, written = I.expected_xyzw()
    ds, dd, dmo = _dev(c.src.reshape(-1, 2)), _dev(c.dst.reshape(-1, 2)), _dev(c.moff)
    dPs, dPd = _dev(c.P_src), _dev(c.P_dst)
    q = torch.full((len(c.src) + 2, 4), D_SENT, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.triangulate_points_segmented_device(ds.data_ptr(), dd.data_ptr(), dmo.data_ptr(), len(c.labels), c.m_cap,
                                            dPs.data_ptr(), dPd.data_ptr(), q.data_ptr())
    ctx.sync()
    got = q.cpu().numpy()
    # bit for bit wherever the oracle's row is finite; the NaN-poisoned rows must be NaN in the same
    # places (a NaN an operation creates carries the sign bit on x86-64 and not on gfx950: the one
    # difference between the two IEEE implementations, and only in a value that is no number)
    fin = written & np.isfinite(exp).all(axis=1)
    assert fin.sum() > 1500 and got[:c.m_cap][fin].tobytes() == exp[fin].tobytes()
    bad = written & ~fin
    assert bad.any() and (np.isnan(got[:c.m_cap][bad]) == np.isnan(exp[bad])).all()
    assert (got[:c.m_cap][~written] == D_SENT).all() and (got[c.m_cap:] == D_SENT).all()


def test_gpu_entry_point_rules(ctx, siftgpu):
    """With a live context: nothing to do returns SIFT_OK whatever the buffers; a null required
    buffer, a negative count and a bad k_per_segment are SIFT_E_INVALID with a message."""
    L, h = siftgpu.lib(), ctx.h
    E = siftgpu.SIFT_E_INVALID
    p = _dev(np.zeros(256, np.float64)).data_ptr()
    pose = lambda a, nseg=1, cap=4, k=0: L.sift_recover_pose_segmented_device(  # noqa: E731
        h, a[0], a[1], a[2], nseg, cap, a[3], a[4], a[5], a[6], k, None, 50.0, a[7], None, a[8], a[9], None, None)
    assert pose([None] * 10, 0, 5) == 0 and pose([None] * 10, 3, 0) == 0
    assert L.sift_recover_pose_segmented(h, None, None, None, 0, 0, None, None, None, None, 0, None, 50.0, None, None,
                                         None, None, None, None) == 0
    for k in range(10):
        a = [p] * 10
        a[k] = None
        assert pose(a) == E and b"null" in L.sift_last_error(h), k
    assert pose([p] * 10, -1) == E and pose([p] * 10, 1, -1) == E and pose([p] * 10, k=2) == E
    tri = lambda a, nseg=1, cap=4: L.sift_triangulate_points_segmented_device(h, *a[:3], nseg, cap, *a[3:])  # noqa: E731
    assert tri([None] * 6, 0, 5) == 0 and tri([None] * 6, 3, 0) == 0
    for k in range(6):
        a = [p] * 6
        a[k] = None
        assert tri(a) == E and b"null" in L.sift_last_error(h), k
    assert tri([p] * 6, -1) == E


def test_gpu_fundamental_feeds_pose_feeds_triangulation(any_ctx, siftgpu):
    """A chain on the context stream with no synchronisation and no host value between the calls:
    find_fundamental_segmented_device -> recover_pose_segmented_device ->
    triangulate_points_segmented_device.  The result equals the same chain through the host forms,
    and the bytes of d_F / d_found / d_inlier_mask are what the estimate left."""
    import torch
    ctx = any_ctx
    n_seg, per = 3, 120
    pairs = [FI.data(60 + b, per, 0.3, 0.25)[:2] for b in range(n_seg)]
    src, dst = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    offs = np.arange(n_seg + 1, dtype=np.int32) * per
    cap = n_seg * per
    K = FI.K.reshape(9)
    eye = np.tile(np.array(PO.IDENTITY_CAMERA), (n_seg, 1))
    ds, dd, dmo, dK, dI = _dev(src), _dev(dst), _dev(offs), _dev(K), _dev(eye)
    dF = torch.full((n_seg, 9), D_SENT, dtype=torch.float64, device="cuda")
    df = torch.full((n_seg,), I_SENT, dtype=torch.int32, device="cuda")
    dm = torch.full((cap,), M_SENT, dtype=torch.uint8, device="cuda")
    pose = torch.full((n_seg, 12), D_SENT, dtype=torch.float64, device="cuda")
    pf = torch.full((n_seg,), I_SENT, dtype=torch.int32, device="cuda")
    ng = torch.full((n_seg,), I_SENT, dtype=torch.int32, device="cuda")
    mo = torch.full((cap,), M_SENT, dtype=torch.uint8, device="cuda")
    xyz = torch.full((cap, 3), D_SENT, dtype=torch.float64, device="cuda")
    q = torch.full((cap, 4), D_SENT, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.find_fundamental_segmented_device(ds.data_ptr(), dd.data_ptr(), dmo.data_ptr(), n_seg, cap, dF.data_ptr(),
                                          df.data_ptr(), dm.data_ptr())
    ctx.recover_pose_segmented_device(ds.data_ptr(), dd.data_ptr(), dmo.data_ptr(), n_seg, cap, dF.data_ptr(),
                                      df.data_ptr(), dK.data_ptr(), dK.data_ptr(), pose.data_ptr(), pf.data_ptr(),
                                      ng.data_ptr(), 0, dm.data_ptr(), 50.0, None, mo.data_ptr(), xyz.data_ptr())
    ctx.triangulate_points_segmented_device(ds.data_ptr(), dd.data_ptr(), dmo.data_ptr(), n_seg, cap, dI.data_ptr(),
                                            pose.data_ptr(), q.data_ptr())
    ctx.sync()
    F, found, mask = dF.cpu().numpy(), df.cpu().numpy(), dm.cpu().numpy()
    for b in range(n_seg):
        lo, hi = int(offs[b]), int(offs[b + 1])
        hF, hm = siftgpu.findFundamentalMat(src[lo:hi], dst[lo:hi])
        assert found[b] == 1 and hF.tobytes() == F[b].tobytes() and hm.tobytes() == mask[lo:hi].tobytes()  # unchanged
        R, t, E, m, p3, g = siftgpu.recoverPose(hF, K, K, src[lo:hi], dst[lo:hi], hm)
        assert R is not None and pf.cpu().numpy()[b] == 1 and ng.cpu().numpy()[b] == g > 60
        assert np.c_[R, t].tobytes() == pose.cpu().numpy()[b].tobytes()
        assert m.tobytes() == mo.cpu().numpy()[lo:hi].tobytes() and p3.tobytes() == xyz.cpu().numpy()[lo:hi].tobytes()
        hq = siftgpu.triangulatePoints(PO.IDENTITY_CAMERA, np.c_[R, t], src[lo:hi], dst[lo:hi])
        assert hq.tobytes() == q.cpu().numpy()[lo:hi].tobytes()
        assert np.abs(R - FI.R_TRUE).max() < 2e-2
