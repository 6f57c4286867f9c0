"""Absolute pose (PnP RANSAC over P3P) on the GPU (-m gpu): every pose, found flag,
inlier count and mask byte of the segmented device call equals pnp_oracle.py run
per segment, and the host sift_solve_pnp run per segment, bit for bit.  Inputs
and expected values are pnp_inputs.py's (one call of 16 segments, computed once
per process); every output is sentinel-filled with two spare rows and 64 spare
bytes, so a write outside the segments' range shows.  Then the chain fundamental
-> pose recovery -> PnP on one stream against the host forms chained the same
way."""
import numpy as np
import pytest

from conftest import assert_bits_equal

import fundamental_inputs as FI
import pnp_inputs as I

pytestmark = pytest.mark.gpu
D_SENT, I_SENT, M_SENT = -7.0, -77, 0xEE


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pnp_device(ctx, c, with_row_mask=True, k_per_segment=1, with_mask_out=True, iters=None, conf=None):
    """Device form into sentinel-filled outputs -> dict of numpy arrays."""
    import torch
    rows, nseg = len(c.X), len(c.labels)
    ins = [_dev(c.X), _dev(c.xy), _dev(c.moff), _dev(c.K if k_per_segment else c.K[0]), _dev(c.mask)]
    keep = [t.clone() for t in ins]
    o = {"pose": torch.full((nseg + 2, 12), D_SENT, dtype=torch.float64, device="cuda"),
         "found": torch.full((nseg + 2,), I_SENT, dtype=torch.int32, device="cuda"),
         "n_inliers": torch.full((nseg + 2,), I_SENT, dtype=torch.int32, device="cuda"),
         "mask": torch.full((rows + 64,), M_SENT, dtype=torch.uint8, device="cuda")}
    torch.cuda.synchronize()                  # the context's stream does not wait for torch's
    ctx.solve_pnp_segmented_device(
        ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), nseg, c.m_cap, ins[3].data_ptr(),
        o["pose"].data_ptr(), o["found"].data_ptr(), o["n_inliers"].data_ptr(), k_per_segment,
        ins[4].data_ptr() if with_row_mask else None, c.thr, c.iters if iters is None else iters,
        c.conf if conf is None else conf, o["mask"].data_ptr() if with_mask_out else None)
    ctx.sync()
    for t, k in zip(ins, keep):               # the inputs are only read
        assert torch.equal(t.view(torch.uint8), k.view(torch.uint8))
    return {k: v.cpu().numpy() for k, v in o.items()}


def _same_pose(got, exp):
    """Bit for bit; a NaN a kernel creates is compared as NaN in the same places (the sign of a
    created NaN is the one difference between x86-64 and gfx950)."""
    if np.isnan(exp).any():
        return (np.isnan(got) == np.isnan(exp)).all() and got[~np.isnan(exp)].tobytes() == exp[~np.isnan(exp)].tobytes()
    return got.tobytes() == exp.tobytes()


def _check(out, exp, c, what, skip_mask=False):
    """Segments equal the expected values; per-segment rows past n_seg and bytes outside the
    segments still hold their sentinels."""
    nseg = len(c.labels)
    assert_bits_equal(out["found"][:nseg], exp["found"], what + " found")
    assert_bits_equal(out["n_inliers"][:nseg], exp["n_inliers"], what + " n_inliers")
    for b in range(nseg):
        assert _same_pose(out["pose"][b], exp["pose"][b]), f"{what}: pose of segment {b} ({c.labels[b]})"
    for k, sent in (("pose", D_SENT), ("found", I_SENT), ("n_inliers", I_SENT)):
        assert (out[k][nseg:] == sent).all(), f"{what}: {k} rows past n_segments written"
    if skip_mask:
        assert (out["mask"] == M_SENT).all()
        return
    w = exp["written"]
    assert_bits_equal(out["mask"][:c.m_cap][w], exp["mask"][w], what + " mask")
    assert (out["mask"][:c.m_cap][~w] == M_SENT).all() and (out["mask"][c.m_cap:] == M_SENT).all(), \
        what + ": mask bytes outside the segments written"


def _host_per_segment(siftgpu, c, with_row_mask=True, k_per_segment=1):
    nseg = len(c.labels)
    e = {"pose": np.zeros((nseg, 12)), "found": np.zeros(nseg, np.int32), "n_inliers": np.zeros(nseg, np.int32),
         "mask": np.zeros(c.m_cap, np.uint8), "written": np.zeros(c.m_cap, bool)}
    for b in range(nseg):
        lo, hi = c.bounds(b)
        R, t, m, ni = siftgpu.solvePnPRansac(c.X[lo:hi], c.xy[lo:hi], c.K[b if k_per_segment else 0], c.thr, c.iters,
                                             c.conf, c.mask[lo:hi] if with_row_mask else None)
        if R is not None:
            e["pose"][b], e["found"][b], e["n_inliers"][b] = np.c_[R, t].reshape(12), 1, ni
        e["mask"][lo:hi] = m
        e["written"][lo:hi] = True
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
    """The one call of pnp_inputs.gpu_call() against the oracle and the host path; then with the
    optional buffers NULL and with one calibration for all segments; invalid RANSAC parameters; then
    the host-buffer form."""
    ctx, c = any_ctx, I.gpu_call()
    exp = I.expected()
    out = _pnp_device(ctx, c)
    for b, label in enumerate(c.labels):
        print(f"{label}: n={c.size(b)} found={out['found'][b]} n_inliers={out['n_inliers'][b]} "
              f"(oracle {exp['found'][b]} {exp['n_inliers'][b]}, {exp['iters'][b]} iterations)")
    _check(out, exp, c, "pnp")
    host = _host_per_segment(siftgpu, c)
    _check(out, host, c, "pnp against the host path")
    nseg = len(c.labels)
    found = out["found"][:nseg].astype(bool)
    assert np.isfinite(out["pose"][:nseg][found]).all()
    # d_inlier_mask NULL: the remaining outputs keep the same bytes; d_row_mask NULL; one K for all
    _check(_pnp_device(ctx, c, with_mask_out=False), exp, c, "pnp, inlier mask NULL", skip_mask=True)
    _check(_pnp_device(ctx, c, with_row_mask=False), _host_per_segment(siftgpu, c, with_row_mask=False), c,
           "pnp, row mask NULL")
    one = _pnp_device(ctx, c, k_per_segment=0)
    _check(one, _host_per_segment(siftgpu, c, k_per_segment=0), c, "pnp, one K for all segments")
    assert one["found"][c.index("singular_K")] == 1 and out["found"][c.index("singular_K")] == 0
    # max_iters < 1 or a confidence outside (0, 1): every segment found = 0
    for iters, conf in ((0, 0.99), (-3, 0.99), (100, 0.0), (100, 1.0), (100, float("nan"))):
        z = _pnp_device(ctx, c, iters=iters, conf=conf)
        assert not z["found"][:nseg].any() and not z["pose"][:nseg].any() and not z["n_inliers"][:nseg].any()
        assert not z["mask"][:c.m_cap][exp["written"]].any() and (z["mask"][c.m_cap:] == M_SENT).all()
    # the host-buffer form: rows up to m_cap
    res = ctx.solvePnPBatch(c.X[:c.m_cap], c.xy[:c.m_cap], c.moff, c.K, c.thr, c.iters, c.conf, c.mask[:c.m_cap])
    assert len(res) == nseg
    for b, (R, t, m, ni) in enumerate(res):
        lo, hi = c.bounds(b)
        assert (R is None) == (out["found"][b] == 0) and ni == out["n_inliers"][b], b
        if R is not None:
            assert np.c_[R, t].tobytes() == out["pose"][b].tobytes(), b
        assert_bits_equal(m, out["mask"][lo:hi], f"host form mask of segment {b}")


def test_gpu_entry_point_rules(ctx, siftgpu):
    """With a live context: nothing to do returns SIFT_OK whatever the buffers; a null required
    buffer, a negative count and a bad k_per_segment are SIFT_E_INVALID with a message, and nothing
    is written."""
    import torch
    L, h = siftgpu.lib(), ctx.h
    E = siftgpu.SIFT_E_INVALID
    buf = torch.full((256,), D_SENT, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    # a: xyz, xy, offsets, K, pose, found, n_inliers
    pnp = lambda a, nseg=1, cap=4, k=0: L.sift_solve_pnp_segmented_device(  # noqa: E731
        h, a[0], a[1], a[2], nseg, cap, None, a[3], k, 8.0, 100, 0.99, a[4], a[5], a[6], None)
    assert pnp([None] * 7, 0, 5) == 0 and pnp([None] * 7, 3, 0) == 0
    assert L.sift_solve_pnp_segmented(h, None, None, None, 0, 0, None, None, 0, 8.0, 100, 0.99, None, None, None,
                                      None) == 0
    for k in range(7):
        a = [p] * 7
        a[k] = None
        assert pnp(a) == E and b"null" in L.sift_last_error(h), k
    assert pnp([p] * 7, -1) == E and pnp([p] * 7, 1, -1) == E and pnp([p] * 7, k=2) == E and pnp([p] * 7, k=-1) == E
    assert L.sift_solve_pnp_segmented_device(None, p, p, p, 1, 4, None, p, 0, 8.0, 100, 0.99, p, p, p, None) == E
    ctx.sync()
    assert (buf == D_SENT).all()              # nothing was enqueued


def _chain_inputs(n_seg, per):
    """Pairs of fundamental_inputs' two views (30 % outliers, 0.25 px noise) and a planted third view
    whose row i sees point i: the 3-D points are data()'s first draws."""
    src, dst, xy3 = [], [], []
    a = 0.12
    R3 = np.array([[np.cos(a), 0, -np.sin(a)], [0, 1, 0], [np.sin(a), 0, np.cos(a)]]) @ \
        np.array([[1, 0, 0], [0, np.cos(0.05), -np.sin(0.05)], [0, np.sin(0.05), np.cos(0.05)]])
    t3 = np.array([0.9, -0.2, 0.4])
    for b in range(n_seg):
        s, d, _ = FI.data(60 + b, per, 0.3, 0.25)
        rng = np.random.default_rng(60 + b)
        P = np.c_[rng.uniform(-2, 2, per), rng.uniform(-1.5, 1.5, per), rng.uniform(4, 10, per)]
        src.append(s), dst.append(d)
        xy3.append(I.project(FI.K, P @ R3.T + t3).astype(np.float32))
    return np.concatenate(src), np.concatenate(dst), np.concatenate(xy3), R3, t3


def test_gpu_chain_fundamental_pose_pnp(any_ctx, siftgpu):
    """find_fundamental_segmented_device -> recover_pose_segmented_device (which leaves d_xyz and
    d_mask_out) -> solve_pnp_segmented_device for a planted third view, on the context stream with no
    synchronisation and no host value between the calls.  The result equals the host forms chained
    the same way, byte for byte; the bytes the first two calls left are what they leave without the
    third; and the third pose is the planted one up to the scale |t| = 1 fixes.  The pixels carry
    0.25 px of noise and F comes from RANSAC, so the planted pose is met to the 2e-2 / 5e-2 that
    test_pose.py allows its RANSAC inputs, not to the reference bound of test_pnp.py."""
    import torch
    ctx = any_ctx
    n_seg, per = 3, 120
    src, dst, xy3, R3, t3 = _chain_inputs(n_seg, per)
    offs = np.arange(n_seg + 1, dtype=np.int32) * per
    cap = n_seg * per
    K = FI.K.reshape(9)
    ds, dd, d3, dmo, dK = _dev(src), _dev(dst), _dev(xy3), _dev(offs), _dev(K)
    f64 = lambda *shape: torch.full(shape, D_SENT, dtype=torch.float64, device="cuda")  # noqa: E731
    i32 = lambda *shape: torch.full(shape, I_SENT, dtype=torch.int32, device="cuda")  # noqa: E731
    u8 = lambda *shape: torch.full(shape, M_SENT, dtype=torch.uint8, device="cuda")  # noqa: E731

    def run(with_pnp):
        o = {"F": f64(n_seg + 1, 9), "found": i32(n_seg + 1), "fmask": u8(cap + 64), "pose": f64(n_seg + 1, 12),
             "pf": i32(n_seg + 1), "ng": i32(n_seg + 1), "mo": u8(cap + 64), "xyz": f64(cap + 2, 3),
             "pose3": f64(n_seg + 1, 12), "f3": i32(n_seg + 1), "ni": i32(n_seg + 1), "m3": u8(cap + 64)}
        torch.cuda.synchronize()
        ctx.find_fundamental_segmented_device(ds.data_ptr(), dd.data_ptr(), dmo.data_ptr(), n_seg, cap,
                                              o["F"].data_ptr(), o["found"].data_ptr(), o["fmask"].data_ptr())
        ctx.recover_pose_segmented_device(ds.data_ptr(), dd.data_ptr(), dmo.data_ptr(), n_seg, cap, o["F"].data_ptr(),
                                          o["found"].data_ptr(), dK.data_ptr(), dK.data_ptr(), o["pose"].data_ptr(),
                                          o["pf"].data_ptr(), o["ng"].data_ptr(), 0, o["fmask"].data_ptr(), 50.0, None,
                                          o["mo"].data_ptr(), o["xyz"].data_ptr())
        if with_pnp:
            ctx.solve_pnp_segmented_device(o["xyz"].data_ptr(), d3.data_ptr(), dmo.data_ptr(), n_seg, cap,
                                           dK.data_ptr(), o["pose3"].data_ptr(), o["f3"].data_ptr(),
                                           o["ni"].data_ptr(), 0, o["mo"].data_ptr(), 8.0, 100, 0.99,
                                           o["m3"].data_ptr())
        ctx.sync()
        return {k: v.cpu().numpy() for k, v in o.items()}

    got, bare = run(True), run(False)
    for k in ("F", "found", "fmask", "pose", "pf", "ng", "mo", "xyz"):     # unchanged around the new call
        assert got[k].tobytes() == bare[k].tobytes(), k
    for k in ("pose3", "f3", "ni", "m3"):
        assert (bare[k] == (D_SENT if k == "pose3" else I_SENT if k in ("f3", "ni") else M_SENT)).all()
    assert (got["pose3"][n_seg:] == D_SENT).all() and (got["m3"][cap:] == M_SENT).all()
    scale = np.linalg.norm(FI.T_TRUE)
    for b in range(n_seg):
        lo, hi = int(offs[b]), int(offs[b + 1])
        hF, hm = siftgpu.findFundamentalMat(src[lo:hi], dst[lo:hi])
        R, t, E, m, p3, g = siftgpu.recoverPose(hF, K, K, src[lo:hi], dst[lo:hi], hm)
        assert R is not None and p3.tobytes() == got["xyz"][lo:hi].tobytes() and m.tobytes() == got["mo"][lo:hi].tobytes()
        Rp, tp, mp, ni = siftgpu.solvePnPRansac(p3, xy3[lo:hi], K, 8.0, 100, 0.99, m)
        assert Rp is not None and got["f3"][b] == 1 and got["ni"][b] == ni > 60
        assert np.c_[Rp, tp].tobytes() == got["pose3"][b].tobytes()
        assert mp.tobytes() == got["m3"][lo:hi].tobytes() and not (mp.astype(bool) & ~m.astype(bool)).any()
        print(f"segment {b}: n_inliers {ni}, |R - planted| {np.abs(Rp - R3).max():.3g}, "
              f"|t - planted / |T|| {np.abs(tp - t3 / scale).max():.3g}")
        assert np.abs(Rp - R3).max() < 2e-2 and np.abs(tp - t3 / scale).max() < 5e-2
