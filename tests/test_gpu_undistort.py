"""GPU tests of lens undistortion (csrc/undistort.hip) under the default flags and under
SIFT_FLAG_NO_GRAPH: the image kernel against the numpy restatement (tests/undistort_oracle.py) and
the host-buffer form, byte for byte, with sentinels in row and image padding and around the
buffers; the point kernel in one call of 16 segments against the restatement and the host path;
and the chain undistort -> fundamental matrix -> pose on one stream against the same chain through
the host forms.  (A NaN is compared as "a NaN, here": warp_inputs.canonical.)"""
import numpy as np
import pytest

import undistort_inputs as I
import undistort_oracle as UO
import warp_inputs as W
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GROUP = 8          # images a workgroup walks under a shared camera (csrc/undistort.hip kUndGroup)


@pytest.fixture(scope="module", params=["default", "no_graph"])
def uctx(request, siftgpu):
    """The context's creation limits do not apply: 8 x 8 serves every shape here."""
    flags = siftgpu.SIFT_FLAG_NO_GRAPH if request.param == "no_graph" else 0
    c = siftgpu.Context(8, 8, 1, device=0, flags=flags)
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
    if layout == "aligned":     # rows on 16-byte boundaries: the wide stores, with padding after each row
        return row + 3 * bpp, 0, (orow + 15) // 16 * 16 + 16
    if kind == "f32":           # base and pitch multiples of 4 only
        return row + 4, 4, orow + 4
    return row + 5, 1, orow + (1 if orow % 2 == 0 else 2)   # an odd pitch from an odd base


def run_device(ctx, kind, srcs, K, dist, newK, per, out_shape, layout):
    """srcs: one array per image; K / dist / newK one camera or [n] of them (per).  Returns the n
    images; asserts that no byte outside their pixels was written."""
    import torch
    pixel, ch, bpp = W.pixel_args(kind)
    n = len(srcs)
    rows, cols = srcs[0].shape[:2]
    orows, ocols = out_shape
    spitch, doff, dpitch = _layout(kind, cols, ocols, layout)
    simg = rows * spitch + 16
    dimg = orows * dpitch + (32 if layout == "aligned" else 4 if kind == "f32" else 7)
    src = np.full(simg * n, 0x5A, np.uint8)
    for b, s in enumerate(srcs):
        blk = src[b * simg:b * simg + rows * spitch].reshape(rows, spitch)
        blk[:, :cols * bpp] = np.ascontiguousarray(s).view(np.uint8).reshape(rows, cols * bpp)
    dst = torch.full((doff + n * dimg + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    src_t = _dev(src)
    K_t, d_t = _dev(np.ascontiguousarray(K, np.float64)), _dev(np.ascontiguousarray(dist, np.float64))
    N_t = None if newK is None else _dev(np.ascontiguousarray(newK, np.float64))
    ctx.undistort_batch_device(pixel, ch, src_t.data_ptr(), rows, cols, spitch, simg, K_t.data_ptr(), d_t.data_ptr(),
                               0 if N_t is None else N_t.data_ptr(), per, n, dst.data_ptr() + doff, orows, ocols,
                               dpitch, dimg)
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


def _same(got, want, what):
    assert_bits_equal(UO.canonical(got), UO.canonical(want), what)


# ---- images ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", I.PIXELS)
def test_case_table(uctx, kind):
    """Every camera of the CPU table (distortions, skew, newK, outside, den = 0, W = 0, no rule) and its
    shapes, one image a call, on aligned and unaligned destination rows."""
    for case in I.IMAGE_CASES:
        if case["kind"] != kind:
            continue
        for layout in ("aligned", "unaligned"):
            got, = run_device(uctx, kind, [case["src"]], case["K"], case["dist"], case["newK"], 0, case["out_shape"],
                              layout)
            _same(got, I.expected_image(case), f"{case['name']} ({layout})")


# tile edges: a tile is 256 columns by 8 rows
EDGE_SHAPES = [(1, 1), (7, 255), (8, 256), (9, 257), (9, 300)]


@pytest.mark.parametrize("kind", I.PIXELS)
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=[f"{r}x{c}" for r, c in EDGE_SHAPES])
def test_tile_edges_and_image_groups(uctx, kind, shape):
    """Shared camera at 1, 3, GROUP - 1, GROUP and GROUP + 1 images; an output size that differs."""
    rows, cols = shape
    K, d, _ = I.image_cameras(max(rows, 9), max(cols, 31))["all_eight"]
    srcs = [W.pixels(kind, shape, 900 + b) for b in range(GROUP + 1)]
    want = {}
    for n in (1, 3, GROUP - 1, GROUP, GROUP + 1):
        layout = "aligned" if n % 2 else "unaligned"
        got = run_device(uctx, kind, srcs[:n], K, d, None, 0, shape, layout)
        for b in range(n):
            if b not in want:
                want[b] = UO.undistort_ref(srcs[b], K, d, None, shape)
            _same(got[b], want[b], f"{kind} {shape} n {n} image {b}")
    out_shape = (rows + 2, cols + 5)
    got = run_device(uctx, kind, srcs[:3], K, d, K, 0, out_shape, "aligned")
    for b in range(3):
        _same(got[b], UO.undistort_ref(srcs[b], K, d, K, out_shape), f"{kind} {shape} to {out_shape} image {b}")


@pytest.mark.parametrize("kind", I.PIXELS)
def test_per_image_cameras_with_a_singular_one_between_two_good_ones(uctx, kind):
    shape = (9, 300)
    cams = I.image_cameras(*shape)
    names = ["barrel", "singular_K", "newK_zoom", "nan_dist", "all_eight"]
    K = np.stack([cams[n][0] for n in names])
    d = np.stack([cams[n][1] for n in names])
    N = np.stack([cams[n][0] if cams[n][2] is None else cams[n][2] for n in names])
    srcs = [W.pixels(kind, shape, 950 + b) for b in range(len(names))]
    for layout in ("aligned", "unaligned"):
        got = run_device(uctx, kind, srcs, K, d, N, 1, shape, layout)
        for b, n in enumerate(names):
            want = UO.undistort_ref(srcs[b], K[b], d[b], N[b], shape)
            assert want.any() == (n not in I.NO_RULE)
            _same(got[b], want, f"{kind} per-image {n} ({layout})")
    # d_newK = NULL with a camera per image
    got = run_device(uctx, kind, srcs, K, d, None, 1, shape, "aligned")
    for b in range(len(names)):
        _same(got[b], UO.undistort_ref(srcs[b], K[b], d[b], None, shape), f"{kind} per-image, no newK, {b}")


@pytest.mark.parametrize("kind", I.PIXELS)
def test_host_form_equals_the_device_form(uctx, kind, siftgpu):
    shape = (67, 131)
    cams = I.image_cameras(*shape)
    src = W.pixels(kind, shape, 970)
    for name in ("zero", "barrel", "newK_zoom"):
        K, d, N = cams[name]
        got = uctx.undistort(src, K, d, N, dsize=(259, 70))
        _same(got, UO.undistort_ref(src, K, d, N, (70, 259)), f"{kind} host form {name}")
    assert_bits_equal(uctx.undistort(src, *cams["zero"]), src, "zero distortion reproduces the source")
    with pytest.raises(siftgpu.SiftError):
        uctx.undistort(src, *cams["singular_K"])


def test_image_entry_point_rules(uctx, siftgpu):
    import torch
    E, SZ = siftgpu.SIFT_E_INVALID, siftgpu.SIFT_E_SIZE
    src = torch.zeros(64, dtype=torch.float32, device="cuda")
    dst = torch.full((64,), 3.0, dtype=torch.float32, device="cuda")
    K, d = _dev(np.eye(3)), _dev(np.zeros(8))

    def call(pixel=0, ch=1, s=src.data_ptr(), rows=4, cols=4, rs=0, ims=0, k=K.data_ptr(), dd=d.data_ptr(), per=0, n=1,
             o=dst.data_ptr(), orows=4, ocols=4, ors=0, oims=0):
        return uctx._L.sift_undistort_batch_device(uctx.h, pixel, ch, s, rows, cols, rs, ims, k, dd, None, per, n, o,
                                                   orows, ocols, ors, oims)
    assert call(n=0, s=None, o=None) == siftgpu.SIFT_OK            # nothing enqueued
    for kw in (dict(n=-1), dict(s=None), dict(k=None), dict(dd=None), dict(o=None), dict(rows=0), dict(ocols=0),
               dict(pixel=0, ch=3), dict(pixel=1, ch=2), dict(pixel=2), dict(per=2), dict(per=-1), dict(rs=12),
               dict(ors=8), dict(rs=18), dict(s=src.data_ptr() + 2), dict(n=2, oims=32)):
        assert call(**kw) == E, kw
    assert call(cols=(1 << 30) + 1) == SZ
    uctx.sync()
    assert (dst.cpu().numpy() == 3.0).all()
    assert call() == siftgpu.SIFT_OK
    uctx.sync()


# ---- points --------------------------------------------------------------------------------------
def _run_points(ctx, call, stride, in_place, per, with_P):
    """The one call; returns (dst rows uint8 [m_cap + 2 guard rows, stride], ok int32 [16 + 2 guards])."""
    import torch
    n = len(call.xy)
    src = I.as_rows(call.xy, stride, fill=0x5A)
    src_t = _dev(src)
    if in_place:
        dst_t = src_t
    else:
        dst_t = torch.full((call.m_cap + 2, stride), SENTINEL, dtype=torch.uint8, device="cuda")
    base = dst_t.data_ptr() + (0 if in_place else stride)            # a guard row in front
    ok = torch.full((18,), -7, dtype=torch.int32, device="cuda")
    K_t, d_t, P_t, mo = _dev(call.K), _dev(call.dist), _dev(call.P), _dev(call.moff)
    ctx.undistort_points_segmented_device(src_t.data_ptr(), base, stride, mo.data_ptr(), 16, call.m_cap,
                                          K_t.data_ptr(), d_t.data_ptr(), P_t.data_ptr() if with_P else 0, per, 5,
                                          ok.data_ptr() + 4)
    ctx.sync()
    assert n >= call.m_cap
    return dst_t.cpu().numpy(), ok.cpu().numpy()


@pytest.mark.parametrize("stride", [8, I.KP_STRIDE])
@pytest.mark.parametrize("in_place", [False, True], ids=["out_of_place", "in_place"])
def test_points_one_call_of_16_segments(uctx, stride, in_place):
    call = I.gpu_call()
    for per, with_P in ((1, True), (0, True), (1, False)):
        want, written, want_ok, twice = call.expected(per=bool(per), with_P=with_P)
        rows, ok = _run_points(uctx, call, stride, in_place, per, with_P)
        what = f"stride {stride} in_place {in_place} per {per} P {with_P}"
        assert ok[0] == -7 and ok[17] == -7 and ok[1:17].tolist() == want_ok.tolist(), what
        assert want_ok[call.index("singular_K")] == (0 if per else 1) and want_ok[call.index("nan_row")] == 1
        body = rows[:call.m_cap] if in_place else rows[1:call.m_cap + 1]
        # rows that two segments own: the same values when their cameras agree and the call is not in place
        check = written & ~twice if (in_place or per) else written
        _same(I.rows_xy(body)[check], want[check], what)
        if in_place:
            src = I.as_rows(call.xy, stride, fill=0x5A)
            assert (body[~written] == src[:call.m_cap][~written]).all(), what + ": rows outside the segments"
            assert (rows[call.m_cap:] == src[call.m_cap:]).all(), what + ": rows past m_cap"
            assert (body[:, 8:] == 0x5A).all(), what + ": the other fields of a row"
        else:
            assert (body[~written] == SENTINEL).all() and (rows[0] == SENTINEL).all() and (rows[-1] == SENTINEL).all()
            assert (body[:, 8:] == SENTINEL).all(), what + ": the other fields of a row"
    lo, hi = call.bounds(call.index("nan_row"))
    assert np.isnan(want[lo:hi]).any() and np.isfinite(want[lo + 4:hi]).all()


def test_points_host_buffer_form_and_host_path(uctx, siftgpu):
    call = I.gpu_call()
    want, written, want_ok, twice = call.expected()
    xy = call.xy[:call.m_cap].copy()
    got, ok = uctx.undistortPointsSegmented(xy, call.moff, call.K, call.dist, call.P)
    assert ok.tolist() == want_ok.tolist()
    check = written & ~twice
    _same(got[check], want[check], "host-buffer form")
    assert got[~written].tobytes() == xy[~written].tobytes()
    for b in range(16):       # the host path, per segment
        lo, hi = call.bounds(b)
        if want_ok[b]:
            h = siftgpu.undistortPoints(call.xy[lo:hi], call.K[b], call.dist[b], call.P[b])
            keep = ~twice[lo:hi]
            _same(h[keep], got[lo:hi][keep], f"host path, segment {call.labels[b]}")
    kp = np.zeros(call.m_cap, siftgpu.KEYPOINT_DTYPE)
    kp["x"], kp["y"], kp["angle"], kp["class_id"] = xy[:, 0], xy[:, 1], 33.0, 5
    gk, ok = uctx.undistortPointsSegmented(kp, call.moff, call.K[0], call.dist[0], None)
    w0 = call.expected(per=False, with_P=False)[0]
    _same(np.stack([gk["x"], gk["y"]], 1)[written], w0[written], "keypoint rows, one camera, no P")
    assert (gk["angle"] == 33.0).all() and (gk["class_id"] == 5).all() and ok.all()


def test_points_entry_point_rules(uctx, siftgpu):
    import torch
    E = siftgpu.SIFT_E_INVALID
    xy = torch.zeros((8, 2), dtype=torch.float32, device="cuda")
    out = torch.full((8, 2), 3.0, dtype=torch.float32, device="cuda")
    mo, ok = _dev(np.array([0, 8], np.int32)), torch.full((1,), -7, dtype=torch.int32, device="cuda")
    K, d = _dev(np.eye(3)), _dev(np.zeros(8))

    def call(s=xy.data_ptr(), o=out.data_ptr(), stride=8, m=mo.data_ptr(), nseg=1, cap=8, k=K.data_ptr(),
             dd=d.data_ptr(), per=0, iters=5, f=ok.data_ptr()):
        return uctx._L.sift_undistort_points_segmented_device(uctx.h, s, o, stride, m, nseg, cap, k, dd, None, per,
                                                              iters, f)
    for kw in (dict(nseg=-1), dict(cap=-1), dict(per=2), dict(iters=-1), dict(iters=101), dict(stride=4),
               dict(stride=10), dict(stride=0), dict(s=None), dict(o=None), dict(m=None), dict(k=None), dict(dd=None),
               dict(f=None), dict(s=xy.data_ptr() + 2)):
        assert call(**kw) == E, kw
    assert call(nseg=0, s=None, o=None, m=None, k=None, dd=None, f=None) == siftgpu.SIFT_OK
    uctx.sync()
    assert (out.cpu().numpy() == 3.0).all() and ok.cpu().numpy()[0] == -7
    assert call(cap=0, s=None, o=None) == siftgpu.SIFT_OK          # m_cap == 0 still reports the flag
    uctx.sync()
    assert ok.cpu().numpy()[0] == 1 and (out.cpu().numpy() == 3.0).all()


# ---- one chain on one stream ---------------------------------------------------------------------
def test_undistort_feeds_fundamental_feeds_pose(uctx, siftgpu):
    """undistort both sides -> find_fundamental_segmented_device -> recover_pose_segmented_device on the
    context stream with no synchronisation and no host value in between, against the same chain
    through the host forms, bit for bit."""
    import torch
    from test_undistort import chain_scene
    n_seg = 3
    scenes = [chain_scene(200, 30 + b) for b in range(n_seg)]
    src, dst = np.concatenate([s["src"] for s in scenes]), np.concatenate([s["dst"] for s in scenes])
    d = scenes[0]["d"]
    offs = np.arange(n_seg + 1, dtype=np.int32) * 200
    cap = n_seg * 200
    ds, dd, dmo, dK, dD = _dev(src), _dev(dst), _dev(offs), _dev(I.PT_K), _dev(d)
    us, ud = torch.empty_like(ds), torch.empty_like(dd)
    oks = torch.full((2, n_seg), -7, dtype=torch.int32, device="cuda")
    dF = torch.zeros((n_seg, 9), dtype=torch.float64, device="cuda")
    df = torch.zeros((n_seg,), dtype=torch.int32, device="cuda")
    dm = torch.zeros((cap,), dtype=torch.uint8, device="cuda")
    pose = torch.zeros((n_seg, 12), dtype=torch.float64, device="cuda")
    pf, ng = torch.zeros((n_seg,), dtype=torch.int32, device="cuda"), torch.zeros((n_seg,), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for a, b, k in ((ds, us, 0), (dd, ud, 1)):
        uctx.undistort_points_segmented_device(a.data_ptr(), b.data_ptr(), 8, dmo.data_ptr(), n_seg, cap, dK.data_ptr(),
                                               dD.data_ptr(), dK.data_ptr(), 0, 5, oks[k].data_ptr())
    uctx.find_fundamental_segmented_device(us.data_ptr(), ud.data_ptr(), dmo.data_ptr(), n_seg, cap, dF.data_ptr(),
                                           df.data_ptr(), dm.data_ptr())
    uctx.recover_pose_segmented_device(us.data_ptr(), ud.data_ptr(), dmo.data_ptr(), n_seg, cap, dF.data_ptr(),
                                       df.data_ptr(), dK.data_ptr(), dK.data_ptr(), pose.data_ptr(), pf.data_ptr(),
                                       ng.data_ptr(), 0, dm.data_ptr(), 50.0)
    uctx.sync()
    assert (oks.cpu().numpy() == 1).all()
    hs, hd = siftgpu.undistortPoints(src, I.PT_K, d, I.PT_K), siftgpu.undistortPoints(dst, I.PT_K, d, I.PT_K)
    assert hs.tobytes() == us.cpu().numpy().tobytes() and hd.tobytes() == ud.cpu().numpy().tobytes()
    for b in range(n_seg):
        lo, hi = int(offs[b]), int(offs[b + 1])
        hF, hm = siftgpu.findFundamentalMat(hs[lo:hi], hd[lo:hi])
        assert df.cpu().numpy()[b] == 1 and hF.tobytes() == dF.cpu().numpy()[b].tobytes()
        R, t, _, _, _, g = siftgpu.recoverPose(hF, I.PT_K, I.PT_K, hs[lo:hi], hd[lo:hi], hm)
        assert R is not None and pf.cpu().numpy()[b] == 1 and ng.cpu().numpy()[b] == g > 100
        assert np.c_[R, t].tobytes() == pose.cpu().numpy()[b].tobytes()
        assert np.abs(R - scenes[b]["R"]).max() < 1e-3
