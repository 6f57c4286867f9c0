"""The squared-L2 kNN matcher on 8-bit descriptors (integer MFMA).

Expected values come from match_l2_inputs.py alone: an int64 sum of (q - t)^2
and a stable argsort per segment on the clamped offsets, compared bit for bit
(indices, float distances that hold the exact integer).
CPU: the three entry points are declared, exported, wrapped and reject a null
context; NORM_L2SQR and BFMatcher(5); the layout program passes; the tie inputs
still tie under the new metric.
GPU (-m gpu): device forms into sentinel-filled outputs with extra rows."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal

import match_l2_inputs as L2
import match_u8_inputs as U
import test_match_batch as B

NEW = ["sift_knn_match_l2sqr_u8_segmented_device", "sift_knn_match_l2sqr_u8_segmented", "sift_knn_match_l2sqr_u8"]
RATIO2 = 0.86 * 0.86    # the application's 0.86 on squared distances


# ---- CPU -------------------------------------------------------------------------
def test_l2_entry_points_declared_exported_and_wrapped(siftgpu):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sift_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert getattr(siftgpu.lib(), name).argtypes is not None, name
    for meth in ["knn_match_l2sqr_u8_segmented_device", "knnMatchL2SqrU8Segmented", "knnMatchL2SqrU8"]:
        assert callable(getattr(siftgpu.Context, meth)), meth


def test_l2_entry_points_reject_null_context(siftgpu):
    L = siftgpu.lib()
    f = np.zeros(128, np.float32)
    u = np.zeros(128, np.uint8)
    off = np.array([0, 1], np.int32)
    ix = np.zeros(2, np.int32)
    pf = f.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    pi = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))  # noqa: E731
    E = siftgpu.SIFT_E_INVALID
    assert L.sift_knn_match_l2sqr_u8_segmented_device(None, u.ctypes.data, off.ctypes.data, 1, 1, u.ctypes.data, None,
                                                      1, 2, ix.ctypes.data, f.ctypes.data) == E
    assert L.sift_knn_match_l2sqr_u8_segmented(None, u.ctypes.data, pi(off), 1, 1, u.ctypes.data, None, 1, 2, pi(ix),
                                               pf) == E
    assert L.sift_knn_match_l2sqr_u8(None, u.ctypes.data, 1, u.ctypes.data, 1, 2, pi(ix), pf) == E
    # and with nothing to do: the null context is still rejected first
    assert L.sift_knn_match_l2sqr_u8_segmented_device(None, None, None, 0, 0, None, None, 0, 2, None, None) == E
    assert L.sift_knn_match_l2sqr_u8_segmented(None, None, None, 0, 0, None, None, 0, 2, None, None) == E
    assert L.sift_knn_match_l2sqr_u8(None, None, 0, None, 0, 2, None, None) == E


def test_l2_norm_constant_and_bfmatcher(siftgpu):
    assert siftgpu.NORM_L2SQR == 5
    m = siftgpu.BFMatcher(5)
    assert isinstance(siftgpu.BFMatcher(siftgpu.NORM_L2SQR), siftgpu.BFMatcher)
    f = np.zeros((2, 128), np.float32)
    u = np.zeros((2, 128), np.uint8)
    for q, t in ((f, f), (u, f), (f, u)):     # raised before any context is made
        with pytest.raises(ValueError):
            m.knnMatch(q, t, 2)
    with pytest.raises(ValueError):
        siftgpu.BFMatcher(normType=4)         # plain NORM_L2 stays out
    with pytest.raises(ValueError):
        siftgpu.BFMatcher(siftgpu.NORM_L2SQR, crossCheck=True)


def test_match_l2_u8_layouts(tmp_path):
    """tests/cpp/match_l2_u8_layout.cpp, built like test_match_u8.py::test_match_u8_layouts:
    with the address and undefined-behaviour sanitizers (runtimes linked
    statically into the program) where the host compiler has them."""
    src = os.path.join(ROOT, "tests", "cpp", "match_l2_u8_layout.cpp")
    exe = tmp_path / "match_l2_u8_layout"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "match l2 u8 layouts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("n", range(len(U.TIE_IDS)), ids=U.TIE_IDS)
def test_l2_tie_inputs_census(n):
    """On the reference alone: under squared L2 every tie input still has at least
    three query rows tied for first place and three tied for second behind a unique
    nearer row (the planted ties are copies of rows)."""
    first, second = L2.tie_census(n)
    assert first >= 3 and second >= 3, (first, second)


def test_l2_extremes_reference_scores_the_maximum():
    c = L2.extremes_case()
    assert L2.DIST_MAX == 8323200
    assert (c.dist[:3] == 8323200.0).all() and c.idx[:3].tolist() == [[0, 1]] * 3
    assert (L2.distances(c.q[:3], c.t[:5]) == 8323200).all()


# ---- GPU: matcher ------------------------------------------------------------------------
def _l2_device(ctx, c, k, extra=64, train_is_query=False, toff_ptr_from_q=False):
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
    ctx.knn_match_l2sqr_u8_segmented_device(dq.data_ptr(), dqo.data_ptr(), len(c.qoff) - 1 - toff_ptr_from_q, c.q_cap,
                                            dt.data_ptr(), to_ptr, c.t_cap, k, di.data_ptr(), dd.data_ptr())
    ctx.sync()
    return di.cpu().numpy(), dd.cpu().numpy()


def _check_case(ctx, c, k):
    """The device form equals the reference on the live rows and writes no other."""
    ridx, rdist = c.ref(k)
    idx, dist = _l2_device(ctx, c, k)
    B._check_live(idx, dist, ridx, rdist, c.qoff, c.q_cap, f"{c.name} k={k}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
@pytest.mark.parametrize("seg_train", [False, True], ids=["shared", "segmented"])
def test_gpu_l2_random_bytes_tile_edges(ctx, k, seg_train):
    c = L2.edges_case(seg_train)
    _check_case(ctx, c, k)
    if seg_train:   # local indices; -1 / +inf where the range has fewer than k rows
        idx, dist = c.ref(k)
        for b, nt in enumerate(U.T_SIZES):
            seg = idx[c.qoff[b]:c.qoff[b + 1]]
            assert (seg < max(nt, 1)).all()
            if nt < k and len(seg):
                assert (seg[:, nt:] == -1).all() and np.isposinf(dist[c.qoff[b]:c.qoff[b + 1], nt:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
def test_gpu_l2_granules_blocks_and_chunks(ctx, k):
    """Query segments of 31 / 32 / 33 rows (the 32-query block of a lane) and train
    ranges of 2,047 / 2,048 / 2,049 / 2,177 rows in one split: a wave's 512-row
    chunk one row short, full, and followed by a second one, with ties planted
    across chunks and waves."""
    c = L2.chunks_case()
    assert len(c.qoff) - 1 == L2.CHUNK_NSEG
    _check_case(ctx, c, k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
def test_gpu_l2_extremes_and_sign_bias(ctx, k):
    c = L2.extremes_case()
    _check_case(ctx, c, k)
    idx, dist = _l2_device(ctx, c, k, extra=0)
    assert (dist[:3, 0] == 8323200.0).all() and (dist[73:143, 0] == 0).all()
    assert (idx[143:, 0] == 2).all() and (dist[143:, 0] == 0).all()     # 0x80 against 0x7F / 0x80 / 0x81


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
def test_gpu_l2_operand_map_distinct_weights(ctx, k):
    _check_case(ctx, L2.weights_case(), k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
@pytest.mark.parametrize("n", range(len(U.TIE_IDS)), ids=U.TIE_IDS)
def test_gpu_l2_ties(ctx, n, k):
    _check_case(ctx, L2.tie_case(n), k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
def test_gpu_l2_ties_segmented_train(ctx, k):
    _check_case(ctx, L2.tie_segmented_case(), k)


@pytest.mark.gpu
def test_gpu_l2_short_train_sets(ctx, siftgpu):
    """n_train of 0 and 1 with k = 2: -1 / +inf, and the ratio stage skips those rows."""
    rng = np.random.default_rng(46)
    q = rng.integers(0, 256, (70, 128), dtype=np.uint8)
    t = rng.integers(0, 256, (1, 128), dtype=np.uint8)
    qoff = U.offsets([5, 65])
    c = L2.Case("short", q, qoff, t, U.offsets([0, 1]))
    _check_case(ctx, c, 2)
    idx, dist = _l2_device(ctx, c, 2, extra=0)
    assert (idx[:5] == -1).all() and np.isposinf(dist[:5]).all()
    assert (idx[5:] == [0, -1]).all() and np.isposinf(dist[5:, 1]).all() and np.isfinite(dist[5:, 0]).all()
    m, moff, _, _ = B._ratio_device(ctx, siftgpu, idx, dist, qoff, len(q), 1.0, extra=8)
    assert moff.tolist() == [0, 0, 0] and (m.view(np.int32) == -77).all()
    for nt in (0, 1):
        hi, hd = ctx.knnMatchL2SqrU8(q, t[:nt], 2)
        assert (hi[:, nt:] == -1).all() and np.isposinf(hd[:, nt:]).all() and (hi[:, :nt] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(5), ids=["q_cap", "q_cap-shared", "t_cap", "t_cap-shared", "first-offset"])
def test_gpu_l2_capacity_clamps(ctx, n):
    c = L2.clamp_cases()[n]
    assert c.name == ["q_cap", "q_cap-shared", "t_cap", "t_cap-shared", "first-offset"][n]
    _check_case(ctx, c, 2)


@pytest.mark.gpu
def test_gpu_l2_many_segments(ctx):
    c = L2.many_segments_case()
    assert len(c.qoff) - 1 == 257
    _check_case(ctx, c, 2)


@pytest.mark.gpu
def test_gpu_l2_consecutive_frames_aliased(ctx):
    """d_train = d_query, d_t_offsets = d_q_offsets + 1: frame b against frame b + 1."""
    rng = np.random.default_rng(47)
    off = U.offsets([130, 0, 65, 257, 3])
    d = rng.integers(0, 8, (int(off[-1]), 128), dtype=np.uint8)
    c = L2.Case("aliased", d, off[:-1], d, off[1:])
    assert len(np.unique(c.dist[:, 0])) > 3 and (c.idx[:130] == -1).all()   # frame 0 searches the empty frame 1
    a = U.Case("aliased", d, off, d, None)    # the device reads both offset arrays from `off`
    idx, dist = _l2_device(ctx, a, 2, train_is_query=True, toff_ptr_from_q=True)
    B._check_live(idx, dist, c.idx, c.dist, c.qoff, c.q_cap, "aliased")


@pytest.mark.gpu
def test_gpu_l2_batch_flow_in_stream_order(ctx, siftgpu):
    """synth_images (4 x 240x320), detect_compute_batch, the quantiser, the
    squared-L2 matcher on consecutive frames and the ratio stage with ratio
    0.86^2 and keypoints, all enqueued; one sync.  Matches, offsets and point
    pairs equal the reference computed from the copied-back descriptors."""
    import torch
    Bn, R, C, cap = 4, 240, 320, 4096
    imgs = torch.empty((Bn, R, C), dtype=torch.float32, device="cuda")
    kpts = torch.zeros((cap, 7), dtype=torch.int32, device="cuda")
    desc = torch.zeros((cap, 128), dtype=torch.float32, device="cuda")
    d8 = torch.full((cap, 128), 0xEE, dtype=torch.uint8, device="cuda")
    offs = torch.zeros((Bn + 1,), dtype=torch.int32, device="cuda")
    idx = torch.full((cap, 2), -77, dtype=torch.int32, device="cuda")
    dist = torch.full((cap, 2), -5.0, dtype=torch.float32, device="cuda")
    mt = torch.full((cap, 4), -77, dtype=torch.int32, device="cuda")
    src = torch.full((cap, 2), -5.0, dtype=torch.float32, device="cuda")
    dst = torch.full((cap, 2), -5.0, dtype=torch.float32, device="cuda")
    moff = torch.full((Bn,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.synth_images(imgs.data_ptr(), Bn, R, C, C, R * C, 0)
    ctx.detect_compute_batch(imgs.data_ptr(), Bn, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                             offs.data_ptr())
    ctx.descriptors_to_u8_device(desc.data_ptr(), offs.data_ptr() + 4 * Bn, cap, d8.data_ptr())
    ctx.knn_match_l2sqr_u8_segmented_device(d8.data_ptr(), offs.data_ptr(), Bn - 1, cap, d8.data_ptr(),
                                            offs.data_ptr() + 4, cap, 2, idx.data_ptr(), dist.data_ptr())
    ctx.ratio_matches_device(idx.data_ptr(), dist.data_ptr(), offs.data_ptr(), Bn - 1, cap, RATIO2,
                             kpts.data_ptr(), kpts.data_ptr(), offs.data_ptr() + 4, mt.data_ptr(), src.data_ptr(),
                             dst.data_ptr(), cap, moff.data_ptr())
    ctx.sync()
    o = offs.cpu().numpy()
    n = int(o[-1])
    assert 0 < n <= cap and (np.diff(o) > 0).all()
    kp = kpts.cpu().numpy().view(siftgpu.KEYPOINT_DTYPE).reshape(-1)
    q8 = U.quant_ref(desc.cpu().numpy())
    assert_bits_equal(d8.cpu().numpy()[:n], q8[:n], "quantised rows")
    ridx, rdist = L2.seg_ref(q8, o[:-1], q8, o[1:], 2, q_cap=cap, t_cap=cap)
    B._check_live(idx.cpu().numpy(), dist.cpu().numpy(), ridx, rdist, o[:-1], cap, "consecutive frames")
    rec, rmoff, rsrc, rdst = B._ref_ratio(ridx, rdist, o[:-1], cap, RATIO2, kp, kp, o[1:])
    m = mt.cpu().numpy().view(siftgpu.MATCH_DTYPE).reshape(-1)
    k = len(rec)
    assert k > 0
    assert_bits_equal(moff.cpu().numpy(), rmoff, "moff")
    assert_bits_equal(m[:k], B._rec_array(siftgpu, rec), "records")
    assert_bits_equal(src.cpu().numpy()[:k], rsrc, "src_xy")
    assert_bits_equal(dst.cpu().numpy()[:k], rdst, "dst_xy")
    assert (m[k:].view(np.int32) == -77).all()


@pytest.mark.gpu
def test_gpu_l2_host_forms_equal_device_forms(ctx, siftgpu):
    for c in (L2.edges_case(True), L2.edges_case(False)):
        for k in (2, 1):
            di, dd = _l2_device(ctx, c, k, extra=0)
            hi, hd = ctx.knnMatchL2SqrU8Segmented(c.q, c.qoff, c.t, c.toff, k)
            assert_bits_equal(hi, c.ref(k)[0], f"{c.name} host idx k={k}")
            assert_bits_equal(hd, c.ref(k)[1], f"{c.name} host dist k={k}")
            lo, hi_ = int(c.qoff[0]), int(c.qoff[-1])
            assert_bits_equal(hi[lo:hi_], di[lo:hi_], f"{c.name} host idx equals device k={k}")
            assert_bits_equal(hd[lo:hi_], dd[lo:hi_], f"{c.name} host dist equals device k={k}")
    c = L2.tie_case(len(U.DENSE) + 5)    # 300 x 257, unsegmented
    for k in (2, 1):
        hi, hd = ctx.knnMatchL2SqrU8(c.q, c.t, k)
        assert_bits_equal(hi, c.ref(k)[0], f"knnMatchL2SqrU8 idx k={k}")
        assert_bits_equal(hd, c.ref(k)[1], f"knnMatchL2SqrU8 dist k={k}")
    lists = siftgpu.BFMatcher(siftgpu.NORM_L2SQR, ctx=ctx).knnMatch(c.q, c.t, 2)
    assert [[m.trainIdx for m in row] for row in lists] == c.idx.tolist()
    assert [[m.distance for m in row] for row in lists] == c.dist.tolist()
    assert [m.queryIdx for row in lists for m in row] == np.repeat(np.arange(len(c.q)), 2).tolist()
    with pytest.raises(ValueError):
        ctx.knnMatchL2SqrU8(c.q.astype(np.float32), c.t)
