"""8-bit descriptors: the quantiser and the integer L1 kNN matcher.

Expected values come from match_u8_inputs.py alone: an int64 |a - b| sum and a
stable argsort per segment, compared bit for bit (indices, float distances that
hold the exact integer).  On every matcher input the unchanged float matcher,
run on the same bytes as float32, is a second reference on the GPU:
integer-valued floats sum exactly in any order.
CPU: the five entry points are declared, exported, wrapped and reject a null
context; the layout program passes; the tie inputs tie where they claim.
GPU (-m gpu): device forms into sentinel-filled outputs with extra rows."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal, load_golden

import match_u8_inputs as U
import test_match_batch as B

NEW = ["sift_descriptors_to_u8_device", "sift_descriptors_to_u8", "sift_knn_match_l1_u8_segmented_device",
       "sift_knn_match_l1_u8_segmented", "sift_knn_match_l1_u8"]


# ---- CPU -------------------------------------------------------------------------
def test_u8_entry_points_declared_exported_and_wrapped(siftgpu):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sift_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert getattr(siftgpu.lib(), name).argtypes is not None, name
    for meth in ["descriptors_to_u8_device", "descriptorsToU8", "knn_match_u8_segmented_device", "knnMatchU8Segmented",
                 "knnMatchU8"]:
        assert callable(getattr(siftgpu.Context, meth)), meth


def test_u8_entry_points_reject_null_context(siftgpu):
    L = siftgpu.lib()
    f = np.zeros(128, np.float32)
    u = np.zeros(128, np.uint8)
    off = np.array([0, 1], np.int32)
    ix = np.zeros(2, np.int32)
    pf = f.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    pi = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))  # noqa: E731
    E = siftgpu.SIFT_E_INVALID
    assert L.sift_descriptors_to_u8_device(None, f.ctypes.data, None, 1, u.ctypes.data) == E
    assert L.sift_descriptors_to_u8(None, pf, 1, u.ctypes.data) == E
    assert L.sift_knn_match_l1_u8_segmented_device(None, u.ctypes.data, off.ctypes.data, 1, 1, u.ctypes.data, None, 1,
                                                   2, ix.ctypes.data, f.ctypes.data) == E
    assert L.sift_knn_match_l1_u8_segmented(None, u.ctypes.data, pi(off), 1, 1, u.ctypes.data, None, 1, 2, pi(ix),
                                            pf) == E
    assert L.sift_knn_match_l1_u8(None, u.ctypes.data, 1, u.ctypes.data, 1, 2, pi(ix), pf) == E
    # and with nothing to do: the null context is still rejected first
    assert L.sift_knn_match_l1_u8_segmented_device(None, None, None, 0, 0, None, None, 0, 2, None, None) == E
    assert L.sift_descriptors_to_u8_device(None, None, None, 0, None) == E


def test_match_u8_layouts(tmp_path):
    """tests/cpp/match_u8_layout.cpp, built like test_abi.py::test_scratch_layouts:
    with the address and undefined-behaviour sanitizers (runtimes linked
    statically into the program) where the host compiler has them."""
    src = os.path.join(ROOT, "tests", "cpp", "match_u8_layout.cpp")
    exe = tmp_path / "match_u8_layout"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "match u8 layouts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("n", range(len(U.TIE_IDS)), ids=U.TIE_IDS)
def test_u8_tie_inputs_census(n):
    """On the reference alone: at least three query rows tied for first place and
    three tied for second behind a unique nearer row -- places the index decides."""
    first, second = U.tie_census(U.tie_case(n))
    assert first >= 3 and second >= 3, (first, second)


def test_u8_quantiser_reference_rounds_to_even():
    x = np.array([0.5, 1.5, 2.5, 254.5, 255.5, 300, -1], np.float32) / np.float32(512)
    assert U.quant_ref(x).tolist() == [0, 2, 2, 254, 255, 255, 0]
    e = U.quant_edges()
    assert np.isposinf(e).sum() == 1 and np.isneginf(e).sum() == 1 and not np.isnan(e).any()
    assert set(np.unique(U.quant_ref(e))) == set(range(256))


# ---- GPU: quantiser --------------------------------------------------------------------
def _quant_device(ctx, x, n_rows, row_cap, extra=8):
    """Device form into a sentinel-filled (0xEE) output of row_cap + extra rows."""
    import torch
    dx = B._dev(x)
    dn = None if n_rows is None else B._dev(np.array([n_rows], np.int32))
    out = torch.full((row_cap + extra, 128), 0xEE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.descriptors_to_u8_device(dx.data_ptr(), None if dn is None else dn.data_ptr(), row_cap, out.data_ptr())
    ctx.sync()
    return out.cpu().numpy()


@pytest.mark.gpu
def test_gpu_quantiser_edges_and_book(ctx):
    for name, x in (("edges", U.quant_edges()), ("book", load_golden("book")["desc"])):
        x = np.ascontiguousarray(x, np.float32).reshape(-1, 128)
        want = U.quant_ref(x)
        got = _quant_device(ctx, x, None, len(x))
        assert_bits_equal(got[:len(x)], want, name)
        assert (got[len(x):] == 0xEE).all(), name + ": rows past row_cap written"
        assert_bits_equal(ctx.descriptorsToU8(x), want, name + " host form")
    assert len(ctx.descriptorsToU8(np.zeros((0, 128), np.float32))) == 0


@pytest.mark.gpu
def test_gpu_quantiser_row_count(ctx):
    """*d_n_rows below, equal to and above row_cap, negative, and NULL: rows at
    or past min(*d_n_rows, row_cap) keep the sentinel."""
    rng = np.random.default_rng(45)
    x = (rng.random((41, 128)).astype(np.float32) * np.float32(0.6))
    want = U.quant_ref(x)
    row_cap = 33
    for n_rows in (0, 1, 20, 33, 41, 2 ** 31 - 1, -3, None):
        got = _quant_device(ctx, x, n_rows, row_cap)
        live = row_cap if n_rows is None else max(0, min(n_rows, row_cap))
        assert_bits_equal(got[:live], want[:live], f"n_rows {n_rows}")
        assert (got[live:] == 0xEE).all(), f"n_rows {n_rows}: rows past the bound written"


# ---- GPU: matcher ------------------------------------------------------------------------
def _u8_device(ctx, c, k, extra=64, train_is_query=False, toff_ptr_from_q=False):
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
    ctx.knn_match_u8_segmented_device(dq.data_ptr(), dqo.data_ptr(), len(c.qoff) - 1 - toff_ptr_from_q, c.q_cap,
                                      dt.data_ptr(), to_ptr, c.t_cap, k, di.data_ptr(), dd.data_ptr())
    ctx.sync()
    return di.cpu().numpy(), dd.cpu().numpy()


def _check_case(ctx, c, k):
    """The u8 device form equals the reference on the live rows and writes no
    other; the float matcher on the same bytes gives the same idx and dist bits."""
    ridx, rdist = c.ref(k)
    idx, dist = _u8_device(ctx, c, k)
    B._check_live(idx, dist, ridx, rdist, c.qoff, c.q_cap, f"{c.name} k={k}")
    fidx, fdist = B._knn_device(ctx, c.q.astype(np.float32), c.qoff, c.t.astype(np.float32), c.toff, k,
                                q_cap=c.q_cap, t_cap=c.t_cap, extra=64)
    assert_bits_equal(fidx, idx, f"{c.name} k={k}: float matcher idx")
    assert_bits_equal(fdist, dist, f"{c.name} k={k}: float matcher dist")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
@pytest.mark.parametrize("seg_train", [False, True], ids=["shared", "segmented"])
def test_gpu_u8_random_bytes_tile_edges(ctx, k, seg_train):
    c = U.edges_case(seg_train)
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
def test_gpu_u8_extremes(ctx, k):
    _check_case(ctx, U.extremes_case(), k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
@pytest.mark.parametrize("n", range(len(U.TIE_IDS)), ids=U.TIE_IDS)
def test_gpu_u8_ties(ctx, n, k):
    _check_case(ctx, U.tie_case(n), k)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
def test_gpu_u8_ties_segmented_train(ctx, k):
    _check_case(ctx, U.tie_segmented_case(), k)


@pytest.mark.gpu
def test_gpu_u8_short_train_sets(ctx, siftgpu):
    """n_train of 0 and 1 with k = 2: -1 / +inf, and the ratio stage skips those rows."""
    rng = np.random.default_rng(46)
    q = rng.integers(0, 256, (70, 128), dtype=np.uint8)
    t = rng.integers(0, 256, (1, 128), dtype=np.uint8)
    qoff = U.offsets([5, 65])
    c = U.Case("short", q, qoff, t, U.offsets([0, 1]))
    _check_case(ctx, c, 2)
    idx, dist = _u8_device(ctx, c, 2, extra=0)
    assert (idx[:5] == -1).all() and np.isposinf(dist[:5]).all()
    assert (idx[5:] == [0, -1]).all() and np.isposinf(dist[5:, 1]).all() and np.isfinite(dist[5:, 0]).all()
    m, moff, _, _ = B._ratio_device(ctx, siftgpu, idx, dist, qoff, len(q), 1.0, extra=8)
    assert moff.tolist() == [0, 0, 0] and (m.view(np.int32) == -77).all()
    for nt in (0, 1):
        hi, hd = ctx.knnMatchU8(q, t[:nt], 2)
        assert (hi[:, nt:] == -1).all() and np.isposinf(hd[:, nt:]).all() and (hi[:, :nt] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(5), ids=["q_cap", "q_cap-shared", "t_cap", "t_cap-shared", "first-offset"])
def test_gpu_u8_capacity_clamps(ctx, n):
    c = U.clamp_cases()[n]
    assert c.name == ["q_cap", "q_cap-shared", "t_cap", "t_cap-shared", "first-offset"][n]
    _check_case(ctx, c, 2)


@pytest.mark.gpu
def test_gpu_u8_many_segments(ctx):
    c = U.many_segments_case()
    assert len(c.qoff) - 1 == 257
    _check_case(ctx, c, 2)


@pytest.mark.gpu
def test_gpu_u8_consecutive_frames_aliased(ctx):
    """d_train = d_query, d_t_offsets = d_q_offsets + 1: frame b against frame b + 1."""
    rng = np.random.default_rng(47)
    off = U.offsets([130, 0, 65, 257, 3])
    d = rng.integers(0, 8, (int(off[-1]), 128), dtype=np.uint8)
    c = U.Case("aliased", d, off[:-1], d, off[1:])
    assert len(np.unique(c.dist[:, 0])) > 3 and (c.idx[:130] == -1).all()   # frame 0 searches the empty frame 1
    a = U.Case("aliased", d, off, d, None)    # the device reads both offset arrays from `off`
    a.idx, a.dist = c.idx, c.dist
    idx, dist = _u8_device(ctx, a, 2, train_is_query=True, toff_ptr_from_q=True)
    B._check_live(idx, dist, c.idx, c.dist, c.qoff, c.q_cap, "aliased")


@pytest.mark.gpu
def test_gpu_u8_batch_flow_in_stream_order(ctx, siftgpu):
    """synth_images (4 x 240x320), detect_compute_batch, the quantiser with
    d_n_rows = d_img_offsets + 4, the u8 matcher on consecutive frames and the
    ratio stage with keypoints, all enqueued; one sync.  Matches, offsets and
    point pairs equal the reference computed from the copied-back float
    descriptors."""
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
    ctx.knn_match_u8_segmented_device(d8.data_ptr(), offs.data_ptr(), Bn - 1, cap, d8.data_ptr(),
                                      offs.data_ptr() + 4, cap, 2, idx.data_ptr(), dist.data_ptr())
    ctx.ratio_matches_device(idx.data_ptr(), dist.data_ptr(), offs.data_ptr(), Bn - 1, cap, 0.86,
                             kpts.data_ptr(), kpts.data_ptr(), offs.data_ptr() + 4, mt.data_ptr(), src.data_ptr(),
                             dst.data_ptr(), cap, moff.data_ptr())
    ctx.sync()
    o = offs.cpu().numpy()
    n = int(o[-1])
    assert 0 < n <= cap and (np.diff(o) > 0).all()
    kp = kpts.cpu().numpy().view(siftgpu.KEYPOINT_DTYPE).reshape(-1)
    q8 = U.quant_ref(desc.cpu().numpy())
    got8 = d8.cpu().numpy()
    assert_bits_equal(got8[:n], q8[:n], "quantised rows")
    assert (got8[n:] == 0xEE).all(), "rows past the total written"
    ridx, rdist = U.seg_ref(q8, o[:-1], q8, o[1:], 2, q_cap=cap, t_cap=cap)
    B._check_live(idx.cpu().numpy(), dist.cpu().numpy(), ridx, rdist, o[:-1], cap, "consecutive frames")
    rec, rmoff, rsrc, rdst = B._ref_ratio(ridx, rdist, o[:-1], cap, 0.86, kp, kp, o[1:])
    m = mt.cpu().numpy().view(siftgpu.MATCH_DTYPE).reshape(-1)
    k = len(rec)
    assert k > 0
    assert_bits_equal(moff.cpu().numpy(), rmoff, "moff")
    assert_bits_equal(m[:k], B._rec_array(siftgpu, rec), "records")
    assert_bits_equal(src.cpu().numpy()[:k], rsrc, "src_xy")
    assert_bits_equal(dst.cpu().numpy()[:k], rdst, "dst_xy")
    assert (m[k:].view(np.int32) == -77).all()


@pytest.mark.gpu
def test_gpu_u8_host_forms_equal_device_forms(ctx, siftgpu):
    for c in (U.edges_case(True), U.edges_case(False)):
        for k in (2, 1):
            di, dd = _u8_device(ctx, c, k, extra=0)
            hi, hd = ctx.knnMatchU8Segmented(c.q, c.qoff, c.t, c.toff, k)
            assert_bits_equal(hi, c.ref(k)[0], f"{c.name} host idx k={k}")
            assert_bits_equal(hd, c.ref(k)[1], f"{c.name} host dist k={k}")
            lo, hi_ = int(c.qoff[0]), int(c.qoff[-1])
            assert_bits_equal(hi[lo:hi_], di[lo:hi_], f"{c.name} host idx equals device k={k}")
            assert_bits_equal(hd[lo:hi_], dd[lo:hi_], f"{c.name} host dist equals device k={k}")
    c = U.tie_case(len(U.DENSE) + 5)    # 300 x 257, unsegmented
    for k in (2, 1):
        hi, hd = ctx.knnMatchU8(c.q, c.t, k)
        assert_bits_equal(hi, c.ref(k)[0], f"knnMatchU8 idx k={k}")
        assert_bits_equal(hd, c.ref(k)[1], f"knnMatchU8 dist k={k}")
    lists = siftgpu.BFMatcher(siftgpu.NORM_L1, ctx=ctx).knnMatch(c.q, c.t, 2)
    assert [[m.trainIdx for m in row] for row in lists] == c.idx.tolist()
    assert [[m.distance for m in row] for row in lists] == c.dist.tolist()
    assert [m.queryIdx for row in lists for m in row] == np.repeat(np.arange(len(c.q)), 2).tolist()
    # float input still takes the float matcher: same values here, since the bytes are exact in float32
    flists = siftgpu.BFMatcher(siftgpu.NORM_L1, ctx=ctx).knnMatch(c.q.astype(np.float32), c.t.astype(np.float32), 2)
    assert [[m.trainIdx for m in row] for row in flists] == c.idx.tolist()
    with pytest.raises(ValueError):
        ctx.knnMatchU8(c.q.astype(np.float32), c.t)
