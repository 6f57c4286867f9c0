"""Matching a whole batch on the device: the segmented L1 kNN, the ratio test
with ordered compaction and the point-pair gather (src/main.cpp:25-52 for every
image of a batch, offsets read on the device).

Expected values always come from the unchanged oracle/match.py applied segment
by segment -- M.knn_match(q[seg], t[tseg], k) and M.ratio_test -- and are
compared bit for bit (indices, float distances, xy bytes).
CPU: the four entry points are declared, exported, wrapped, and reject a null
context.  GPU (-m gpu): shared and segmented train, many segments, the capacity
clamps with sentinel rows, the ratio stage on crafted input, the stream-ordered
end-to-end flow after detect_compute_batch, and the host forms."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal, book_image

import match as M

NEW = ["sift_knn_match_l1_segmented_device", "sift_knn_match_l1_segmented", "sift_ratio_matches_device",
       "sift_ratio_matches"]
Q_SIZES = [0, 1, 63, 64, 65, 130, 0, 200]
T_SIZES = [5, 0, 1, 2, 64, 65, 4097, 10]
# the issue's sizes pair the 4097-row train segment with an empty query segment; rotated by one,
# the 200-row query segment searches it (many splits) and the 63-row one an empty train segment
T_SIZES_ROT = [10, 5, 0, 1, 2, 64, 65, 4097]


def _rootsift_like(rng, n):
    x = rng.random((n, 128)).astype(np.float32) ** 3
    x /= x.sum(1, keepdims=True)
    return np.sqrt(x).astype(np.float32)


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def _clamped(off, cap):
    return np.clip(np.asarray(off, np.int64), 0, cap)


def _ref_knn(q, qoff, t, toff, k, q_cap=None, t_cap=None):
    """Oracle per segment on the clamped bounds; rows outside the live range None-marked by `live`."""
    q_cap = len(q) if q_cap is None else q_cap
    t_cap = len(t) if t_cap is None else t_cap
    qo = _clamped(qoff, q_cap)
    to = None if toff is None else _clamped(toff, t_cap)
    idx = np.full((q_cap, k), -1, np.int32)
    dist = np.full((q_cap, k), np.inf, np.float32)
    for b in range(len(qo) - 1):
        ts = t[:t_cap] if to is None else t[to[b]:max(to[b], to[b + 1])]
        i, d = M.knn_match(q[qo[b]:qo[b + 1]], ts, k)
        idx[qo[b]:qo[b + 1]], dist[qo[b]:qo[b + 1]] = i, d
    return idx, dist


def _ref_ratio(idx, dist, qoff, q_cap, ratio=M.RATIO, q_kpts=None, t_kpts=None, toff=None):
    """(records as (query, train, distance, segment) rows, moff, src, dst) from M.ratio_test per segment."""
    qo = _clamped(qoff, q_cap)
    rec, moff, src, dst = [], [0], [], []
    for b in range(len(qo) - 1):
        for i, j, d in M.ratio_test(idx[qo[b]:qo[b + 1]], dist[qo[b]:qo[b + 1]], ratio):
            rec.append((i, j, np.float32(d), b))
            if q_kpts is not None:
                tb = 0 if toff is None else int(toff[b])
                src.append((q_kpts["x"][qo[b] + i], q_kpts["y"][qo[b] + i]))
                dst.append((t_kpts["x"][tb + j], t_kpts["y"][tb + j]))
        moff.append(len(rec))
    return rec, np.array(moff, np.int32), np.array(src, np.float32).reshape(-1, 2), \
        np.array(dst, np.float32).reshape(-1, 2)


def _rec_array(siftgpu, rec):
    out = np.zeros(len(rec), siftgpu.MATCH_DTYPE)
    for n, (i, j, d, b) in enumerate(rec):
        out[n] = (i, j, d, b)
    return out


def _case(seed, q_sizes, nt=None, t_sizes=None):
    """Descriptors with a duplicated train row and a query equal to it (a real tie) where sizes allow."""
    rng = np.random.default_rng(seed)
    qoff = _offsets(q_sizes)
    q = _rootsift_like(rng, int(qoff[-1]))
    if t_sizes is None:
        t, toff = _rootsift_like(rng, nt), None
        if nt > 3:
            t[nt // 2] = t[1]
            for b in range(len(q_sizes)):
                if q_sizes[b]:
                    q[qoff[b]] = t[1]
    else:
        toff = _offsets(t_sizes)
        t = _rootsift_like(rng, int(toff[-1]))
        for b in range(len(q_sizes)):
            if t_sizes[b] > 3 and q_sizes[b]:
                t[toff[b] + t_sizes[b] // 2] = t[toff[b] + 1]
                q[qoff[b]] = t[toff[b] + 1]
    return q, qoff, t, toff


def _kpts(siftgpu, rng, n):
    k = np.zeros(n, siftgpu.KEYPOINT_DTYPE)
    k["x"] = rng.random(n).astype(np.float32) * 1000
    k["y"] = rng.random(n).astype(np.float32) * 1000
    k["size"] = 3
    return k


# ---- CPU -------------------------------------------------------------------------
def test_new_entry_points_declared_exported_and_wrapped(siftgpu):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sift_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
    assert "typedef struct sift_match" in text
    for meth in ["knn_match_segmented_device", "ratio_matches_device", "knnMatchSegmented", "ratioMatches"]:
        assert callable(getattr(siftgpu.Context, meth)), meth
    assert siftgpu.MATCH_DTYPE.itemsize == 16
    assert siftgpu.MATCH_DTYPE.names == ("query", "train", "distance", "segment")


def test_new_entry_points_reject_null_context(siftgpu):
    L = siftgpu.lib()
    one = np.zeros(128, np.float32)
    off = np.array([0, 1], np.int32)
    ix = np.zeros(2, np.int32)
    pf = one.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    pi = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))  # noqa: E731
    E = siftgpu.SIFT_E_INVALID
    assert L.sift_knn_match_l1_segmented_device(None, one.ctypes.data, off.ctypes.data, 1, 1, one.ctypes.data, None,
                                                1, 2, ix.ctypes.data, one.ctypes.data) == E
    assert L.sift_knn_match_l1_segmented(None, pf, pi(off), 1, 1, pf, None, 1, 2, pi(ix), pf) == E
    assert L.sift_ratio_matches_device(None, ix.ctypes.data, one.ctypes.data, off.ctypes.data, 1, 1, 0.86, None,
                                       None, None, one.ctypes.data, None, None, 1, off.ctypes.data) == E
    assert L.sift_ratio_matches(None, pi(ix), pf, pi(off), 1, 1, 0.86, None, None, 0, None, one.ctypes.data, None,
                                None, 1, pi(off)) == E


# ---- GPU: device forms on torch buffers -------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_kpts(k):
    return _dev(np.ascontiguousarray(k).view(np.int32).reshape(len(k), 7))


def _knn_device(ctx, q, qoff, t, toff, k, q_cap=None, t_cap=None, extra=0, train_is_query=False):
    """Device form into sentinel-filled outputs of q_cap + extra rows -> (idx, dist) numpy."""
    import torch
    q_cap = len(q) if q_cap is None else q_cap
    t_cap = len(t) if t_cap is None else t_cap
    dq, dqo = _dev(q), _dev(qoff)
    dt = dq if train_is_query else _dev(t)
    dto = None if toff is None else _dev(toff)
    di = torch.full((q_cap + extra, k), -77, dtype=torch.int32, device="cuda")
    dd = torch.full((q_cap + extra, k), -5.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()                  # the context's stream does not wait for torch's
    ctx.knn_match_segmented_device(dq.data_ptr(), dqo.data_ptr(), len(qoff) - 1, q_cap, dt.data_ptr(),
                                   None if dto is None else dto.data_ptr(), t_cap, k, di.data_ptr(), dd.data_ptr())
    ctx.sync()
    return di.cpu().numpy(), dd.cpu().numpy()


def _ratio_device(ctx, siftgpu, idx, dist, qoff, q_cap, ratio=M.RATIO, q_kpts=None, t_kpts=None, toff=None,
                  m_cap=None, extra=0):
    """Device form into sentinel-filled outputs -> (matches, moff, src, dst) numpy, all m_cap + extra rows."""
    import torch
    m_cap = q_cap if m_cap is None else m_cap
    di, dd, dqo = _dev(idx), _dev(dist), _dev(qoff)
    dto = None if toff is None else _dev(toff)
    dm = torch.full((m_cap + extra, 4), -77, dtype=torch.int32, device="cuda")
    ds = torch.full((m_cap + extra, 2), -5.0, dtype=torch.float32, device="cuda")
    dt = torch.full((m_cap + extra, 2), -5.0, dtype=torch.float32, device="cuda")
    dmo = torch.full((len(qoff),), -77, dtype=torch.int32, device="cuda")
    dqk = None if q_kpts is None else _dev_kpts(q_kpts)
    dtk = None if t_kpts is None else _dev_kpts(t_kpts)
    torch.cuda.synchronize()
    ctx.ratio_matches_device(di.data_ptr(), dd.data_ptr(), dqo.data_ptr(), len(qoff) - 1, q_cap, ratio,
                             None if dqk is None else dqk.data_ptr(), None if dtk is None else dtk.data_ptr(),
                             None if dto is None else dto.data_ptr(), dm.data_ptr(), ds.data_ptr(), dt.data_ptr(),
                             m_cap, dmo.data_ptr())
    ctx.sync()
    return dm.cpu().numpy().view(siftgpu.MATCH_DTYPE).reshape(-1), dmo.cpu().numpy(), ds.cpu().numpy(), \
        dt.cpu().numpy()


def _check_live(idx, dist, ridx, rdist, qoff, q_cap, what):
    """Live rows equal the oracle; every other row (sentinel tail included) is untouched."""
    lo, hi = (int(v) for v in _clamped([qoff[0], qoff[-1]], q_cap))
    assert_bits_equal(idx[lo:hi], ridx[lo:hi], what + " idx")
    assert_bits_equal(dist[lo:hi], rdist[lo:hi], what + " dist")
    dead = np.r_[0:lo, hi:len(idx)]
    assert (idx[dead] == -77).all() and (dist[dead] == -5.0).all(), what + ": rows outside the live range written"


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
def test_gpu_segmented_shared_train(ctx, k):
    q, qoff, t, _ = _case(21, Q_SIZES, nt=333)
    idx, dist = _knn_device(ctx, q, qoff, t, None, k, extra=64)
    ridx, rdist = _ref_knn(q, qoff, t, None, k)
    _check_live(idx, dist, ridx, rdist, qoff, len(q), f"shared k={k}")
    if k == 2:  # the exact hit and its duplicate tie at distance 0, earlier index first
        first = int(qoff[1])
        assert idx[first].tolist() == [1, 333 // 2] and dist[first].tolist() == [0.0, 0.0]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
@pytest.mark.parametrize("T_SIZES", [T_SIZES, T_SIZES_ROT], ids=["issue", "rotated"])
def test_gpu_segmented_train_local_indices(ctx, k, T_SIZES):
    q, qoff, t, toff = _case(22, Q_SIZES, t_sizes=T_SIZES)
    idx, dist = _knn_device(ctx, q, qoff, t, toff, k, extra=64)
    ridx, rdist = _ref_knn(q, qoff, t, toff, k)
    _check_live(idx, dist, ridx, rdist, qoff, len(q), f"segmented k={k}")
    for b, nt in enumerate(T_SIZES):        # local indices; -1 where the segment has fewer than k rows
        seg = idx[qoff[b]:qoff[b + 1]]
        assert (seg < max(nt, 1)).all()
        if nt < k and len(seg):
            assert (seg[:, nt:] == -1).all()


@pytest.mark.gpu
def test_gpu_many_segments(ctx):
    rng = np.random.default_rng(23)
    sizes = rng.integers(1, 4, 130).tolist()
    q, qoff, t, _ = _case(24, sizes, nt=70)
    idx, dist = _knn_device(ctx, q, qoff, t, None, 2, extra=64)
    ridx, rdist = _ref_knn(q, qoff, t, None, 2)
    _check_live(idx, dist, ridx, rdist, qoff, len(q), "130 segments")


@pytest.mark.gpu
def test_gpu_query_capacity_clamp(ctx):
    """qoff[-1] = q_cap + 37 and the last segment straddles q_cap: rows below
    q_cap equal the oracle on the clamped segments, the 64 rows after are untouched."""
    q, qoff, t, toff = _case(25, Q_SIZES, t_sizes=T_SIZES)
    q_cap = int(qoff[-1]) - 37
    assert qoff[-2] < q_cap < qoff[-1]
    for tt, to in ((t, toff), (t[:333], None)):
        idx, dist = _knn_device(ctx, q, qoff, tt, to, 2, q_cap=q_cap, extra=64)
        ridx, rdist = _ref_knn(q, qoff, tt, to, 2, q_cap=q_cap)
        _check_live(idx, dist, ridx, rdist, qoff, q_cap, "q_cap clamp")
    # a first offset above 0: the rows before it are untouched too
    qoff2 = qoff.copy()
    qoff2[0] = qoff2[1] = 1
    idx, dist = _knn_device(ctx, q, qoff2, t, toff, 2, q_cap=q_cap, extra=64)
    ridx, rdist = _ref_knn(q, qoff2, t, toff, 2, q_cap=q_cap)
    _check_live(idx, dist, ridx, rdist, qoff2, q_cap, "qoff[0] > 0")


@pytest.mark.gpu
@pytest.mark.parametrize("t_sizes,straddler", [(T_SIZES, 6), (T_SIZES_ROT, 7)], ids=["issue", "rotated"])
def test_gpu_train_capacity_clamp(ctx, t_sizes, straddler):
    """toff[-1] = t_cap + 37 (rotated: the straddling train segment is the one the
    200 queries search; issue sizes: their train segment is clipped away
    entirely).  The train rows past t_cap are copies of those queries, so a
    read past t_cap would win with distance 0."""
    q, qoff, t, toff = _case(26, Q_SIZES, t_sizes=t_sizes)
    t_cap = int(toff[straddler + 1]) - 37
    assert toff[straddler] < t_cap < toff[straddler + 1]
    tp = t.copy()
    tp[t_cap:] = q[qoff[7]:qoff[7] + len(t) - t_cap]
    idx, dist = _knn_device(ctx, q, qoff, tp, toff, 2, t_cap=t_cap, extra=64)
    ridx, rdist = _ref_knn(q, qoff, t, toff, 2, t_cap=t_cap)
    _check_live(idx, dist, ridx, rdist, qoff, len(q), "t_cap clamp")
    if straddler == 6:
        assert (idx[qoff[7]:qoff[8]] == -1).all()    # its train segment lies past t_cap entirely
    idx, dist = _knn_device(ctx, q, qoff, tp, None, 2, t_cap=t_cap, extra=64)
    ridx, rdist = _ref_knn(q, qoff, t, None, 2, t_cap=t_cap)
    _check_live(idx, dist, ridx, rdist, qoff, len(q), "t_cap clamp, shared")


@pytest.mark.gpu
def test_gpu_match_capacity_clamp(ctx, siftgpu):
    """m_cap below the kept count: m_cap records, true totals in moff, sentinel intact."""
    q, qoff, t, toff = _case(27, Q_SIZES, t_sizes=T_SIZES)
    rng = np.random.default_rng(28)
    qk, tk = _kpts(siftgpu, rng, len(q)), _kpts(siftgpu, rng, len(t))
    ridx, rdist = _ref_knn(q, qoff, t, toff, 2)
    rec, rmoff, rsrc, rdst = _ref_ratio(ridx, rdist, qoff, len(q), 0.97, qk, tk, toff)
    m_cap = len(rec) - 11
    assert m_cap > 64
    m, moff, src, dst = _ratio_device(ctx, siftgpu, ridx, rdist, qoff, len(q), 0.97, qk, tk, toff, m_cap=m_cap,
                                      extra=64)
    assert_bits_equal(moff, rmoff, "moff holds the true totals")
    assert_bits_equal(m[:m_cap], _rec_array(siftgpu, rec)[:m_cap], "records")
    assert_bits_equal(src[:m_cap], rsrc[:m_cap], "src_xy")
    assert_bits_equal(dst[:m_cap], rdst[:m_cap], "dst_xy")
    assert (m[m_cap:].view(np.int32) == -77).all() and (src[m_cap:] == -5.0).all() and (dst[m_cap:] == -5.0).all()
    # and with the query offsets running past q_cap: the clamped rows only
    q_cap = len(q) - 37
    rec, rmoff, rsrc, rdst = _ref_ratio(ridx, rdist, qoff, q_cap, 0.97, qk, tk, toff)
    m, moff, src, dst = _ratio_device(ctx, siftgpu, ridx, rdist, qoff, q_cap, 0.97, qk, tk, toff, extra=64)
    n = len(rec)
    assert_bits_equal(moff, rmoff, "moff, clamped")
    assert_bits_equal(m[:n], _rec_array(siftgpu, rec), "records, clamped")
    assert_bits_equal(src[:n], rsrc, "src_xy, clamped")
    assert (m[n:].view(np.int32) == -77).all() and (src[n:] == -5.0).all()


@pytest.mark.gpu
def test_gpu_ratio_stage_crafted(ctx, siftgpu):
    """test_ratio_test_semantics' pairs through the device: (0.86f, 1.0f) is
    rejected and (0.859f, 1.0f) kept (the comparison is in double); idx2 = -1 is
    skipped; empty segments and one with nothing kept; record order, segment
    field, moff; xy bytes with keypoints and none written without."""
    sizes = [0, 3, 0, 2, 300, 0, 4, 0]
    qoff = _offsets(sizes)
    n = int(qoff[-1])
    rng = np.random.default_rng(29)
    idx = np.stack([rng.integers(0, 50, n), rng.integers(0, 50, n)], 1).astype(np.int32)
    d2 = rng.random(n).astype(np.float32) + np.float32(0.5)
    d1 = (d2 * rng.choice(np.array([0.5, 0.85, 0.87, 0.99], np.float32), n)).astype(np.float32)
    dist = np.stack([d1, d2], 1)
    a = int(qoff[1])                                      # segment 1: the three rows of test_ratio_test_semantics
    idx[a:a + 3] = [[3, 4], [5, -1], [1, 2]]
    dist[a:a + 3] = [[0.86, 1.0], [0.1, np.inf], [0.9, 1.0]]
    c = int(qoff[3])                                      # segment 3: nothing kept
    dist[c:c + 2] = [[0.9, 1.0], [1.0, 1.0]]
    e = int(qoff[6])                                      # segment 6: the kept boundary pair, a skip, equal pair at ratio 1
    idx[e:e + 4] = [[7, 8], [9, -1], [2, 1], [4, 6]]
    dist[e:e + 4] = [[0.859, 1.0], [0.0, np.inf], [0.5, 1.0], [0.875, 1.0]]
    qk, tk = _kpts(siftgpu, rng, n), _kpts(siftgpu, rng, 50)
    rec, rmoff, rsrc, rdst = _ref_ratio(idx, dist, qoff, n, M.RATIO, qk, tk, None)
    assert rmoff[2] - rmoff[1] == 0 and rmoff[4] - rmoff[3] == 0           # 0.86f rejected; segment 3 empty
    assert [r[:2] for r in rec if r[3] == 6] == [(0, 7), (2, 2)]            # 0.859f kept
    m, moff, src, dst = _ratio_device(ctx, siftgpu, idx, dist, qoff, n, M.RATIO, qk, tk, None, extra=64)
    k = len(rec)
    assert_bits_equal(moff, rmoff, "moff")
    assert_bits_equal(m[:k], _rec_array(siftgpu, rec), "records")
    assert (np.diff(m["segment"][:k]) >= 0).all()
    assert_bits_equal(src[:k], rsrc, "src_xy")
    assert_bits_equal(dst[:k], rdst, "dst_xy")
    assert (m[k:].view(np.int32) == -77).all() and (src[k:] == -5.0).all() and (dst[k:] == -5.0).all()
    # segmented train offsets move the train keypoint base, not the records
    toff = _offsets([3, 5, 0, 9, 11, 2, 8, 12])
    tk2 = _kpts(siftgpu, rng, int(toff[-1]) + 50)
    rec2, _, rsrc2, rdst2 = _ref_ratio(idx, dist, qoff, n, M.RATIO, qk, tk2, toff)
    m2, moff2, src2, dst2 = _ratio_device(ctx, siftgpu, idx, dist, qoff, n, M.RATIO, qk, tk2, toff)
    assert_bits_equal(m2[:k], m[:k], "records, segmented train")
    assert_bits_equal(dst2[:k], rdst2, "dst_xy, segmented train")
    # no keypoints: records and moff as before, no xy written
    m3, moff3, src3, dst3 = _ratio_device(ctx, siftgpu, idx, dist, qoff, n, M.RATIO)
    assert_bits_equal(m3[:k], m[:k], "records without keypoints")
    assert_bits_equal(moff3, rmoff, "moff without keypoints")
    assert (src3 == -5.0).all() and (dst3 == -5.0).all()


CROPS = [(0, 0), (7, 11), (3, 5), (12, 2)]   # (dy, dx) of the four book_image() crops


@pytest.mark.gpu
def test_gpu_batch_flow_in_stream_order(ctx, siftgpu):
    """detect_compute_batch on four crops, then -- with no sync in between --
    the consecutive-frame matcher (train = query, t_offsets = q_offsets + 1, 3
    segments) and the ratio stage with keypoints; one sync, then download.
    Every segment equals the oracle's kNN + ratio test on the downloaded
    descriptors, the xy are the downloaded keypoints' (x, y), and per segment
    >= 10 matches are kept of which >= 80 % agree with the crops' relative
    shift within 1.5 px (test_gpu_reference_app_flow's bounds).
    The CPU oracle (oracle.py SIFT + M.knn_match + M.ratio_test) on these crops
    keeps 89 / 105 / 91 matches of which 82 / 103 / 85 agree (92 / 98 / 93 %)."""
    import torch
    img = book_image()
    R, C = img.shape[0] - 16, img.shape[1] - 16
    B = len(CROPS)
    imgs = torch.from_numpy(np.stack([img[dy:dy + R, dx:dx + C] for dy, dx in CROPS])).contiguous().cuda()
    cap = 1024
    kpts = torch.zeros((cap, 7), dtype=torch.int32, device="cuda")
    desc = torch.zeros((cap, 128), dtype=torch.float32, device="cuda")
    offs = torch.zeros((B + 1,), dtype=torch.int32, device="cuda")
    idx = torch.full((cap, 2), -77, dtype=torch.int32, device="cuda")
    dist = torch.full((cap, 2), -5.0, dtype=torch.float32, device="cuda")
    mt = torch.full((cap, 4), -77, dtype=torch.int32, device="cuda")
    src = torch.full((cap, 2), -5.0, dtype=torch.float32, device="cuda")
    dst = torch.full((cap, 2), -5.0, dtype=torch.float32, device="cuda")
    moff = torch.full((B,), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # warm the matcher's scratch so that the three calls below enqueue without a wait
    ctx.knn_match_segmented_device(desc.data_ptr(), offs.data_ptr(), B - 1, cap, desc.data_ptr(),
                                   offs.data_ptr() + 4, cap, 2, idx.data_ptr(), dist.data_ptr())
    ctx.sync()
    ctx.detect_compute_batch(imgs.data_ptr(), B, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                             offs.data_ptr())
    ctx.knn_match_segmented_device(desc.data_ptr(), offs.data_ptr(), B - 1, cap, desc.data_ptr(),
                                   offs.data_ptr() + 4, cap, 2, idx.data_ptr(), dist.data_ptr())
    ctx.ratio_matches_device(idx.data_ptr(), dist.data_ptr(), offs.data_ptr(), B - 1, cap, M.RATIO,
                             kpts.data_ptr(), kpts.data_ptr(), offs.data_ptr() + 4, mt.data_ptr(), src.data_ptr(),
                             dst.data_ptr(), cap, moff.data_ptr())
    ctx.sync()
    o = offs.cpu().numpy()
    assert 0 < o[-1] <= cap and (np.diff(o) > 0).all()
    kp = kpts.cpu().numpy().view(siftgpu.KEYPOINT_DTYPE).reshape(-1)
    d = desc.cpu().numpy()
    ridx, rdist = _ref_knn(d, o[:-1], d, o[1:], 2, q_cap=cap, t_cap=cap)
    _check_live(idx.cpu().numpy(), dist.cpu().numpy(), ridx, rdist, o[:-1], cap, "consecutive frames")
    rec, rmoff, rsrc, rdst = _ref_ratio(ridx, rdist, o[:-1], cap, M.RATIO, kp, kp, o[1:])
    m = mt.cpu().numpy().view(siftgpu.MATCH_DTYPE).reshape(-1)
    n = len(rec)
    assert_bits_equal(moff.cpu().numpy(), rmoff, "moff")
    assert_bits_equal(m[:n], _rec_array(siftgpu, rec), "records")
    assert_bits_equal(src.cpu().numpy()[:n], rsrc, "src_xy")
    assert_bits_equal(dst.cpu().numpy()[:n], rdst, "dst_xy")
    assert (m[n:].view(np.int32) == -77).all()
    s, t = src.cpu().numpy(), dst.cpu().numpy()
    for b in range(B - 1):
        sl = slice(int(rmoff[b]), int(rmoff[b + 1]))
        sy, sx = CROPS[b][0] - CROPS[b + 1][0], CROPS[b][1] - CROPS[b + 1][1]
        kept = sl.stop - sl.start
        assert kept >= 10, (b, kept)
        ok = int(np.count_nonzero((np.abs(s[sl, 0] + sx - t[sl, 0]) < 1.5) & (np.abs(s[sl, 1] + sy - t[sl, 1]) < 1.5)))
        assert ok >= 0.8 * kept, (b, ok, kept)


@pytest.mark.gpu
def test_gpu_host_forms_equal_device_forms(ctx, siftgpu):
    q, qoff, t, toff = _case(22, Q_SIZES, t_sizes=T_SIZES)
    rng = np.random.default_rng(30)
    qk, tk = _kpts(siftgpu, rng, len(q)), _kpts(siftgpu, rng, len(t))
    for k in (2, 1):
        di, dd = _knn_device(ctx, q, qoff, t, toff, k)
        hi, hd = ctx.knnMatchSegmented(q, qoff, t, toff, k)
        assert_bits_equal(hi, di, f"host idx k={k}")
        assert_bits_equal(hd, dd, f"host dist k={k}")
    si, sd = ctx.knnMatchSegmented(q, qoff, t[:333], None, 2)
    ri, rd = _ref_knn(q, qoff, t[:333], None, 2)
    assert_bits_equal(si, ri, "host shared idx")
    assert_bits_equal(sd, rd, "host shared dist")
    di, dd = _knn_device(ctx, q, qoff, t, toff, 2)
    for ratio in (M.RATIO, 0.97):
        m, moff, src, dst = _ratio_device(ctx, siftgpu, di, dd, qoff, len(q), ratio, qk, tk, toff)
        hm, hmoff, hsrc, hdst = ctx.ratioMatches(di, dd, qoff, ratio, qk, tk, toff)
        n = int(moff[-1])
        assert len(hm) == n
        assert_bits_equal(hmoff, moff, "host moff")
        assert_bits_equal(hm, m[:n], "host records")
        assert_bits_equal(hsrc, src[:n], "host src_xy")
        assert_bits_equal(hdst, dst[:n], "host dst_xy")
    hm2, hmoff2, s2, d2 = ctx.ratioMatches(di, dd, qoff, M.RATIO)
    assert s2 is None and d2 is None
    assert_bits_equal(hmoff2, _ref_ratio(di, dd, qoff, len(q))[1], "host moff, no keypoints")
