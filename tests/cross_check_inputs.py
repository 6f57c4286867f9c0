"""Inputs and the reference of the cross-check (mutual nearest neighbour) stage.

The reference is a restatement of the keep rule of include/sift_hip.h
(sift_cross_check_matches_device) in plain loops, and a brute-force matcher per
metric: int64 sums for byte rows (match_u8_inputs / match_l2_inputs), and for
float rows oracle/match.py's distance with a stable argsort (M.knn_match).
Everything is built once (lru_cache) and shared, read-only.

keep_flags()   per query row: live, passes the reverse test, passes the ratio test.
stage_ref()    records, m_offsets and point pairs from two tables.
crafted()      idx / ridx / dist tables written directly, no descriptors.
descriptors()  three segments per metric with planted duplicates; frames().
"""
import functools

import numpy as np

import match as M
import match_l2_inputs as L2
import match_u8_inputs as U

MATCH_DTYPE = np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<f4"), ("segment", "<i4")])
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
L1_F32, L1_U8, L2SQR_U8 = 0, 1, 2
METRIC_IDS = ["l1_f32", "l1_u8", "l2sqr_u8"]
RATIO = 0.86
RATIOS = [0.0, RATIO, RATIO * RATIO]
# non-zero float32 (d0, d1) with d0 == ratio * d1 exactly in double (the product is rounded to double)
EXACT = {RATIO: (43.0, 50.0), RATIO * RATIO: (16641.0, 22500.0)}
SENT_I, SENT_F = -77, -5.0


def clamped(off, cap):
    return np.clip(np.asarray(off, np.int64), 0, cap)


def _cols(a):
    a = np.asarray(a)
    return a.reshape(len(a), -1)


# ---- the keep rule -------------------------------------------------------------------
def keep_flags(idx, dist, ridx, qoff, toff, q_cap, t_cap, ratio):
    """(seg, rev_ok, ratio_ok) per row of [0, q_cap): seg is the row's segment or -1
    for a row of no segment; rev_ok: j = idx[i][0] >= 0 is a row of the segment's
    clamped train range and ridx[tlo + j][0] == i - qlo; ratio_ok: ratio == 0, or
    idx[i][1] >= 0 and (double)dist[i][0] <= ratio * (double)dist[i][1].  No value of
    a row outside the live range is looked at."""
    idx, ridx = _cols(idx), _cols(ridx)
    dist = None if dist is None else _cols(dist)
    qo, to = clamped(qoff, q_cap), clamped(toff, t_cap)
    seg = np.full(q_cap, -1, np.int64)
    rev_ok = np.zeros(q_cap, bool)
    ratio_ok = np.zeros(q_cap, bool)
    for b in range(len(qo) - 1):
        for i in range(int(qo[b]), int(qo[b + 1])):
            seg[i] = b
            j = int(idx[i, 0])
            rev_ok[i] = j >= 0 and to[b] + j < to[b + 1] and int(ridx[to[b] + j, 0]) == i - qo[b]
            if ratio > 0:
                ratio_ok[i] = j >= 0 and int(idx[i, 1]) >= 0 and float(dist[i, 0]) <= ratio * float(dist[i, 1])
            else:
                ratio_ok[i] = j >= 0
    return seg, rev_ok, ratio_ok


def stage_ref(idx, dist, ridx, qoff, toff, q_cap, t_cap, ratio, q_kpts=None, t_kpts=None):
    """(records [MATCH_DTYPE], m_offsets int32 [n_segments + 1], src_xy, dst_xy float32 [n, 2]
    or None, flags) in query order within a segment and in segment order overall."""
    flags = keep_flags(idx, dist, ridx, qoff, toff, q_cap, t_cap, ratio)
    seg, rev_ok, ratio_ok = flags
    idx, dist = _cols(idx), _cols(dist)
    qo, to = clamped(qoff, q_cap), clamped(toff, t_cap)
    rows = np.flatnonzero((seg >= 0) & rev_ok & ratio_ok)
    rec = np.zeros(len(rows), MATCH_DTYPE)
    b = seg[rows]
    rec["query"], rec["train"], rec["distance"], rec["segment"] = rows - qo[b], idx[rows, 0], dist[rows, 0], b
    moff = np.array([np.count_nonzero(rows < qo[s]) for s in range(len(qo))], np.int32)
    src = dst = None
    if q_kpts is not None:
        tg = to[b] + idx[rows, 0]
        src = np.stack([q_kpts["x"][rows], q_kpts["y"][rows]], 1).astype(np.float32).reshape(-1, 2)
        dst = np.stack([t_kpts["x"][tg], t_kpts["y"][tg]], 1).astype(np.float32).reshape(-1, 2)
    return rec, moff, src, dst, flags


def knn_from_distances(d, k):
    """The matchers' order on a distance matrix: stable argsort, the lower index first."""
    d = np.asarray(d)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(d, order, axis=1).astype(np.float32)


# ---- a hand-written 6 x 5 case ---------------------------------------------------------
# Column 0 ties between q0 and q1 (q0, the lower, wins: q1 is one-sided); q2 ties between
# t1 and t2 (t1 wins, and t1's nearest is q2); q3 and q4 both choose t3, whose nearest is
# q4; column 4 ties between q3 and q5 (q3 wins, but q3 chose t3: q5 is one-sided).
HAND_D = np.array([[1, 5, 5, 9, 9],
                   [1, 4, 6, 9, 9],
                   [7, 3, 3, 8, 8],
                   [9, 9, 9, 2, 6],
                   [9, 9, 9, 1, 7],
                   [9, 9, 9, 9, 6]], np.float32)
HAND_IDX = [[0, 1], [0, 1], [1, 2], [3, 4], [3, 4], [4, 0]]
HAND_RIDX = [0, 2, 2, 4, 3]
HAND_KEPT = [(0, 0), (2, 1), (4, 3)]          # (query, train), cross-check only
HAND_KEPT_RATIO = [(0, 0), (4, 3)]            # and the 0.86 ratio test: q2's 3 <= 0.86 * 3 fails


# ---- keypoints -------------------------------------------------------------------------
def kpts(rng, n):
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"] = rng.random(n).astype(np.float32) * 1000
    k["y"] = rng.random(n).astype(np.float32) * 1000
    k["size"] = 3
    return k


# ---- crafted tables ------------------------------------------------------------------
# The first group: the stage's 256-row block and its neighbours, two blocks and a row,
# with an empty segment between two full ones; then 257 segments of 0-3 rows.
GROUP1 = [255, 256, 0, 257, 513]
N_SMALL = 257
Q_FIRST, T_FIRST = 3, 2
EXTRA = 64                                     # rows past the capacities in every buffer
GARBAGE = np.array([0x7fffffff, -0x80000000, -123456789, 0x7ffffff0], np.int64).astype(np.int32)


class Crafted:
    pass


@functools.lru_cache(maxsize=None)
def crafted(variant):
    """variant "overflow": the last offsets exceed q_cap and t_cap (the batch call's overflow
    convention: the last segments are clipped); "slack": both buffers have 40 rows of
    no segment after the last offset.  The rows of no segment of idx (before the first
    offset, past the last, and the EXTRA rows past q_cap) hold 0x7fffffff and negative
    garbage.  ridx has EXTRA rows past t_cap, so a j that a correct stage rejects by
    its bound still names a row of the buffer.
    Tables are [rows][2]; column 1 of idx / dist is the second neighbour (the ratio
    test), column 1 of ridx is never read.  Planted per segment: mutual pairs, one-sided
    pairs, idx -1, a reverse entry equal to the query's global row number, a mutual
    pair on the segment's last train row, a j one past the train range whose row names
    the query, and dist pairs exactly at and either side of each ratio's boundary."""
    rng = np.random.default_rng(71 + (variant == "slack"))
    q_sizes = GROUP1 + rng.integers(0, 4, N_SMALL).tolist()
    t_sizes = [n + 5 for n in GROUP1] + rng.integers(0, 5, N_SMALL).tolist()
    t_sizes[2] = 4                              # the empty query segment has train rows
    qoff, toff = U.offsets(q_sizes, Q_FIRST), U.offsets(t_sizes, T_FIRST)
    c = Crafted()
    c.variant, c.qoff, c.toff = variant, qoff, toff
    c.q_cap = int(qoff[-1]) + (40 if variant == "slack" else -2)
    c.t_cap = int(toff[-1]) + (40 if variant == "slack" else -12)   # deeper: live query rows whose train range is clipped
    nq, nt = c.q_cap + EXTRA, c.t_cap + EXTRA
    idx = np.full((nq, 2), -1, np.int32)
    ridx = np.full((nt, 2), -1, np.int32)
    d1 = rng.random(nq).astype(np.float32) + np.float32(0.5)
    d0 = (d1 * rng.choice(np.array([0.5, 0.7, 0.8, 0.99], np.float32), nq)).astype(np.float32)
    qo, to = clamped(qoff, c.q_cap), clamped(toff, c.t_cap)
    for b in range(len(q_sizes)):
        ql, qn, tl, tn = int(qo[b]), int(qo[b + 1] - qo[b]), int(to[b]), int(to[b + 1] - to[b])
        if qn:                                  # one-sided at random, a second neighbour for most rows
            idx[ql:ql + qn, 0] = rng.integers(0, tn, qn) if tn else -1
            idx[ql:ql + qn, 1] = rng.integers(0, tn, qn) if tn else -1
            idx[ql:ql + qn, 1][rng.random(qn) < 0.1] = -1
        if tn:
            ridx[tl:tl + tn, 0] = rng.integers(0, qn, tn) if qn else -1
        n = min(qn, tn)
        if n == 0:
            continue
        rows, cols = rng.permutation(qn)[:n], rng.permutation(tn)[:n]
        m = max(1, n // 2)                      # mutual pairs
        idx[ql + rows[:m], 0], ridx[tl + cols[:m], 0] = cols[:m], rows[:m]
        if n >= 4:
            idx[ql + rows[m], 0] = -1                                                    # no neighbour
            idx[ql + rows[m + 1], 0], ridx[tl + cols[m + 1], 0] = cols[m + 1], ql + rows[m + 1]  # global row number
        if n >= 2:                              # a mutual pair on the last train row
            r = rows[0]
            idx[ql + r, 0], ridx[tl + tn - 1, 0] = tn - 1, r
    for b in range(len(q_sizes)):               # one past the train range: the next segment's row 0, or past t_cap
        ql, qn, tl, tn = int(qo[b]), int(qo[b + 1] - qo[b]), int(to[b]), int(to[b + 1] - to[b])
        if qn and tl + tn >= c.t_cap:
            ridx[tl + tn, 0] = qn - 1
        v = int(ridx[tl + tn, 0])
        if 0 <= v < qn:
            idx[ql + v, 0] = tn
    # At each ratio's boundary, on rows that pass the reverse test.  The stage compares
    # (double)d0 with the ROUNDED double product ratio * (double)d1, so d0 == ratio * d1 holds
    # exactly for many float32 pairs -- among them integer distances as the byte matchers
    # produce them: 0.86 * 50 == 43 and (0.86 * 0.86) * 22500 == 16641 (129^2 / 150^2) in
    # double.  Per ratio: that exact pair (kept), the pair one float32 ulp above it
    # (rejected), and for d1 = 1 the two float32 either side of the ratio (float32(0.86) is
    # above the double 0.86: rejected; the one below: kept).  And (0, 0), kept by every ratio.
    live = np.arange(int(qo[0]), int(qo[-1]))
    seg, rev_ok, _ = keep_flags(idx, None, ridx, qoff, toff, c.q_cap, c.t_cap, 0.0)
    good = [i for i in live if rev_ok[i] and idx[i, 1] >= 0]
    assert len(good) > 64
    pairs = [(0.0, 0.0)]
    for r in RATIOS[1:]:
        e0, e1 = EXACT[r]
        above = np.float32(r) if float(np.float32(r)) > r else np.nextafter(np.float32(r), np.float32(2))
        pairs += [(e0, e1), (np.nextafter(np.float32(e0), np.float32(np.inf)), e1), (above, 1.0),
                  (np.nextafter(above, np.float32(0)), 1.0)]
    for n, (a, bb) in enumerate(pairs):
        d0[good[3 * n]], d1[good[3 * n]] = a, bb
    rows = [int(good[3 * n]) for n in range(len(pairs))]
    # row of (0, 0); then per ratio (exact, one ulp above the exact, above at d1 = 1, below at d1 = 1)
    c.zero_row, c.boundary_rows = rows[0], {RATIOS[1]: rows[1:5], RATIOS[2]: rows[5:9]}
    dead = np.r_[0:int(qo[0]), int(qo[-1]):nq]
    idx[dead] = GARBAGE[rng.integers(0, len(GARBAGE), (len(dead), 2))]
    ridx[:, 1] = GARBAGE[rng.integers(0, len(GARBAGE), nt)]
    c.idx, c.ridx, c.dist = idx, ridx, np.stack([d0, d1], 1)
    c.q_kpts, c.t_kpts = kpts(rng, nq), kpts(rng, nt)
    c.n_group1 = len(GROUP1)
    for a in (c.idx, c.ridx, c.dist, c.q_kpts, c.t_kpts):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def crafted_ref(variant, ratio):
    c = crafted(variant)
    return stage_ref(c.idx, c.dist, c.ridx, c.qoff, c.toff, c.q_cap, c.t_cap, ratio, c.q_kpts, c.t_kpts)


def tables(c, fwd_k, rev_k, ratio):
    """The crafted tables with fwd_k / rev_k columns; a column the stage must not read is poisoned."""
    idx, dist, ridx = c.idx[:, :fwd_k].copy(), c.dist[:, :fwd_k].copy(), c.ridx[:, :rev_k].copy()
    if fwd_k == 2 and ratio == 0:
        idx[:, 1] = GARBAGE[np.arange(len(idx)) % len(GARBAGE)]
        dist[:, 1] = np.nan
    return np.ascontiguousarray(idx), np.ascontiguousarray(dist), np.ascontiguousarray(ridx)


# ---- descriptors -----------------------------------------------------------------------
Q_SIZES, T_SIZES = [70, 129, 300], [65, 300, 128]


def _rows(rng, n, metric):
    if metric == L1_F32:
        x = rng.random((n, 128)).astype(np.float32) ** 3
        x /= x.sum(1, keepdims=True)
        return np.sqrt(x).astype(np.float32)
    return rng.integers(0, 256, (n, 128), dtype=np.uint8)


def seg_knn(q, qoff, t, toff, k, metric, q_cap=None, t_cap=None):
    """The brute-force segmented matcher of the metric: (idx, dist) [q_cap, k]."""
    if metric == L1_U8:
        return U.seg_ref(q, qoff, t, toff, k, q_cap, t_cap)
    if metric == L2SQR_U8:
        return L2.seg_ref(q, qoff, t, toff, k, q_cap, t_cap)
    q_cap = len(q) if q_cap is None else q_cap
    t_cap = len(t) if t_cap is None else t_cap
    qo, to = clamped(qoff, q_cap), clamped(toff, t_cap)
    idx = np.full((q_cap, k), -1, np.int32)
    dist = np.full((q_cap, k), np.inf, np.float32)
    for b in range(len(qo) - 1):
        if qo[b + 1] > qo[b]:
            idx[qo[b]:qo[b + 1]], dist[qo[b]:qo[b + 1]] = M.knn_match(q[qo[b]:qo[b + 1]],
                                                                      t[to[b]:max(to[b], to[b + 1])], k)
    return idx, dist


class Desc:
    pass


def _finish(c, metric):
    c.metric = metric
    c.q_cap, c.t_cap = len(c.q), len(c.t)
    c.idx, c.dist = seg_knn(c.q, c.qoff, c.t, c.toff, 2, metric)
    c.ridx, _ = seg_knn(c.t, c.toff, c.q, c.qoff, 1, metric)
    for a in (c.q, c.t, c.idx, c.dist, c.ridx, c.q_kpts, c.t_kpts):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def descriptors(metric):
    """3 query segments of 70 / 129 / 300 rows against train segments of 65 / 300 / 128
    rows.  Planted in every segment: two queries (rows 3 and 40) identical to train row
    7 -- the train row's two nearest queries tie at 0 and row 3 wins -- and two train
    rows (11 and 50) identical to query 20, which takes 11."""
    rng = np.random.default_rng(81 + metric)
    c = Desc()
    c.qoff, c.toff = U.offsets(Q_SIZES), U.offsets(T_SIZES)
    c.q, c.t = _rows(rng, int(c.qoff[-1]), metric), _rows(rng, int(c.toff[-1]), metric)
    for b in range(3):
        ql, tl = int(c.qoff[b]), int(c.toff[b])
        c.q[ql + 3] = c.q[ql + 40] = c.t[tl + 7]
        c.t[tl + 11] = c.t[tl + 50] = c.q[ql + 20]
    c.q_kpts, c.t_kpts = kpts(rng, len(c.q)), kpts(rng, len(c.t))
    return _finish(c, metric)


@functools.lru_cache(maxsize=None)
def frames(metric):
    """Consecutive frames of a 4-frame set (90 / 140 / 0 / 75 rows; an empty frame in
    the middle): query segment b is frame b, its train segment frame b + 1 of the same
    buffer -- t_offsets = q_offsets + 1.  Frame 1 repeats rows of frame 0."""
    rng = np.random.default_rng(91 + metric)
    c = Desc()
    c.off = U.offsets([90, 140, 0, 75])
    d = _rows(rng, int(c.off[-1]), metric)
    d[90 + 5] = d[90 + 60] = d[10]
    d[33] = d[44] = d[90 + 100]
    c.q = c.t = d
    c.qoff, c.toff = c.off[:-1], c.off[1:]
    c.q_kpts = c.t_kpts = kpts(rng, len(d))
    return _finish(c, metric)


def ratio_of(metric):
    return RATIO * RATIO if metric == L2SQR_U8 else RATIO
