"""Inputs and the restatement of the epipolar matcher
(sift_knn_match_epipolar_segmented_device, include/sift_hip.h), numpy only.

epipolar_ref() is brute force:
  * the window test is match_window_inputs.admissible_row around the query's own
    position;
  * the band test is fmath::is_inlier in np.float32, operation by operation in
    its order (the nine coefficients cast to float32, a = (f0 x + f1 y) + f2 ...,
    s = 1 / (a a + b b), d = (X a + Y b) + c, (d d) s <= t for the dst side and
    the same with F transposed for the src side, t = float32(band * band) with
    the product in float64); a NaN compares false;
  * the k nearest admissible rows by match_window_inputs.dense_seg_ref's rule:
    a stable sort on (distance, local index), a float row at +inf never a
    neighbour.
Everything is built once (lru_cache) and shared, read-only.
"""
import functools
import math

import numpy as np

import match_u8_inputs as U
import match_window_inputs as W

f32 = np.float32
ROWS, COLS = 64, 96
BAND, RADIUS = 3.0, f32(20.0)
WIN_GROUP = W.WIN_GROUP
INF = float("inf")


def limit(band):
    with np.errstate(over="ignore"):
        return f32(np.float64(band) * np.float64(band))


def errors(F9, x, y, X, Y):
    """(err_dst, err_src) float32 arrays over the train rows for one query, in is_inlier's order."""
    f = np.asarray(F9, np.float64).reshape(9).astype(np.float32)
    x, y = f32(x), f32(y)
    X, Y = np.asarray(X, np.float32), np.asarray(Y, np.float32)
    with np.errstate(all="ignore"):
        a = f[0] * x + f[1] * y + f[2]
        b = f[3] * x + f[4] * y + f[5]
        c = f[6] * x + f[7] * y + f[8]
        s_dst = f32(1) / (a * a + b * b)
        d_dst = X * a + Y * b + c
        a2 = f[0] * X + f[3] * Y + f[6]
        b2 = f[1] * X + f[4] * Y + f[7]
        c2 = f[2] * X + f[5] * Y + f[8]
        s_src = f32(1) / (a2 * a2 + b2 * b2)
        d_src = x * a2 + y * b2 + c2
        e_dst, e_src = d_dst * d_dst * s_dst, d_src * d_src * s_src
    for v in (a, s_dst, d_dst, a2, s_src, d_src, e_dst, e_src):
        assert v.dtype == np.float32
    return e_dst, e_src


def band_row(F9, x, y, X, Y, band):
    """bool [n_train]: both errors <= float32(band^2); a NaN error is False."""
    e_dst, e_src = errors(F9, x, y, X, Y)
    t = limit(band)
    with np.errstate(invalid="ignore"):
        return (e_dst <= t) & (e_src <= t)


def has_model(F, found, b):
    return F is not None and not (found is not None and found[b] == 0)


def seg_of(qo, i):
    """The segment of live row i: the largest b with qo[b] <= i, found by the matchers'
    bisection (for offsets that do not decrease, the segment whose range holds i)."""
    lo, hi = 0, len(qo) - 1
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if qo[mid] <= i:
            lo = mid
        else:
            hi = mid
    return lo


def epipolar_ref(metric, q, qk, qoff, t, tk, toff, F=None, found=None, band=BAND, radius=RADIUS, k=2, q_cap=None,
                 t_cap=None):
    """(idx int32, dist float32 [q_cap, k], adm): rows of no segment stay -1 / +inf; adm[i] is
    the array of admissible local train rows of live query i (None elsewhere)."""
    q_cap = len(q) if q_cap is None else q_cap
    t_cap = len(t) if t_cap is None else t_cap
    qo = U.clamped(qoff, q_cap)
    to = None if toff is None else U.clamped(toff, t_cap)
    Fm = None if F is None else np.asarray(F, np.float64).reshape(-1, 9)
    idx = np.full((q_cap, k), -1, np.int32)
    dist = np.full((q_cap, k), np.inf, np.float32)
    adm_of = [None] * q_cap
    live = np.arange(int(qo[0]), int(qo[-1]))
    seg = np.array([seg_of(qo, i) for i in live], np.int64)
    for b in np.unique(seg):
        rows = live[seg == b]
        tl, th = (0, t_cap) if to is None else (int(to[b]), int(max(to[b], to[b + 1])))
        tx, ty = tk["x"][tl:th].astype(np.float32), tk["y"][tl:th].astype(np.float32)
        d = W.distances(metric, q[rows], t[tl:th]) if th > tl else np.zeros((len(rows), 0))
        for r, i in enumerate(rows):
            x, y = qk["x"][i], qk["y"][i]
            ok = W.admissible_row(x, y, tx, ty, radius)
            if has_model(Fm, found, b):
                ok = ok & band_row(Fm[b], x, y, tx, ty, band)
            adm = np.flatnonzero(ok)
            adm_of[i] = adm
            di = d[r, adm]
            if metric == W.L1_F32:
                adm, di = adm[di != np.inf], di[di != np.inf]
            order = np.argsort(di, kind="stable")[:k]
            idx[i, :len(order)] = adm[order]
            dist[i, :len(order)] = di[order]
    return idx, dist, adm_of


# scratch.hpp's window_cell_cap / epipolar_grid at scale 1, for the census of the crowded cell
def grid_of(radius, band, rows, cols, t_cap, n_grids):
    per = (t_cap + n_grids - 1) // n_grids * 4
    cap = 1 if per < 1 else min(per, 4096)
    cell = max(min(float(radius), float(band)), 1.0)
    if not cell <= 2e9:
        return 1, 1, f32(0)
    while True:
        nx, ny = math.ceil(cols / cell), math.ceil(rows / cell)
        if nx * ny <= cap:
            return nx, ny, f32(1.0 / cell)
        cell *= 1.125


def cell_of(v, inv_cell, n):
    with np.errstate(all="ignore"):
        return np.clip(np.floor(np.asarray(v, np.float32) * f32(inv_cell)), 0, n - 1).astype(np.int64)


class Case:
    def __init__(self, name, metric, q, qk, qoff, t, tk, toff, F, found, band=BAND, radius=RADIUS, q_cap=None,
                 t_cap=None, rows=ROWS, cols=COLS):
        self.name, self.metric, self.q, self.qk, self.t, self.tk = name, metric, q, qk, t, tk
        self.qoff = np.asarray(qoff, np.int32)
        self.toff = None if toff is None else np.asarray(toff, np.int32)
        self.F = None if F is None else np.ascontiguousarray(F, np.float64).reshape(-1, 9)
        self.found = None if found is None else np.asarray(found, np.int32)
        self.band, self.radius, self.rows, self.cols = float(band), f32(radius), rows, cols
        self.q_cap = len(q) if q_cap is None else q_cap
        self.t_cap = len(t) if t_cap is None else t_cap
        self.idx, self.dist, self.adm = epipolar_ref(metric, q, qk, self.qoff, t, tk, self.toff, self.F, self.found,
                                                     self.band, self.radius, 2, self.q_cap, self.t_cap)
        for a in (self.q, self.qk, self.t, self.tk, self.idx, self.dist):
            a.setflags(write=False)

    def ref(self, k):
        return self.idx[:, :k], self.dist[:, :k]

    def live(self):
        qo = U.clamped(self.qoff, self.q_cap)
        return np.arange(int(qo[0]), int(qo[-1]))


# ---- the fundamental matrices of the edge case ----------------------------------------------
F_HORIZONTAL = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float64)      # rectified stereo: Y = y
F_VERTICAL = np.array([0, 0, -1, 0, 0, 0, 1, 0, 0], np.float64)        # X = x
# [e2]_x A with e2 = (48, 32) and A = [[1, .25, -8], [0, 1, 4], [0, 0, 1]]: the pencil through e2 in
# the train image; the query-side epipole is e1 = (49, 28), where F [e1; 1] is exactly (0, 0, 0)
F_OBLIQUE = np.array([0, -1, 28, 1, 0.25, -56, -32, 40, 448], np.float64)
E1, E2 = (49.0, 28.0), (48.0, 32.0)
CLUSTER_N = 12          # more than a lane group: a cell run that takes two steps of eight


def pencil_F(e2, A):
    """[e2]_x A for a 3 x 3 A: every query's line passes through e2."""
    ex = np.array([[0, -1, e2[1]], [1, 0, -e2[0]], [-e2[1], e2[0], 0]], np.float64)
    return (ex @ np.asarray(A, np.float64).reshape(3, 3)).reshape(9)


def _edge_points():
    """(query xy, train xy) per segment, metric-independent; the planted rows come first."""
    rng = np.random.default_rng(11)
    Q, T = [], []
    # 0: horizontal lines.  Query 0 (20, 30): train 0 admitted, train 1 in the band but outside the
    # window, train 2 exactly on the band's edge (|Y - y| = 3).  Query 1 (10, 30): train 3 lies
    # left of the image.  Query 2 (38, 30.2): CLUSTER_N rows within 0.04 px, all admitted.  Query 3
    # (80, 10): exactly one admissible row (train 4).  Query 4 (90, 60): none.
    cl = np.stack([40.5 + rng.random(CLUSTER_N) * 0.04, 30.2 + rng.random(CLUSTER_N) * 0.04], 1)
    T.append(np.concatenate([[[30, 30], [50, 30], [25, 33], [-5, 30.5], [85, 10.5]], cl,
                             np.stack([rng.random(23) * 70, 14 + rng.random(23) * 40], 1)]))
    Q.append(np.concatenate([[[20, 30], [10, 30], [38, 30.2], [80, 10], [90, 60]],
                             np.stack([rng.random(25) * 70, 14 + rng.random(25) * 40], 1)]))
    # 1: vertical lines over a cloud that leaves the extent on every side
    T.append(np.stack([-10 + rng.random(26) * 115, -10 + rng.random(26) * 85], 1))
    Q.append(np.stack([rng.random(20) * 96, rng.random(20) * 64], 1))
    # 2: the oblique pencil.  Query 0 sits on the epipole e1: every error is NaN.  Query 1
    # (60, 20) against train 0 (48.5, 32.5), half a pixel from e2: the dst side passes, the src
    # side does not.  Query 2 (49.5, 28.5), half a pixel from e1, against train 1 (60, 30): the src
    # side passes, the dst side does not.
    T.append(np.concatenate([[[48.5, 32.5], [60, 30]], np.stack([rng.random(38) * 96, rng.random(38) * 64], 1)]))
    Q.append(np.concatenate([[E1, [60, 20], [49.5, 28.5]], np.stack([rng.random(37) * 96, rng.random(37) * 64], 1)]))
    # 3: found = 0 over a NaN model: the window alone
    T.append(np.stack([rng.random(12) * 96, rng.random(12) * 64], 1))
    Q.append(np.stack([rng.random(10) * 96, rng.random(10) * 64], 1))
    return [np.asarray(a, np.float32).reshape(-1, 2) for a in Q], [np.asarray(a, np.float32).reshape(-1, 2) for a in T]


def edge_models():
    F = np.stack([F_HORIZONTAL, F_VERTICAL, F_OBLIQUE, np.full(9, np.nan)])
    return F, np.array([1, 1, 5, 0], np.int32)


@functools.lru_cache(maxsize=None)
def edges_case(metric, seg_train, band=BAND):
    Qxy, Txy = _edge_points()
    rng = np.random.default_rng(170 + metric)
    qd = [W.rows_of(rng, len(a), metric) for a in Qxy]
    td = [W.rows_of(rng, len(a), metric) for a in Txy]
    qoff = U.offsets([len(a) for a in Qxy])
    toff = U.offsets([len(a) for a in Txy])
    F, found = edge_models()
    c = Case(f"edges-{W.METRIC_IDS[metric]}-{'segmented' if seg_train else 'shared'}-band{band:g}", metric,
             np.concatenate(qd), W.kpts_at(np.concatenate(Qxy)), qoff, np.concatenate(td),
             W.kpts_at(np.concatenate(Txy)), toff if seg_train else None, F, found, band)
    c.seg_qoff, c.seg_toff = qoff, toff
    return c


def census(c, c_down):
    """The kinds of (q, t) pairs the issue asks of the edge case, counted on the restatement
    alone.  c_down is the same case at band = down(band)."""
    F, t = c.F, limit(c.band)
    kinds = dict(window_only=0, dst_only=0, src_only=0, nan=0, boundary=0, outside=0, crowded=0, one=0, none=0)
    qo = U.clamped(c.qoff, c.q_cap)
    n_grids = 1 if c.toff is None else len(qo) - 1
    nx, ny, inv = grid_of(c.radius, c.band, c.rows, c.cols, c.t_cap, n_grids)
    for b in range(len(qo) - 1):
        tl, th = (0, c.t_cap) if c.toff is None else (int(c.toff[b]), int(c.toff[b + 1]))
        tx, ty = c.tk["x"][tl:th], c.tk["y"][tl:th]
        cells = cell_of(ty, inv, ny) * nx + cell_of(tx, inv, nx)
        for i in range(int(qo[b]), int(qo[b + 1])):
            adm = c.adm[i]
            kinds["one"] += len(adm) == 1
            kinds["none"] += len(adm) == 0
            kinds["boundary"] += len(np.setdiff1d(adm, c_down.adm[i]))
            kinds["outside"] += int(((tx[adm] < 0) | (tx[adm] >= c.cols) | (ty[adm] < 0) | (ty[adm] >= c.rows)).sum())
            if len(adm):
                kinds["crowded"] += int(np.bincount(cells[adm]).max() > WIN_GROUP)
            if not has_model(F, c.found, b):
                continue
            w = W.admissible_row(c.qk["x"][i], c.qk["y"][i], tx, ty, c.radius)
            e_dst, e_src = errors(F[b], c.qk["x"][i], c.qk["y"][i], tx, ty)
            with np.errstate(invalid="ignore"):
                kinds["window_only"] += int((~w & (e_dst <= t) & (e_src <= t)).sum())
                kinds["dst_only"] += int((w & (e_dst > t) & (e_src <= t)).sum())
                kinds["src_only"] += int((w & (e_src > t) & (e_dst <= t)).sum())
                kinds["nan"] += int((w & (np.isnan(e_dst) | np.isnan(e_src))).sum())
    return kinds


# ---- contract cases ---------------------------------------------------------------------------
def _random_models(rng, n):
    """n regular pencils with the epipole inside or near a 96 x 64 image."""
    F = np.zeros((n, 9))
    for b in range(n):
        A = np.array([[1 + rng.normal() * 0.05, rng.normal() * 0.05, rng.normal() * 6],
                      [rng.normal() * 0.05, 1 + rng.normal() * 0.05, rng.normal() * 6], [0, 0, 1]])
        F[b] = pencil_F((rng.random() * 96, rng.random() * 64), A)
    return F


@functools.lru_cache(maxsize=None)
def clamp_case(metric, seg_train):
    """match_window_inputs.clamp_case's buffers (offsets past the capacities, garbage rows of no
    segment, copies of queries past t_cap) under three regular models."""
    w = W.clamp_case(metric, seg_train)
    F = _random_models(np.random.default_rng(190 + metric), 3)
    return Case(f"clamp-{W.METRIC_IDS[metric]}-{'segmented' if seg_train else 'shared'}", metric, w.q, w.qk, w.qoff,
                w.t, w.tk, w.toff, F, None, band=6.0, radius=30.0, q_cap=w.q_cap, t_cap=w.t_cap)


@functools.lru_cache(maxsize=None)
def nonmonotone_case(metric):
    """q_offsets = [0, 30, 20, 50]: by the matchers' bisection rows 0..29 are segment 0's and rows
    30..49 segment 2's; segment 1 gets none."""
    rng = np.random.default_rng(195 + metric)
    nq, nt = 50, 90
    qxy = np.stack([rng.random(nq) * 96, rng.random(nq) * 64], 1)
    txy = np.stack([rng.random(nt) * 96, rng.random(nt) * 64], 1)
    return Case(f"nonmonotone-{W.METRIC_IDS[metric]}", metric, W.rows_of(rng, nq, metric), W.kpts_at(qxy),
                [0, 30, 20, 50], W.rows_of(rng, nt, metric), W.kpts_at(txy), [0, 30, 60, 90], _random_models(rng, 3),
                None, band=6.0, radius=INF)


@functools.lru_cache(maxsize=None)
def many_segments_case(metric):
    """200 segments of 0 to 3 rows on either side."""
    rng = np.random.default_rng(197 + metric)
    q_sizes, t_sizes = rng.integers(0, 4, 200), rng.integers(0, 4, 200)
    qoff, toff = U.offsets(q_sizes), U.offsets(t_sizes)
    nq, nt = int(qoff[-1]), int(toff[-1])
    qxy = np.stack([rng.random(nq) * 96, rng.random(nq) * 64], 1)
    txy = np.stack([rng.random(nt) * 96, rng.random(nt) * 64], 1)
    found = (rng.random(200) < 0.8).astype(np.int32)
    return Case(f"200-segments-{W.METRIC_IDS[metric]}", metric, W.rows_of(rng, nq, metric), W.kpts_at(qxy), qoff,
                W.rows_of(rng, nt, metric), W.kpts_at(txy), toff, _random_models(rng, 200), found, band=12.0,
                radius=INF)
