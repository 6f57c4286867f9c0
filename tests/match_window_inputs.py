"""Inputs and the reference of the windowed (spatially gated) segmented matcher.

The reference restates the contract of sift_knn_match_window_segmented_device
(include/sift_hip.h), numpy only:
  * the predicted position of a query is its keypoint's (x, y), or
    oracle/homography.py's perspective_transform of H[b] at that point;
  * train row t is admissible iff |tx - px| <= radius and |ty - py| <= radius,
    every operation in np.float32, one query at a time (a NaN compares false);
  * distances are the dense references' own: oracle/match.py l1_distances for
    float rows, match_u8_inputs.distances / match_l2_inputs.distances for bytes;
  * the k nearest admissible rows by a stable sort on (distance, local index); a
    float row at distance +inf is never a neighbour (the dense matcher's rule).
Everything is built once (lru_cache) and shared, read-only.
"""
import functools

import numpy as np

import homography as HG
import match as M
import match_l2_inputs as L2
import match_u8_inputs as U

L1_F32, L1_U8, L2SQR_U8 = 0, 1, 2
METRIC_IDS = ["l1_f32", "l1_u8", "l2sqr_u8"]
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
SENT_I, SENT_F = -77, -5.0
f32 = np.float32

# match_window.hip: kWinGroup lanes per query, kWinBlock lanes per workgroup (the
# binning kernels use 256-lane workgroups too, the scan 1024 over at most 4096 cells)
WIN_GROUP, WIN_BLOCK = 8, 256
# more points in one cell than a lane group (8) or a workgroup (256) is wide, and
# not a multiple of either: 256 + 8 + 3
ONE_CELL_N = WIN_BLOCK + WIN_GROUP + 3
RADIUS = f32(16.0)
# deliberately smaller than the point cloud (about [-40, 300] x [-40, 200] and
# infinities): points outside fall into the border cells.  With radius 16 the
# cell boundaries are the multiples of 16.
ROWS, COLS = 64, 96


def up(v):
    return np.nextafter(f32(v), f32(np.inf))


def down(v):
    return np.nextafter(f32(v), f32(-np.inf))


def distances(metric, q, t):
    if metric == L1_F32:
        return M.l1_distances(q, t)
    return (U.distances if metric == L1_U8 else L2.distances)(q, t)


def dense_seg_ref(metric, q, qoff, t, toff, k, q_cap=None, t_cap=None):
    """The existing dense references: cross_check_inputs.seg_knn's three cases."""
    if metric == L1_U8:
        return U.seg_ref(q, qoff, t, toff, k, q_cap, t_cap)
    if metric == L2SQR_U8:
        return L2.seg_ref(q, qoff, t, toff, k, q_cap, t_cap)
    q_cap = len(q) if q_cap is None else q_cap
    t_cap = len(t) if t_cap is None else t_cap
    qo = U.clamped(qoff, q_cap)
    to = None if toff is None else U.clamped(toff, t_cap)
    idx = np.full((q_cap, k), -1, np.int32)
    dist = np.full((q_cap, k), np.inf, np.float32)
    for b in range(len(qo) - 1):
        ts = t[:t_cap] if to is None else t[to[b]:max(to[b], to[b + 1])]
        if qo[b + 1] > qo[b]:
            idx[qo[b]:qo[b + 1]], dist[qo[b]:qo[b + 1]] = M.knn_match(q[qo[b]:qo[b + 1]], ts, k)
    return idx, dist


def predicted(qk, qoff, q_cap, H=None, found=None):
    """float32 [q_cap, 2]: the predicted position of every live query row (others 0)."""
    qo = U.clamped(qoff, q_cap)
    out = np.zeros((q_cap, 2), np.float32)
    for b in range(len(qo) - 1):
        lo, hi = int(qo[b]), int(qo[b + 1])
        if hi <= lo:
            continue
        xy = np.stack([qk["x"][lo:hi], qk["y"][lo:hi]], 1).astype(np.float32)
        if H is None or (found is not None and found[b] == 0):
            out[lo:hi] = xy
        else:
            with np.errstate(all="ignore"):
                out[lo:hi] = HG.perspective_transform(np.asarray(H, np.float64).reshape(-1, 9)[b], xy)
    return out


def admissible_row(px, py, tx, ty, radius):
    """bool [n_train] for one query: fabsf(tx - px) <= radius && fabsf(ty - py) <= radius in float32."""
    px, py, radius = f32(px), f32(py), f32(radius)
    with np.errstate(invalid="ignore"):
        dx, dy = np.abs(tx - px), np.abs(ty - py)      # float32 arrays minus a float32 scalar
        assert dx.dtype == np.float32 and dy.dtype == np.float32
        return (dx <= radius) & (dy <= radius)


def window_ref(metric, q, qk, qoff, t, tk, toff, radius, H=None, found=None, k=2, q_cap=None, t_cap=None):
    """(idx int32, dist float32 [q_cap, k], n_adm int64 [q_cap]): rows of no segment stay
    -1 / +inf / -1."""
    q_cap = len(q) if q_cap is None else q_cap
    t_cap = len(t) if t_cap is None else t_cap
    qo = U.clamped(qoff, q_cap)
    to = None if toff is None else U.clamped(toff, t_cap)
    pred = predicted(qk, qoff, q_cap, H, found)
    idx = np.full((q_cap, k), -1, np.int32)
    dist = np.full((q_cap, k), np.inf, np.float32)
    n_adm = np.full(q_cap, -1, np.int64)
    for b in range(len(qo) - 1):
        lo, hi = int(qo[b]), int(qo[b + 1])
        if hi <= lo:
            continue
        tl, th = (0, t_cap) if to is None else (int(to[b]), int(max(to[b], to[b + 1])))
        tx, ty = tk["x"][tl:th].astype(np.float32), tk["y"][tl:th].astype(np.float32)
        d = distances(metric, q[lo:hi], t[tl:th]) if th > tl else np.zeros((hi - lo, 0))
        for i in range(lo, hi):
            adm = np.flatnonzero(admissible_row(pred[i, 0], pred[i, 1], tx, ty, radius))
            n_adm[i] = len(adm)
            di = d[i - lo, adm]
            if metric == L1_F32:
                adm, di = adm[di != np.inf], di[di != np.inf]
            order = np.argsort(di, kind="stable")[:k]       # adm ascends: ties keep the lower index first
            idx[i, :len(order)] = adm[order]
            dist[i, :len(order)] = di[order]
    return idx, dist, n_adm


# ---- rows and keypoints ----------------------------------------------------------------
def rows_of(rng, n, metric):
    if metric == L1_F32:
        x = rng.random((n, 128)).astype(np.float32) ** 3
        x /= x.sum(1, keepdims=True)
        return np.sqrt(x).astype(np.float32)
    return rng.integers(0, 256, (n, 128), dtype=np.uint8)


def kpts_at(xy):
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    k = np.zeros(len(xy), KEYPOINT_DTYPE)
    k["x"], k["y"], k["size"] = xy[:, 0], xy[:, 1], 3
    return k


class Case:
    """One call: rows of the metric's type, keypoints, offsets (toff None = shared), the
    capacities, radius, the prior, and the k = 2 reference with the admissible counts."""

    def __init__(self, name, metric, q, qk, qoff, t, tk, toff, radius=RADIUS, H=None, found=None, q_cap=None,
                 t_cap=None, rows=ROWS, cols=COLS):
        self.name, self.metric, self.q, self.qk, self.t, self.tk = name, metric, q, qk, t, tk
        self.qoff = np.asarray(qoff, np.int32)
        self.toff = None if toff is None else np.asarray(toff, np.int32)
        self.radius, self.H, self.found, self.rows, self.cols = f32(radius), H, found, rows, cols
        self.q_cap = len(q) if q_cap is None else q_cap
        self.t_cap = len(t) if t_cap is None else t_cap
        self.idx, self.dist, self.n_adm = window_ref(metric, q, qk, self.qoff, t, tk, self.toff, self.radius, H,
                                                     found, 2, self.q_cap, self.t_cap)
        for a in (self.q, self.qk, self.t, self.tk, self.idx, self.dist, self.n_adm):
            a.setflags(write=False)

    def ref(self, k):
        return self.idx[:, :k], self.dist[:, :k]

    def live(self):
        qo = U.clamped(self.qoff, self.q_cap)
        return np.arange(int(qo[0]), int(qo[-1]))


# ---- the edges case ------------------------------------------------------------------
def _edge_points():
    """(query xy, train xy) per segment, metric-independent.  Returns lists of arrays."""
    rng = np.random.default_rng(7)
    r = float(RADIUS)
    Q, T = [], []
    # 0: no query rows, 5 train rows.  1: 7 query rows, no train rows.
    Q.append(np.zeros((0, 2)))
    T.append(rng.random((5, 2)) * 60)
    Q.append(rng.random((7, 2)) * 60)
    T.append(np.zeros((0, 2)))
    # 2: exactly one train row: inside the window of three queries, outside two others'
    Q.append([[40, 20], [50, 30], [40 + r, 20 - r], [40 + r + 1, 20], [40, 20 + 3 * r]])
    T.append([[40, 20]])
    # 3: ONE_CELL_N train points in the one cell [32, 48) x [16, 32); queries inside, at its
    # rim (windows that cut the cloud) and outside every point's reach
    T.append(np.stack([33 + rng.random(ONE_CELL_N) * 14, 17 + rng.random(ONE_CELL_N) * 14], 1))
    Q.append(np.concatenate([np.stack([30 + rng.random(14) * 20, 14 + rng.random(14) * 20], 1),
                             [[40, 24], [20, 24], [60, 5], [40, 60], [100, 100], [47.5, 31.5]]]))
    # 4: train points at exactly radius from a predicted position in x, in y and in both, one
    # float32 ulp beyond each, on both sides; points exactly on cell boundaries; and a point one
    # ulp below px - radius whose float32 difference rounds to exactly radius (15.999999 - 32 ->
    # -16): admissible by the rule although it lies in the cell below floor((px - radius) / 16)
    # (py - radius = 24 >= 16, so that one ulp below it is a whole ulp of the difference away)
    px, py = f32(50.0), f32(40.0)
    T.append([[px + RADIUS, py], [px, py + RADIUS], [px + RADIUS, py + RADIUS],
              [up(px + RADIUS), py], [px, up(py + RADIUS)], [up(px + RADIUS), up(py + RADIUS)],
              [px - RADIUS, py], [px, py - RADIUS], [px - RADIUS, py - RADIUS],
              [down(px - RADIUS), py], [px, down(py - RADIUS)], [down(px - RADIUS), down(py - RADIUS)],
              [32, 16], [48, 32], [32, 32], [48, 16], [64, 48], [16, 16], [0, 0],
              [down(16.0), 40], [40, down(16.0)], [down(16.0), down(16.0)]])
    Q.append([[px, py], [48, 32], [32, 16], [32, 32], [16, 16], [0, 0], [32, 40], [40, 32], [64, 32],
              [up(px), py], [down(px), py], [px, up(py)], [px, down(py)]])
    # 5: negative coordinates, coordinates beyond rows / cols, infinities, a NaN train row and
    # a NaN query row; identical descriptors at distinct admissible positions (planted below)
    t5 = np.concatenate([np.stack([-40 + rng.random(40) * 340, -40 + rng.random(40) * 240], 1),
                         [[-30, -30], [-25, -35], [-35, -25], [290, 190], [295, 195], [285, 185],
                          [np.inf, 10], [10, -np.inf], [np.nan, 20], [20, np.nan], [-np.inf, np.inf]]])
    q5 = np.concatenate([np.stack([-40 + rng.random(20) * 340, -40 + rng.random(20) * 240], 1),
                         [[-30, -30], [290, 190], [np.inf, 10], [10, -np.inf], [np.nan, 20], [20, np.nan],
                          [-1e30, 1e30], [300, -40]]])
    T.append(t5)
    Q.append(q5)
    # 6: a random cloud somewhat larger than rows x cols: about 18 admissible rows per query
    T.append(np.stack([-20 + rng.random(300) * 150, -20 + rng.random(300) * 120], 1))
    Q.append(np.stack([-20 + rng.random(300) * 150, -20 + rng.random(300) * 120], 1))
    return [np.asarray(a, np.float32).reshape(-1, 2) for a in Q], [np.asarray(a, np.float32).reshape(-1, 2) for a in T]


# segment 5: query row 20 (at (-30, -30)) and train rows 40, 41, 42 (all within its window)
# hold one descriptor; segment 6: train rows i, j admissible for query 0 hold its descriptor
@functools.lru_cache(maxsize=None)
def edges_case(metric, seg_train, finite_only=False, radius=float(RADIUS)):
    """finite_only: without the rows that have a NaN or an infinite coordinate, for the
    comparison with the dense matcher at radius = +inf (inf - inf is NaN: two points at the
    same infinity are not comparable, so the gate would drop that pair even there)."""
    Qxy, Txy = _edge_points()
    rng = np.random.default_rng(70 + metric)
    qd = [rows_of(rng, len(a), metric) for a in Qxy]
    td = [rows_of(rng, len(a), metric) for a in Txy]
    td[5][40] = td[5][41] = td[5][42] = qd[5][20]
    adm = np.flatnonzero(admissible_row(Qxy[6][0, 0], Qxy[6][0, 1], Txy[6][:, 0], Txy[6][:, 1], RADIUS))
    assert len(adm) >= 3
    td[6][adm[-1]] = td[6][adm[1]] = qd[6][0]           # the lower index, adm[1], must win
    if finite_only:
        for xy, d in ((Qxy, qd), (Txy, td)):
            for s in range(len(xy)):
                keep = np.isfinite(xy[s]).all(1)
                xy[s], d[s] = xy[s][keep], d[s][keep]
    qoff = U.offsets([len(a) for a in Qxy])
    q, qk = np.concatenate(qd), kpts_at(np.concatenate(Qxy))
    t, tk = np.concatenate(td), kpts_at(np.concatenate(Txy))
    toff = U.offsets([len(a) for a in Txy]) if seg_train else None
    c = Case(f"edges-{METRIC_IDS[metric]}-{'segmented' if seg_train else 'shared'}", metric, q, qk, qoff, t, tk, toff,
             radius)
    c.tie_rows = (int(qoff[5]) + 20, int(qoff[6]), int(adm[1]), int(adm[-1]))
    c.seg_sizes = ([len(a) for a in Qxy], [len(a) for a in Txy])
    return c


def census(c):
    """What the issue asks of a case, on the reference: counts of live queries with 0, 1, 2
    and >= 2 admissible rows, and the queries whose admissible set differs from the dense top-2."""
    live = c.live()
    n = c.n_adm[live]
    dense_idx, _ = dense_seg_ref(c.metric, c.q, c.qoff, c.t, c.toff, 2, c.q_cap, c.t_cap)
    differs = int(np.count_nonzero((dense_idx[live] != c.idx[live]).any(1)))
    return dict(live=len(live), zero=int((n == 0).sum()), one=int((n == 1).sum()), two=int((n == 2).sum()),
                two_or_more=int((n >= 2).sum()), differs=differs)


# ---- clamps ------------------------------------------------------------------------------
EXTRA = 16          # rows past the capacities in every input buffer


@functools.lru_cache(maxsize=None)
def clamp_case(metric, seg_train):
    """q_offsets / t_offsets run past q_cap / t_cap, q_offsets[0] = 3 and t_offsets[0] = 2;
    the rows of no segment hold garbage (NaN descriptors for floats, 0xFF bytes, coordinates
    1e30), and the rows past t_cap are copies of queries at the queries' positions: a read
    past the capacity would win at distance 0."""
    rng = np.random.default_rng(90 + metric)
    q_sizes, t_sizes = [30, 50, 40], [40, 60, 50]
    qoff, toff = U.offsets(q_sizes, 3), U.offsets(t_sizes, 2)
    q_cap, t_cap = int(qoff[-1]) - 11, int(toff[-1]) - 13
    nq, nt = int(qoff[-1]) + EXTRA, int(toff[-1]) + EXTRA
    q, t = rows_of(rng, nq, metric), rows_of(rng, nt, metric)
    qxy = np.stack([rng.random(nq) * 90, rng.random(nq) * 60], 1).astype(np.float32)
    txy = np.stack([rng.random(nt) * 90, rng.random(nt) * 60], 1).astype(np.float32)
    n_past = nt - t_cap
    src = int(qoff[2]) + np.arange(n_past) % (q_cap - int(qoff[2]))     # live queries of the last segment
    t[t_cap:], txy[t_cap:] = q[src], qxy[src]
    bad = 0xFF if metric != L1_F32 else np.nan
    q[:3], q[q_cap:] = bad, bad
    qxy[:3], qxy[q_cap:] = 1e30, 1e30
    t[:2], txy[:2] = bad, 1e30
    return Case(f"clamp-{METRIC_IDS[metric]}-{'segmented' if seg_train else 'shared'}", metric, q, kpts_at(qxy), qoff,
                t, kpts_at(txy), toff if seg_train else None, q_cap=q_cap, t_cap=t_cap)


# ---- many small segments -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_segments_case(metric):
    rng = np.random.default_rng(95 + metric)
    q_sizes, t_sizes = rng.integers(0, 21, 40), rng.integers(0, 21, 40)
    q_sizes[[0, 3, 17]], t_sizes[[5, 17, 39]] = 0, 0
    qoff, toff = U.offsets(q_sizes), U.offsets(t_sizes)
    nq, nt = int(qoff[-1]), int(toff[-1])
    qxy = np.stack([rng.random(nq) * 60, rng.random(nq) * 40], 1)
    txy = np.stack([rng.random(nt) * 60, rng.random(nt) * 40], 1)
    return Case(f"40-segments-{METRIC_IDS[metric]}", metric, rows_of(rng, nq, metric), kpts_at(qxy), qoff,
                rows_of(rng, nt, metric), kpts_at(txy), toff)


# ---- radius 0 --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def coincident_case(metric):
    """Half the train points coincide exactly with a query point (several with the same
    one); the others are one float32 ulp away in x or in y."""
    rng = np.random.default_rng(97 + metric)
    qxy = np.stack([rng.random(60) * 90, rng.random(60) * 60], 1).astype(np.float32)
    pick = rng.integers(0, 60, 120)
    txy = qxy[pick].copy()
    txy[60:90, 0] = np.nextafter(txy[60:90, 0], f32(np.inf))
    txy[90:, 1] = np.nextafter(txy[90:, 1], f32(-np.inf))
    c = Case(f"radius0-{METRIC_IDS[metric]}", metric, rows_of(rng, 60, metric), kpts_at(qxy), [0, 60],
             rows_of(rng, 120, metric), kpts_at(txy), [0, 120], radius=0.0)
    c.pick = pick
    return c


# ---- priors ------------------------------------------------------------------------------------
X0 = 37.0           # queries with x == X0 have w == 0 under the projective H below


@functools.lru_cache(maxsize=None)
def prior_case(metric, use_found):
    """Segment 0: a pure translation.  Segment 1: a projective H with w = x - X0, so the
    queries at x == X0 (and one within FLT_EPSILON of it) are predicted at (0, 0), where train
    points wait.  Segment 2: H is all NaN; with found[2] == 0 the prior is the identity, with
    found == None it is used as given (w is NaN, |w| > FLT_EPSILON is false: (0, 0)).
    Segment 3: the identity matrix times 2 (w = 2)."""
    rng = np.random.default_rng(99 + metric)
    n = 80
    qxy = [np.stack([rng.random(n) * 90, rng.random(n) * 60], 1).astype(np.float32) for _ in range(4)]
    qxy[1][:10, 0] = X0
    qxy[1][10, 0] = up(X0)          # |w| = 3.8e-6 > FLT_EPSILON: a huge but finite prediction
    H = np.zeros((4, 9))
    H[0] = [1, 0, 25.5, 0, 1, -12.25, 0, 0, 1]
    H[1] = [3, 0.5, 2, -0.25, 2, 1, 1, 0, -X0]
    H[2] = np.nan
    H[3] = [2, 0, 0, 0, 2, 0, 0, 0, 2]
    found = np.array([1, 1, 0, 7], np.int32) if use_found else None
    txy = []
    for b in range(4):
        with np.errstate(all="ignore"):
            p = HG.perspective_transform(H[b], qxy[b]) if b != 2 else qxy[b].copy()
        p = np.where(np.isfinite(p), p, 0).astype(np.float32)
        jit = (rng.random((n, 2)) * 40 - 20).astype(np.float32)        # half inside a 16-px window
        extra = (rng.random((20, 2)) * 30 - 15).astype(np.float32)     # around (0, 0)
        txy.append(np.concatenate([p + jit, extra]))
    qoff, toff = U.offsets([n] * 4), U.offsets([n + 20] * 4)
    q, t = rows_of(rng, 4 * n, metric), rows_of(rng, 4 * (n + 20), metric)
    return Case(f"priors-{METRIC_IDS[metric]}-{'found' if use_found else 'nofound'}", metric, q,
                kpts_at(np.concatenate(qxy)), qoff, t, kpts_at(np.concatenate(txy)), toff, H=H, found=found)


# ---- consecutive frames ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames_case(metric):
    """Four frames of 90 / 140 / 0 / 75 rows in one buffer: query segment b is frame b, its
    train segment frame b + 1 -- t_offsets = q_offsets + 1.  Frame 1 holds frame 0's points
    moved by up to 10 px, with frame 0's descriptors on half of them."""
    rng = np.random.default_rng(101 + metric)
    off = U.offsets([90, 140, 0, 75])
    n = int(off[-1])
    d = rows_of(rng, n, metric)
    xy = np.stack([rng.random(n) * 90, rng.random(n) * 60], 1).astype(np.float32)
    xy[90:180] = xy[:90] + (rng.random((90, 2)) * 20 - 10).astype(np.float32)
    d[90:135] = d[:45]
    c = Case(f"frames-{METRIC_IDS[metric]}", metric, d, kpts_at(xy), off[:-1], d, kpts_at(xy), off[1:])
    c.off = off
    return c
