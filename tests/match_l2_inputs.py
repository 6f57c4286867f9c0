"""Inputs and the exact reference of the squared-L2 matcher on 8-bit descriptors.

The squared L2 distance of two uint8 rows is an integer of at most 128 * 255^2
= 8,323,200 < 2^24, exact in float32, so the reference needs no float: (q - t)^2
summed in int64, then a stable argsort (the lower train index first at equal
distance), per segment on the clamped offsets.

The data builders are match_u8_inputs'; its Case objects carry L1 references,
so l2() re-scores a case (once per case object, shared, read-only).  This
matcher's own: a fourth segment of extremes_case (bytes either side of the sign
bias), weights_case (a distinct weight per row and per element) and chunks_case
(the kernel's 32-row, 128-row and 512-row granules).
"""
import functools

import numpy as np

import match_u8_inputs as U

DIST_MAX = 128 * 255 * 255


def distances(q, t):
    """[nq, nt] int64 sum (q - t)^2 of uint8 rows."""
    q, t = np.asarray(q), np.asarray(t)
    assert q.dtype == np.uint8 and t.dtype == np.uint8
    qi, ti = q.astype(np.int64), t.astype(np.int64)
    d = np.empty((len(qi), len(ti)), np.int64)
    for s in range(0, len(qi), 16):
        e = qi[s:s + 16, None, :] - ti[None, :, :]
        d[s:s + 16] = (e * e).sum(-1, dtype=np.int64)
    return d


def knn_ref(q, t, k):
    """(idx int32, dist float32) [nq, k]; -1 / +inf where there are fewer than k train rows."""
    d = distances(q, t)
    idx = np.full((len(q), k), -1, np.int32)
    dist = np.full((len(q), k), np.inf, np.float32)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    m = order.shape[1]
    if m and len(q):
        idx[:, :m] = order
        dist[:, :m] = np.take_along_axis(d, order, axis=1)   # <= 8,323,200 < 2^24: exact in float32
    return idx, dist


def seg_ref(q, qoff, t, toff, k, q_cap=None, t_cap=None):
    """knn_ref per segment on the clamped bounds, [q_cap, k]; rows of no segment stay -1 / +inf."""
    q_cap = len(q) if q_cap is None else q_cap
    t_cap = len(t) if t_cap is None else t_cap
    qo = U.clamped(qoff, q_cap)
    to = None if toff is None else U.clamped(toff, t_cap)
    idx = np.full((q_cap, k), -1, np.int32)
    dist = np.full((q_cap, k), np.inf, np.float32)
    for b in range(len(qo) - 1):
        ts = t[:t_cap] if to is None else t[to[b]:max(to[b], to[b + 1])]
        if qo[b + 1] > qo[b]:
            idx[qo[b]:qo[b + 1]], dist[qo[b]:qo[b + 1]] = knn_ref(q[qo[b]:qo[b + 1]], ts, k)
    return idx, dist


class Case:
    """One call: q, qoff, t, toff (None = shared), capacities, and the k = 2 squared-L2 reference."""

    def __init__(self, name, q, qoff, t, toff, q_cap=None, t_cap=None):
        self.name, self.q, self.qoff, self.t, self.toff = name, q, np.asarray(qoff, np.int32), t, toff
        self.q_cap = len(q) if q_cap is None else q_cap
        self.t_cap = len(t) if t_cap is None else t_cap
        self.idx, self.dist = seg_ref(q, self.qoff, t, toff, 2, self.q_cap, self.t_cap)
        for a in (self.idx, self.dist):      # shared by every test that needs them
            a.setflags(write=False)

    def ref(self, k):
        return self.idx[:, :k], self.dist[:, :k]


_rescored = {}


def l2(c):
    """A match_u8_inputs.Case (cached there, so the same object every time) with the squared-L2 reference."""
    if id(c) not in _rescored:
        _rescored[id(c)] = (c, Case(c.name, c.q, c.qoff, c.t, c.toff, c.q_cap, c.t_cap))
    return _rescored[id(c)][1]


def edges_case(seg_train):
    return l2(U.edges_case(seg_train))


def tie_case(n):
    return l2(U.tie_case(n))


def tie_segmented_case():
    return l2(U.tie_segmented_case())


def many_segments_case():
    return l2(U.many_segments_case())


@functools.lru_cache(maxsize=None)
def clamp_cases():
    return [Case(c.name, c.q, c.qoff, c.t, c.toff, c.q_cap, c.t_cap) for c in U.clamp_cases()]


def tie_census(n):
    """(rows with d1 == d2, rows with d1 < d2 == d3) of U.tie_case(n) under squared L2."""
    c = U.tie_case(n)
    first, second, _ = U.I.census(distances(c.q, c.t))
    return first, second


# ---- extremes and the sign bias ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extremes_case():
    """match_u8_inputs.extremes_case (all-255 against all-0: 8,323,200; bytes >= 0x80
    against bytes < 0x80; queries equal to train rows) and a fourth segment: every
    query byte 0x80 (zero after the bias x ^ 0x80), train rows that mix 0x7F / 0x80 /
    0x81 (-1 / 0 / +1 after it).  The distance of train row j is its count of bytes
    that are not 0x80; rows 0 and 1 are all 0x7F and all 0x81 (128 each), row 2 is all
    0x80 (0), row 3 is one 0x7F (1), row 4 one 0x81 (1), the rest are random mixes."""
    u = U.extremes_case()
    rng = np.random.default_rng(48)
    t4 = rng.choice(np.array([0x7F, 0x80, 0x81], np.uint8), (70, 128))
    t4[0], t4[1], t4[2] = 0x7F, 0x81, 0x80
    t4[3], t4[4] = 0x80, 0x80
    t4[3, 17], t4[4, 90] = 0x7F, 0x81
    q4 = np.full((33, 128), 0x80, np.uint8)
    q = np.concatenate([u.q, q4])
    t = np.concatenate([u.t, t4])
    c = Case("extremes", q, U.offsets([3, 70, 70, 33]), t, U.offsets([5, 70, 70, 70]))
    assert (c.dist[:3] == DIST_MAX).all() and c.idx[:3].tolist() == [[0, 1]] * 3
    assert (c.dist[73:143, 0] == 0).all() and (c.idx[73:143, 0] == np.arange(70)).all()
    assert c.idx[143:].tolist() == [[2, 3]] * 33 and c.dist[143:].tolist() == [[0.0, 1.0]] * 33
    return c


# ---- a distinct weight per row and per element -----------------------------------------
@functools.lru_cache(maxsize=None)
def weights_case():
    """q[i][e] = (7 i + 3 e) mod 251, t[j][e] = (5 j + 11 e + 1) mod 241: asymmetric in
    row and in element, so a swapped row / column write or two operands loaded with
    different element maps changes almost every distance.  70 x 75 rows behind a
    three-row train range: more than one tile each way, off the granules."""
    i, j, e = np.arange(70)[:, None], np.arange(78)[:, None], np.arange(128)[None, :]
    q = ((7 * i + 3 * e) % 251).astype(np.uint8)
    t = ((5 * j + 11 * e + 1) % 241).astype(np.uint8)
    c = Case("weights", q, U.offsets([0, 70]), t, U.offsets([3, 75]))
    d = distances(q, t[3:])
    assert len(np.unique(d)) > d.size // 2 and not (d[:70, :70] == d[:70, :70].T).all()
    return c


# ---- the kernel's granules -----------------------------------------------------------------
# A workgroup's four waves score 32-row tiles of a quarter of the split each, and fold their
# keys every 512 rows.  With 2,100 segments the launch has one split, so a train range of n
# rows gives every wave ceil(n / 128) * 32 rows: 2,047 and 2,048 rows are one full 512-row
# chunk per wave (one row short of it in the last wave), 2,049 and 2,177 go into a second chunk.
# Query segments of 31 / 32 / 33 rows sit either side of the 32-query block of a lane.
CHUNK_SEGS = {7: (31, 2047), 300: (32, 2048), 1033: (33, 2049), 2099: (9, 2177)}
CHUNK_NSEG = 2100


def chunk_pairs(nt):
    """Train rows (local) that hold the same bytes, pair by pair: inside wave 0's first
    chunk; either side of row 512 (a chunk's end, and wave 0's where a wave has 512
    rows); in wave 0 and wave 1; in the first and the last wave."""
    per_wave = -(-nt // 128) * 32
    return [(1, 511), (510, 512), (509, per_wave + 3), (2, nt - 1)]


@functools.lru_cache(maxsize=None)
def chunks_case():
    """Segmented train, ranges off every granule (the first starts at row 5).  In every
    live segment each pair of chunk_pairs() holds a copy of one row; query p equals
    pair p's row (the pair tied at 0, lower index first) and query 4 + p differs from
    it by one in one byte (the pair tied at 1)."""
    rng = np.random.default_rng(49)
    q_sizes, t_sizes = np.zeros(CHUNK_NSEG, np.int64), np.zeros(CHUNK_NSEG, np.int64)
    for b, (nq, nt) in CHUNK_SEGS.items():
        q_sizes[b], t_sizes[b] = nq, nt
    qoff, toff = U.offsets(q_sizes), U.offsets(t_sizes, 5)
    q = rng.integers(0, 256, (int(qoff[-1]), 128), dtype=np.uint8)
    t = rng.integers(0, 256, (int(toff[-1]) + 2, 128), dtype=np.uint8)
    for b, (nq, nt) in CHUNK_SEGS.items():
        for p, (lo, hi) in enumerate(chunk_pairs(nt)):
            base = t[toff[b] + lo].copy()
            base[0] = 100
            t[toff[b] + lo] = t[toff[b] + hi] = base
            q[qoff[b] + p] = q[qoff[b] + 4 + p] = base
            q[qoff[b] + 4 + p, 0] = 101
    c = Case("chunks", q, qoff, t, toff)
    for b, (nq, nt) in CHUNK_SEGS.items():
        for p, pair in enumerate(chunk_pairs(nt)):
            for row, d in ((qoff[b] + p, 0.0), (qoff[b] + 4 + p, 1.0)):
                assert c.idx[row].tolist() == list(pair) and c.dist[row].tolist() == [d, d]
    return c
