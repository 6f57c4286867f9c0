"""Inputs and the exact reference of the 8-bit descriptor path.

The L1 distance of two uint8 rows is an integer of at most 128 * 255 = 32,640,
exact in any summation order, so the reference needs no float: |a - b| summed in
int64, then a stable argsort (the lower train index first at equal distance).

quant_ref()      saturate_cast<uchar>(x * 512): float32 multiply, rint (ties to
                 even), clip to 0..255.
quant_edges()    every byte value's exact, neighbouring and half-way inputs,
                 and the special values.
knn_ref()        one query set against one train set.
seg_ref()        knn_ref per segment on the clamped offsets.
The cases below are built once (lru_cache) and shared, read-only.
"""
import functools

import numpy as np

import match_inputs as I

SENT_I, SENT_D = -77, -5.0     # what the tests fill the outputs with (test_match_batch._knn_device)
DIST_MAX = 128 * 255


def quant_ref(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        y = np.rint(x * np.float32(512))
    return np.clip(y, 0, 255).astype(np.uint8)


def quant_edges():
    """float32 [n, 128] (padded with 0.25): for every byte b, b/512 and its two
    float neighbours, (b + 0.5)/512 and its two neighbours; then -0.0, a
    negative, the smallest denormal, 1.0, 1e30, +inf, -inf."""
    vals = []
    for b in range(256):
        for c in (np.float32(b) / np.float32(512), np.float32(b + 0.5) / np.float32(512)):
            vals += [np.nextafter(c, np.float32(-1)), c, np.nextafter(c, np.float32(2))]
    vals += [np.float32(-0.0), np.float32(-0.3), np.float32(1e-45), np.float32(1.0), np.float32(1e30),
             np.float32(np.inf), np.float32(-np.inf)]
    x = np.full(-(-len(vals) // 128) * 128, 0.25, np.float32)
    x[:len(vals)] = np.array(vals, np.float32)
    return x.reshape(-1, 128)


def distances(q, t):
    """[nq, nt] int64 sum |q - t| of uint8 rows."""
    q, t = np.asarray(q), np.asarray(t)
    assert q.dtype == np.uint8 and t.dtype == np.uint8
    qi, ti = q.astype(np.int16), t.astype(np.int16)
    d = np.empty((len(qi), len(ti)), np.int64)
    for s in range(0, len(qi), 16):
        d[s:s + 16] = np.abs(qi[s:s + 16, None, :] - ti[None, :, :]).sum(-1, dtype=np.int64)
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
        dist[:, :m] = np.take_along_axis(d, order, axis=1)   # <= 32,640: exact in float32
    return idx, dist


def offsets(sizes, first=0):
    return (first + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int32)


def clamped(off, cap):
    return np.clip(np.asarray(off, np.int64), 0, cap)


def seg_ref(q, qoff, t, toff, k, q_cap=None, t_cap=None):
    """knn_ref per segment on the clamped bounds, [q_cap, k]; rows of no segment stay -1 / +inf."""
    q_cap = len(q) if q_cap is None else q_cap
    t_cap = len(t) if t_cap is None else t_cap
    qo = clamped(qoff, q_cap)
    to = None if toff is None else clamped(toff, t_cap)
    idx = np.full((q_cap, k), -1, np.int32)
    dist = np.full((q_cap, k), np.inf, np.float32)
    for b in range(len(qo) - 1):
        ts = t[:t_cap] if to is None else t[to[b]:max(to[b], to[b + 1])]
        if qo[b + 1] > qo[b]:
            idx[qo[b]:qo[b + 1]], dist[qo[b]:qo[b + 1]] = knn_ref(q[qo[b]:qo[b + 1]], ts, k)
    return idx, dist


class Case:
    """One call: q, qoff, t, toff (None = shared), capacities, and the k = 2 reference."""

    def __init__(self, name, q, qoff, t, toff, q_cap=None, t_cap=None):
        self.name, self.q, self.qoff, self.t, self.toff = name, q, np.asarray(qoff, np.int32), t, toff
        self.q_cap = len(q) if q_cap is None else q_cap
        self.t_cap = len(t) if t_cap is None else t_cap
        self.idx, self.dist = seg_ref(q, self.qoff, t, toff, 2, self.q_cap, self.t_cap)
        for a in (self.idx, self.dist):      # shared by every test that needs them
            a.setflags(write=False)

    def ref(self, k):
        return self.idx[:, :k], self.dist[:, :k]


# ---- random bytes at the tile edges ------------------------------------------------
# 0 first, between and last; 63 / 64 / 65 ... 257: one below, at and one above 64 x Q for Q <= 4
Q_SIZES = [0, 1, 63, 0, 64, 65, 127, 128, 129, 255, 256, 257, 0]
# every train size of the issue, each behind a non-empty query segment at least once; the
# ranges start at rows 5, 8, 8, 9, 16, 18, 21, 84, 148, 213, 4310, 4310, 8407
T_SIZES = [3, 0, 1, 7, 2, 3, 63, 64, 65, 4097, 0, 4097, 9]
T_FIRST = 5


@functools.lru_cache(maxsize=None)
def edges_case(seg_train):
    rng = np.random.default_rng(40 + seg_train)
    qoff = offsets(Q_SIZES)
    q = rng.integers(0, 256, (int(qoff[-1]), 128), dtype=np.uint8)
    if seg_train:
        toff = offsets(T_SIZES, T_FIRST)
        t = rng.integers(0, 256, (int(toff[-1]) + 3, 128), dtype=np.uint8)
        for b in range(len(Q_SIZES)):               # a real tie where sizes allow: a copy of a row, and a query on it
            if T_SIZES[b] > 3 and Q_SIZES[b]:
                t[toff[b] + T_SIZES[b] // 2] = t[toff[b] + 1]
                q[qoff[b]] = t[toff[b] + 1]
    else:
        toff, t = None, rng.integers(0, 256, (333, 128), dtype=np.uint8)
        t[333 // 2] = t[1]
        q[qoff[2]] = t[1]
    return Case("edges-" + ("segmented" if seg_train else "shared"), q, qoff, t, toff)


# ---- extremes ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extremes_case():
    """Segment 0: all-255 queries against all-0 rows (32,640).  Segment 1: queries
    >= 0x80 against rows < 0x80.  Segment 2: the queries are the train rows."""
    rng = np.random.default_rng(42)
    hi = rng.integers(0x80, 0x100, (70, 128), dtype=np.uint8)
    lo = rng.integers(0, 0x80, (70, 128), dtype=np.uint8)
    same = rng.integers(0, 256, (70, 128), dtype=np.uint8)
    q = np.concatenate([np.full((3, 128), 255, np.uint8), hi, same])
    t = np.concatenate([np.zeros((5, 128), np.uint8), lo, same])
    c = Case("extremes", q, offsets([3, 70, 70]), t, offsets([5, 70, 70]))
    assert (c.dist[:3] == DIST_MAX).all() and c.idx[:3].tolist() == [[0, 1]] * 3
    assert (c.dist[73:, 0] == 0).all() and (c.idx[73:, 0] == np.arange(70)).all()
    return c


# ---- ties ------------------------------------------------------------------------------
# (nq, nt, levels) of tests/test_match_ties.py's dense cases, and {0, 1} bytes on six columns
# against the train sizes of the issue with 300 queries (two tiles, every Q slot)
DENSE = [(64, 5, 2), (65, 8, 3), (64, 63, 2), (65, 64, 3), (130, 65, 2), (64, 128, 3), (65, 129, 2),
         (130, 333, 2), (64, 4097, 3)]
BITS_NT = [5, 8, 63, 64, 65, 257, 4097]
TIE_IDS = [f"dense{nq}x{nt}" for nq, nt, _ in DENSE] + [f"bits300x{nt}" for nt in BITS_NT]


@functools.lru_cache(maxsize=None)
def tie_case(n):
    """match_inputs.dense_case cast to uint8: copies of one train row planted at
    chosen rows (every pair of waves inside a 64-row granule, rows in different
    granules -- different splits --, triples and quadruples), a unique nearer
    row beside each set, and queries that see the set tied for first place or
    tied for second behind the nearer row.  The bits cases shuffle the queries,
    so the planted ones fall into every Q slot of both tiles."""
    if n < len(DENSE):
        nq, nt, levels = DENSE[n]
        q, t, _ = I.dense_case(100 + n, nq, nt, levels)
    else:
        nt = BITS_NT[n - len(DENSE)]
        q, t, _ = I.dense_case(200 + n, 300, nt, 2)
        q = q[np.random.default_rng(n).permutation(len(q))]
    assert q.max() < 256 and t.max() < 256 and q.min() >= 0
    q, t = q.astype(np.uint8), t.astype(np.uint8)
    return Case(TIE_IDS[n], q, offsets([len(q)]), t, None)


@functools.lru_cache(maxsize=None)
def tie_segmented_case():
    """Every tie case as one segment with its own train range, behind a segment of
    no queries and three train rows: the ranges start off the 64-row granule."""
    cases = [tie_case(n) for n in range(len(TIE_IDS))]
    qoff = offsets([0] + [len(c.q) for c in cases])
    toff = offsets([3] + [len(c.t) for c in cases])
    q = np.concatenate([c.q for c in cases])
    t = np.concatenate([np.full((3, 128), 7, np.uint8)] + [c.t for c in cases])
    c = Case("ties-segmented", q, qoff, t, toff)
    assert (c.idx == np.concatenate([x.idx for x in cases])).all()
    return c


def tie_census(case):
    """(rows with d1 == d2, rows with d1 < d2 == d3): places decided by the index alone."""
    first, second, _ = I.census(distances(case.q, case.t))
    return first, second


# ---- many segments, clamps ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_segments_case():
    rng = np.random.default_rng(43)
    sizes = rng.integers(0, 4, 257)
    qoff = offsets(sizes)
    q = rng.integers(0, 4, (int(qoff[-1]), 128), dtype=np.uint8)
    t = rng.integers(0, 4, (70, 128), dtype=np.uint8)
    return Case("257-segments", q, qoff, t, None)


@functools.lru_cache(maxsize=None)
def clamp_cases():
    """q_offsets[n] above q_cap (the last live segment straddles it); a train
    range straddling t_cap, the rows past it copies of the queries that search
    it (a read past t_cap would win at distance 0); q_offsets[0] > 0."""
    rng = np.random.default_rng(44)
    q_sizes, t_sizes = [1, 63, 0, 200, 130], [5, 64, 2, 300, 4097]
    qoff, toff = offsets(q_sizes), offsets(t_sizes, 3)
    q = rng.integers(0, 256, (int(qoff[-1]), 128), dtype=np.uint8)
    t = rng.integers(0, 256, (int(toff[-1]), 128), dtype=np.uint8)
    out = [Case("q_cap", q, qoff, t, toff, q_cap=int(qoff[-1]) - 37),
           Case("q_cap-shared", q, qoff, t[:333], None, q_cap=int(qoff[-1]) - 37)]
    t_cap = int(toff[-1]) - 37
    tp = t.copy()
    tp[t_cap:] = q[qoff[4]:qoff[4] + 37]
    out.append(Case("t_cap", q, qoff, tp, toff, t_cap=t_cap))
    out.append(Case("t_cap-shared", q, qoff, tp, None, t_cap=t_cap))
    qoff2 = qoff.copy()
    qoff2[0] = qoff2[1] = 1
    out.append(Case("first-offset", q, qoff2, t, toff, q_cap=int(qoff[-1]) - 37))
    return out
