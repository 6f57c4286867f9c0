"""Inputs and the bit-exact oracle of the squared-L2 matcher on float descriptors.

The rule (include/sift_hip.h), restated: PI is one fixed permutation of 0..127,
    PI[8 c + 2 j + h] = 8 c + 4 h + j        (c < 16, j < 4, h < 2),
    chain(x, y) = fmaf(x[PI[127]], y[PI[127]], ... fmaf(x[PI[0]], y[PI[0]], 0.0f)),
    dot = chain(q, t), nq = chain(q, q), nt = chain(t, t),
    s = nq + nt (one float32 rounding), d = fmaf(-2.0f, dot, s), d = d < 0 ? 0 : d.
d is the squared distance; neighbours ascend by (d, train index), a row at d =
+inf or at d = NaN (finite rows give inf - inf) is never one, missing entries are
idx -1 / dist +inf, so the result holds no NaN.

fma32() is a correctly rounded float32 fma in numpy, vectorised over pairs: the
product of two float32 is exact in float64; the float64 sum with the addend is
rounded once there and once more by the cast to float32, and the two roundings
differ from one only where the float64 sum lands exactly on a float32 midpoint
while the real sum does not.  Those elements are found, the real sum's side of
the midpoint is taken from the TwoSum residual, and the cast's choice is moved to
the other neighbour where it went the wrong way.

The cases are built once (lru_cache) and shared, read-only.  Their shapes sit on
the kernel's seams: 32 queries to a lane block, 64 to a wave, 256 to a
workgroup; 32 train rows to a tile, 64 to a step and to a split granule.
"""
import functools

import numpy as np

import match_l2_inputs as L2
import match_u8_inputs as U

f32, f64 = np.float32, np.float64

PI = np.array([8 * c + 4 * h + j for c in range(16) for j in range(4) for h in range(2)], np.int64)
assert sorted(PI.tolist()) == list(range(128)) and PI[:8].tolist() == [0, 4, 1, 5, 2, 6, 3, 7]

Q_BLOCK, Q_WAVE, Q_TILE = 32, 64, 256     # queries of a lane block, a wave, a workgroup
T_TILE, T_STEP = 32, 64                   # train rows of an MFMA tile, of a step (and split granule)


# ---- a correctly rounded float32 fma ---------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) element-wise on float32 arrays (broadcast), one rounding."""
    a, b, c = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32), np.asarray(c, f32))
    shape = a.shape
    p = a.astype(f64).ravel() * b.astype(f64).ravel()      # exact: 24 + 24 bits
    c64 = c.astype(f64).ravel()
    with np.errstate(invalid="ignore"):
        s = p + c64                                        # rounded to 53 bits (inf - inf: NaN)
    with np.errstate(over="ignore"):
        r = s.astype(f32)                                  # rounded again
    # a float32 midpoint has, as a float64, the low 29 fraction bits 1000...0 (normal
    # range); below it (float32 subnormals) every element takes the full test
    cand = ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000) | (np.abs(s) < 2.0 ** -125)
    i = np.nonzero(cand)[0]
    if len(i):
        si, pi_, ci, ri = s[i], p[i], c64[i], r[i]
        bb = si - pi_                                      # TwoSum: p + c = s + e exactly
        e = (pi_ - (si - bb)) + (ci - bb)
        d = si - ri.astype(f64)                            # exact; its sign is the side s lies on
        nb = np.nextafter(ri, np.where(d > 0, np.inf, -np.inf).astype(f32))
        with np.errstate(over="ignore", invalid="ignore"):
            mid = (d != 0) & ((ri.astype(f64) + nb.astype(f64)) * 0.5 == si)
        wrong = mid & (e != 0) & ((e > 0) == (d > 0))      # the real sum lies beyond the midpoint
        r[i] = np.where(wrong, nb, ri)
    return r.reshape(shape)


def chain(x, y, order=PI):
    """chain(x, y) over the last axis (128), broadcast over the others."""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    acc = np.zeros(np.broadcast_shapes(x.shape[:-1], y.shape[:-1]), f32)
    for e in order:
        acc = fma32(x[..., e], y[..., e], acc)
    return acc


def distances(q, t, order=PI, clamp=True):
    """[nq, nt] float32 d by the rule; clamp=False: the value before d < 0 ? 0 : d."""
    q, t = np.asarray(q, f32).reshape(-1, 128), np.asarray(t, f32).reshape(-1, 128)
    d = np.empty((len(q), len(t)), f32)
    if not len(q) or not len(t):
        return d
    nq, nt = chain(q, q, order), chain(t, t, order)
    step = max(1, 200000 // len(t))
    for a in range(0, len(q), step):
        dot = chain(q[a:a + step, None, :], t[None, :, :], order)
        with np.errstate(over="ignore"):
            s = nq[a:a + step, None] + nt[None, :]         # float32 + float32: one rounding
        v = fma32(f32(-2), dot, s)
        d[a:a + step] = np.where(v < 0, f32(0), v) if clamp else v
    return d


def knn_from(d, k):
    """(idx int32, dist float32) [nq, k] of a distance table: stable order on (d, index).
    A NaN distance counts as +inf: strict '<' is false on it, as on +inf against an empty slot."""
    d = np.where(np.isnan(d), f32(np.inf), d)
    idx = np.full((len(d), k), -1, np.int32)
    dist = np.full((len(d), k), np.inf, f32)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    m = order.shape[1]
    if m and len(d):
        dd = np.take_along_axis(d, order, axis=1)
        idx[:, :m] = np.where(np.isposinf(dd), -1, order)  # a row at +inf or NaN is never a neighbour
        dist[:, :m] = dd
    return idx, dist


def knn_ref(q, t, k, order=PI):
    return knn_from(distances(q, t, order), k)


def seg_ref(q, qoff, t, toff, k, q_cap=None, t_cap=None, order=PI):
    """knn_ref per segment on the clamped bounds, [q_cap, k]; rows of no segment stay -1 / +inf."""
    q_cap = len(q) if q_cap is None else q_cap
    t_cap = len(t) if t_cap is None else t_cap
    qo = U.clamped(qoff, q_cap)
    to = None if toff is None else U.clamped(toff, t_cap)
    idx = np.full((q_cap, k), -1, np.int32)
    dist = np.full((q_cap, k), np.inf, f32)
    for b in range(len(qo) - 1):
        ts = t[:t_cap] if to is None else t[to[b]:max(to[b], to[b + 1])]
        if qo[b + 1] > qo[b]:
            idx[qo[b]:qo[b + 1]], dist[qo[b]:qo[b + 1]] = knn_ref(q[qo[b]:qo[b + 1]], ts, k, order)
    return idx, dist


class Case:
    """One call: q, qoff, t, toff (None = shared), capacities, and the k = 2 oracle result."""

    def __init__(self, name, q, qoff, t, toff, q_cap=None, t_cap=None):
        self.name, self.q, self.qoff, self.t, self.toff = name, q, np.asarray(qoff, np.int32), t, toff
        self.q_cap = len(q) if q_cap is None else q_cap
        self.t_cap = len(t) if t_cap is None else t_cap
        self.idx, self.dist = seg_ref(q, self.qoff, t, toff, 2, self.q_cap, self.t_cap)
        for a in (self.idx, self.dist):
            a.setflags(write=False)

    def ref(self, k):
        return self.idx[:, :k], self.dist[:, :k]


def rows(rng, n):
    """Non-dyadic float rows in the range of SIFT descriptors (0 .. 0.4)."""
    return (rng.random((n, 128), f32) * f32(0.4)).astype(f32)


# ---- ties across the kernel's seams ------------------------------------------------------
def seam_triples(nt):
    """(lo, hi, near): train rows lo and hi (local) hold the same values and row `near`
    differs from them in one element.  The pairs sit either side of a half-wave's four
    rows, of a 32-row tile, of a 64-row step (and split granule), and at the two ends."""
    out, used = [], set()
    for lo, hi, near in ((3, 4, 6), (30, 33, 35), (62, 65, 67), (1, nt - 1, 8), (0, 2, 5)):
        s = {lo, hi, near}
        if len(s) == 3 and max(s) < nt and min(s) >= 0 and not (s & used):
            out.append((lo, hi, near))
            used |= s
    return out


def plant(q_seg, t_seg):
    """Writes the triples into a segment's train rows (a view) and two queries per triple
    while they last: query 2 p equals the pair's row (the pair tied for first place at 0,
    lower index first), query 2 p + 1 equals `near` (near alone at 0, the pair tied for
    second place).  Returns [(query, expected idx pair)]."""
    want = []
    for p, (lo, hi, near) in enumerate(seam_triples(len(t_seg))):
        t_seg[hi] = t_seg[lo]
        t_seg[near] = t_seg[lo]
        t_seg[near, 17] += f32(0.03125)
        if 2 * p + 1 < len(q_seg):
            q_seg[2 * p] = t_seg[lo]
            q_seg[2 * p + 1] = t_seg[near]
            want += [(2 * p, [lo, hi]), (2 * p + 1, [near, lo])]
    return want


# 0 first, between and last; one below, at and one above a lane block, a wave and a workgroup
Q_SIZES = [0, 1, 31, 32, 33, 0, 63, 64, 65, 255, 256, 257, 0]
# behind them: fewer than k rows (0, 1), one below / at / above a tile's neighbours, a step and two
# steps; the ranges start off every granule (row 5).  An even share of the buffer is below one
# step, so the launch has one split and a workgroup walks every step of a range itself.
T_SIZES = [3, 0, 1, 63, 64, 65, 2, 127, 128, 129, 0, 193, 9]
T_FIRST = 5
T_SHARED = 130      # three splits of one step each, the last with two rows


@functools.lru_cache(maxsize=None)
def edges_case(seg_train):
    rng = np.random.default_rng(140 + seg_train)
    qoff = U.offsets(Q_SIZES)
    q = rows(rng, int(qoff[-1]))
    planted = []
    if seg_train:
        toff = U.offsets(T_SIZES, T_FIRST)
        t = rows(rng, int(toff[-1]) + 3)
        for b in range(len(Q_SIZES)):
            for row, pair in plant(q[qoff[b]:qoff[b + 1]], t[toff[b]:toff[b + 1]]):
                planted.append((int(qoff[b]) + row, pair))
    else:
        toff, t = None, rows(rng, T_SHARED)
        for row, pair in plant(q[qoff[11]:qoff[12]], t):
            planted.append((int(qoff[11]) + row, pair))
    c = Case("f32-edges-" + ("segmented" if seg_train else "shared"), q, qoff, t, toff)
    c.planted = planted
    for row, pair in planted:
        assert c.idx[row].tolist() == pair, (c.name, row, pair, c.idx[row])
    return c


@functools.lru_cache(maxsize=None)
def splits_case():
    """Segmented train with few segments: three splits per range, of which the 200-row
    range fills two (128 rows each way of the seam at 128) and leaves one empty, and
    the 130-row range puts two rows into its last."""
    rng = np.random.default_rng(142)
    qoff, toff = U.offsets([257, 70]), U.offsets([200, 130], 3)
    q, t = rows(rng, int(qoff[-1])), rows(rng, int(toff[-1]) + 2)
    planted = []
    for b in range(2):
        for row, pair in plant(q[qoff[b]:qoff[b + 1]], t[toff[b]:toff[b + 1]]):
            planted.append((int(qoff[b]) + row, pair))
    for lo, hi in ((126, 129), (127, 128)):      # either side of the split seam of the first range
        t[toff[0] + hi] = t[toff[0] + lo]
        q[qoff[0] + 20 + len(planted)] = t[toff[0] + lo]
        planted.append((int(qoff[0]) + 20 + len(planted), [lo, hi]))
    c = Case("f32-splits", q, qoff, t, toff)
    for row, pair in planted:
        assert c.idx[row].tolist() == pair, (row, pair, c.idx[row])
    return c


@functools.lru_cache(maxsize=None)
def many_segments_case():
    rng = np.random.default_rng(143)
    sizes = rng.integers(0, 4, 257)
    qoff = U.offsets(sizes)
    return Case("f32-257-segments", rows(rng, int(qoff[-1])), qoff, rows(rng, 70), None)


@functools.lru_cache(maxsize=None)
def weights_case():
    """One distinct weight per row and element, asymmetric in both: a missing or doubled
    k, a swapped operand map or a swapped row / column changes almost every distance."""
    i, j, e = np.arange(70)[:, None], np.arange(78)[:, None], np.arange(128)[None, :]
    q = (((7 * i + 3 * e) % 251) / f32(251 * 3)).astype(f32)
    t = (((5 * j + 11 * e + 1) % 241) / f32(241 * 3)).astype(f32)
    c = Case("f32-weights", q, U.offsets([0, 70]), t, U.offsets([3, 75]))
    d = distances(q, t[3:])
    assert len(np.unique(d)) > d.size // 2
    return c


@functools.lru_cache(maxsize=None)
def clamp_cases():
    """q_offsets[n] above q_cap; a train range straddling t_cap with copies of the queries
    past it (a read past t_cap would win at distance 0); q_offsets[0] > 0."""
    rng = np.random.default_rng(144)
    q_sizes, t_sizes = [1, 63, 0, 200, 130], [5, 64, 2, 100, 197]
    qoff, toff = U.offsets(q_sizes), U.offsets(t_sizes, 3)
    q, t = rows(rng, int(qoff[-1])), rows(rng, int(toff[-1]))
    out = [Case("q_cap", q, qoff, t, toff, q_cap=int(qoff[-1]) - 37),
           Case("q_cap-shared", q, qoff, t[:133], None, q_cap=int(qoff[-1]) - 37)]
    t_cap = int(toff[-1]) - 37
    tp = t.copy()
    tp[t_cap:] = q[qoff[4]:qoff[4] + 37]
    out.append(Case("t_cap", q, qoff, tp, toff, t_cap=t_cap))
    out.append(Case("t_cap-shared", q, qoff, tp, None, t_cap=t_cap))
    qoff2 = qoff.copy()
    qoff2[0] = qoff2[1] = 1
    out.append(Case("first-offset", q, qoff2, t, toff, q_cap=int(qoff[-1]) - 37))
    return out


# ---- dyadic rows: u / 512 of byte rows --------------------------------------------------
def dyadic(u):
    """Byte rows as floats u / 512 (exact).  Every product, sum and norm of such rows is
    an integer below 2^24 in units of 2^-18, so the rule's d is the integer squared
    distance times 2^-18 in any summation order."""
    return (np.asarray(u, np.uint8).astype(f32) / f32(512)).astype(f32)


SCALE = f32(2.0 ** 18)


def dyadic_sources():
    """The byte cases whose float forms the GPU compares with the byte matcher: tile
    edges (shared and segmented), the maximum distance with the sign bias, every tie
    input and the segmented ties."""
    return [L2.edges_case(False), L2.edges_case(True), L2.extremes_case(), L2.tie_segmented_case()] + \
        [L2.tie_case(n) for n in range(len(U.TIE_IDS))]


def census(c, k_rows=None):
    """(rows with d1 == d2, rows with d1 < d2 == d3) of a float case under the rule."""
    first = second = 0
    qo = U.clamped(c.qoff, c.q_cap)
    to = None if c.toff is None else U.clamped(c.toff, c.t_cap)
    for b in range(len(qo) - 1):
        ts = c.t[:c.t_cap] if to is None else c.t[to[b]:max(to[b], to[b + 1])]
        if qo[b + 1] > qo[b] and len(ts) >= 3:
            d = np.sort(distances(c.q[qo[b]:qo[b + 1]], ts), axis=1)
            first += int((d[:, 0] == d[:, 1]).sum())
            second += int(((d[:, 0] < d[:, 1]) & (d[:, 1] == d[:, 2])).sum())
    return first, second


# ---- values: signs, cancellation, subnormals, overflow ----------------------------------
# The four value cases share one shape.  Query segments of 33 and 65 rows: their last rows
# are the last busy lane of a block with idle lanes behind it.  Train: 130 shared rows (three
# splits: 64, 64 and a tail step of two rows), or ranges of 130 and 97 rows from row 3 (two
# splits each: 128 and a tail of 2; 64 and a tail of 33).  The special rows of a case sit
# either side of every seam of its ranges and on the last row of the tail step.
V_Q, V_T, V_FIRST = [33, 65], [130, 97], 3


def split_rows(q_cap, nseg, t_cap, seg_train, nt):
    """Train rows per split of a range of nt rows: knn_l2_f32_seg_splits and the kernel's
    `per` (match_l2_f32.hip), restated."""
    gx = q_cap // Q_TILE + nseg
    share = -(-t_cap // nseg) if seg_train else t_cap
    splits = max(1, min(-(-1024 // gx), -(-share // T_STEP)))
    return -(-(-(-nt // splits)) // T_STEP) * T_STEP


def value_shape(seg_train, q_sizes=V_Q, t_sizes=V_T):
    """(qoff, toff or None, train rows, [(first row, rows, rows per split)] per segment)."""
    qoff = U.offsets(q_sizes)
    nq, nseg = int(qoff[-1]), len(q_sizes)
    if not seg_train:
        return qoff, None, T_SHARED, [(0, T_SHARED, split_rows(nq, nseg, T_SHARED, False, T_SHARED))] * nseg
    toff = U.offsets(t_sizes, V_FIRST)
    n_t = int(toff[-1]) + 2
    return qoff, toff, n_t, [(int(toff[b]), t_sizes[b], split_rows(nq, nseg, n_t, True, t_sizes[b]))
                             for b in range(nseg)]


def seams(nt, per):
    """{s: kind}: local rows s with a seam between s - 1 and s -- a half-wave's four rows,
    the 32-row tiles, the 64-row steps, the splits; the coarsest kind of each."""
    out = {4: "half"} if nt > 4 else {}
    out.update({s: "tile" for s in range(T_TILE, nt, T_TILE)})
    out.update({s: "step" for s in range(T_STEP, nt, T_STEP)})
    out.update({s: "split" for s in range(per, nt, per)})
    return out


def seam_rows(nt, per):
    """The rows either side of every seam and the last row (of a tail step where nt % 64)."""
    return sorted({r for s in seams(nt, per) for r in (s - 1, s)} | {nt - 1})


def seg_tables(c):
    """(b, first query row, queries, train rows) of every non-empty segment, on the clamped bounds."""
    qo = U.clamped(c.qoff, c.q_cap)
    to = None if c.toff is None else U.clamped(c.toff, c.t_cap)
    for b in range(len(qo) - 1):
        ts = c.t[:c.t_cap] if to is None else c.t[to[b]:max(to[b], to[b + 1])]
        if qo[b + 1] > qo[b]:
            yield b, int(qo[b]), c.q[qo[b]:qo[b + 1]], ts


def subnormal(x):
    """Non-zero and below 2^-126 in magnitude."""
    x = np.abs(np.asarray(x, f64))
    return (x > 0) & (x < 2.0 ** -126)


# ---- signed rows --------------------------------------------------------------------------
def signed_rows(rng, n):
    """Non-dyadic rows uniform in [-0.4, 0.4)."""
    return ((rng.random((n, 128), f32) - f32(0.5)) * f32(0.8)).astype(f32)


@functools.lru_cache(maxsize=None)
def signed_case(seg_train):
    """Signed rows.  In every segment queries 2 and n - 2 are all zero.  The seam rows of a
    train range are exact negations of a query (dot = -nq, d = 4 nq: the farthest row, and
    the nearest, at 0, to a matcher blind to an operand's sign), alternately of the segment's
    last query and of queries 1, 3, 5, ...; but row 31 of the first range (and of the shared
    set) is all zero.  A zero row is at d = nq, about half the distance of any other, so it is
    every query's nearest row: one such row leaves the second neighbour, and the whole of
    the second range, to the signed rows."""
    rng = np.random.default_rng(160 + seg_train)
    qoff, toff, n_t, ranges = value_shape(seg_train)
    nseg = len(qoff) - 1
    q, t = signed_rows(rng, int(qoff[-1])), signed_rows(rng, n_t)
    for b in range(nseg):
        q[qoff[b] + 2] = 0
        q[qoff[b + 1] - 2] = 0
    negated = []                             # (segment, local query, local train row)
    for b, (ts, nt, per) in enumerate(ranges if seg_train else ranges[:1]):
        for i, r in enumerate(seam_rows(nt, per)):
            if b == 0 and r == T_TILE - 1:
                t[ts + r] = 0
                continue
            seg = b if seg_train else (i // 2) % nseg
            j = int(qoff[seg + 1] - qoff[seg]) - 1 if i % 2 == 0 else i
            t[ts + r] = -q[qoff[seg] + j]
            negated.append((seg, j, r))
    c = Case("f32-signed-" + ("segmented" if seg_train else "shared"), q, qoff, t, toff)
    c.negated = negated
    return c


# ---- near-copies: the clamp -------------------------------------------------------------
CANCEL_SEED = {False: 172, True: 171}        # chosen on the oracle alone: cancel_census() meets the test's counts
CANCEL_PLANTED = {False: [20, 30], True: [28, 40]}   # planted queries per segment


def cancel_pairs(nt, per, n):
    """n disjoint (lo, hi, kind) pairs of local rows: four across every seam ((s - 1, s),
    (s - 2, s + 1), ...), then consecutive free rows (kind "inside")."""
    used, out = set(), []

    def take(lo, hi, kind):
        if 0 <= lo < hi < nt and not ({lo, hi} & used) and len(out) < n:
            used.update((lo, hi))
            out.append((lo, hi, kind))

    for w in range(4):
        for s, kind in seams(nt, per).items():
            take(s - 1 - w, s + w, kind)
    assert nt - 1 in used                    # the last row of the tail step holds a near-copy
    free = [r for r in range(nt) if r not in used]
    for lo, hi in zip(free[0::2], free[1::2]):
        take(lo, hi, "inside")
    return out


@functools.lru_cache(maxsize=None)
def cancel_case(seg_train):
    """Near-duplicates.  A planted query has two near-copies among the train rows and no
    exact copy: itself with one element moved one ulp up in one row, and another element one
    ulp down in the other.  Their true distance, about 1e-16, is far below the rule's
    absolute error (about 1e-4 here), so the sign of fmaf(-2, dot, s) is rounding noise and
    the clamp decides the result.  A planted query is an ordinary row times 1/4 with the two
    moved elements set to 1.5 .. 2: each carries close to half of the norm, so that its ulp
    is about an ulp of the norm.  (On ordinary rows an element carries a fortieth of the
    norm at most, its ulp changes no rounding of the chain, and fmaf(-2, dot, s) is exactly 0
    on 98 % of such pairs: 0 to 4 non-zero values among 100 to 136 pairs, over 30 seeds.)
    The pairs sit across the seams (cancel_pairs); the first planted query of a segment is
    its last row.  c.planted: (query row, segment, lo, hi, kind)."""
    rng = np.random.default_rng(CANCEL_SEED[seg_train])
    qoff, toff, n_t, ranges = value_shape(seg_train)
    nseg = len(qoff) - 1
    q, t = rows(rng, int(qoff[-1])), rows(rng, n_t)
    local = [[int(qoff[b + 1] - qoff[b]) - 1] + list(range(int(qoff[b + 1] - qoff[b]) - 1)) for b in range(nseg)]
    counts = CANCEL_PLANTED[seg_train]
    if seg_train:
        plan = [(b, local[b][n], pair) for b, (ts, nt, per) in enumerate(ranges)
                for n, pair in enumerate(cancel_pairs(nt, per, counts[b]))]
    else:                                    # one train set: its pairs go to the segments in turn
        slots = [(b, local[b][n]) for n in range(max(counts)) for b in range(nseg) if n < counts[b]]
        plan = [s + (pair,) for s, pair in zip(slots, cancel_pairs(ranges[0][1], ranges[0][2], len(slots)))]
    planted = []
    for n, (b, j, (lo, hi, kind)) in enumerate(plan):
        row, ts = int(qoff[b]) + j, ranges[b][0]
        e_up, e_down = (int(e) for e in rng.choice(128, 2, replace=False))
        q[row] *= f32(0.25)
        q[row, [e_up, e_down]] = f32(1.5) + rng.random(2, f32) * f32(0.5)
        up, down = (lo, hi) if n % 2 == 0 else (hi, lo)
        t[ts + up] = q[row]
        t[ts + up, e_up] = np.nextafter(q[row, e_up], f32(np.inf))
        t[ts + down] = q[row]
        t[ts + down, e_down] = np.nextafter(q[row, e_down], f32(-np.inf))
        planted.append((row, b, lo, hi, kind))
    c = Case("f32-cancel-" + ("segmented" if seg_train else "shared"), q, qoff, t, toff)
    c.planted, c.ranges = planted, ranges
    return c


def cancel_census(c):
    """Of the planted (query, near-copy) pairs: how many have fmaf(-2, dot, s) < 0 and > 0;
    the kinds of the planted queries both of whose near-copies clamp to 0 (a tie, by index)."""
    neg = pos = 0
    tied = []
    for row, b, lo, hi, kind in c.planted:
        ts = c.ranges[b][0]
        v = distances(c.q[row:row + 1], c.t[[ts + lo, ts + hi]], clamp=False)[0]
        neg += int((v < 0).sum())
        pos += int((v > 0).sum())
        if (v <= 0).all():
            tied.append(kind)
    return neg, pos, tied


# ---- subnormals -------------------------------------------------------------------------
def subnormal_rows(rng, n):
    """Rows of float32 subnormals (random fractions, either sign) with six normal elements of
    about 2^-60 each."""
    bits = rng.integers(1, 1 << 23, (n, 128)).astype(np.int32) | (rng.integers(0, 2, (n, 128)).astype(np.int32) << 31)
    x = bits.view(f32).copy()
    for i in range(n):
        e = rng.choice(128, 6, replace=False)
        x[i, e] = rows(rng, 1)[0, e] * f32(2.0 ** -58)
    return x


@functools.lru_cache(maxsize=None)
def subnormal_case(seg_train):
    """Rows of three kinds by (local row % 3), queries and train alike, so that every tile
    and every seam mixes them: 0 -- ordinary rows times 2^-70 (normal elements; products,
    dots and norms in the subnormal range or below it); 1 -- subnormal_rows(); 2 -- ordinary
    rows.  The nearest rows of a kind-0 query are kind-0 rows at subnormal distances."""
    rng = np.random.default_rng(180 + seg_train)
    qoff, toff, n_t, ranges = value_shape(seg_train)
    q, t = rows(rng, int(qoff[-1])), rows(rng, n_t)

    def fill(x, first, n):
        kind = np.arange(n) % 3
        x[first:first + n][kind == 0] *= f32(2.0 ** -70)
        x[first:first + n][kind == 1] = subnormal_rows(rng, int((kind == 1).sum()))

    for b in range(len(qoff) - 1):
        fill(q, int(qoff[b]), int(qoff[b + 1] - qoff[b]))
    for ts, nt, _ in (ranges if seg_train else ranges[:1]):
        fill(t, ts, nt)
    return Case("f32-subnormal-" + ("segmented" if seg_train else "shared"), q, qoff, t, toff)


def subnormal_census(c):
    """(products q[e] t[e] in the subnormal range, subnormal distances in the table, NaN
    distances in the table, subnormal distances in the k = 2 result)."""
    prod = dsub = nan = 0
    for _, _, qs, ts in seg_tables(c):
        for a in range(0, len(qs), 16):
            prod += int(subnormal(qs[a:a + 16, None, :].astype(f64) * ts[None, :, :].astype(f64)).sum())
        d = distances(qs, ts)
        dsub += int(subnormal(d).sum())
        nan += int(np.isnan(d).sum())
    return prod, dsub, nan, int(subnormal(c.dist).sum())


# ---- overflow: +inf and NaN distances of finite rows -----------------------------------
BIG_NORM = 2.4e38        # the norm of a big row: finite, and two of them sum past float32 (3.4e38)
HUGE = f32(1e20)         # rows() times HUGE: elements up to 4e19, the norm +inf
O_Q, O_T = [33, 65, 10], [130, 97, 9]


def big(x):
    """Rows scaled to a norm of BIG_NORM each: elements of about 1e18."""
    return (x * np.sqrt(BIG_NORM / chain(x, x).astype(f64))[:, None]).astype(f32)


def fused_pair(rng):
    """Finite rows (y, t), near-copies of each other, with chain(y, y) and chain(t, t) below
    2^127 and chain(y, t) >= 2^127: s = nq + nt is finite and -2 dot alone is -inf, but the
    fused d = fmaf(-2, dot, s) is finite (negative: it clamps to 0).  Found by walking the
    scale of one row up in ulps across 2^127 with 48 one-ulp jitters at each."""
    x = rows(rng, 1)[0]
    top = f32(2.0 ** 127)
    scale = f32(np.sqrt(2.0 ** 127 / float(chain(x, x))) * (1 - 2.0 ** -20))
    for _ in range(64):
        base = (x * scale).astype(f32)[None, :].repeat(48, 0)
        step = rng.integers(-1, 2, base.shape)
        cand = np.where(step > 0, np.nextafter(base, f32(np.inf)), np.where(step < 0, np.nextafter(base, f32(0)), base))
        cand = cand.astype(f32)
        ok = np.nonzero(chain(cand, cand) < top)[0]
        if len(ok) > 1:
            dot = chain(cand[ok][:, None, :], cand[ok][None, :, :])
            hit = [(i, j) for i, j in np.argwhere(dot >= top) if i != j]
            if hit:
                return cand[ok[hit[0][0]]], cand[ok[hit[0][1]]]
        scale = np.nextafter(scale, f32(np.inf))
    raise AssertionError("no fused pair found")


@functools.lru_cache(maxsize=None)
def overflow_case(seg_train):
    """Finite elements only.  Train rows are ordinary ("o"), big(rows()) ("b": against a big
    query s = +inf and d = +inf, against an ordinary one d is about 2e38), rows() * HUGE ("h":
    nt = +inf; against a big query dot = +inf and d = inf - inf = NaN, against an ordinary one
    d = +inf) or rows() * -HUGE ("n": dot = -inf against a big query, d = +inf).  Queries are
    ordinary or big.  Against the ordinary train rows a big query has d = nq
    for every one of them (2 dot and nt are below half an ulp of nq): a tie by index.
    Range 0 (130 rows, shared too): h, n, b on rows 0..2, cycling over the seam rows and on
    the last row, ordinary elsewhere; row 10 and query 5 are fused_pair().  Range 1 (97
    rows): h, n, b cycling everywhere, h on the last row, one ordinary row (40): a big query
    has one finite neighbour.  Range 2 (9 rows): h, n, b only, all ten queries big: none."""
    rng = np.random.default_rng(190 + seg_train)
    qoff, toff, n_t, ranges = value_shape(seg_train, O_Q if seg_train else V_Q, O_T)
    nseg = len(qoff) - 1
    q, t = rows(rng, int(qoff[-1])), rows(rng, n_t)
    big_q = np.zeros(len(q), bool)
    for b in range(nseg):
        n = int(qoff[b + 1] - qoff[b])
        big_q[qoff[b]:qoff[b + 1]] = [np.arange(n) % 2 == 1, np.arange(n) % 3 == 0, np.ones(n, bool)][b]
        big_q[qoff[b + 1] - 1] = True        # the last query of every segment
    q[big_q] = big(q[big_q])
    kinds = np.full(n_t, "o")
    for b, (ts, nt, per) in enumerate(ranges if seg_train else ranges[:1]):
        if b == 0:
            special = sorted(set(seam_rows(nt, per)) | {0, 1, 2})
            kinds[[ts + r for r in special]] = [("h", "n", "b")[i % 3] for i in range(len(special))]
        else:
            kinds[ts:ts + nt] = [("h", "n", "b")[i % 3] for i in range(nt)]
            if b == 1:
                kinds[ts + 40] = "o"
        kinds[ts + nt - 1] = "h"             # the last row of the tail step, the stand-in for its masked rows
    t[kinds == "b"] = big(t[kinds == "b"])
    t[kinds == "h"] *= HUGE
    t[kinds == "n"] *= -HUGE
    fused_q, fused_t = int(qoff[0]) + 5, ranges[0][0] + 10
    q[fused_q], t[fused_t] = fused_pair(rng)
    big_q[fused_q], kinds[fused_t] = True, "f"
    assert np.isfinite(q).all() and np.isfinite(t).all()
    c = Case("f32-overflow-" + ("segmented" if seg_train else "shared"), q, qoff, t, toff)
    c.big_q, c.kinds, c.fused, c.ranges = big_q, kinds, (fused_q, fused_t), ranges
    return c


def overflow_census(c):
    """Counts by the oracle: NaN and +inf distances in the tables; queries with two finite
    neighbours of which the nearer has a NaN / +inf row before it in index order; queries
    with exactly one finite neighbour; queries with none."""
    out = dict(nan=0, inf=0, two_behind=0, one=0, none=0)
    for _, q0, qs, ts in seg_tables(c):
        d = distances(qs, ts)
        out["nan"] += int(np.isnan(d).sum())
        out["inf"] += int(np.isposinf(d).sum())
        idx = c.idx[q0:q0 + len(qs)]
        for i in range(len(qs)):
            if idx[i, 1] >= 0:
                out["two_behind"] += bool((~np.isfinite(d[i, :idx[i, 0]])).any())
            elif idx[i, 0] >= 0:
                out["one"] += 1
            else:
                out["none"] += 1
    return out
