"""Inputs and the bit-exact oracle of the squared-L2 matcher on float descriptors.

The rule (include/sift_hip.h), restated: PI is one fixed permutation of 0..127,
    PI[8 c + 2 j + h] = 8 c + 4 h + j        (c < 16, j < 4, h < 2),
    chain(x, y) = fmaf(x[PI[127]], y[PI[127]], ... fmaf(x[PI[0]], y[PI[0]], 0.0f)),
    dot = chain(q, t), nq = chain(q, q), nt = chain(t, t),
    s = nq + nt (one float32 rounding), d = fmaf(-2.0f, dot, s), d = d < 0 ? 0 : d.
d is the squared distance; neighbours ascend by (d, train index), a row at d =
+inf is never one, missing entries are idx -1 / dist +inf.

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
    s = p + c64                                            # rounded to 53 bits
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


def distances(q, t, order=PI):
    """[nq, nt] float32 d by the rule."""
    q, t = np.asarray(q, f32).reshape(-1, 128), np.asarray(t, f32).reshape(-1, 128)
    d = np.empty((len(q), len(t)), f32)
    if not len(q) or not len(t):
        return d
    nq, nt = chain(q, q, order), chain(t, t, order)
    step = max(1, 200000 // len(t))
    for a in range(0, len(q), step):
        dot = chain(q[a:a + step, None, :], t[None, :, :], order)
        s = nq[a:a + step, None] + nt[None, :]             # float32 + float32: one rounding
        v = fma32(f32(-2), dot, s)
        d[a:a + step] = np.where(v < 0, f32(0), v)
    return d


def knn_from(d, k):
    """(idx int32, dist float32) [nq, k] of a distance table: stable order on (d, index)."""
    idx = np.full((len(d), k), -1, np.int32)
    dist = np.full((len(d), k), np.inf, f32)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    m = order.shape[1]
    if m and len(d):
        dd = np.take_along_axis(d, order, axis=1)
        idx[:, :m] = np.where(np.isposinf(dd), -1, order)  # a row at +inf is never a neighbour
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
