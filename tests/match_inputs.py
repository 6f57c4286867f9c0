"""Seeded matcher inputs whose distances tie, with an exact reference.

Every descriptor here is a small integer (or such an integer times one power
of two), so every partial sum of the float L1 stays below 2^24 and the distance
is exact in any summation order: the reference needs no float at all.

exact_knn()      |q - t| summed in int64, a stable argsort, (distance, index).
dense_case()     descriptors in {0,1} / {0,1,2} on a few columns (ties dominate)
                 with planted tied sets: copies of one train row at chosen
                 indices, a unique nearer row beside them, and queries that see
                 the set in first place (d1 == d2) or in second (d1 < d2 == d3).
designed_case()  every pattern of distances in {0,1,2}^nt as one query each
                 (nt <= 4): every tie configuration of a short train set.
census()         the counts the tests require of a dense case, from the
                 reference alone.
"""
import itertools

import numpy as np

KTC = 64             # train rows per staged chunk (match.hip kTC)
NWAVE = 4            # waves per workgroup: wave w scores rows r = w (mod 4) of a chunk
DENSE_COLS = 6       # non-zero columns of the seeded part
MARK0, MARK = 64, 50  # planted set p: value MARK in column MARK0 + p
NEAR_COL = 127       # the unique nearer row differs from the tied rows here


def exact_distances(q, t, scale=1.0):
    """[nq, nt] int64 sum |q - t| of integer-valued descriptors (after dividing by scale)."""
    qi = np.rint(np.asarray(q, np.float64) / scale).astype(np.int64)
    ti = np.rint(np.asarray(t, np.float64) / scale).astype(np.int64)
    assert (qi * scale == q).all() and (ti * scale == t).all(), "descriptors are not integer multiples of scale"
    d = np.empty((len(qi), len(ti)), np.int64)
    for s in range(0, len(qi), 16):
        d[s:s + 16] = np.abs(qi[s:s + 16, None, :] - ti[None, :, :]).sum(-1)
    assert d.size == 0 or d.max() < 2 ** 24
    return d


def exact_knn(q, t, k, scale=1.0):
    """(idx int32, dist float32) [nq, k] from the int64 distances and a stable
    argsort; -1 / +inf where there are fewer than k train rows."""
    d = exact_distances(q, t, scale)
    idx = np.full((len(q), k), -1, np.int32)
    dist = np.full((len(q), k), np.inf, np.float32)
    order = np.argsort(d, axis=1, kind="stable")[:, :k]
    m = order.shape[1]
    if m and len(q):
        idx[:, :m] = order
        exact = np.take_along_axis(d, order, axis=1).astype(np.float64) * scale
        dist[:, :m] = exact.astype(np.float32)
        assert (dist[:, :m].astype(np.float64) == exact).all()
    return idx, dist


# ---- planted tied sets ------------------------------------------------------------
def planted_sets(nt):
    """[(tied indices ascending, index of the unique nearer row)], all indices
    distinct.  In order: the 16 residue pairs (i mod 4, j mod 4) inside chunk 0,
    those with i mod 4 > j mod 4 first (they need the index comparison in the
    wave merge), with a triple and a quadruple of descending residues after
    them; pairs with the members in chunks 0 | 1 and in the first | last chunk
    (one split or two, by the split count); triples and quadruples across chunks.  A set that does not
    fit into nt rows is left out."""
    free = [True] * nt
    nchunk = (nt + KTC - 1) // KTC
    sets = []

    def members(spec, above):   # the lowest free rows that fit spec, ascending; None if none do
        if not spec:
            return []
        (c, res), hi = spec[0], min(nt, (spec[0][0] + 1) * KTC)
        for i in range(max(c * KTC, above + 1), hi):
            if free[i] and i % NWAVE == res:
                rest = members(spec[1:], i)
                if rest is not None:
                    return [i] + rest
        return None

    def plant(spec):   # spec: [(chunk, residue)] per member, ascending chunks
        got = members(spec, -1)
        if got is None:
            return
        for g in got:
            free[g] = False
        # the nearer row comes from the residue class with the most free rows, low and high by turns
        room = [sum(free[r::NWAVE]) for r in range(NWAVE)]
        cand = [i for i in range(nt) if free[i] and i % NWAVE == room.index(max(room))]
        near = (cand[0] if len(sets) % 2 == 0 else cand[-1]) if cand else None
        if near is None:
            for g in got:
                free[g] = True
            return
        free[near] = False
        sets.append((tuple(got), near))

    pairs = sorted(itertools.product(range(NWAVE), repeat=2), key=lambda ab: (ab[0] <= ab[1], ab))
    last = nchunk - 1
    if nchunk > 1:          # first, or a short last chunk is gone to the nearer rows
        plant([(0, 3), (1, 0)])
    if nchunk > 2:
        plant([(0, 3), (last, 0)])
    for a, b in pairs[:6]:
        plant([(0, a), (0, b)])
    plant([(0, 3), (0, 2), (0, 1)])
    plant([(0, 3), (0, 2), (0, 1), (0, 0)])
    for a, b in pairs[6:]:
        plant([(0, a), (0, b)])
    if nchunk > 1:
        for a, b in [(1, 0), (2, 1), (0, 3)]:
            plant([(0, a), (1, b)])
    if nchunk > 2:
        for a, b in [(2, 1), (3, 2), (0, 0)]:
            plant([(0, a), (last, b)])
        for a, b in [(3, 1), (1, 0)]:
            plant([(nchunk // 2, a), (last, b)])
    if nchunk > 1:
        plant([(0, 3), (0, 1), (1, 0)])
        plant([(0, 2), (1, 3), (1, 1), (1, 0)])
    if nchunk > 2:
        plant([(0, 3), (1, 2), (last, 1)])
        plant([(0, 3), (1, 2), (nchunk // 2, 1), (last, 0)])
    return sets


def dense_case(seed, nq, nt, levels):
    """(q, t, sets): seeded {0..levels-1} values on DENSE_COLS columns; planted
    sets as of planted_sets(nt).  The rows of a set are copies of one row that
    carries MARK in a column of its own, the nearer row is that row plus 1 in
    NEAR_COL.  The first queries are planted, round robin over (set, place):
    the row itself sees the set tied at distance 0 and the nearer row at 1; the
    row plus 2 in NEAR_COL sees the nearer row at 1 and the set tied at 2.
    Every other row is at least MARK away from a planted query."""
    rng = np.random.default_rng(seed)
    q = np.zeros((nq, 128), np.float32)
    t = np.zeros((nt, 128), np.float32)
    q[:, :DENSE_COLS] = rng.integers(0, levels, (nq, DENSE_COLS))
    t[:, :DENSE_COLS] = rng.integers(0, levels, (nt, DENSE_COLS))
    sets = planted_sets(nt)
    assert len(sets) <= NEAR_COL - MARK0
    bases = []
    for p, (tied, near) in enumerate(sets):
        base = t[tied[0]].copy()
        base[MARK0 + p] = MARK
        for i in tied:
            t[i] = base
        t[near] = base
        t[near, NEAR_COL] = 1
        bases.append(base)
    n_planted = min(nq - nq // 4, max(2 * len(sets), 12)) if sets else 0
    for i in range(n_planted):
        p, place = (i // 2) % len(sets), i % 2
        q[i] = bases[p]
        q[i, NEAR_COL] = 2 * place
    return q, t, sets


def designed_case(nt):
    """(q, t) with 3^nt queries: query i is at distance 260 - 2 * pattern_i[j] from
    train row j, over every pattern in {0,1,2}^nt.  Query i is 4 in column i;
    train row j is pattern_i[j] in column i and fills columns 120.. so that every
    train row sums to 256."""
    pats = list(itertools.product(range(3), repeat=nt))
    assert len(pats) <= 120
    q = np.zeros((len(pats), 128), np.float32)
    t = np.zeros((nt, 128), np.float32)
    for i, pat in enumerate(pats):
        q[i, i] = 4
        t[:, i] = pat
    fill = 256 - t.sum(1)
    for c in range(120, 128):
        part = np.minimum(fill, 32)
        t[:, c] = part
        fill = fill - part
    assert (fill == 0).all() and (t.sum(1) == 256).all()
    return q, t


def census(d):
    """Of the int64 distances [nq, nt]: rows with d1 == d2; rows with
    d1 < d2 == d3; rows where, in the tied group that decides first place (or
    second, behind a unique first), the lowest index has a larger
    index mod 4 than another member -- it is scored by a later wave and wins
    the merge by the index comparison only.  Indices are local to the train
    range, as the kernel's are."""
    first = second = phase = 0
    for row in d:
        order = np.argsort(row, kind="stable")
        s = row[order]
        if len(s) >= 2 and s[0] == s[1]:
            first += 1
            group = order[s == s[0]]
        elif len(s) >= 3 and s[1] == s[2]:
            second += 1
            group = order[s == s[1]]
        else:
            continue
        res = group % NWAVE
        phase += bool((res[1:] < res[0]).any())
    return first, second, phase
