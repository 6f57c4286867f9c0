"""Inputs of the match-join tests (test_join.py on the CPU, test_gpu_join.py on the
GPU): one call of 14 segments, generated from a seed and computed once per
process.  call() is the census the issue lists; expected(a_side, b_side, masks)
is join_oracle.py's answer for it, cached.

Both indices of every record are keys of the same range, so the one call is run
under each of the four settings of (a_key_side, b_key_side)."""
import functools

import numpy as np

import join_oracle as JO

MATCH = np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<f4"), ("segment", "<i4")])
KRB = 256                       # rows per block of the stage (scratch.hpp's kJoinRows)
SIDES = [(0, 0), (0, 1), (1, 0), (1, 1)]
J_CAP = 1000                    # below the joined total of every side setting: the last rows are cut

# label, A rows, B rows, keys
CENSUS = [("b0", 50, 0, 40), ("b1", 30, 1, 20), ("b255", 300, 255, 150), ("b256", 200, 256, 180),
          ("b257", 257, 257, 140), ("b600", 600, 600, 350), ("a0", 0, 40, 30), ("dup_dist", 120, 100, 60),
          ("dup_equal", 90, 80, 50), ("dup_masked", 90, 80, 50), ("bad_keys", 100, 100, 64), ("dup_b", 60, 128, 40),
          ("backwards", 0, 0, 10), ("past_cap", 70, 90, 45)]
LABELS = [c[0] for c in CENSUS]
A_CUT, B_CUT, KEY_CUT = 7, 9, 4      # the last offsets lie this far past the capacities
A_BACK, B_BACK = 3, 5                # how far the backwards pair steps back


class Call:
    pass


def _table(rng, n, n_keys):
    t = np.zeros(n, MATCH)
    t["query"] = rng.integers(0, n_keys, n)
    t["train"] = rng.integers(0, n_keys, n)
    t["distance"] = rng.integers(0, 12, n).astype(np.float32) / 4       # few values: ties are common
    t["segment"] = rng.integers(-5, 99, n)                              # never read
    return t


def _segment(label, rng, na, nb, nk):
    a, b = _table(rng, na, nk), _table(rng, nb, nk)
    am, bm = (rng.random(na) < 0.8).astype(np.uint8), (rng.random(nb) < 0.85).astype(np.uint8)
    both = lambda t, rows, key: [t[f].__setitem__(rows, key) for f in ("query", "train")]  # noqa: E731

    def only(t, rows, key, spare):   # `rows` name `key` on both sides, and no other row of the table does
        others = [r for r in range(len(t)) if r not in rows and key in (t["query"][r], t["train"][r])]
        both(t, others, spare)
        both(t, rows, key)

    if label == "dup_dist":          # key 7: rows 10, 20, 30 at 2.5, 0.5, 1.5 -> row 20
        only(a, [10, 20, 30], 7, 8)
        a["distance"][[10, 20, 30]] = [2.5, 0.5, 1.5]
        am[[10, 20, 30]] = 1
        both(b, [0, 50], 7)
        bm[[0, 50]] = 1
    if label == "dup_equal":         # key 9: rows 40, 15, 60 all at 0.75 -> row 15
        only(a, [40, 15, 60], 9, 10)
        a["distance"][[40, 15, 60]] = 0.75
        am[[40, 15, 60]] = 1
        both(b, [3], 9)
        bm[3] = 1
    if label == "dup_masked":        # key 11: row 5 at 0.25 masked out, row 70 at 1.0 wins over row 71 at 1.25
        only(a, [5, 70, 71], 11, 12)
        a["distance"][[5, 70, 71]] = [0.25, 1.0, 1.25]
        am[[5, 70, 71]] = [0, 1, 1]
        both(b, [4], 11)
        bm[4] = 1
    if label == "bad_keys":
        both(a, [0, 1], -1), both(a, [2, 3], nk), both(a, [4], 2 ** 31 - 1), both(a, [5], -2 ** 31)
        both(b, [0, 1], -1), both(b, [2, 3], nk), both(b, [4], 2 ** 31 - 1), both(b, [5], -2 ** 31)
        # keys 20..25 have exactly these candidates: -0.0 beats 0.5; +inf is a candidate; NaN and -1.0 are none
        for key, rows in ((20, [10, 11]), (21, [12]), (22, [13]), (23, [14]), (24, [15, 16]), (25, [17, 18])):
            only(a, rows, key, 30)
        a["distance"][[10, 11, 12, 13, 14, 15, 16, 17, 18]] = [0.5, -0.0, np.inf, np.nan, -1.0, np.nan, 3.0, 0.0, -0.0]
        am[6:19] = 1
        for k, r in zip((20, 21, 22, 23, 24, 25), (10, 11, 12, 13, 14, 15)):
            both(b, [r], k)
        bm[:16] = 1
    if label == "dup_b":             # B rows 0..7 all name key 3, which has a winner
        both(a, [2], 3)
        am[2] = 1
        both(b, list(range(8)), 3)
        bm[:8] = 1
    return a, b, am, bm


@functools.lru_cache(maxsize=None)
def call():
    rng = np.random.default_rng(20260)
    c = Call()
    c.labels = LABELS
    A, B, AM, BM = [], [], [], []
    a_off, b_off, k_off = [0], [0], [0]
    for label, na, nb, nk in CENSUS:
        if label == "backwards":     # the pair steps back: an empty segment; the next one starts inside "dup_b"
            a_off.append(a_off[-1] - A_BACK), b_off.append(b_off[-1] - B_BACK), k_off.append(k_off[-1] + nk)
            continue
        a, b, am, bm = _segment(label, rng, na, nb, nk)
        if label == "dup_b":         # its last B rows belong to "past_cap" too: no key, so both leave a 0 there
            for f in ("query", "train"):
                b[f][-B_BACK:] = -1
        A.append(a), B.append(b), AM.append(am), BM.append(bm)
        a_off.append(a_off[-1] + na), b_off.append(b_off[-1] + nb), k_off.append(k_off[-1] + nk)
    # the last segment's rows follow the stepped-back offsets, and its end lies past the capacities
    c.a, c.b = np.concatenate(A), np.concatenate(B)
    c.a_mask, c.b_mask = np.concatenate(AM), np.concatenate(BM)
    c.a_off, c.b_off, c.k_off = (np.array(o, np.int32) for o in (a_off, b_off, k_off))
    c.a_cap, c.b_cap, c.key_cap = len(c.a) - A_BACK - A_CUT, len(c.b) - B_BACK - B_CUT, int(c.k_off[-1]) - KEY_CUT
    c.a, c.a_mask, c.b, c.b_mask = c.a[:c.a_cap], c.a_mask[:c.a_cap], c.b[:c.b_cap], c.b_mask[:c.b_cap]
    # the gathered rows: 3-D points whose bytes must survive (NaN payloads, -0.0, infinities, denormals)
    c.a_xyz = rng.standard_normal((c.a_cap, 3)) * 5
    odd = np.array([0x7ff8000000abcdef, 0xfff0000000000001, 0x8000000000000000, 0x7ff0000000000000, 1], np.uint64)
    c.a_xyz.view(np.uint64).reshape(-1)[::37] = np.resize(odd, len(c.a_xyz.reshape(-1)[::37]))
    c.b_xy = (rng.random((c.b_cap, 2)) * 640).astype(np.float32)
    c.b_xy.view(np.uint32).reshape(-1)[::41] = 0x7fc12345
    c.j_cap = J_CAP
    c.n_segments = len(LABELS)
    return c


def index(label):
    return LABELS.index(label)


def bounds(c, s):
    """(alo, ahi, blo, bhi, n_keys) of segment s, clamped as the library clamps."""
    alo, ahi = JO.clamp(c.a_off[s], c.a_cap), JO.clamp(c.a_off[s + 1], c.a_cap)
    blo, bhi = JO.clamp(c.b_off[s], c.b_cap), JO.clamp(c.b_off[s + 1], c.b_cap)
    return alo, max(ahi, alo), blo, max(bhi, blo), JO.clamp(c.k_off[s + 1], c.key_cap) - JO.clamp(c.k_off[s], c.key_cap)


@functools.lru_cache(maxsize=None)
def expected(a_side, b_side, masks=True, j_cap=J_CAP):
    c = call()
    return JO.join_segmented(c.a, c.a_off, c.a_cap, a_side, c.a_mask if masks else None, c.a_xyz, c.b, c.b_off, c.b_cap,
                             b_side, c.b_mask if masks else None, c.b_xy, c.k_off, c.key_cap, j_cap)


def tiles(off, cap):
    """The blocks of KRB rows a table's segments take, and the most the stage launches."""
    n = len(off) - 1
    used = sum(-(-(max(JO.clamp(off[s + 1], cap) - JO.clamp(off[s], cap), 0)) // KRB) for s in range(n))
    return used, cap // KRB + n
