"""The matcher where its other tests do not look: equal distances, the scan
loops' second trip, and distances that are +inf or denormal.

Ties.  lex_lt's index comparison decides a result only in the four-wave merge
of knn_l1_kernel / knn_l1_seg_kernel (wave w scores rows r = w mod 4 of a
chunk; everywhere else candidates arrive in ascending index), and only when a
lower index sits in a later wave than an equal-distance higher one.  The
inputs of match_inputs.py tie densely and plant such pairs on purpose.  Their
expected values come from an exact integer reference (exact_knn), which
oracle/match.py must equal; the library is compared with both, bit for bit.
model_knn() replays the kernel's insertion schedule on the CPU and proves,
without a GPU, that the inputs tell a kernel without either index comparison
from a correct one, for every split count.

Scan carries.  seg_tiles_kernel scans 256 segments per trip, ratio_scan_kernel
1024 blocks of 256 rows per trip; segment counts 255..600 and q_cap of 1024,
1025 and 1028.x blocks take the second and third trips, and q_offsets[n] ==
q_cap at a multiple of 256 takes ratio_emit_kernel's blk == nblk.

+inf and denormals.  A candidate at distance +inf is never a neighbour
(sift_hip.h); distances made of multiples of 2^-149 are exact.

GPU (-m gpu) tests go through the C ABI into sentinel-filled outputs; the CPU
tests (reference, census, model, oracle, the +inf rule) need none."""
import functools

import numpy as np
import pytest

from conftest import assert_bits_equal

import match as M
import match_inputs as I
import test_match_batch as B

# (nq, nt, levels): the dense cases, each with the planted sets its nt has room for
DENSE = [(64, 5, 2), (65, 8, 3), (64, 63, 2), (65, 64, 3), (130, 65, 2), (64, 128, 3), (65, 129, 2),
         (130, 333, 2), (64, 4097, 3)]
DENSE_IDS = [f"{nq}x{nt}" for nq, nt, _ in DENSE]
# short train sets: every distance pattern over {0,1,2}^nt, and one query against nt copies of one row
SMALL_IDS = ["designed2", "designed3", "designed4"] + [f"copies{nt}" for nt in (2, 3, 4, 5, 8, 65)]
DENORM = 2.0 ** -149


@functools.lru_cache(maxsize=None)
def _dense(n):
    nq, nt, levels = DENSE[n]
    q, t, sets = I.dense_case(100 + n, nq, nt, levels)
    idx, dist = I.exact_knn(q, t, 2)
    case = dict(q=q, t=t, sets=sets, d=I.exact_distances(q, t), idx=idx, dist=dist)
    for a in (idx, dist, case["d"]):      # shared by every test that needs them
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _small(name):
    if name.startswith("designed"):
        q, t = I.designed_case(int(name[8:]))
    else:
        nt = int(name[6:])
        rng = np.random.default_rng(nt)
        t = np.tile(rng.integers(0, 256, (1, 128)).astype(np.float32), (nt, 1))
        q = t[:1].copy()
        q[0, 7] += 3
    idx, dist = I.exact_knn(q, t, 2)
    return dict(q=q, t=t, idx=idx, dist=dist)


def _k(case, k):
    return case["idx"][:, :k], case["dist"][:, :k]


# ---- C: a CPU model of the insertion schedule ------------------------------------------
def _insert(b, d, i, drop_first, drop_second):
    """match.hip's insert() on arrays; a switch drops that branch's index comparison."""
    d1, d2, i1, i2 = b
    lt1 = (d < d1) if drop_first else (d < d1) | ((d == d1) & (i < i1))
    lt2 = ~lt1 & ((d < d2) if drop_second else (d < d2) | ((d == d2) & (i < i2)))
    return (np.where(lt1, d, d1), np.where(lt1, d1, np.where(lt2, d, d2)),
            np.where(lt1, i, i1), np.where(lt1, i1, np.where(lt2, i, i2)))


def _empty(shape):
    return (np.full(shape, np.inf), np.full(shape, np.inf), np.full(shape, -1), np.full(shape, -1))


def model_knn(d, splits, drop_first=False, drop_second=False):
    """knn_l1_kernel + knn_merge_kernel on distances [nq, nt]: split s owns rows
    [s * per, (s + 1) * per), wave w of it inserts its rows r = w (mod 4) chunk
    after chunk in ascending index; wave 0 then inserts the lists of waves 1..3;
    the merge kernel inserts the splits' lists in split order.  Rows past nt are
    +inf, which insert() never takes."""
    nq, nt = d.shape
    per = -(-(-(-nt // splits)) // I.KTC) * I.KTC
    dd = np.full((nq, splits * per), np.inf)
    dd[:, :nt] = d
    dd = dd.reshape(nq, splits, per // I.NWAVE, I.NWAVE)
    ii = np.arange(splits * per).reshape(1, splits, per // I.NWAVE, I.NWAVE)
    sw = (drop_first, drop_second)
    b = _empty((nq, splits, I.NWAVE))
    for pos in range(per // I.NWAVE):                      # every (split, wave) advances one row
        b = _insert(b, dd[:, :, pos, :], ii[:, :, pos, :], *sw)
    m = tuple(x[..., 0] for x in b)
    for w in range(1, I.NWAVE):                            # the LDS merge by wave 0
        m = _insert(m, b[0][..., w], b[2][..., w], *sw)
        m = _insert(m, b[1][..., w], b[3][..., w], *sw)
    out = _empty((nq,))
    for s in range(splits):                                # knn_merge_kernel
        out = _insert(out, m[0][:, s], m[2][:, s], *sw)
        out = _insert(out, m[1][:, s], m[3][:, s], *sw)
    return np.stack([out[2], out[3]], 1).astype(np.int32), np.stack([out[0], out[1]], 1).astype(np.float32)


def _split_counts(nt):
    """Every split count from 1 to the number of chunks; counts that give the same rows per split once."""
    seen, out = set(), []
    for s in range(1, -(-nt // I.KTC) + 1):
        per = -(-(-(-nt // s)) // I.KTC) * I.KTC
        if per not in seen:
            seen.add(per)
            out.append(s)
    return out


# ---- CPU -----------------------------------------------------------------------------------
def test_planted_sets_cover_what_they_claim():
    for nt in (63, 64, 65, 128, 129, 333, 4097):
        sets = I.planted_sets(nt)
        used = [i for tied, near in sets for i in tied + (near,)]
        assert len(used) == len(set(used)) and max(used) < nt
        pairs = {(a % 4, b % 4) for (tied, _) in sets if len(tied) == 2 and tied[1] < 64 for a, b in [tied]}
        assert {(a, b) for a in range(4) for b in range(a)} <= pairs, nt    # the six that need the comparison
        assert len(pairs) == (16 if nt > 64 else 15), nt                     # 63 / 64 rows have room for 15
        sizes = {len(tied) for tied, _ in sets}
        assert {2, 3, 4} <= sizes, nt
        assert all(list(tied) == sorted(tied) for tied, _ in sets)
        if nt > 64:      # members in two chunks: one split or two, by the split count
            assert any(tied[0] // 64 != tied[-1] // 64 for tied, _ in sets), nt
        if nt > 128:     # first chunk | last chunk: two splits at every split count above 1
            assert any(tied[0] < 64 and tied[-1] // 64 == (nt - 1) // 64 for tied, _ in sets), nt
    assert I.planted_sets(5) == [((1, 4), 0)]
    assert [s[0] for s in I.planted_sets(8)] == [(1, 4), (3, 5)]


@pytest.mark.parametrize("n", range(len(DENSE)), ids=DENSE_IDS)
def test_census_of_dense_cases(n):
    """Conditions, asserted on the reference alone: >= 5 rows with d1 == d2, >= 5
    with d1 < d2 == d3, >= 3 where the lower tied index is scored by a later wave."""
    c = _dense(n)
    first, second, phase = I.census(c["d"])
    assert first >= 5 and second >= 5 and phase >= 3, (first, second, phase)
    # the planted queries see their set where the construction says
    tied, near = c["sets"][0]
    assert c["idx"][0].tolist() == list(tied[:2]) and c["dist"][0].tolist() == [0, 0]
    assert c["idx"][1].tolist() == [near, tied[0]] and c["dist"][1].tolist() == [1, 2]


def test_oracle_equals_exact_reference_on_every_input():
    for n in range(len(DENSE)):
        c = _dense(n)
        idx, dist = M.knn_match(c["q"], c["t"], 2)
        assert_bits_equal(idx, c["idx"], DENSE_IDS[n] + " idx")
        assert_bits_equal(dist, c["dist"], DENSE_IDS[n] + " dist")
        i1, d1 = M.knn_match(c["q"], c["t"], 1)
        assert_bits_equal(i1, c["idx"][:, :1], DENSE_IDS[n] + " idx k=1")
        assert_bits_equal(d1, c["dist"][:, :1], DENSE_IDS[n] + " dist k=1")
    for name in SMALL_IDS:
        c = _small(name)
        idx, dist = M.knn_match(c["q"], c["t"], 2)
        assert_bits_equal(idx, c["idx"], name + " idx")
        assert_bits_equal(dist, c["dist"], name + " dist")
    q, t, ridx, rdist = _denormal_case()
    idx, dist = M.knn_match(q, t, 2)
    assert_bits_equal(idx, ridx, "denormal idx")
    assert_bits_equal(dist, rdist, "denormal dist")


def test_designed_cases_hold_every_pattern():
    for nt in (2, 3, 4):
        q, t = I.designed_case(nt)
        d = I.exact_distances(q, t)
        assert len({tuple(r) for r in d.tolist()}) == 3 ** nt and set(np.unique(d)) == {256, 258, 260}


@pytest.mark.parametrize("n", range(len(DENSE)), ids=DENSE_IDS)
def test_model_needs_both_index_comparisons(n):
    """For every split count the faithful replay equals the reference, and the
    replay without the first (second) branch's index comparison does not: the
    case would fail a kernel with either mutation however its train is split."""
    c = _dense(n)
    d = c["d"].astype(np.float64)
    for splits in _split_counts(d.shape[1]):
        idx, dist = model_knn(d, splits)
        assert_bits_equal(idx, c["idx"], f"model idx, {splits} splits")
        assert_bits_equal(dist, c["dist"], f"model dist, {splits} splits")
        for sw in ((True, False), (False, True)):
            midx, _ = model_knn(d, splits, *sw)
            assert (midx != c["idx"]).any(), f"{splits} splits: dropping {sw} goes unseen"
            assert (midx[:, 0] != c["idx"][:, 0]).any() or not sw[0], f"{splits} splits: k = 1 does not see {sw}"


def test_model_on_short_train_sets():
    for name in SMALL_IDS:
        c = _small(name)
        idx, dist = model_knn(I.exact_distances(c["q"], c["t"]).astype(np.float64), 1)
        assert_bits_equal(idx, c["idx"], name)
        assert_bits_equal(dist, c["dist"], name)


# ---- E on the CPU: +inf is never a neighbour -------------------------------------------------
def _inf_case():
    """Train rows 0 / 2 are +-3e38 in every column, rows 1 / 3 / 4 ordinary.  Query
    0 (ordinary) has three finite candidates; query 1 (= train row 0) only row 0,
    at distance 0; query 2 (3e38 and -3e38 by halves) none.  No input is
    non-finite, no distance is NaN."""
    rng = np.random.default_rng(7)
    t = rng.integers(0, 256, (5, 128)).astype(np.float32)
    t[0], t[2] = 3e38, -3e38
    q = np.zeros((3, 128), np.float32)
    q[0] = t[3]
    q[0, 5] += 2
    q[1] = 3e38
    q[2, :64], q[2, 64:] = 3e38, -3e38
    d = I.exact_distances(q[:1], t[[1, 3, 4]])[0]
    near = np.array([1, 3, 4])[np.argsort(d, kind="stable")[:2]]
    idx = np.array([near, [0, -1], [-1, -1]], np.int32)
    dist = np.array([np.sort(d)[:2], [0, np.inf], [np.inf, np.inf]], np.float32)
    return q, t, idx, dist


def _oracle_knn(q, t, k):
    with np.errstate(over="ignore"):
        return M.knn_match(q, t, k)


def test_oracle_never_returns_a_candidate_at_inf():
    idx, dist = _oracle_knn(np.zeros((1, 128), np.float32), np.full((2, 128), 3e38, np.float32), 2)
    assert idx.tolist() == [[-1, -1]] and np.isposinf(dist).all()
    q, t, ridx, rdist = _inf_case()
    with np.errstate(over="ignore"):
        assert np.isposinf(M.l1_distances(q, t)).sum() == 2 + 4 + 5
    for k in (2, 1):
        idx, dist = _oracle_knn(q, t, k)
        assert_bits_equal(idx, ridx[:, :k], f"idx k={k}")
        assert_bits_equal(dist, rdist[:, :k], f"dist k={k}")
    assert [r[:2] for r in M.ratio_test(ridx, rdist, 1.0)] == [(0, 3)]      # queries 1 and 2 are skipped


def _denormal_case():
    """The 130x65 dense case shifted to signed values, some zeros as -0.0, all
    times 2^-149: every difference and every sum is an exact denormal."""
    c = _dense(4)
    q, t = c["q"] - 1, c["t"] - 1
    q[:, 100:110] = 0.0
    q[::3, 100:110] = -0.0
    t[::2, 100:110] = 0.0
    t[1::2, 100:110] = -0.0
    q, t = (q * np.float32(DENORM)).astype(np.float32), (t * np.float32(DENORM)).astype(np.float32)
    assert np.signbit(t[1, 100]) and t[1, 100] == 0 and (np.abs(t[t != 0]) < 2.0 ** -126).all()
    assert (q < 0).any() and (q > 0).any()
    idx, dist = I.exact_knn(q, t, 2, DENORM)
    assert_bits_equal(idx, c["idx"], "a shift and a scale move no neighbour")
    assert_bits_equal(dist, (c["dist"].astype(np.float64) * DENORM).astype(np.float32), "nor a distance, but by 2^-149")
    return q, t, idx, dist


# ---- GPU: ties through the three entry points -------------------------------------------------
def _plain_device(ctx, q, t, k, extra=8):
    import torch
    dq, dt = B._dev(q), B._dev(t)
    di = torch.full((len(q) + extra, k), -77, dtype=torch.int32, device="cuda")
    dd = torch.full((len(q) + extra, k), -5.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.knn_match_device(dq.data_ptr(), len(q), dt.data_ptr(), len(t), k, di.data_ptr(), dd.data_ptr())
    ctx.sync()
    idx, dist = di.cpu().numpy(), dd.cpu().numpy()
    assert (idx[len(q):] == -77).all() and (dist[len(q):] == -5.0).all(), "rows past n_query written"
    return idx[:len(q)], dist[:len(q)]


def _check_plain(ctx, q, t, k, ridx, rdist, what):
    for form, (idx, dist) in (("host", ctx.knnMatch(q, t, k)), ("device", _plain_device(ctx, q, t, k))):
        assert_bits_equal(idx, ridx, f"{what} {form} idx k={k}")
        assert_bits_equal(dist, rdist, f"{what} {form} dist k={k}")


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
@pytest.mark.parametrize("n", range(len(DENSE)), ids=DENSE_IDS)
def test_gpu_dense_ties_plain(ctx, n, k):
    c = _dense(n)
    _check_plain(ctx, c["q"], c["t"], k, *_k(c, k), DENSE_IDS[n])


@pytest.mark.gpu
@pytest.mark.parametrize("name", SMALL_IDS)
def test_gpu_short_train_sets_plain(ctx, name):
    c = _small(name)
    for k in (2, 1):
        _check_plain(ctx, c["q"], c["t"], k, *_k(c, k), name)


@pytest.mark.gpu
def test_gpu_plain_two_chunks_per_split(ctx):
    """The 64x4097 case's queries 33 times over: 33 query tiles make knn_splits
    63, so a split holds two chunks, and the planted pairs in chunks 0 | 1 meet
    inside one wave's list while those in chunks 0 | 64 meet in the split merge."""
    c = _dense(8)
    q = np.tile(c["q"], (33, 1))
    idx, dist = _plain_device(ctx, q, c["t"], 2)
    assert_bits_equal(idx, np.tile(c["idx"], (33, 1)), "idx")
    assert_bits_equal(dist, np.tile(c["dist"], (33, 1)), "dist")


def _shared_segments(k):
    """130x333 and 64x4097 (the latter among 100 mostly empty segments: 21
    splits of four chunks) cut into segments at tile edges and off them."""
    out = []
    for n, sizes in ((7, [0, 1, 0, 63, 1, 65]), (8, [0] * 40 + [1, 63] + [0] * 58)):
        c = _dense(n)
        qoff = B._offsets(sizes)
        assert qoff[-1] == len(c["q"])
        out.append((c["q"], qoff, c["t"], *_k(c, k)))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
def test_gpu_dense_ties_segmented_shared_train(ctx, k):
    for q, qoff, t, ridx, rdist in _shared_segments(k):
        idx, dist = B._knn_device(ctx, q, qoff, t, None, k, extra=64)
        B._check_live(idx, dist, ridx, rdist, qoff, len(q), f"shared train, {len(t)} rows, k={k}")


@functools.lru_cache(maxsize=None)
def _segmented_train_case():
    """Every dense case as one segment, behind a segment of no queries and three
    train rows: the train ranges start at 3, 8, 16, 79, 143, 208, 336, 465, 798
    (residues 3, 0, 0, 3, 3, 0, 0, 1, 2 mod 4; only one a multiple of 64), so the
    local index order is out of phase with the global row number and with the
    16-byte alignment of a chunk.  Nine splits from the capacities: the 4097-row
    range gets eight chunks per split, the 333-row range one."""
    cases = [_dense(n) for n in range(len(DENSE))]
    qoff = B._offsets([0] + [len(c["q"]) for c in cases])
    toff = B._offsets([3] + [len(c["t"]) for c in cases])
    assert toff[1:-1].tolist() == [3, 8, 16, 79, 143, 208, 336, 465, 798]
    q = np.concatenate([c["q"] for c in cases])
    t = np.concatenate([np.full((3, 128), 7, np.float32)] + [c["t"] for c in cases])
    ridx = np.concatenate([c["idx"] for c in cases])
    rdist = np.concatenate([c["dist"] for c in cases])
    oidx, odist = B._ref_knn(q, qoff, t, toff, 2)             # oracle/match.py per segment
    assert_bits_equal(oidx, ridx, "oracle idx")
    assert_bits_equal(odist, rdist, "oracle dist")
    return q, qoff, t, toff, ridx, rdist


def test_segmented_case_oracle_equals_reference():
    _segmented_train_case()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 1])
def test_gpu_dense_ties_segmented_train(ctx, k):
    q, qoff, t, toff, ridx, rdist = _segmented_train_case()
    idx, dist = B._knn_device(ctx, q, qoff, t, toff, k, extra=64)
    B._check_live(idx, dist, ridx[:, :k], rdist[:, :k], qoff, len(q), f"segmented train k={k}")


# ---- D: scan carries and block boundaries ---------------------------------------------------------
def _quantised(rng, n):
    x = np.zeros((n, 128), np.float32)
    x[:, :8] = rng.integers(0, 3, (n, 8))
    return x


@functools.lru_cache(maxsize=None)
def _many_segments(nseg, seg_train):
    """Segments of 0..3 query rows and two of 65: segment 100 (first trip of
    seg_tiles_kernel's scan) and the last one or, with 600, segment 520 (past
    the second trip).  Train: 70 shared rows, or 0..5 rows per segment and 70
    for the two long ones."""
    rng = np.random.default_rng(nseg * 2 + seg_train)
    long = (100, 520 if nseg > 520 else nseg - 1)
    q_sizes = rng.integers(0, 4, nseg)
    q_sizes[list(long)] = 65
    qoff = B._offsets(q_sizes)
    q = _quantised(rng, int(qoff[-1]))
    if seg_train:
        t_sizes = rng.integers(0, 6, nseg)
        t_sizes[list(long)] = 70
        toff = B._offsets(t_sizes)
        t = _quantised(rng, int(toff[-1]))
    else:
        toff, t = None, _quantised(rng, 70)
    ridx, rdist = B._ref_knn(q, qoff, t, toff, 2)
    return q, qoff, t, toff, ridx, rdist


@pytest.mark.gpu
@pytest.mark.parametrize("seg_train", [False, True], ids=["shared", "segmented"])
@pytest.mark.parametrize("nseg", [255, 256, 257, 513, 600])
def test_gpu_segment_counts_past_one_scan_trip(ctx, siftgpu, nseg, seg_train):
    q, qoff, t, toff, ridx, rdist = _many_segments(nseg, seg_train)
    idx, dist = B._knn_device(ctx, q, qoff, t, toff, 2, extra=64)
    B._check_live(idx, dist, ridx, rdist, qoff, len(q), f"{nseg} segments")
    # the ratio stage with keypoints over the same offsets
    rng = np.random.default_rng(nseg)
    qk, tk = B._kpts(siftgpu, rng, len(q)), B._kpts(siftgpu, rng, len(t))
    rec, rmoff, rsrc, rdst = B._ref_ratio(ridx, rdist, qoff, len(q), M.RATIO, qk, tk, toff)
    assert len(rec) > nseg // 4 and len(np.unique(rmoff)) > nseg // 8
    m, moff, src, dst = B._ratio_device(ctx, siftgpu, idx[:len(q)], dist[:len(q)], qoff, len(q), M.RATIO, qk, tk, toff,
                                         extra=64)
    _check_ratio(siftgpu, (m, moff, src, dst), (rec, rmoff, rsrc, rdst), len(q), f"{nseg} segments")


def _check_ratio(siftgpu, got, want, m_cap, what, xy=True):
    """moff holds the true totals; the first min(kept, m_cap) records (and xy)
    equal the reference; nothing else is written."""
    (m, moff, src, dst), (rec, rmoff, rsrc, rdst) = got, want
    n = min(len(rec), m_cap)
    assert_bits_equal(moff, rmoff, what + " moff")
    assert_bits_equal(m[:n], B._rec_array(siftgpu, rec[:n]), what + " records")
    assert (m[n:].view(np.int32) == -77).all(), what + ": records past the kept count written"
    if xy:
        assert_bits_equal(src[:n], rsrc[:n], what + " src_xy")
        assert_bits_equal(dst[:n], rdst[:n], what + " dst_xy")
    assert (src[n if xy else 0:] == -5.0).all() and (dst[n if xy else 0:] == -5.0).all(), what + ": xy written"


RB = 256          # rows per block of the ratio stage (match.hip kRB)
TRIP = 1024 * RB  # rows per trip of ratio_scan_kernel


@functools.lru_cache(maxsize=None)
def _ratio_blocks_case(q_cap, layout):
    """idx / dist of q_cap rows, none kept but the planted ones.
    "edges": kept rows in the first block, in blocks 1023 and 1024 (either side
    of the scan's trip), in block 500 and in the last block (its last row too);
    q_offsets[n] == q_cap, with keypoints.
    "gap": q_offsets[0] = 3 (rows 0..2 would be kept but are not live), kept rows
    in the first block and block 900, then none until the last block: a stretch
    of no kept row across the trip; q_offsets[n] = q_cap + 1000.
    Segment bounds on and off multiples of 256, one at the trip exactly.  Rows
    whose second index is -1 pass the comparison and must not count."""
    nblk = -(-q_cap // RB)
    rows = np.arange(q_cap)
    idx = np.stack([rows % 50, (rows + 1) % 50], 1).astype(np.int32)
    dist = np.ones((q_cap, 2), np.float32)
    last = (nblk - 1) * RB
    if layout == "edges":
        kept = [0, 5, 255, 500 * RB + 1, 500 * RB + 64, 500 * RB + 200, 1023 * RB, 1023 * RB + 63, 1023 * RB + 255,
                TRIP, TRIP + 1, TRIP + 76, TRIP + 77, last, q_cap - 1]
        qoff = [0, 256, 1000, 1023 * RB, TRIP, TRIP + 77, q_cap]
    else:
        kept = [0, 1, 2, 3, 4, 200, 900 * RB + 7, 900 * RB + 255, last, last + 1, q_cap - 1]
        qoff = [3, 256, 1000, 1023 * RB + 1, TRIP, TRIP + 77, q_cap + 1000]
    kept = sorted({r for r in kept if r < q_cap})
    dist[kept, 0] = 0.5
    skipped = [r for r in (9, 1023 * RB + 9, TRIP + 9, q_cap - 2) if r < q_cap]
    dist[skipped, 0] = 0.25
    idx[skipped, 1] = -1
    dist[skipped, 1] = np.inf
    qoff = np.array(qoff, np.int32)
    want = B._ref_ratio(idx, dist, qoff, q_cap)
    assert len(want[0]) == len(kept) - (3 if layout == "gap" else 0)
    return idx, dist, qoff, want


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["edges", "gap"])
@pytest.mark.parametrize("q_cap", [262144, 262400, 263185])
def test_gpu_ratio_stage_past_one_scan_trip(ctx, siftgpu, q_cap, layout):
    """q_cap of exactly 1024 blocks, 1025 blocks, and 1028 blocks and a partial
    one; m_cap above and below the kept count."""
    idx, dist, qoff, want = _ratio_blocks_case(q_cap, layout)
    kept = len(want[0])
    for m_cap in (kept + 5, kept - 4):
        got = B._ratio_device(ctx, siftgpu, idx, dist, qoff, q_cap, m_cap=m_cap, extra=64)
        _check_ratio(siftgpu, got, want, m_cap, f"q_cap {q_cap} {layout} m_cap {m_cap}", xy=False)
    if layout == "edges" and q_cap == 262144:
        rng = np.random.default_rng(31)
        qk, tk = B._kpts(siftgpu, rng, q_cap), B._kpts(siftgpu, rng, 50)
        want = B._ref_ratio(idx, dist, qoff, q_cap, M.RATIO, qk, tk, None)
        got = B._ratio_device(ctx, siftgpu, idx, dist, qoff, q_cap, M.RATIO, qk, tk, None, m_cap=kept, extra=64)
        _check_ratio(siftgpu, got, want, kept, "with keypoints")


@pytest.mark.gpu
def test_gpu_ratio_stage_last_offset_on_the_last_block_edge(ctx, siftgpu):
    """q_cap = 512 = q_offsets[n]: the boundary wave of the last offset takes
    blk == nblk and reads the scan's total; a bound at 256 takes a whole block."""
    q_cap = 512
    rows = np.arange(q_cap)
    idx = np.stack([rows % 50, (rows + 1) % 50], 1).astype(np.int32)
    dist = np.ones((q_cap, 2), np.float32)
    dist[[0, 99, 100, 255, 256, 300, 511], 0] = 0.5
    qoff = np.array([0, 100, 256, 512], np.int32)
    want = B._ref_ratio(idx, dist, qoff, q_cap)
    assert want[1].tolist() == [0, 2, 4, 7]
    for m_cap in (512, 7, 3):
        got = B._ratio_device(ctx, siftgpu, idx, dist, qoff, q_cap, m_cap=m_cap, extra=64)
        _check_ratio(siftgpu, got, want, m_cap, f"m_cap {m_cap}", xy=False)


# ---- E on the GPU ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_never_returns_a_candidate_at_inf(ctx, siftgpu):
    q, t, ridx, rdist = _inf_case()
    for k in (2, 1):
        _check_plain(ctx, q, t, k, ridx[:, :k], rdist[:, :k], "+inf")
    big = np.full((2, 128), 3e38, np.float32)
    idx, dist = ctx.knnMatch(np.zeros((1, 128), np.float32), big, 2)
    assert idx.tolist() == [[-1, -1]] and np.isposinf(dist).all()
    # segmented: the three queries as three segments of the shared train, then each against its own rows
    qoff = np.array([0, 1, 2, 3], np.int32)
    idx, dist = B._knn_device(ctx, q, qoff, t, None, 2, extra=64)
    B._check_live(idx, dist, ridx, rdist, qoff, 3, "+inf, shared train")
    toff = np.array([0, 5, 5, 5], np.int32)                    # segment 0: all rows; 1 and 2: none
    idx, dist = B._knn_device(ctx, q, qoff, t, toff, 2, extra=64)
    assert_bits_equal(idx[:1], ridx[:1], "+inf, segmented train")
    assert (idx[1:3] == -1).all() and np.isposinf(dist[1:3]).all()
    # the ratio stage skips the queries without a second neighbour
    idx, dist = B._knn_device(ctx, q, qoff, t, None, 2)
    want = B._ref_ratio(ridx, rdist, qoff, 3, 1.0)
    assert [r[:2] for r in want[0]] == [(0, 3)] and want[1].tolist() == [0, 1, 1, 1]
    got = B._ratio_device(ctx, siftgpu, idx, dist, qoff, 3, 1.0, extra=64)
    _check_ratio(siftgpu, got, want, 3, "+inf ratio stage", xy=False)
    # BFMatcher.knnMatch returns the short lists
    lists = siftgpu.BFMatcher(siftgpu.NORM_L1, ctx=ctx).knnMatch(q, t, 2)
    assert [[m.trainIdx for m in row] for row in lists] == [ridx[0].tolist(), [0], []]
    assert [m.trainIdx for m in siftgpu.ratio_test(lists, 1.0)] == [3]


@pytest.mark.gpu
def test_gpu_denormal_distances_are_exact(ctx):
    """Inputs, differences and sums are multiples of 2^-149 below 2^-126: a
    kernel that flushed denormals would return zeros and the first two indices."""
    q, t, ridx, rdist = _denormal_case()
    assert (rdist[12:] > 0).any() and rdist.max() < 2.0 ** -126
    for k in (2, 1):
        _check_plain(ctx, q, t, k, ridx[:, :k], rdist[:, :k], "denormal")
    qoff = B._offsets([1, 64, 65])
    idx, dist = B._knn_device(ctx, q, qoff, t, None, 2, extra=64)
    B._check_live(idx, dist, ridx, rdist, qoff, len(q), "denormal, segmented")
