"""The squared-L2 kNN matcher on float descriptors: what holds without a GPU.

The exports, the null-context checks, the Python names, the layout program, and
the oracle of match_l2_f32_inputs on its own: its float32 fma against libm's
fmaf, the dyadic identity against the integer reference, a census of rows whose
bits depend on the summation order, a census of the planted ties, and the
rule's error bound on real descriptors against float64; the NaN rule of
knn_from, and the censuses of the value cases (signed rows, near-copies around
the clamp, subnormals, overflow) with the mutations of the rule they tell apart."""
import ctypes
import ctypes.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal

import match_l2_f32_inputs as F
import match_l2_inputs as L2
import match_u8_inputs as U

NEW = ["sift_knn_match_l2sqr_f32_segmented_device", "sift_knn_match_l2sqr_f32_segmented", "sift_knn_match_l2sqr_f32"]
f32 = np.float32


def test_l2_f32_entry_points_declared_exported_and_wrapped(siftgpu):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sift_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert getattr(siftgpu.lib(), name).argtypes is not None, name
    assert re.search(r"#define\s+SIFT_METRIC_L2SQR_F32\s+3\b", text)
    assert b"match_l2sqr_f32_segmented\0" in open(siftgpu.LIB_PATH, "rb").read()     # the stage's name


def test_l2_f32_entry_points_reject_null_context(siftgpu):
    L = siftgpu.lib()
    f = np.zeros(128, np.float32)
    off = np.array([0, 1], np.int32)
    ix = np.zeros(2, np.int32)
    pf = f.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    pi = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))  # noqa: E731
    E = siftgpu.SIFT_E_INVALID
    assert L.sift_knn_match_l2sqr_f32_segmented_device(None, f.ctypes.data, off.ctypes.data, 1, 1, f.ctypes.data, None,
                                                       1, 2, ix.ctypes.data, f.ctypes.data) == E
    assert L.sift_knn_match_l2sqr_f32_segmented(None, pf, pi(off), 1, 1, pf, None, 1, 2, pi(ix), pf) == E
    assert L.sift_knn_match_l2sqr_f32(None, pf, 1, pf, 1, 2, pi(ix), pf) == E
    # and with nothing to do: the null context is still rejected first
    assert L.sift_knn_match_l2sqr_f32_segmented_device(None, None, None, 0, 0, None, None, 0, 2, None, None) == E
    assert L.sift_knn_match_l2sqr_f32_segmented(None, None, None, 0, 0, None, None, 0, 2, None, None) == E
    assert L.sift_knn_match_l2sqr_f32(None, None, 0, None, 0, 2, None, None) == E


def test_l2_f32_python_names_and_pinned_rejections(siftgpu):
    for meth in ["knn_match_l2sqr_f32_segmented_device", "knnMatchL2SqrF32Segmented", "knnMatchL2SqrF32"]:
        assert callable(getattr(siftgpu.Context, meth)), meth
    assert siftgpu.SIFT_METRIC_L2SQR_F32 == 3
    sig = inspect.signature(siftgpu.l2_match)
    assert list(sig.parameters) == ["query", "train", "k", "squared", "ctx"]
    assert [sig.parameters[p].default for p in ("k", "squared", "ctx")] == [2, False, None]
    f = np.zeros((2, 128), np.float32)
    with pytest.raises(ValueError):
        siftgpu.BFMatcher(4)                                       # plain NORM_L2 stays out of BFMatcher
    with pytest.raises(ValueError):
        siftgpu.BFMatcher(siftgpu.NORM_L2SQR).knnMatch(f, f, 2)    # raised before any context is made
    with pytest.raises(ValueError):
        siftgpu.cross_check_match(f, f, siftgpu.NORM_L2SQR)
    with pytest.raises(ValueError):
        siftgpu.window_match(f, None, f, None, 1.0, normType=siftgpu.NORM_L2SQR)
    for doc in (siftgpu.BFMatcher.__doc__, siftgpu.cross_check_match.__doc__, siftgpu.window_match.__doc__):
        assert "l2_match" in doc


def test_match_l2_f32_layouts(tmp_path):
    """tests/cpp/match_l2_f32_layout.cpp, built like test_match_l2_u8.py::test_match_l2_u8_layouts:
    with the address and undefined-behaviour sanitizers (runtimes linked
    statically into the program) where the host compiler has them."""
    src = os.path.join(ROOT, "tests", "cpp", "match_l2_f32_layout.cpp")
    exe = tmp_path / "match_l2_f32_layout"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "match l2 f32 layouts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- the oracle's fma --------------------------------------------------------------------
def _libm_fmaf(a, b, c):
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    return np.array([m.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], f32)


def test_fma32_equals_libm_fmaf():
    rng = np.random.default_rng(150)
    n = 20000
    a, b = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    c = (rng.standard_normal(n) * rng.choice([1e-6, 1e-3, 1.0, 1e3], n)).astype(f32)
    a[:5000], b[:5000] = F.rows(rng, 40).ravel()[:5000], F.rows(rng, 40).ravel()[:5000]   # descriptor-like
    c[:5000] = np.abs(c[:5000])
    assert_bits_equal(F.fma32(a, b, c), _libm_fmaf(a, b, c), "random triples")
    # crafted midpoints: the product of two odd 12.x-bit integers in [2^24, 2^25) is an odd 25-bit
    # integer, exactly half way between two float32; an addend far below float64's last bit of the
    # sum decides the side, but the float64 sum drops it and the cast then goes to even
    m = 4000
    x = (2 * rng.integers(2048, 2896, m) + 1).astype(f32)
    y = (2 * rng.integers(2048, 2896, m) + 1).astype(f32)
    prod = x.astype(np.int64) * y.astype(np.int64)
    assert ((prod >= 1 << 24) & (prod < 1 << 25) & (prod % 2 == 1)).all()
    scale = (2.0 ** rng.integers(-30, 10, m)).astype(f32)
    z = (rng.choice([-1.0, 1.0], m) * 2.0 ** rng.integers(-60, -40, m)).astype(f32)
    z[:m // 8] = 0                                                                      # true ties: to even
    x, z = x * scale, z * scale
    ref = _libm_fmaf(x, y, z)
    assert_bits_equal(F.fma32(x, y, z), ref, "midpoint products with an addend below float64's rounding")
    naive = (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(f32)
    assert (naive.view(np.int32) != ref.view(np.int32)).sum() > m // 8, "the crafted cases do trap a double rounding"
    # and in the subnormal range of float32
    x, y, z = x[:500] * f32(2.0 ** -100), y[:500] * f32(2.0 ** -60), z[:500] * f32(2.0 ** -100)
    assert_bits_equal(F.fma32(x, y, z), _libm_fmaf(x, y, z), "subnormal results")


# ---- the dyadic identity -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["weights", "extremes", "dense65x64", "bits300x65"])
def test_oracle_dyadic_identity(name):
    """On rows u / 512 the oracle's d is the int64 squared distance times 2^-18 exactly,
    indices included: every product, sum and norm is an integer below 2^24 in units of
    2^-18, so no summation order matters."""
    u = {"weights": L2.weights_case, "extremes": L2.extremes_case,
         "dense65x64": lambda: L2.tie_case(U.TIE_IDS.index("dense65x64")),
         "bits300x65": lambda: L2.tie_case(U.TIE_IDS.index("bits300x65"))}[name]()
    idx, dist = F.seg_ref(F.dyadic(u.q), u.qoff, F.dyadic(u.t), u.toff, 2, u.q_cap, u.t_cap)
    assert_bits_equal(idx, u.idx, name + " idx")
    assert_bits_equal(dist * F.SCALE, u.dist, name + " dist * 2^18")
    rev = F.seg_ref(F.dyadic(u.q), u.qoff, F.dyadic(u.t), u.toff, 2, u.q_cap, u.t_cap, order=F.PI[::-1])
    assert_bits_equal(rev[1], dist, name + " in the reversed order")


# ---- the censuses ------------------------------------------------------------------------
def test_oracle_order_census():
    """On the random float inputs the oracle under PI and under the reversed order differ in
    the bits of the nearest distance on at least a tenth of the rows (a sum of 128 products
    rounded 128 times lands on another float for most orders), so the GPU's bit comparison
    pins the order and is not vacuous."""
    c = F.edges_case(False)
    q = c.q[c.qoff[11]:c.qoff[12]]
    a = F.knn_ref(q, c.t, 1)[1]
    b = F.knn_ref(q, c.t, 1, order=F.PI[::-1])[1]
    ident = F.knn_ref(q, c.t, 1, order=np.arange(128))[1]
    differ = int((a.view(np.int32) != b.view(np.int32)).sum())
    differ_id = int((a.view(np.int32) != ident.view(np.int32)).sum())
    print(f"rows whose d1 differs: reversed {differ}, identity {differ_id} of {len(q)}")
    assert differ >= len(q) // 10 and differ_id >= len(q) // 10


@pytest.mark.parametrize("which", ["shared", "segmented", "splits"])
def test_oracle_tie_census(which):
    """Every tie input still has rows tied for first place, and rows tied for second place
    behind a unique nearer row: the planted ones, by the oracle's distances."""
    c = {"shared": lambda: F.edges_case(False), "segmented": lambda: F.edges_case(True), "splits": F.splits_case}[which]()
    first, second = F.census(c)
    print(f"{c.name}: {first} rows tied for first place, {second} for second")
    assert first >= 4 and second >= 4


# ---- sanity of the rule itself -----------------------------------------------------------
def real_pairs():
    """(name, query, train) from the descriptors of the golden images."""
    g = lambda n: np.load(os.path.join(ROOT, "tests", "golden", n), allow_pickle=False)  # noqa: E731
    book, synth, m = g("book.npz")["desc"], g("ref_synth_240x320.npz")["desc"], g("match.npz")
    # (match.npz's "dup" rows are copies planted for ties: no gap to rank by, so they are not used here)
    return [("book-synth", book, synth), ("synth-book", synth, book), ("noisy-book", m["noisy"], book)]


GAMMA130 = 130 * 2.0 ** -24 / (1 - 130 * 2.0 ** -24)


def check_against_float64(name, q, t, idx, dist):
    """Asserts |d - d64| <= B = 2 gamma_130 (nq + nt) on the returned neighbours and that the
    indices are the float64 ranking's on every row whose 1st-2nd and 2nd-3rd gaps exceed 2 B.
    Returns the number of rows exempt from the index check."""
    q64, t64 = np.asarray(q, np.float64), np.asarray(t, np.float64)
    d64 = ((q64[:, None, :] - t64[None, :, :]) ** 2).sum(-1)
    bound = 2 * GAMMA130 * ((q64 ** 2).sum(-1)[:, None] + (t64 ** 2).sum(-1)[None, :])
    rows = np.arange(len(q))
    for j in range(2):
        err = np.abs(dist[:, j].astype(np.float64) - d64[rows, idx[:, j]])
        lim = bound[rows, idx[:, j]]
        print(f"{name}: column {j} max |d - d64| = {err.max():.3e}, min slack = {(lim - err).min():.3e}")
        assert (err <= lim).all(), name
    order = np.argsort(d64, axis=1, kind="stable")
    s = np.take_along_axis(d64, order[:, :3], axis=1)
    b = bound.max(axis=1)
    clear = ((s[:, 1] - s[:, 0]) > 2 * b) & ((s[:, 2] - s[:, 1]) > 2 * b)
    assert (idx[clear] == order[clear, :2]).all(), name
    print(f"{name}: {int((~clear).sum())} of {len(q)} rows exempt")
    return int((~clear).sum())


def test_oracle_rule_against_float64_on_real_descriptors():
    """The oracle alone stays within the bound and within 1 % exempt rows on the chosen images."""
    for name, q, t in real_pairs():
        idx, dist = F.knn_ref(q, t, 2)
        exempt = check_against_float64(name, q, t, idx, dist)
        assert exempt <= 0.01 * len(q), (name, exempt, len(q))


# ---- values: the NaN rule, signs, cancellation, subnormals, overflow ---------------------
def test_knn_from_treats_nan_as_inf():
    """A row at a NaN distance is never a neighbour, exactly like one at +inf; the missing
    entries are -1 / +inf and no NaN reaches the result."""
    nan, inf = np.nan, np.inf
    d = np.array([[nan, 1.0, inf, 0.5], [nan, inf, nan, inf], [nan, 2.0, nan, nan], [0.0, nan, 0.0, -0.0]], f32)
    idx, dist = F.knn_from(d, 2)
    assert idx.tolist() == [[3, 1], [-1, -1], [1, -1], [0, 2]]
    assert_bits_equal(dist, np.array([[0.5, 1.0], [inf, inf], [2.0, inf], [0.0, 0.0]], f32), "dist")
    assert F.knn_from(d, 1)[0].tolist() == [[3], [-1], [1], [0]]


class _Dyadic:
    """The float form of a byte case, as the GPU test feeds it."""

    def __init__(self, u):
        self.name, self.qoff, self.toff, self.q_cap, self.t_cap = u.name, u.qoff, u.toff, u.q_cap, u.t_cap
        self.q, self.t = F.dyadic(u.q), F.dyadic(u.t)


def test_no_case_from_before_the_nan_rule_has_a_nan_distance():
    """knn_from's NaN rule changes no expected value that existed before it: no distance of
    any earlier case is NaN (nor infinite, nor negative), scored pair by scored pair."""
    cases = [F.edges_case(False), F.edges_case(True), F.splits_case(), F.many_segments_case(), F.weights_case()]
    cases += F.clamp_cases() + [_Dyadic(u) for u in F.dyadic_sources()]
    pairs = 0
    for c in cases:
        dyadic = isinstance(c, _Dyadic)
        for _, _, qs, ts in F.seg_tables(c):
            if dyadic and len(qs) * len(ts) > 20000:
                # the large byte cases: elements in [0, 0.5), so every norm and |dot| is at most
                # 32 and fmaf(-2, dot, s) is finite; the first and last queries stand for the table
                assert (qs >= 0).all() and (qs < 0.5).all() and (ts >= 0).all() and (ts < 0.5).all(), c.name
                qs = np.concatenate([qs[:16], qs[-16:]])
            d = F.distances(qs, ts)
            assert np.isfinite(d).all() and (d >= 0).all(), c.name
            pairs += d.size
    print(f"{len(cases)} cases, {pairs} scored pairs, none NaN")
    assert pairs > 100000


def _float64_by_segment(c):
    exempt = 0
    for b, q0, qs, ts in F.seg_tables(c):
        exempt += check_against_float64(f"{c.name}[{b}]", qs, ts, c.idx[q0:q0 + len(qs)], c.dist[q0:q0 + len(qs)])
    return exempt


@pytest.mark.parametrize("seg_train", [False, True], ids=["shared", "segmented"])
def test_signed_case_census(seg_train):
    """At least a quarter of all dots are negative; a zero query against a zero train row
    gives d = +0.0 in bits; a negated query is at d = 4 nq up to the rule's bound, the
    farthest row of its query; and the rule's float64 bound holds on signed rows."""
    c = F.signed_case(seg_train)
    assert (c.q < 0).mean() > 0.4 and (c.t < 0).mean() > 0.4
    neg = total = zero_pairs = 0
    for b, q0, qs, ts in F.seg_tables(c):
        dot = F.chain(qs[:, None, :], ts[None, :, :])
        neg, total = neg + int((dot < 0).sum()), total + dot.size
        d = F.distances(qs, ts)
        zq, zt = ~qs.any(axis=1), ~ts.any(axis=1)
        assert zq.sum() == 2 and zt.sum() == (b == 0 or not seg_train)
        zero_pairs += int((d[np.ix_(zq, zt)].view(np.int32) == 0).sum())
        assert (d[np.ix_(zq, zt)].view(np.int32) == 0).all()
        for seg, j, r in c.negated:
            if seg == b:
                nq = float(F.chain(qs[j], qs[j]))
                assert dot[j, r] == -F.chain(qs[j], qs[j]) and abs(float(d[j, r]) - 4 * nq) <= 4 * GAMMA130 * nq
                assert d[j, r] == d[j].max()
    print(f"{c.name}: {neg} of {total} dots negative, {zero_pairs} zero pairs at +0.0, {len(c.negated)} negated rows")
    assert 4 * neg >= total and zero_pairs >= 1 and len(c.negated) >= 6
    assert np.isfinite(c.dist).all()
    _float64_by_segment(c)


@pytest.mark.parametrize("seg_train", [False, True], ids=["shared", "segmented"])
def test_cancel_case_census(seg_train):
    """Of the planted (query, near-copy) pairs at least 16 have fmaf(-2, dot, s) < 0 and at
    least 16 have it > 0; at least 4 planted queries have both near-copies clamped to 0 (a
    tie by index), one of them across a tile seam that is no split seam and one across a
    split seam.  Every planted distance is within the rule's bound B of 0, and the float64
    nearest two of a planted query are its two near-copies, as are the oracle's."""
    c = F.cancel_case(seg_train)
    neg, pos, tied = F.cancel_census(c)
    print(f"{c.name}: {2 * len(c.planted)} planted pairs, {neg} below 0, {pos} above, {len(tied)} tied queries: "
          + ", ".join(f"{tied.count(k)} {k}" for k in sorted(set(tied))))
    assert len(c.planted) >= 32
    assert neg >= 16 and pos >= 16 and len(tied) >= 4 and "tile" in tied and "split" in tied
    kinds = {kind for *_, kind in c.planted}
    assert {"half", "tile", "split"} <= kinds and (seg_train or "step" not in kinds)   # shared: every step seam a split seam
    segs = {b: (q0, qs, ts) for b, q0, qs, ts in F.seg_tables(c)}
    for b, (q0, qs, ts) in segs.items():
        assert any(row == q0 + len(qs) - 1 for row, *_ in c.planted)           # the segment's last query
        assert any(hi == len(ts) - 1 for _, pb, _, hi, _ in c.planted if pb == b or not seg_train)   # the tail's last row
    for row, b, lo, hi, kind in c.planted:
        q0, qs, ts = segs[b]
        q64, t64 = qs[row - q0].astype(np.float64), ts.astype(np.float64)
        d64 = ((q64[None, :] - t64) ** 2).sum(-1)
        assert (d64 > 0).all()                                                    # no exact copy
        assert sorted(np.argsort(d64, kind="stable")[:2].tolist()) == [lo, hi] and d64[[lo, hi]].max() < 1e-13
        bound = 2 * GAMMA130 * ((q64 ** 2).sum() + (t64[[lo, hi]] ** 2).sum(-1))
        assert sorted(c.idx[row].tolist()) == [lo, hi]
        assert (c.dist[row].astype(np.float64) <= bound.min()).all()
        if (c.dist[row] == 0).all():
            assert c.idx[row].tolist() == [lo, hi]                                # the tie, by index
    exempt = _float64_by_segment(c)
    assert exempt <= len(c.planted)          # only the planted rows have no gap to rank by


@pytest.mark.parametrize("seg_train", [False, True], ids=["shared", "segmented"])
def test_subnormal_case_census(seg_train):
    """At least 1000 products q[e] t[e] lie in the subnormal range, at least 100 distances
    are subnormal and not zero, none is NaN; the expected result itself holds subnormal
    distances (the nearest rows of the 2^-70 queries), and subnormal elements are present."""
    c = F.subnormal_case(seg_train)
    prod, dsub, nan, in_result = F.subnormal_census(c)
    print(f"{c.name}: {prod} subnormal products, {dsub} subnormal distances, {in_result} of them in the result")
    assert prod >= 1000 and dsub >= 100 and nan == 0 and in_result >= 20
    assert F.subnormal(c.q).sum() >= 1000 and F.subnormal(c.t).sum() >= 1000
    assert np.isfinite(c.dist).all() and (c.idx >= 0).all()
    for _, _, qs, ts in F.seg_tables(c):     # the norms of the 2^-70 rows are subnormal, and not zero
        assert F.subnormal(F.chain(qs[0::3], qs[0::3])).all() and F.subnormal(F.chain(ts[0::3], ts[0::3])).all()


@pytest.mark.parametrize("seg_train", [False, True], ids=["shared", "segmented"])
def test_overflow_case_census(seg_train):
    """Finite rows give at least 8 NaN and 8 +inf distances; queries with two finite
    neighbours behind NaN / +inf rows, with exactly one ([i, -1] / [d, +inf]) and with none
    ([-1, -1]) occur (the last two in the segmented case); -2 dot alone overflows on the
    fused pair, whose d clamps to 0; the expected result holds no NaN."""
    c = F.overflow_case(seg_train)
    assert np.isfinite(c.q).all() and np.isfinite(c.t).all()
    n = F.overflow_census(c)
    print(f"{c.name}: {n}")
    assert n["nan"] >= 8 and n["inf"] >= 8 and n["two_behind"] >= 8
    if seg_train:
        assert n["one"] >= 8 and n["none"] >= 8
    assert not np.isnan(c.dist).any()
    assert ((c.idx < 0) == np.isposinf(c.dist)).all()
    one = (c.idx[:, 0] >= 0) & (c.idx[:, 1] < 0)
    assert np.isfinite(c.dist[one, 0]).all()
    # the tail step's last row and both sides of a split seam give NaN or +inf
    for b, q0, qs, ts in F.seg_tables(c):
        nt, per = c.ranges[b][1], c.ranges[b][2]
        d = F.distances(qs, ts)
        big = c.big_q[q0:q0 + len(qs)]
        assert np.isnan(d[big, nt - 1]).all() and np.isposinf(d[~big, nt - 1]).all()
        for s, kind in F.seams(nt, per).items():
            if kind == "split":
                assert not np.isfinite(d[big][:, [s - 1, s]]).any()
    fq, ft = c.fused
    y, t = c.q[fq], c.t[ft]
    dot, nq, nt = F.chain(y, t), F.chain(y, y), F.chain(t, t)
    with np.errstate(over="ignore"):
        assert np.isneginf(f32(-2) * dot) and np.isfinite(nq + nt)
    v = F.distances(y, t, clamp=False)[0, 0]
    assert np.isfinite(v) and v <= 0 and c.dist[fq, 0] == 0 and c.idx[fq, 0] == ft - c.ranges[0][0]
    # a big query is at d = nq from every ordinary row: its neighbours are the first two by index
    ordinary = np.nonzero(c.kinds[c.ranges[0][0]:c.ranges[0][0] + c.ranges[0][1]] == "o")[0][:2]
    row = int(c.qoff[1]) - 1                 # the last query of segment 0, a big one
    assert c.idx[row].tolist() == ordinary.tolist() and c.dist[row, 0] == c.dist[row, 1] == F.chain(c.q[row], c.q[row])


def _mutant(c, how):
    """The k = 2 result of a rule that differs from sift_hip.h's in one line."""
    idx = np.full((c.q_cap, 2), -1, np.int32)
    dist = np.full((c.q_cap, 2), np.inf, f32)
    for _, q0, qs, ts in F.seg_tables(c):
        v = F.distances(np.abs(qs) if how == "fabs" else qs, ts, clamp=False)
        with np.errstate(invalid="ignore"):
            d = {"no-clamp": v, "fmax": np.fmax(v, f32(0)), "fabs": np.where(v < 0, f32(0), v),
                 "nan-inserted": np.where(v < 0, f32(0), v)}[how]
        if how == "nan-inserted":            # a NaN that compares below everything, as a total order would have it
            d = np.where(np.isnan(d), f32(-1), d)
        idx[q0:q0 + len(qs)], dist[q0:q0 + len(qs)] = F.knn_from(d, 2)
    return idx, dist


@pytest.mark.parametrize("how, case", [("no-clamp", F.cancel_case), ("fmax", F.overflow_case),
                                       ("nan-inserted", F.overflow_case), ("fabs", F.signed_case)])
def test_value_cases_tell_the_rule_from_its_mutations(how, case):
    """Dropping the clamp, writing it as fmaxf (NaN becomes 0), letting a NaN distance into
    the list, or taking the magnitude of an operand: each changes the expected result of
    the case made for it, shared and segmented, and none changes the result of a case that
    existed before (whose GPU tests therefore cannot tell)."""
    for seg_train in (False, True):
        c = case(seg_train)
        idx, dist = _mutant(c, how)
        rows = int(((idx != c.idx) | (dist.view(np.int32) != c.dist.view(np.int32))).any(axis=1).sum())
        print(f"{how}: {rows} rows of {c.name} differ")
        assert rows >= 8
    for old in (F.edges_case(True), F.splits_case(), F.weights_case()):
        idx, dist = _mutant(old, how)
        assert_bits_equal(idx, old.idx, old.name + " idx under " + how)
        assert_bits_equal(dist, old.dist, old.name + " dist under " + how)
