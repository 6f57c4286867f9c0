"""Cross-check (mutual nearest neighbour) matching for a whole batch: what can be
checked without a GPU.

The three entry points are declared, exported and wrapped, the module constants
exist and BFMatcher(crossCheck=True) still raises; the argument checks reject a
null context whatever else is wrong with the call (test_gpu_cross_check.py
repeats them on a real context, where each one is the only fault); the layout
program passes; and the numpy reference of cross_check_inputs.py, which every
GPU comparison rests on, gives the literally listed kept set on a hand-written
6 x 5 distance matrix."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import cross_check_inputs as X

NEW = ["sift_cross_check_matches_device", "sift_cross_check_matches", "sift_cross_match_segmented_device"]


def test_cross_entry_points_declared_exported_and_wrapped(siftgpu):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sift_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert getattr(siftgpu.lib(), name).argtypes is not None, name
    for meth in ["cross_check_matches_device", "cross_match_segmented_device", "crossCheckMatches"]:
        assert callable(getattr(siftgpu.Context, meth)), meth
    assert callable(siftgpu.cross_check_match)
    for n, name in enumerate(["SIFT_METRIC_L1_F32", "SIFT_METRIC_L1_U8", "SIFT_METRIC_L2SQR_U8"]):
        assert re.search(r"#define\s+" + name + r"\s+" + str(n) + r"\b", text), name
        assert getattr(siftgpu, name) == n == [X.L1_F32, X.L1_U8, X.L2SQR_U8][n]
    assert X.MATCH_DTYPE == siftgpu.MATCH_DTYPE and X.KEYPOINT_DTYPE == siftgpu.KEYPOINT_DTYPE


def test_cross_entry_points_reject_bad_arguments_on_a_null_context(siftgpu):
    L = siftgpu.lib()
    f = np.zeros(128, np.float32)
    ix = np.zeros(4, np.int32)
    off = np.array([0, 1], np.int32)
    pf = f.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    pi = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))  # noqa: E731
    E = siftgpu.SIFT_E_INVALID
    d, o, i = f.ctypes.data, off.ctypes.data, ix.ctypes.data

    def stage(fk=1, rk=1, ratio=0.0, toff=o):
        return L.sift_cross_check_matches_device(None, i, d, fk, o, 1, 1, i, rk, toff, 1, ratio, None, None, d, None,
                                                 None, 1, o)

    def host(fk=1, rk=1, ratio=0.0, toff=pi(off)):
        return L.sift_cross_check_matches(None, pi(ix), pf, fk, pi(off), 1, 1, pi(ix), rk, toff, 1, ratio, None, None,
                                          d, None, None, 1, pi(off))

    def one(metric=0, ratio=0.0, toff=o):
        return L.sift_cross_match_segmented_device(None, metric, d, o, 1, 1, d, toff, 1, ratio, None, None, d, None,
                                                   None, 1, o)

    assert stage() == E and host() == E and one() == E                       # the null context alone
    assert stage(fk=1, ratio=0.86) == E and host(fk=1, ratio=0.86) == E      # a ratio test on a k = 1 result
    for k in (0, 3):
        assert stage(fk=k) == E and stage(rk=k) == E and host(fk=k) == E and host(rk=k) == E
    assert stage(toff=None) == E and host(toff=None) == E and one(toff=None) == E   # a shared train set
    for metric in (-1, 3):
        assert one(metric=metric) == E
    # and with nothing to do: the null context is still rejected first
    assert L.sift_cross_check_matches_device(None, None, None, 1, None, 0, 0, None, 1, None, 0, 0.0, None, None, None,
                                             None, None, 0, None) == E
    assert L.sift_cross_match_segmented_device(None, 0, None, None, 0, 0, None, None, 0, 0.0, None, None, None, None,
                                               None, 0, None) == E


def test_cross_module_constants_and_bfmatcher_still_raises(siftgpu):
    assert (siftgpu.SIFT_METRIC_L1_F32, siftgpu.SIFT_METRIC_L1_U8, siftgpu.SIFT_METRIC_L2SQR_U8) == (0, 1, 2)
    for norm in (siftgpu.NORM_L1, siftgpu.NORM_L2SQR):
        with pytest.raises(ValueError):
            siftgpu.BFMatcher(norm, crossCheck=True)
    assert "cross_check_match" in siftgpu.BFMatcher.__doc__
    f = np.zeros((2, 128), np.float32)
    u = np.zeros((2, 128), np.uint8)
    for q, t in ((f, f), (u, f), (f, u)):     # raised before any context is made
        with pytest.raises(ValueError):
            siftgpu.cross_check_match(q, t, siftgpu.NORM_L2SQR)
    with pytest.raises(ValueError):
        siftgpu.cross_check_match(u, u, 4)    # plain NORM_L2 stays out


def test_cross_check_layouts(tmp_path):
    """tests/cpp/cross_check_layout.cpp, built like test_match_l2_u8.py::test_match_l2_u8_layouts:
    with the address and undefined-behaviour sanitizers (runtimes linked
    statically into the program) where the host compiler has them."""
    src = os.path.join(ROOT, "tests", "cpp", "cross_check_layout.cpp")
    exe = tmp_path / "cross_check_layout"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "cross check layouts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_reference_on_the_hand_written_case():
    """6 queries x 5 train rows, one segment: the tables and the kept set, listed literally."""
    idx, dist = X.knn_from_distances(X.HAND_D, 2)
    ridx, _ = X.knn_from_distances(X.HAND_D.T, 1)
    assert idx.tolist() == X.HAND_IDX and ridx[:, 0].tolist() == X.HAND_RIDX
    qoff, toff = [0, 6], [0, 5]
    for k in (1, 2):
        rec, moff, src, dst, _ = X.stage_ref(idx[:, :k], dist[:, :k], ridx, qoff, toff, 6, 5, 0.0)
        assert list(zip(rec["query"].tolist(), rec["train"].tolist())) == X.HAND_KEPT == [(0, 0), (2, 1), (4, 3)]
        assert rec["distance"].tolist() == [1.0, 3.0, 1.0] and rec["segment"].tolist() == [0, 0, 0]
        assert moff.tolist() == [0, 3] and src is None and dst is None
    rec, moff, _, _, (seg, rev_ok, ratio_ok) = X.stage_ref(idx, dist, ridx, qoff, toff, 6, 5, X.RATIO)
    assert list(zip(rec["query"].tolist(), rec["train"].tolist())) == X.HAND_KEPT_RATIO == [(0, 0), (4, 3)]
    assert rev_ok.tolist() == [True, False, True, False, True, False]
    assert ratio_ok.tolist() == [True, True, False, True, True, True] and moff.tolist() == [0, 2]


@pytest.mark.parametrize("variant", ["overflow", "slack"])
def test_crafted_tables_hold_every_case(variant):
    """On the reference alone: what the GPU test on the crafted tables relies on."""
    c = X.crafted(variant)
    qo, to = X.clamped(c.qoff, c.q_cap), X.clamped(c.toff, c.t_cap)
    assert c.qoff[0] > 0 and len(c.qoff) - 1 == len(X.GROUP1) + 257 and np.diff(c.qoff)[2] == 0
    assert np.diff(c.qoff)[:5].tolist() == [255, 256, 0, 257, 513] and set(np.diff(c.qoff)[5:]) == {0, 1, 2, 3}
    for ratio in X.RATIOS:
        rec, moff, _, _, (seg, rev_ok, ratio_ok) = X.crafted_ref(variant, ratio)
        kept = rev_ok & ratio_ok
        for b in range(len(X.GROUP1)):          # every non-empty segment of the first group keeps and drops
            s = slice(int(qo[b]), int(qo[b + 1]))
            assert qo[b + 1] == qo[b] or (kept[s].any() and not kept[s].all()), (ratio, b)
        assert (~rev_ok & ratio_ok & (seg >= 0)).any()             # dropped by the reverse test alone
        if ratio > 0:
            assert (rev_ok & ~ratio_ok).any()                      # dropped by the ratio test alone
        assert moff[-1] == len(rec) == np.count_nonzero(kept) and (np.diff(moff) >= 0).all()
    seg, rev_ok, _ = X.crafted_ref(variant, 0.0)[4]
    live = seg >= 0
    j = c.idx[:c.q_cap, 0].astype(np.int64)
    tn = (to[1:] - to[:-1])[np.maximum(seg, 0)]
    glob = np.array([live[i] and 0 <= j[i] < tn[i] and c.ridx[to[seg[i]] + j[i], 0] == i for i in range(c.q_cap)])
    assert glob.any() and not (glob & rev_ok)[qo[1]:].any()        # the global row number is never a match past segment 0
    assert (live & (j == -1)).any() and (live & (j == tn - 1) & rev_ok).any() and (live & (j == tn) & (tn > 0)).any()
    # the boundary pairs: (0, 0) passes every ratio; per ratio a non-zero pair with d0 == ratio * d1
    # exactly in double (kept) beside the pair one float32 ulp above it (rejected), and the two
    # float32 either side of the ratio at d1 = 1
    r0 = c.zero_row
    assert c.dist[r0].tolist() == [0.0, 0.0] and X.RATIOS[1] * 50.0 == 43.0 and X.RATIOS[2] * 22500.0 == 16641.0
    for ratio in X.RATIOS[1:]:
        exact, over, above, below = c.boundary_rows[ratio]
        rec, _, _, _, (seg, rev_ok, ok) = X.crafted_ref(variant, ratio)
        d0, d1 = float(c.dist[exact, 0]), float(c.dist[exact, 1])
        assert d0 == ratio * d1 and d0 != 0 and (d0, d1) == X.EXACT[ratio]       # exactly at the boundary, in double
        assert ok[exact] and rev_ok[exact] and not ok[over] and rev_ok[over]     # kept; one ulp above is dropped
        assert c.dist[over, 0] == np.nextafter(c.dist[exact, 0], np.float32(np.inf)) and c.dist[over, 1] == d1
        assert float(c.dist[over, 0]) > ratio * d1
        kept_rows = rec["query"] + X.clamped(c.qoff, c.q_cap)[rec["segment"]]
        assert exact in kept_rows and below in kept_rows and over not in kept_rows and above not in kept_rows
        assert ok[r0] and not ok[above] and ok[below]
        assert float(c.dist[above, 0]) > ratio > float(c.dist[below, 0]) and c.dist[above, 1] == c.dist[below, 1] == 1
        assert np.nextafter(c.dist[above, 0], np.float32(0)) == c.dist[below, 0]
    # rows of no segment hold garbage the stage must never use as an index
    dead = np.r_[0:int(qo[0]), int(qo[-1]):len(c.idx)]
    assert len(dead) >= X.EXTRA + 3 and np.isin(c.idx[dead], X.GARBAGE).all() and (c.idx[dead] == 0x7fffffff).any()
    # a j one past the range still names a row of the ridx buffer
    assert len(c.ridx) >= c.t_cap + X.EXTRA and (to[np.maximum(seg, 0)] + np.maximum(j, 0))[live].max() < len(c.ridx)
    assert ((to[np.maximum(seg, 0)] + j)[live] >= c.t_cap).any() == (variant == "overflow")


def test_reference_segments_offsets_and_clamps():
    """Two segments behind a first offset, the second clipped by both capacities: local
    indices, the segment's own train range, m_offsets, and rows of no segment ignored."""
    qoff, toff = [1, 3, 6], [2, 4, 9]
    idx = np.array([[0x7fffffff], [1], [0], [0], [2], [-5]], np.int32)[:5]      # q_cap = 5: row 5 is clipped
    ridx = np.array([-9, -9, 1, 0, 0, 2, 1, 1], np.int32)[:6]                   # t_cap = 6
    dist = np.arange(5, dtype=np.float32).reshape(5, 1)
    # seg 0: q rows 1, 2 (local 0, 1), train rows 2, 3: row 1 -> t 1 (global 3) -> q 0: kept; row 2 -> t 0 -> q 1: kept
    # seg 1: q rows 3, 4 (local 0, 1), train rows 4, 5 (t_cap clips 6..8): row 3 -> t 0 -> q 0: kept; row 4 -> t 2: past the range
    rec, moff, _, _, _ = X.stage_ref(idx, dist, ridx, qoff, toff, 5, 6, 0.0)
    assert rec.tolist() == [(0, 1, 1.0, 0), (1, 0, 2.0, 0), (0, 0, 3.0, 1)] and moff.tolist() == [0, 2, 3]
