"""CPU tests of the windowed (spatially gated) matcher: the reference against
itself and against the dense references, the census of every case the GPU tests
use, the host-only scratch layout and search grid, the ABI and the Python
surface.  No GPU."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal

import match_window_inputs as W

NEW = ["sift_knn_match_window_segmented_device", "sift_knn_match_window_segmented"]


# ---- the reference ---------------------------------------------------------------------
def test_admissibility_rule_on_hand_values():
    r = W.RADIUS
    tx = np.array([66, W.up(66), 34, W.down(34), 50, np.nan, np.inf, W.down(16.0)], np.float32)
    ty = np.full(8, 30, np.float32)
    got = W.admissible_row(50, 30, tx, ty, r)
    assert got.tolist() == [True, False, True, False, True, False, False, False]
    # closed in y as well, and both must hold
    assert W.admissible_row(50, 30, ty + 20, np.array([46, W.up(46)] * 4, np.float32), r).tolist() == [True, False] * 4
    # 15.999999 - 32 rounds to -16 in float32: inside, although the point is below px - radius
    assert W.admissible_row(32, 30, tx[7:], ty[7:], r).tolist() == [True]
    # radius 0: coincident points only; +inf: every comparable coordinate, and inf - inf is not one
    assert W.admissible_row(50, 30, np.array([50, W.up(50)], np.float32), ty[:2], 0).tolist() == [True, False]
    assert W.admissible_row(50, 30, tx, ty, np.inf).tolist() == [True] * 5 + [False, True, True]
    assert W.admissible_row(np.inf, 30, tx, ty, np.inf).tolist() == [True] * 5 + [False, False, True]


@pytest.mark.parametrize("seg_train", [True, False], ids=["segmented", "shared"])
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_reference_at_infinite_radius_is_the_dense_reference(metric, seg_train):
    c = W.edges_case(metric, seg_train, True, float("inf"))
    assert np.isfinite(c.qk["x"]).all() and np.isfinite(c.tk["y"]).all() and c.tk["x"].min() < 0
    idx, dist = W.dense_seg_ref(metric, c.q, c.qoff, c.t, c.toff, 2)
    assert_bits_equal(c.idx, idx, "idx")
    assert_bits_equal(c.dist, dist, "dist")
    assert (c.idx[:, 0] >= 0).sum() > 300 and (c.idx[:, 1] < 0).any() == seg_train   # the one-row segment's fill


def test_reference_by_hand():
    """Three train points, two with the same descriptor: the gate picks by position first,
    then (distance, index)."""
    q = np.zeros((2, 128), np.uint8)
    t = np.zeros((4, 128), np.uint8)
    t[0, 0], t[1, 0], t[2, 0], t[3, 0] = 9, 5, 5, 1
    qk = W.kpts_at([[10, 10], [100, 100]])
    tk = W.kpts_at([[12, 12], [20, 20], [11, 26], [60, 60]])
    idx, dist, n = W.window_ref(W.L1_U8, q, qk, [0, 2], t, tk, None, 16.0)
    assert idx.tolist() == [[1, 2], [-1, -1]] and dist[0].tolist() == [5, 5] and n.tolist() == [3, 0]
    idx, dist, n = W.window_ref(W.L2SQR_U8, q, qk, [0, 2], t, tk, None, 10.0, k=1)
    assert idx.tolist() == [[1], [-1]] and dist[0].tolist() == [25] and n.tolist() == [2, 0]
    # a translation by (50, 50) brings query 0 to train 3 and query 1 out of reach
    H = np.array([[1, 0, 50, 0, 1, 50, 0, 0, 1]], np.float64)
    idx, _, n = W.window_ref(W.L1_U8, q, qk, [0, 2], t, tk, None, 16.0, H=H)
    assert idx.tolist() == [[3, -1], [-1, -1]] and n.tolist() == [1, 0]
    idx, _, _ = W.window_ref(W.L1_U8, q, qk, [0, 2], t, tk, None, 16.0, H=H, found=np.array([0]))
    assert idx.tolist() == [[1, 2], [-1, -1]]


# ---- the census of every case ------------------------------------------------------------
@pytest.mark.parametrize("seg_train", [True, False], ids=["segmented", "shared"])
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_edges_case_census(metric, seg_train):
    c = W.edges_case(metric, seg_train)
    s = W.census(c)
    assert s["zero"] >= 1 and s["one"] >= 1 and s["two"] >= 1, s
    assert 2 * s["two_or_more"] >= s["live"], s
    assert s["differs"] >= 1, s                      # the gate provably changes the answer
    q_sizes, t_sizes = c.seg_sizes
    assert q_sizes[0] == 0 and t_sizes[1] == 0 and t_sizes[2] == 1 and t_sizes[3] == W.ONE_CELL_N
    assert W.ONE_CELL_N > W.WIN_BLOCK > W.WIN_GROUP and W.ONE_CELL_N % W.WIN_GROUP
    # the one-cell segment: every train point in the cell [32, 48) x [16, 32) of side radius
    tl = int(np.cumsum([0] + t_sizes)[3])
    x, y = c.tk["x"][tl:tl + W.ONE_CELL_N], c.tk["y"][tl:tl + W.ONE_CELL_N]
    assert (np.floor(x / 16) == 2).all() and (np.floor(y / 16) == 1).all()
    # NaN rows on both sides, coordinates outside rows x cols on every side, infinities
    assert np.isnan(c.qk["x"]).any() and np.isnan(c.tk["y"]).any() and np.isinf(c.tk["x"]).any()
    assert c.tk["x"][np.isfinite(c.tk["x"])].max() > W.COLS + 100 and c.tk["y"][np.isfinite(c.tk["y"])].min() < -20
    if seg_train:
        qo = np.cumsum([0] + q_sizes)
        # exactly one train row, k = 2: the second slot is the fill
        assert c.idx[qo[2]].tolist() == [0, -1] and c.dist[qo[2], 1] == np.inf and c.n_adm[qo[2] + 3] == 0
        # the boundary segment, query (50, 40): rows 0-2 and 6-8 at exactly radius are in, the
        # rows one ulp beyond (3-5, 9-11) are out; query (32, 40) admits row 19 at x = 15.999999
        adm = W.admissible_row(50, 40,c.tk["x"][tl + W.ONE_CELL_N:][:22], c.tk["y"][tl + W.ONE_CELL_N:][:22],
                               W.RADIUS)
        assert adm[:12].tolist() == [True] * 3 + [False] * 3 + [True] * 3 + [False] * 3
        assert W.admissible_row(32, 40, c.tk["x"][tl + W.ONE_CELL_N + 19:][:1],
                                c.tk["y"][tl + W.ONE_CELL_N + 19:][:1], W.RADIUS).tolist() == [True]
        # identical descriptors at distinct admissible positions: the lower index first, distance 0
        r5, r6, lo, hi = c.tie_rows
        assert c.idx[r5].tolist() == [40, 41] and c.dist[r5].tolist() == [0, 0]
        assert c.idx[r6].tolist() == [lo, hi] and c.dist[r6].tolist() == [0, 0] and lo < hi


@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_other_cases_census(metric):
    for seg in (True, False):
        c = W.clamp_case(metric, seg)
        assert c.qoff[0] == 3 and c.qoff[-1] > c.q_cap and (c.toff is None or c.toff[-1] > c.t_cap)
        live = c.live()
        assert len(live) == c.q_cap - 3 and (c.n_adm[live] >= 2).sum() > len(live) // 2
        assert (c.idx[:3] == -1).all() and (c.n_adm[:3] == -1).all()
        assert (c.dist[live, 0] > 0).all()            # nothing at distance 0: no row past t_cap was read
    c = W.many_segments_case(metric)
    assert len(c.qoff) == 41 and (np.diff(c.qoff) == 0).any() and (np.diff(c.toff) == 0).any()
    assert (c.n_adm[c.live()] == 0).any() and (c.n_adm[c.live()] >= 2).any()
    c = W.coincident_case(metric)
    n = c.n_adm
    assert (n == 0).any() and (n == 1).any() and (n >= 2).any()
    for i in np.flatnonzero(n):                        # only exactly coincident points match
        j = c.idx[i, 0]
        assert c.tk["x"][j] == c.qk["x"][i] and c.tk["y"][j] == c.qk["y"][i] and j < 60 and c.pick[j] == i
    a, b = W.prior_case(metric, True), W.prior_case(metric, False)
    pa, pb = (W.predicted(x.qk, x.qoff, x.q_cap, x.H, x.found) for x in (a, b))
    assert (pa[80:90] == 0).all() and np.abs(pa[90]).max() > 1e5          # |w| <= FLT_EPSILON, and just above
    assert_bits_equal(pa[160:240], np.stack([a.qk["x"], a.qk["y"]], 1)[160:240], "found == 0: the identity")
    assert (pb[160:240] == 0).all()                                       # the NaN H as given
    assert_bits_equal(pa[240:], np.stack([a.qk["x"], a.qk["y"]], 1)[240:], "H = 2 I")
    for seg in range(4):
        assert (a.n_adm[80 * seg:80 * seg + 80] >= 1).sum() > 8, seg
    assert (a.n_adm[80:90] >= 2).all() and (a.idx[160:240] != b.idx[160:240]).any()
    c = W.frames_case(metric)
    assert (c.idx[:45, 0] == np.arange(45)).all() and (c.dist[:45, 0] == 0).all()
    assert (c.idx[90:] == -1).all()                    # frame 1 searches the empty frame 2, frame 2 is empty


# ---- the scratch layout and the search grid ------------------------------------------------
def test_match_window_layouts(tmp_path):
    """tests/cpp/match_window_layout.cpp: the windowed matcher's scratch layouts
    (csrc/scratch.hpp, plain host C++) at their smallest and degenerate counts --
    t_cap 0 and 1, one cell, the cell cap -- and the search grid's bounds.  Built
    with the address and undefined-behaviour sanitizers (their runtimes linked
    statically into the program) where the host compiler has them, without
    otherwise."""
    src = os.path.join(ROOT, "tests", "cpp", "match_window_layout.cpp")
    exe = tmp_path / "match_window_layout"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "match window layouts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- the ABI and the Python surface ----------------------------------------------------------
def test_abi_and_argument_checks_without_a_context(siftgpu):
    L = siftgpu.lib()
    for name in NEW:
        assert hasattr(L, name), name
    text = open(os.path.join(ROOT, "include", "sift_hip.h")).read()
    for name in NEW:
        assert name + "(" in text
    assert "gated reverse pass" in text                 # the out-of-scope note
    # a NULL context is SIFT_E_INVALID before anything else, in both forms
    pint = ctypes.POINTER(ctypes.c_int)
    assert L.sift_knn_match_window_segmented_device(None, 0, None, None, None, 0, 0, None, None, None, 0, None, None,
                                                    1.0, 1, 1, 2, None, None) == siftgpu.SIFT_E_INVALID
    assert L.sift_knn_match_window_segmented(None, 0, None, None, pint(), 0, 0, None, None, pint(), 0, None, pint(),
                                             1.0, 1, 1, 2, pint(), None) == siftgpu.SIFT_E_INVALID


def test_python_surface(siftgpu):
    for meth in ["knn_match_window_segmented_device", "knnMatchWindowSegmented"]:
        assert callable(getattr(siftgpu.Context, meth))
    p = inspect.signature(siftgpu.window_match).parameters
    assert list(p)[:9] == ["query_desc", "query_kpts", "train_desc", "train_kpts", "radius", "H", "normType", "k",
                           "image_size"]
    assert p["H"].default is None and p["normType"].default == siftgpu.NORM_L1 and p["k"].default == 2
    assert p["image_size"].default is None
    assert "window_match" in siftgpu.BFMatcher.__doc__
    q8, qf = np.zeros((1, 128), np.uint8), np.zeros((1, 128), np.float32)
    k = np.zeros(1, siftgpu.KEYPOINT_DTYPE)
    with pytest.raises(ValueError):
        siftgpu.window_match(qf, k, q8, k, 1.0, normType=siftgpu.NORM_L2SQR)
    with pytest.raises(ValueError):
        siftgpu.window_match(q8, k, q8, k, 1.0, normType=4)
