"""CPU tests of the epipolar matcher: the exports and the Python surface, the
argument checks that need no device, the restatement by hand, the census of the
edge case the GPU tests use, the cover program of csrc/epipolar_math.hpp and the
host-only scratch layout.  No GPU."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal

import match_epipolar_inputs as E
import match_window_inputs as W

NEW = ["sift_knn_match_epipolar_segmented_device", "sift_knn_match_epipolar_segmented"]


# ---- exports and arguments ---------------------------------------------------------------
def test_exports_and_python_signatures(siftgpu):
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sift_hip.h")).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert getattr(siftgpu.lib(), name).argtypes is not None
    full = open(os.path.join(ROOT, "include", "sift_hip.h")).read()
    for phrase in ("gated reverse pass", "one-sided (train-image-only) distance", "SIFT_METRIC_L2SQR_F32"):
        assert phrase in full[full.index("matching along epipolar lines"):]
    p = inspect.signature(siftgpu.Context.knn_match_epipolar_segmented_device).parameters
    assert list(p)[1:] == ["metric", "query_ptr", "q_kpts_ptr", "q_offsets_ptr", "n_segments", "q_cap", "train_ptr",
                           "t_kpts_ptr", "t_offsets_ptr", "t_cap", "F_ptr", "found_ptr", "band", "radius", "rows",
                           "cols", "k", "idx_ptr", "dist_ptr"]
    assert callable(siftgpu.Context.knnMatchEpipolarSegmented)
    p = inspect.signature(siftgpu.epipolar_match).parameters
    assert list(p)[:9] == ["query_desc", "query_kpts", "train_desc", "train_kpts", "F", "band", "radius", "normType",
                           "k"]
    assert p["band"].default == 3.0 and p["radius"].default == float("inf")
    assert p["normType"].default == siftgpu.NORM_L1 and p["k"].default == 2
    q8, qf = np.zeros((1, 128), np.uint8), np.zeros((1, 128), np.float32)
    k = np.zeros(1, siftgpu.KEYPOINT_DTYPE)
    with pytest.raises(ValueError):
        siftgpu.epipolar_match(qf, k, q8, k, np.eye(3), normType=siftgpu.NORM_L2SQR)
    with pytest.raises(ValueError):
        siftgpu.epipolar_match(q8, k, q8, k, np.eye(3), normType=4)


def test_null_context_is_rejected(siftgpu):
    L = siftgpu.lib()
    pint = ctypes.POINTER(ctypes.c_int)
    assert L.sift_knn_match_epipolar_segmented_device(None, 0, None, None, None, 0, 0, None, None, None, 0, None, None,
                                                      3.0, 1.0, 1, 1, 2, None, None) == siftgpu.SIFT_E_INVALID
    assert L.sift_knn_match_epipolar_segmented(None, 0, None, None, pint(), 0, 0, None, None, pint(), 0, None, pint(),
                                               3.0, 1.0, 1, 1, 2, pint(), None) == siftgpu.SIFT_E_INVALID


def test_argument_checks_in_the_source():
    """Every SIFT_E_INVALID case of the header is a check of apps.hip that names its argument
    (the checks run on a live context in test_gpu_match_epipolar.py)."""
    src = open(os.path.join(ROOT, "sift-gpu_amd", "csrc", "apps.hip")).read()
    body = src[src.index("int check_epipolar("):src.index("int epipolar_device(")]
    assert "!(band >= 0)" in body and '"band must be' in body and "check_window(" in body
    assert "if (!c) return SIFT_E_INVALID;" in body


# ---- the restatement -------------------------------------------------------------------------
def test_band_rule_on_hand_values():
    X = np.array([30, 50, 25, 25, 25, np.nan], np.float32)
    Y = np.array([30, 30, 33, W.up(33), 27, 30], np.float32)
    # rectified: both errors are (Y - y)^2; closed at band, a NaN is out; the window is not its business
    assert E.band_row(E.F_HORIZONTAL, 20, 30, X, Y, 3.0).tolist() == [True, True, True, False, True, False]
    assert E.band_row(E.F_HORIZONTAL, 20, 30, X, Y, float(W.down(3.0))).tolist() == [True, True, False, False, False, False]
    assert E.band_row(E.F_HORIZONTAL, 20, 30, X, Y, 0.0).tolist() == [True, True, False, False, False, False]
    assert E.band_row(E.F_HORIZONTAL, 20, 30, X, Y, np.inf).tolist() == [True] * 5 + [False]
    # the query on the epipole: a = b = c = 0, s = inf, 0 * inf is NaN at every band
    e_dst, e_src = E.errors(E.F_OBLIQUE, *E.E1, X[:3], Y[:3])
    assert np.isnan(e_dst).all() and np.isfinite(e_src).all()
    assert not E.band_row(E.F_OBLIQUE, *E.E1, X[:3], Y[:3], np.inf).any()
    # a non-finite F admits nothing
    assert not E.band_row(np.full(9, np.nan), 20, 30, X, Y, np.inf).any()
    assert E.limit(3.0) == 9 and E.limit(1e30) == np.inf and E.limit(float(W.down(3.0))) < 9


def test_restatement_by_hand():
    q = np.zeros((2, 128), np.uint8)
    t = np.zeros((4, 128), np.uint8)
    t[0, 0], t[1, 0], t[2, 0], t[3, 0] = 9, 5, 5, 1
    qk = W.kpts_at([[10, 10], [100, 100]])
    tk = W.kpts_at([[12, 12], [20, 9], [11, 26], [60, 11]])
    F = E.F_HORIZONTAL.reshape(1, 9)
    idx, dist, adm = E.epipolar_ref(W.L1_U8, q, qk, [0, 2], t, tk, None, F, None, 3.0, np.inf)
    assert idx.tolist() == [[3, 1], [-1, -1]] and dist[0].tolist() == [1, 5] and adm[0].tolist() == [0, 1, 3]
    idx, _, adm = E.epipolar_ref(W.L1_U8, q, qk, [0, 2], t, tk, None, F, None, 3.0, 16.0)
    assert idx.tolist() == [[1, 0], [-1, -1]] and adm[0].tolist() == [0, 1]
    # no model: the window alone, F NULL or found == 0
    for kw in (dict(F=None), dict(F=F, found=np.array([0]))):
        idx, _, adm = E.epipolar_ref(W.L2SQR_U8, q, qk, [0, 2], t, tk, None, band=3.0, radius=16.0, **kw)
        assert idx.tolist() == [[1, 2], [-1, -1]] and adm[0].tolist() == [0, 1, 2]


@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_restatement_without_a_model_is_the_window_reference(metric):
    c = W.edges_case(metric, True)
    for radius in (4.0, 16.0, np.inf):
        wi, wd, _ = W.window_ref(metric, c.q, c.qk, c.qoff, c.t, c.tk, c.toff, radius)
        ei, ed, _ = E.epipolar_ref(metric, c.q, c.qk, c.qoff, c.t, c.tk, c.toff, None, None, 3.0, radius)
        assert_bits_equal(ei, wi, "idx")
        assert_bits_equal(ed, wd, "dist")


# ---- the census --------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_train", [True, False], ids=["segmented", "shared"])
@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_edges_case_census(metric, seg_train):
    c = E.edges_case(metric, seg_train)
    assert (c.rows, c.cols) == (64, 96) and len(c.qoff) == 5 and np.diff(c.seg_qoff).max() == 40
    kinds = E.census(c, E.edges_case(metric, seg_train, float(W.down(E.BAND))))
    for kind, n in kinds.items():
        assert n >= 1, (kind, kinds)
    F, found = E.edge_models()
    assert found.tolist() == [1, 1, 5, 0] and np.isnan(F[3]).all()
    # the planted rows do what their comments say
    q0, q2, t0, t2 = (int(c.seg_qoff[0]), int(c.seg_qoff[2]), int(c.seg_toff[0]) if not seg_train else 0,
                      int(c.seg_toff[2]) if not seg_train else 0)
    adm = c.adm[q0]
    assert t0 + 0 in adm and t0 + 2 in adm and t0 + 1 not in adm
    assert t0 + 2 not in E.edges_case(metric, seg_train, float(W.down(E.BAND))).adm[q0]
    assert t0 + 3 in c.adm[q0 + 1] and c.tk["x"][int(c.seg_toff[0]) + 3] < 0
    cluster = t0 + 5 + np.arange(E.CLUSTER_N)
    assert np.isin(cluster, c.adm[q0 + 2]).all() and E.CLUSTER_N > W.WIN_GROUP
    if seg_train:
        assert c.adm[q0 + 3].tolist() == [4] and c.idx[q0 + 3].tolist() == [4, -1] and c.dist[q0 + 3, 1] == np.inf
        assert len(c.adm[q0 + 4]) == 0
    assert len(c.adm[q2]) == 0                                   # the query on the epipole
    assert t2 + 0 not in c.adm[q2 + 1] and t2 + 1 not in c.adm[q2 + 2]
    # the segment without a model is gated by the window alone
    q3 = int(c.seg_qoff[3])
    wi, _, _ = W.window_ref(metric, c.q, c.qk, c.qoff, c.t, c.tk, c.toff, c.radius)
    assert_bits_equal(c.idx[q3:], wi[q3:], "found == 0")
    assert (c.idx[:q3] != wi[:q3]).any()


@pytest.mark.parametrize("metric", range(3), ids=W.METRIC_IDS)
def test_other_cases_census(metric):
    for seg in (True, False):
        c = E.clamp_case(metric, seg)
        live = c.live()
        assert c.qoff[0] == 3 and c.qoff[-1] > c.q_cap and len(live) == c.q_cap - 3
        assert (c.idx[live, 0] >= 0).sum() > len(live) // 2 and (c.dist[live, 0] > 0).all()
    c = E.nonmonotone_case(metric)
    assert (np.diff(c.qoff) < 0).any() and (c.idx[:, 0] >= 0).sum() > 25
    c = E.many_segments_case(metric)
    assert len(c.qoff) == 201 and (np.diff(c.qoff) == 0).any() and (np.diff(c.toff) == 0).any()
    assert (c.idx[:, 0] >= 0).any() and (c.idx[:, 0] < 0).any() and (c.found == 0).any()


# ---- the cover program and the layout ------------------------------------------------------------
def test_epipolar_cover_program(tmp_path):
    """tests/cpp/epipolar_cover.cpp over csrc/epipolar_math.hpp (host code only): every point
    that passes the exact float test lies in a cell of the range returned for its grid row.
    Built with the address and undefined-behaviour sanitizers where the compiler has their
    runtimes; a program of its own, nothing is preloaded."""
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = tmp_path / "epipolar_cover"
    base = [hipcc, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "--offload-host-only", "-x", "hip",
            os.path.join(ROOT, "tests", "cpp", "epipolar_cover.cpp"), "-o", str(exe)]
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "epipolar cover ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_match_epipolar_layouts(tmp_path):
    """tests/cpp/match_epipolar_layout.cpp: epipolar_grid and epipolar_host_layout of
    csrc/scratch.hpp, built as test_match_window.py builds match_window_layout.cpp."""
    src = os.path.join(ROOT, "tests", "cpp", "match_epipolar_layout.cpp")
    exe = tmp_path / "match_epipolar_layout"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "match epipolar layouts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    # the restated grid of match_epipolar_inputs.py is scratch.hpp's
    text = open(os.path.join(ROOT, "sift-gpu_amd", "csrc", "scratch.hpp")).read()
    assert "#define SIFT_EPIPOLAR_CELL_SCALE 1\n" in text and "cell *= 1.125" in text
