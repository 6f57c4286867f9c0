"""The affine / similarity estimate without a GPU: the entry points are
declared, exported, wrapped and reject a null context; the scratch layout
program compiles and passes; the host sift_estimate_affine equals
affine_oracle.py bit for bit on affine_inputs.cpu_cases; what it estimates is
the least-squares transform of the planted inliers; and the committed inputs of
the GPU test (affine_inputs.gpu_call) are what that test needs -- the census and
the libm margin below hold on the oracle alone.

The calls that need a context (null buffers with a live context, n_segments ==
0 returning SIFT_OK) are in test_gpu_affine.py."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import affine_inputs as I
import affine_oracle as AO
import homography as HO

NEW = ["sift_estimate_affine", "sift_estimate_affine_segmented_device", "sift_estimate_affine_segmented"]
ESTIMATORS = {AO.AFFINE: "estimateAffine2D", AO.SIMILARITY: "estimateAffinePartial2D"}


def test_entry_points_declared_exported_and_wrapped(siftgpu):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sift_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert getattr(siftgpu.lib(), name).argtypes is not None, name
    for meth in ["estimate_affine_segmented_device", "estimateAffineBatch"]:
        assert callable(getattr(siftgpu.Context, meth)), meth
    assert callable(siftgpu.estimateAffine2D) and callable(siftgpu.estimateAffinePartial2D)
    assert (siftgpu.SIFT_MODEL_AFFINE, siftgpu.SIFT_MODEL_SIMILARITY) == (AO.AFFINE, AO.SIMILARITY) == (0, 1)
    assert re.search(r"#define\s+SIFT_MODEL_AFFINE\s+0\b", text) and re.search(r"#define\s+SIFT_MODEL_SIMILARITY\s+1\b", text)
    src = open(os.path.join(ROOT, "sift-gpu_amd", "csrc", "scratch.hpp")).read()
    assert re.search(r"kAffineRound\s*=\s*%d\s*;" % siftgpu.AFFINE_ROUND, src)
    assert I.ROUND == siftgpu.AFFINE_ROUND


def test_entry_points_reject_null_context(siftgpu):
    L = siftgpu.lib()
    xy = np.zeros(16, np.float32)
    off = np.array([0, 4], np.int32)
    H = np.zeros(9, np.float64)
    found = np.zeros(1, np.int32)
    pf = xy.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    pi = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))  # noqa: E731
    E = siftgpu.SIFT_E_INVALID
    for model in I.MODELS:
        assert L.sift_estimate_affine_segmented_device(None, xy.ctypes.data, xy.ctypes.data, off.ctypes.data, 1, 4,
                                                       model, 3.0, 2000, 0.99, H.ctypes.data, found.ctypes.data,
                                                       None) == E
        assert L.sift_estimate_affine_segmented(None, pf, pf, pi(off), 1, 4, model, 3.0, 2000, 0.99,
                                                H.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), pi(found),
                                                None) == E
        # and with nothing to do: the null context is still rejected first
        assert L.sift_estimate_affine_segmented_device(None, None, None, None, 0, 0, model, 3.0, 2000, 0.99, None,
                                                       None, None) == E
        assert L.sift_estimate_affine_segmented(None, None, None, None, 0, 0, model, 3.0, 2000, 0.99, None, None,
                                                None) == E


def test_affine_layouts(tmp_path):
    """tests/cpp/affine_layout.cpp, built like test_homography_batch.py::test_homography_layouts:
    with the address and undefined-behaviour sanitizers (runtimes linked
    statically into the program) where the host compiler has them."""
    src = os.path.join(ROOT, "tests", "cpp", "affine_layout.cpp")
    exe = tmp_path / "affine_layout"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "affine layouts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("model", I.MODELS, ids=[I.NAMES[m] for m in I.MODELS])
def test_host_matches_oracle_bitexact(siftgpu, model):
    """A (six doubles), found and every mask byte, on every case of affine_inputs.cpu_cases."""
    fn = getattr(siftgpu, ESTIMATORS[model])
    labels = []
    for label, s, d, thr, max_iters, conf in I.cpu_cases(model):
        A, m = AO.estimate_affine(s, d, model, thr, max_iters, conf)
        hA, hm = fn(s, d, thr, max_iters, conf)
        print(f"{I.NAMES[model]:10s} {label:16s} n={len(s):3d} found={A is not None} inliers={int(m.sum())}")
        assert (A is None) == (hA is None), label
        if A is not None:
            assert np.array(A, np.float64).tobytes() == hA.tobytes(), f"{label}: {hA.reshape(6)} != {A}"
            assert np.isfinite(hA).all(), label
        assert m.tobytes() == hm.tobytes(), f"{label}: mask"
        labels.append((label, A is not None, int(m.sum())))
    got = {lab: (f, k) for lab, f, k in labels}
    mp = AO.model_points(model)
    # what the cases are there for
    assert [got[f"n{n}"][0] for n in (0, 1, mp - 1, mp, mp + 1)] == [False, False, False, True, True]
    assert got[f"n{mp}"][1] == mp and not got["degenerate"][0] and not got["identical"][0]
    assert got["thr-3"][0] and 2 * got["thr-3"][1] > 80
    assert got["thr1e30"] == (True, 80) and got["thr0"][0] and got["thr0"][1] < got["thr-3"][1]
    assert not got["max_iters0"][0] and not got["confidence0"][0] and not got["confidence1"][0]
    assert got["nan_row"][0] and got["inf_row"][0] and got["inf_row_thr1e30"][0]
    # an unknown model: none, A and the mask zeroed
    s, d = next(c[1:3] for c in I.cpu_cases(model) if c[0] == "outliers40")
    A6 = np.full(6, 5.0)
    mk = np.full(len(s), 7, np.uint8)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = siftgpu.lib().sift_estimate_affine(s.ctypes.data_as(fp), d.ctypes.data_as(fp), len(s), 2, 3.0, 2000, 0.99,
                                            A6.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), mk.ctypes.data)
    assert rc == siftgpu.SIFT_E_INVALID and (A6 == 0).all() and (mk == 0).all()


def _lstsq(model, s, d):
    """numpy.linalg.lstsq of the model on float64 copies of the pairs -> six coefficients."""
    s, d = s.astype(np.float64), d.astype(np.float64)
    n = len(s)
    if model == AO.AFFINE:
        M = np.c_[s, np.ones(n)]
        return np.r_[np.linalg.lstsq(M, d[:, 0], rcond=None)[0], np.linalg.lstsq(M, d[:, 1], rcond=None)[0]]
    M = np.r_[np.c_[s[:, 0], -s[:, 1], np.ones(n), np.zeros(n)], np.c_[s[:, 1], s[:, 0], np.zeros(n), np.ones(n)]]
    a, b, tx, ty = np.linalg.lstsq(M, np.r_[d[:, 0], d[:, 1]], rcond=None)[0]
    return np.array([a, -b, tx, b, a, ty])


# The largest |affine_oracle - lstsq| over the three inputs below, measured on
# the CPU: 2.6e-13 (affine), 2.2e-12 (similarity; its lstsq system has twice the
# rows).  A factor of 4 is allowed for a different summation order in LAPACK.
LSTSQ_BOUND = {AO.AFFINE: 4 * 2.6e-13, AO.SIMILARITY: 4 * 2.2e-12}


@pytest.mark.parametrize("model", I.MODELS, ids=[I.NAMES[m] for m in I.MODELS])
def test_semantics_on_planted_inliers(siftgpu, model):
    """Dyadic coefficients, integer sources below 1024, exact inliers, 40 % gross
    outliers: the mask is the planted inlier set, A is the least-squares
    transform of those inliers, and a similarity has the similarity's shape
    exactly."""
    fn = getattr(siftgpu, ESTIMATORS[model])
    for seed in (60, 61, 62):
        s, d, good = I.data(model, seed, 200, 0.4, 0.0, integer=True)
        A, m = fn(s, d)
        assert A is not None
        assert (m.astype(bool) == good).all(), "the mask is not the planted inlier set"
        ref = _lstsq(model, s[good], d[good])
        diff = float(np.abs(A.reshape(6) - ref).max())
        print(f"{I.NAMES[model]} seed {seed}: |A - lstsq| max {diff:.3g} (bound {LSTSQ_BOUND[model]:.3g}), "
              f"|A - planted| max {float(np.abs(A - I.A_TRUE[model]).max()):.3g}")
        assert diff <= LSTSQ_BOUND[model]      # 4 x the oracle's own largest difference, see above
        if model == AO.SIMILARITY:
            assert A[0, 0] == A[1, 1] and A[0, 1] == -A[1, 0]


def _census():
    """[(model, label, n, found, iterations, wins, update records)] over every segment of both calls."""
    rows = []
    for model in I.MODELS:
        c = I.gpu_call(model)
        _, found, _, census = I.expected(model)
        for b, label in enumerate(c.labels):
            rows.append((model, label, c.size(b), int(found[b]), *census[b]))
    return rows


def test_inputs_census(siftgpu):
    """The GPU inputs exercise the round loop (R = AFFINE_ROUND hypotheses per
    round), counted on the oracle alone: every segment of 63 pairs and more runs
    more than one round and wins more than once, and segments end by niters
    shrinking below a round boundary (after more than one round, before
    max_iters, not on a multiple of R).  The segments of m + 1 .. 4 pairs cannot
    run a second round: their first hypothesis already has m of at most 4 pairs
    as inliers, so niters falls to at most log(1e-6) / log(1 - (m / 4)^m) = 26
    (affine, 4 pairs) or 49 (similarity, 4 pairs) at once."""
    R = siftgpu.AFFINE_ROUND
    for model in I.MODELS:
        c = I.gpu_call(model)
        m = AO.model_points(model)
        census = I.expected(model)[3]
        found = I.expected(model)[1]
        assert [c.size(b) for b in range(5)] == [0, 1, 2, 3, 4]
        sizes = {c.size(b) for b in range(len(c.labels))}
        assert {63, 64, 65, 300, 2 * R + 1} <= sizes
        assert c.size(c.index("backwards")) == 0 and c.moff[c.index("backwards") + 1] < c.moff[c.index("backwards")]
        assert c.moff[-1] > c.m_cap > c.moff[-2] and len(c.src) == c.moff[-1]
        assert np.isnan(c.src[slice(*c.bounds(c.index("nan")))]).any()
        for b, label in enumerate(c.labels):
            iters, wins, _ = census[b]
            print(f"{I.NAMES[model]:10s} {label:18s} n={c.size(b):3d} found={found[b]} iterations={iters} wins={wins}")
            if c.size(b) > m:
                assert found[b] == 1 and 0 < iters < c.max_iters, label
            if c.size(b) >= 63:
                assert iters > R and wins > 1, f"{label}: {iters} iterations, {wins} wins"
        assert any(census[b][0] > R and census[b][0] % R for b in c.big)
        assert any(census[b][0] > 2 * R for b in c.big), "no segment needs a third round"
        assert found[c.index("n%d" % m)] == 1 and census[c.index("n%d" % m)][0] == 0      # the direct fit
        assert not found[:m].any()


def test_inputs_libm_margin():
    """Every update_num_iters call of the census is far from the two places
    where an ulp of log / pow could change its result: num / denom further than
    1e-9 from every half-integer, and -num against max_iters * -denom apart by
    more than 1e-9 relative -- test_homography_batch.py's margin.  A condition on
    the inputs (the seeds)."""
    n_calls = 0
    for model, label, n, found, iters, wins, ups in _census():
        for p, ep, model_points, max_iters, r in ups:
            n_calls += 1
            assert model_points == AO.model_points(model)
            num = max(1. - min(max(p, 0.), 1.), HO.DBL_MIN)
            denom = 1. - math.pow(1. - min(max(ep, 0.), 1.), model_points)
            if ep == 0.0:
                assert denom == 0.0 and r == 0           # the exact case: pow(1, m) = 1
                continue
            assert 0.0 < ep < 1.0 and denom >= HO.DBL_MIN, (label, ep)   # ep == 1 cannot win (good > m - 1)
            num, denom = math.log(num), math.log(denom)
            assert denom < 0
            a, b = -num, max_iters * (-denom)
            assert abs(a - b) > 1e-9 * max(a, b), (label, ep, a, b)
            q = num / denom
            assert abs(q - math.floor(q) - 0.5) > 1e-9, (label, ep, q)
    assert n_calls > 20
