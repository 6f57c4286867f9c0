"""The segmented homography without a GPU: the entry points are declared,
exported, wrapped and reject a null context; the scratch layout program
compiles and passes; and the committed inputs of the GPU tests
(homography_batch_inputs.py) are what those tests need -- the census and the
libm margin below hold on oracle/homography.py alone.

The calls that need a context (null buffers with a live context, n_segments ==
0 returning SIFT_OK) are in test_gpu_homography_batch.py: a context cannot be
created without a GPU."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import homography as HO
import homography_batch_inputs as I

NEW = ["sift_find_homography_segmented_device", "sift_find_homography_segmented",
       "sift_perspective_transform_segmented_device"]


def test_entry_points_declared_exported_and_wrapped(siftgpu):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sift_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert getattr(siftgpu.lib(), name).argtypes is not None, name
    for meth in ["find_homography_segmented_device", "perspective_transform_segmented_device", "findHomographyBatch"]:
        assert callable(getattr(siftgpu.Context, meth)), meth
    src = open(os.path.join(ROOT, "sift-gpu_amd", "csrc", "scratch.hpp")).read()
    assert re.search(r"kHomogRound\s*=\s*%d\s*;" % siftgpu.HOMOGRAPHY_ROUND, src)


def test_entry_points_reject_null_context(siftgpu):
    L = siftgpu.lib()
    xy = np.zeros(16, np.float32)
    off = np.array([0, 4], np.int32)
    H = np.zeros(9, np.float64)
    found = np.zeros(1, np.int32)
    pf = xy.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    pi = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))  # noqa: E731
    E = siftgpu.SIFT_E_INVALID
    assert L.sift_find_homography_segmented_device(None, xy.ctypes.data, xy.ctypes.data, off.ctypes.data, 1, 4, 3.0,
                                                   2000, 0.995, H.ctypes.data, found.ctypes.data, None) == E
    assert L.sift_find_homography_segmented(None, pf, pf, pi(off), 1, 4, 3.0, 2000, 0.995,
                                            H.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), pi(found), None) == E
    assert L.sift_perspective_transform_segmented_device(None, H.ctypes.data, found.ctypes.data, 1, xy.ctypes.data,
                                                         4, xy.ctypes.data) == E
    # and with nothing to do: the null context is still rejected first, as in the matcher
    assert L.sift_find_homography_segmented_device(None, None, None, None, 0, 0, 3.0, 2000, 0.995, None, None,
                                                   None) == E


def test_homography_layouts(tmp_path):
    """tests/cpp/homography_layout.cpp, built like test_abi.py::test_scratch_layouts:
    with the address and undefined-behaviour sanitizers (runtimes linked
    statically into the program) where the host compiler has them."""
    src = os.path.join(ROOT, "tests", "cpp", "homography_layout.cpp")
    exe = tmp_path / "homography_layout"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "homography layouts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def _census():
    """[(call, label, n, found, iterations, update records)] over every segment of every call."""
    e = I.expected()
    rows = []
    for c in I.calls():
        _, found, _, census = e[c.name]
        for b, label in enumerate(c.labels):
            rows.append((c, label, c.sizes[b], int(found[b]), census[b][0], census[b][1]))
    return rows


def test_inputs_census(siftgpu):
    """The committed inputs exercise every exit of the round loop (R =
    HOMOGRAPHY_ROUND hypotheses per round), counted on the oracle alone."""
    R = siftgpu.HOMOGRAPHY_ROUND
    rows = [r for r in _census() if r[2] > 4]
    for c, label, n, found, iters, _ in rows:
        print(f"{c.name:7s} {label:14s} n={n:3d} found={found} iterations={iters} (max_iters {c.max_iters})")
    assert any(found and 0 < it < R for _, _, _, found, it, _ in rows), "no segment ends within the first round"
    assert any(found and R <= it < 2 * R for _, _, _, found, it, _ in rows), "no segment ends in the second round"
    assert any(found and 2 * R < it for _, _, _, found, it, _ in rows), "no segment needs more than 2R iterations"
    assert any(found and it == c.max_iters for c, _, _, found, it, _ in rows), "none reaches max_iters with a model"
    assert any(not found and it == c.max_iters for c, _, _, found, it, _ in rows), "none reaches max_iters with none"
    # the 10000-attempt exit at iteration 0, and the direct fit
    assert any(not found and it == 0 and label == "collinear" for _, label, _, found, it, _ in rows)
    c = I.calls()[0]
    assert I.expected()["MAIN"][1][c.index("four")] == 1 and c.sizes[c.index("four")] == 4


def test_inputs_libm_margin():
    """Every update_num_iters call of the census is far from the two places
    where an ulp of log / pow could change its result: num / denom further than
    1e-9 from every half-integer, and -num against max_iters * -denom apart by
    more than 1e-9 relative.  A condition on the inputs (the seeds)."""
    n_calls = 0
    for c, label, n, found, iters, ups in _census():
        for p, ep, model_points, max_iters, r in ups:
            n_calls += 1
            num = max(1. - min(max(p, 0.), 1.), HO.DBL_MIN)
            denom = 1. - math.pow(1. - min(max(ep, 0.), 1.), model_points)
            if ep == 0.0:
                assert denom == 0.0 and r == 0           # the exact case: pow(1, 4) = 1
                continue
            assert 0.0 < ep < 1.0 and denom >= HO.DBL_MIN, (label, ep)   # ep == 1 cannot win (good > 3)
            num, denom = math.log(num), math.log(denom)
            assert denom < 0
            a, b = -num, max_iters * (-denom)
            assert abs(a - b) > 1e-9 * max(a, b), (label, ep, a, b)
            q = num / denom
            assert abs(q - math.floor(q) - 0.5) > 1e-9, (label, ep, q)
    assert n_calls > 20
