"""The fundamental-matrix estimate without a GPU: the entry points are declared,
exported, wrapped and reject a null context; the host sift_find_fundamental
equals fundamental_oracle.py bit for bit on fundamental_inputs.cpu_cases; what
it estimates is the planted two-view geometry, of rank 2; the host path runs
clean under the address and undefined-behaviour sanitizers as a stand-alone
program; and the committed inputs of the GPU test (fundamental_inputs.gpu_call)
are what that test needs -- the census and the libm margin below hold on the
oracle alone.

The device form carves nothing from the context's scratch block and the
host-buffer form stages through affine_host_layout (tests/cpp/affine_layout.cpp
checks it), so there is no layout program of its own.  The calls that need a
context are in test_gpu_fundamental.py."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np

from conftest import ROOT

import fundamental_inputs as I
import fundamental_oracle as FO
import homography as HO

NEW = ["sift_find_fundamental", "sift_find_fundamental_segmented_device", "sift_find_fundamental_segmented"]


def test_entry_points_declared_exported_and_wrapped(siftgpu):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sift_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert getattr(siftgpu.lib(), name).argtypes is not None, name
    for meth in ["find_fundamental_segmented_device", "findFundamentalBatch"]:
        assert callable(getattr(siftgpu.Context, meth)), meth
    assert callable(siftgpu.findFundamentalMat)
    src = open(os.path.join(ROOT, "sift-gpu_amd", "csrc", "scratch.hpp")).read()
    assert re.search(r"kFundRound\s*=\s*%d\s*;" % siftgpu.FUND_ROUND, src)
    assert I.ROUND == siftgpu.FUND_ROUND and siftgpu.FUND_ROUND in (64, 128, 256)
    assert b"fundamental_segmented\0" in open(siftgpu.LIB_PATH, "rb").read()     # the stage's name


def test_entry_points_reject_null_context(siftgpu):
    L = siftgpu.lib()
    xy = np.zeros(32, np.float32)
    off = np.array([0, 8], np.int32)
    F = np.zeros(9, np.float64)
    found = np.zeros(1, np.int32)
    pf = xy.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    pi = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))  # noqa: E731
    E = siftgpu.SIFT_E_INVALID
    assert L.sift_find_fundamental_segmented_device(None, xy.ctypes.data, xy.ctypes.data, off.ctypes.data, 1, 8, 3.0,
                                                    1000, 0.99, F.ctypes.data, found.ctypes.data, None) == E
    assert L.sift_find_fundamental_segmented(None, pf, pf, pi(off), 1, 8, 3.0, 1000, 0.99,
                                             F.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), pi(found), None) == E
    # and with nothing to do: the null context is still rejected first
    assert L.sift_find_fundamental_segmented_device(None, None, None, None, 0, 0, 3.0, 1000, 0.99, None, None,
                                                    None) == E
    assert L.sift_find_fundamental_segmented(None, None, None, None, 0, 0, 3.0, 1000, 0.99, None, None, None) == E
    # the host call: null buffers and a negative count
    pd = F.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.sift_find_fundamental(None, pf, 8, 3.0, 1000, 0.99, pd, None) == E
    assert L.sift_find_fundamental(pf, pf, 8, 3.0, 1000, 0.99, None, None) == E
    assert L.sift_find_fundamental(pf, pf, -1, 3.0, 1000, 0.99, pd, None) == E


def test_host_matches_oracle_bitexact(siftgpu):
    """F (nine doubles), found and every mask byte, on every case of fundamental_inputs.cpu_cases."""
    got = {}
    for label, s, d, thr, max_iters, conf in I.cpu_cases():
        F, found, m = FO.find_fundamental(s, d, thr, max_iters, conf)
        hF, hm = siftgpu.findFundamentalMat(s, d, thr, max_iters, conf)
        print(f"{label:16s} n={len(s):3d} found={found} inliers={int(m.sum())}")
        assert (F is None) == (hF is None) == (not found), label
        if F is not None:
            assert np.array(F, np.float64).tobytes() == hF.tobytes(), f"{label}: {hF.reshape(9)} != {F}"
            assert np.isfinite(hF).all(), label
        assert m.tobytes() == hm.tobytes(), f"{label}: mask"
        got[label] = (F is not None, int(m.sum()))
    # what the cases are there for
    assert [got[f"n{n}"][0] for n in (0, 1, 7, 8, 9)] == [False, False, False, True, True]
    assert got["n8"][1] == 8 and not got["identical"][0] and not got["collinear"][0]
    assert got["outliers40"][0] and got["noise"][0]
    assert got["thr-3"][0] and 2 * got["thr-3"][1] > 80
    assert got["thr1e30"] == (True, 80) and got["thr0"][1] < got["thr-3"][1]
    assert not got["max_iters0"][0] and not got["confidence0"][0] and not got["confidence1"][0]
    assert got["nan_row"][0] and got["inf_row"][0] and got["inf_row_thr1e30"][0]
    # none: F and the mask are zeroed by the C entry point itself
    s, d = next(c[1:3] for c in I.cpu_cases() if c[0] == "collinear")
    F9 = np.full(9, 5.0)
    mk = np.full(len(s), 7, np.uint8)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = siftgpu.lib().sift_find_fundamental(s.ctypes.data_as(fp), d.ctypes.data_as(fp), len(s), 3.0, 1000, 0.99,
                                             F9.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), mk.ctypes.data)
    assert rc == siftgpu.SIFT_E_INVALID and (F9 == 0).all() and (mk == 0).all()


def test_semantics_on_planted_geometry(siftgpu):
    """0.25 px noise, 30 % outliers moved 50 to 300 px off their epipolar lines,
    thr 3: the model is found, every planted inlier lies within 3 px of its
    epipolar lines under the returned F (a 12 x margin over the noise), and
    every planted outlier (16 x the threshold away at the least) is out of the
    mask."""
    for seed in (60, 61, 62):
        s, d, good = I.data(seed, 200, 0.3, 0.25)
        F, m = siftgpu.findFundamentalMat(s, d)
        assert F is not None
        d2, d1 = I.epipolar_distances(F, s, d)
        worst = float(np.maximum(d1, d2)[good].max())
        print(f"seed {seed}: inliers {int(m.sum())} of {int(good.sum())} planted, worst planted-inlier distance "
              f"{worst:.3f} px, nearest outlier {float(np.maximum(d1, d2)[~good].min()):.1f} px")
        assert worst < 3.0
        assert not m[~good].any(), "a planted outlier is in the mask"


def _reference_8point(s, d):
    """numpy's SVD-truncated normalised 8-point on float64 copies of the pairs, pushed through
    the same denormalisation and scaling -> F 3x3."""
    s, d = s.astype(np.float64), d.astype(np.float64)
    cs, cd = s.mean(0), d.mean(0)
    ks, kd = math.sqrt(2) / np.hypot(*(s - cs).T).mean(), math.sqrt(2) / np.hypot(*(d - cd).T).mean()
    x, X = (s - cs) * ks, (d - cd) * kd
    A = np.c_[X[:, 0] * x[:, 0], X[:, 0] * x[:, 1], X[:, 0], X[:, 1] * x[:, 0], X[:, 1] * x[:, 1], X[:, 1],
              x[:, 0], x[:, 1], np.ones(len(s))]
    F0 = np.linalg.svd(A)[2][-1].reshape(3, 3)
    U, w, Vt = np.linalg.svd(F0)
    F0 = U @ np.diag([w[0], w[1], 0.0]) @ Vt
    Ts = np.array([[ks, 0, -cs[0] * ks], [0, ks, -cs[1] * ks], [0, 0, 1]])
    Td = np.array([[kd, 0, -cd[0] * kd], [0, kd, -cd[1] * kd], [0, 0, 1]])
    F = Td.T @ F0 @ Ts
    return F / F[2, 2]


# sigma_3 / sigma_1 of the reference (numpy's SVD truncation, denormalised) over
# the three inputs below, measured on the CPU: 1.49e-19, 3.74e-19, 2.28e-19 --
# the rounding of the two 3x3 products after an exact truncation (F's entries
# span nine decades once F[8] is 1).  The library takes a different route to the
# same projection (F0 - (F0 v) v^T with v from a Jacobi on F0^T F0), so 16 x the
# reference's ratio is allowed; it measured 1.07e-19, 4.08e-19, 6.11e-19 (2.7 x
# at the most).  The bound is per input, from the reference alone.
RANK_FACTOR = 16.0


def test_rank_two(siftgpu):
    for seed in (60, 61, 62):
        s, d, good = I.data(seed, 200, 0.3, 0.25)
        F, m = siftgpu.findFundamentalMat(s, d)
        assert F is not None
        w = np.linalg.svd(F, compute_uv=False)
        ref = np.linalg.svd(_reference_8point(s[good], d[good]), compute_uv=False)
        ours, theirs = float(w[2] / w[0]), float(ref[2] / ref[0])
        print(f"seed {seed}: sigma3/sigma1 library {ours:.3g}, reference {theirs:.3g}, bound {RANK_FACTOR * theirs:.3g}")
        assert ours <= RANK_FACTOR * theirs


def test_fundamental_rule_program(tmp_path):
    """tests/cpp/fundamental_rule.cpp linked with fundamental.hip alone (host code
    only), with the address and undefined-behaviour sanitizers where the
    compiler has their runtimes: the sanitizer check of the host path, as a
    program of its own."""
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = tmp_path / "fundamental_rule"
    base = [hipcc, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "--offload-host-only", "-x", "hip",
            os.path.join(ROOT, "tests", "cpp", "fundamental_rule.cpp"),
            os.path.join(ROOT, "sift-gpu_amd", "csrc", "fundamental.hip"), "-o", str(exe)]
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "fundamental rule ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_inputs_census(siftgpu):
    """The GPU inputs exercise the round loop (R = FUND_ROUND hypotheses per
    round), counted on the oracle alone: every segment of 63 pairs and more runs
    more than one round and wins more than once, at least one needs a third
    round, and at least one ends off a round boundary before max_iters; the
    segment of 8 pairs is the direct fit with no iteration, and fewer than 8
    pairs find none."""
    R = siftgpu.FUND_ROUND
    c = I.gpu_call()
    _, found, _, census = I.expected()
    assert [c.size(b) for b in range(5)] == [0, 1, 7, 8, 9]
    sizes = {c.size(b) for b in range(len(c.labels))}
    assert {63, 64, 65, 300, 2 * R + 1} <= sizes
    assert c.size(c.index("backwards")) == 0 and c.moff[c.index("backwards") + 1] < c.moff[c.index("backwards")]
    assert c.moff[-1] > c.m_cap > c.moff[-2] and len(c.src) == c.moff[-1]
    assert np.isnan(c.src[slice(*c.bounds(c.index("nan")))]).any()
    for b, label in enumerate(c.labels):
        iters, wins, _ = census[b]
        print(f"{label:18s} n={c.size(b):3d} found={found[b]} iterations={iters} wins={wins}")
        if c.size(b) > FO.M:
            assert found[b] == 1 and 0 < iters < c.max_iters, label
        if c.size(b) >= 63:
            assert iters > R and wins > 1, f"{label}: {iters} iterations, {wins} wins"
    assert any(census[b][0] > R and census[b][0] % R and census[b][0] < c.max_iters for b in c.big)
    assert any(census[b][0] > 2 * R for b in c.big), "no segment needs a third round"
    assert found[c.index("n8")] == 1 and census[c.index("n8")][0] == 0      # the direct fit
    assert not found[:3].any()


def test_inputs_libm_margin():
    """Every update_num_iters call of the census is far from the two places where
    an ulp of log / pow could change its result: num / denom further than 1e-9
    from every half-integer, and -num against max_iters * -denom apart by more
    than 1e-9 relative -- test_affine.py::test_inputs_libm_margin's margins.  A
    condition on the inputs (the seed)."""
    c = I.gpu_call()
    census = I.expected()[3]
    n_calls = 0
    for b, label in enumerate(c.labels):
        for p, ep, model_points, max_iters, r in census[b][2]:
            n_calls += 1
            assert model_points == FO.M
            num = max(1. - min(max(p, 0.), 1.), HO.DBL_MIN)
            denom = 1. - math.pow(1. - min(max(ep, 0.), 1.), model_points)
            if ep == 0.0:
                assert denom == 0.0 and r == 0           # the exact case: pow(1, m) = 1
                continue
            assert 0.0 < ep < 1.0 and denom >= HO.DBL_MIN, (label, ep)   # ep == 1 cannot win (good > 7)
            num, denom = math.log(num), math.log(denom)
            assert denom < 0
            a, bb = -num, max_iters * (-denom)
            assert abs(a - bb) > 1e-9 * max(a, bb), (label, ep, a, bb)
            q = num / denom
            assert abs(q - math.floor(q) - 0.5) > 1e-9, (label, ep, q)
    assert n_calls > 20
