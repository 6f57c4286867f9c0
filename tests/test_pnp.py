"""Absolute pose (solveP3P, solvePnPRansac) without a GPU: the entry points are
declared, exported, wrapped and check their arguments; the host sift_solve_p3p
and sift_solve_pnp equal pnp_oracle.py bit for bit on the censuses of
pnp_inputs.py; what they recover is the planted geometry, within a bound
measured against an independent numpy Gauss-Newton (np.linalg.lstsq, iterated to
convergence); the inputs of the GPU test are what that test needs; and the host
path runs clean under the address and undefined-behaviour sanitizers as a
stand-alone program.  The calls that need a context are in test_gpu_pnp.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

from conftest import ROOT

import pnp_inputs as I
import pnp_oracle as NO

NEW = ["sift_solve_p3p", "sift_solve_pnp", "sift_solve_pnp_segmented_device", "sift_solve_pnp_segmented"]
PD = ctypes.POINTER(ctypes.c_double)
PF = ctypes.POINTER(ctypes.c_float)


def test_entry_points_declared_exported_and_wrapped(siftgpu):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sift_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert getattr(siftgpu.lib(), name).argtypes is not None, name
    for meth in ["solve_pnp_segmented_device", "solvePnPBatch"]:
        assert callable(getattr(siftgpu.Context, meth)), meth
    assert callable(siftgpu.solveP3P) and callable(siftgpu.solvePnPRansac)
    assert b"pnp_segmented\0" in open(siftgpu.LIB_PATH, "rb").read()          # the stage's name
    # the functions the rule calls and must not edit are still there
    src = open(os.path.join(ROOT, "sift-gpu_amd", "csrc", "homography_math.hpp")).read()
    assert "void sym_eig(" in src and "int update_num_iters(" in src
    # the round size the kernel is built with, as scratch.hpp states it
    sc = open(os.path.join(ROOT, "sift-gpu_amd", "csrc", "scratch.hpp")).read()
    assert re.search(r"#define SIFT_PNP_ROUND 256\b", sc) and I.GPU_ITERS == 2 * 256 + 1


def test_argument_checks(siftgpu):
    L = siftgpu.lib()
    E = siftgpu.SIFT_E_INVALID
    xy = np.zeros(16, np.float32)
    M = np.eye(3).reshape(9)
    out = np.zeros(48)
    n = ctypes.c_int(0)
    f, m, o, g = xy.ctypes.data_as(PF), M.ctypes.data_as(PD), out.ctypes.data_as(PD), ctypes.byref(n)
    for a in ((None, f, m, o, g), (o, None, m, o, g), (o, f, None, o, g), (o, f, m, None, g), (o, f, m, o, None)):
        assert L.sift_solve_p3p(*a) == E
    call = lambda x, p, cnt, K, pose, ni: L.sift_solve_pnp(x, p, cnt, None, K, 8.0, 100, 0.99, pose, None, ni)  # noqa: E731
    for a in ((None, f, 5, m, o, g), (o, None, 5, m, o, g), (o, f, 5, None, o, g), (o, f, 5, m, None, g),
              (o, f, 5, m, o, None), (o, f, -1, m, o, g)):
        assert call(*a) == E
    assert call(None, None, 0, m, o, g) == E and n.value == 0       # no rows: valid arguments, no model
    # a null context, also with nothing to do
    p = out.ctypes.data
    assert L.sift_solve_pnp_segmented_device(None, p, p, p, 1, 4, None, p, 0, 8.0, 100, 0.99, p, p, p, None) == E
    assert L.sift_solve_pnp_segmented_device(None, None, None, None, 0, 0, None, None, 0, 8.0, 100, 0.99, None, None,
                                             None, None) == E
    assert L.sift_solve_pnp_segmented(None, None, None, None, 0, 0, None, None, 0, 8.0, 100, 0.99, None, None, None,
                                      None) == E


def test_p3p_matches_oracle_bitexact(siftgpu):
    """sift_solve_p3p on every case of pnp_inputs.p3p_cases: the number of solutions, each pose bit
    for bit in the fixed order, zeros behind them; the census holds every solution count."""
    counts = {}
    assert [c[0] for c in I.p3p_cases()] == I.P3P_CENSUS
    for label, X, xy, K in I.p3p_cases():
        exp = NO.solve_p3p(X, xy, K)
        poses = np.full((5, 12), 5.0)
        ns = ctypes.c_int(-9)
        Xa, Ka = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(K, np.float64)
        rc = siftgpu.lib().sift_solve_p3p(Xa.ctypes.data_as(PD), xy.ctypes.data_as(PF), Ka.ctypes.data_as(PD),
                                          poses.ctypes.data_as(PD), ctypes.byref(ns))
        assert rc == 0 and ns.value == len(exp) and (poses[4] == 5.0).all(), label
        assert poses[:len(exp)].tobytes() == exp.tobytes() and not poses[len(exp):4].any(), label
        assert np.isfinite(exp).all(), label
        counts.setdefault(len(exp), []).append(label)
    print({k: len(v) for k, v in sorted(counts.items())})
    assert set(counts) == {0, 1, 2, 3, 4}
    for label in ("equal_points", "collinear", "K_singular", "K_nan", "xyz_nan", "xy_nan"):
        assert label in counts[0], label
    # a general triple's solutions contain the planted pose, to the float32 pixel quantum
    for k in range(I.N_GENERAL):
        v = I.view(500 + k, 3, I.K_B if k % 2 else I.K_A)
        sols = siftgpu.solveP3P(v["X"], v["xy"], v["K"])
        assert sols and min(max(np.abs(R - v["R"]).max(), np.abs(t - v["t"]).max()) for R, t in sols) < 1e-3, k
    for k in I.ABOVE:
        X, xy, R0, t0 = I.triangle_above(k)
        sols = siftgpu.solveP3P(X, xy, I.K_B)
        assert sols and min(max(np.abs(R - R0).max(), np.abs(t - t0).max()) for R, t in sols) < 1e-3, k


def _host(siftgpu, c):
    """sift_solve_pnp into sentinel-filled outputs -> (rc, pose, mask, n_inliers)."""
    n = len(c.X)
    pose, mask = np.full(12, 5.0), np.full(n + 1, 7, np.uint8)
    ni = ctypes.c_int(-9)
    X = c.X if n else np.zeros((1, 3))
    xy = c.xy if n else np.zeros((1, 2), np.float32)
    rc = siftgpu.lib().sift_solve_pnp(
        X.ctypes.data_as(PD), xy.ctypes.data_as(PF), n, None if c.mask is None else c.mask.ctypes.data,
        np.ascontiguousarray(c.K).ctypes.data_as(PD), c.thr, c.iters, c.conf, pose.ctypes.data_as(PD),
        mask.ctypes.data, ctypes.byref(ni))
    assert mask[n] == 7, c.label + ": a write past n"
    return rc, pose, mask[:n], ni.value


def test_host_matches_oracle_bitexact(siftgpu):
    """pose (twelve doubles), n_inliers and every mask byte on every case of pnp_inputs.cpu_cases;
    no model is SIFT_E_INVALID with every output zeroed."""
    got = {}
    assert [c.label for c in I.cpu_cases()] == I.CENSUS
    for c in I.cpu_cases():
        o = c.oracle()
        rc, pose, mask, ni = _host(siftgpu, c)
        print(f"{c.label:12s} n={len(c.X):3d} found={o.found} n_inliers={o.n_inliers} iterations={o.iters} "
              f"refit steps={o.refit_steps}")
        assert (rc == 0) == bool(o.found) and (rc in (0, siftgpu.SIFT_E_INVALID)), c.label
        assert pose.tobytes() == o.pose.tobytes(), f"{c.label}: pose {pose} != {o.pose}"
        assert ni == o.n_inliers and mask.tobytes() == o.mask.tobytes(), f"{c.label}: n_inliers / mask"
        if o.found:
            assert np.isfinite(pose).all(), c.label
        else:
            assert not pose.any() and ni == 0 and not mask.any(), c.label
        got[c.label] = o
    # what the cases are there for
    for label in ("n0", "n3", "n4_masked", "mask_zero", "thr_nan", "iters_0", "conf_0", "conf_1", "K_singular",
                  "K_nan"):
        assert not got[label].found, label
    assert got["n4"].n_inliers == 4 and got["n4"].mask.all() and got["n5"].n_inliers == 5
    by = {c.label: c for c in I.cpu_cases()}
    for label in ("coplanar", "out30", "out50"):
        assert got[label].mask.astype(bool).tolist() == by[label].view["good"].tolist(), label
    assert got["behind"].n_inliers == 60 and not got["behind"].mask[:20].any()
    assert got["zero_rows"].n_inliers == 60 and not got["zero_rows"].mask[::4].any()
    ones, some = got["mask_ones"], got["mask_some"]
    assert ones.pose.tobytes() == got["out30"].pose.tobytes() and ones.n_inliers == 84
    assert 0 < some.n_inliers < 84 and not (some.mask.astype(bool) & (by["mask_some"].mask == 0)).any()
    assert got["thr_neg8"].pose.tobytes() == got["out30"].pose.tobytes()
    assert got["thr_inf"].found and got["iters_1"].iters == 1 and got["iters_1"].n_inliers == 60
    assert got["mask_zero"].iters == 100           # masked subsets are counted iterations
    for label, rows in (("nan_rows", (3, 10, 40, 41)), ("inf_rows", (5, 12, 50))):
        assert got[label].found and not got[label].mask[list(rows)].any(), label
    # the module-level wrapper returns the same
    c = by["out30"]
    R, t, mask, ni = siftgpu.solvePnPRansac(c.X, c.xy, c.K)
    assert np.c_[R, t].tobytes() == got["out30"].pose.tobytes() and ni == 84
    assert siftgpu.solvePnPRansac(c.X, c.xy, I.K_SINGULAR)[0] is None


# ---- planted geometry against an independent numpy Gauss-Newton ----------------
def _rodrigues(w):
    th = np.linalg.norm(w)
    if th < 1e-300:
        return np.eye(3)
    k = w / th
    S = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * S + (1 - np.cos(th)) * (S @ S)


def _reference(X, uv, R, t):
    """Gauss-Newton on the reprojection error in normalised coordinates from (R, t), the update
    R <- exp([w]x) R by np.linalg.lstsq on the analytic Jacobian, iterated
    until the step is below 1e-15 -> (R, t, steps)."""
    for step in range(50):
        Xc = X @ R.T + t
        r = (Xc[:, :2] / Xc[:, 2:] - uv).reshape(-1)
        J = np.zeros((2 * len(X), 6))
        for i, (x, y, z) in enumerate(Xc):
            Jp = np.array([[1 / z, 0, -x / z ** 2], [0, 1 / z, -y / z ** 2]])
            Rx = Xc[i] - t                                       # d(exp([w]x) R X)/dw = -[R X]x
            S = np.array([[0, -Rx[2], Rx[1]], [Rx[2], 0, -Rx[0]], [-Rx[1], Rx[0], 0]])
            J[2 * i:2 * i + 2] = Jp @ np.c_[-S, np.eye(3)]
        d = np.linalg.lstsq(J, -r, rcond=None)[0]
        R, t = _rodrigues(d[:3]) @ R, t + d[3:]
        if np.abs(d).max() < 1e-15:
            break
    return R, t, step + 1


# The largest difference between the host path and the numpy reference over the 16
# inputs of test_planted_geometry (eight scenes, without and with 30 % outliers),
# measured on the CPU: R 9.1e-14, t 5.6e-13 (MEASURED is the larger); |R^T R - I| of
# the outputs 2.1e-13 at most (P3P's R = Y X^-1 is orthogonal only up to rounding and
# the Cayley update keeps what it is given).  The reference's own distance from the
# planted pose on the same inputs is 1.9e-8 (R) and 1.2e-7 (t): the float32 pixel
# quantum, four orders above the bound, so the bound rests on the reference's
# minimum, not on the planted pose and not on the code under test.  One bound for
# all: 16 x the largest, the margin test_pose.py uses between two double
# implementations of one minimum.  The kernel is bit-equal to the host path
# (test_gpu_pnp.py), so the bound binds it too.
MEASURED = 5.6e-13
BOUND = 16 * MEASURED


def test_planted_geometry(siftgpu):
    """Eight scenes of 300 points under a known pose (scene 3 coplanar, the odd ones with a skewed
    K), pixels rounded to float, without and with 30 % outliers: every planted inlier is in the
    mask at 8 px and no planted outlier; the pose agrees with the numpy reference within BOUND."""
    worst = {"R": 0.0, "t": 0.0, "orth": 0.0, "ref R": 0.0, "ref t": 0.0}
    for k in range(8):
        for out in (0.0, 0.3):
            v = I.planted(k, out)
            R, t, mask, ni = siftgpu.solvePnPRansac(v["X"], v["xy"], v["K"], 8.0, 100, 0.99)
            assert R is not None and mask.astype(bool).tolist() == v["good"].tolist() and ni == v["good"].sum(), (k, out)
            g = v["good"]
            uvw = np.c_[v["xy"][g].astype(np.float64), np.ones(g.sum())] @ np.linalg.inv(v["K"]).T
            rR, rt, steps = _reference(v["X"][g], uvw[:, :2] / uvw[:, 2:], v["R"], v["t"])
            diffs = {"R": np.abs(R - rR).max(), "t": np.abs(t - rt).max(), "orth": np.abs(R.T @ R - np.eye(3)).max(),
                     "ref R": np.abs(rR - v["R"]).max(), "ref t": np.abs(rt - v["t"]).max()}
            print(f"scene {k} outliers {out}: n_inliers {ni}, reference steps {steps}",
                  {a: f"{b:.3g}" for a, b in diffs.items()})
            for a, b in diffs.items():
                worst[a] = max(worst[a], float(b))
            assert steps < 50 and diffs["R"] <= BOUND and diffs["t"] <= BOUND and diffs["orth"] <= BOUND, (k, out, diffs)
            assert np.linalg.det(R) > 0
    print("worst", worst, "bound", BOUND)


def test_pnp_rule_program(tmp_path):
    """tests/cpp/pnp_rule.cpp linked with pnp.hip alone (host code only), with the address and
    undefined-behaviour sanitizers where the compiler has their runtimes: the sanitizer check of
    the host path, as a program of its own."""
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = tmp_path / "pnp_rule"
    base = [hipcc, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "--offload-host-only", "-x", "hip",
            os.path.join(ROOT, "tests", "cpp", "pnp_rule.cpp"),
            os.path.join(ROOT, "sift-gpu_amd", "csrc", "pnp.hip"), "-o", str(exe)]
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "pnp rule ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_gpu_inputs_census(siftgpu):
    """The committed inputs of the GPU test are what that test needs, counted on the oracle alone;
    and the host path equals the oracle on them."""
    c = I.gpu_call()
    e = I.expected()
    assert len(c.labels) == 16
    sizes = [c.size(b) for b in range(len(c.labels))]
    assert {0, 3, 4, 5, 255, 256, 257, 600} <= set(sizes)
    assert c.size(c.index("backwards")) == 0 and c.moff[c.index("backwards") + 1] < c.moff[c.index("backwards")]
    assert c.moff[-1] > c.m_cap > c.moff[-2] and len(c.X) == c.moff[-1]
    for bad in ("nan", "singular_K", "all_masked"):
        b = c.index(bad)
        assert e["found"][b - 1] == 1 and e["found"][b + 1] == 1, bad
    assert e["found"][c.index("singular_K")] == 0 and e["found"][c.index("all_masked")] == 0
    lo, hi = c.bounds(c.index("nan"))
    assert np.isnan(c.X[lo:hi]).any() and np.isnan(c.xy[lo:hi]).any() and e["found"][c.index("nan")] == 1
    assert not c.mask[slice(*c.bounds(c.index("all_masked")))].any()
    # two full rounds of 256 hypotheses and one more, with a model at the end
    assert e["iters"][c.index("long")] == c.iters == 513 and e["found"][c.index("long")] == 1
    assert e["iters"][c.index("all_masked")] == 513
    assert e["found"][c.index("n3")] == 0 and e["n_inliers"][c.index("n4")] == 4 and e["n_inliers"][c.index("n5")] == 5
    assert 300 < e["n_inliers"][c.index("n600")] < 600
    for b in range(len(c.labels)):
        lo, hi = c.bounds(b)
        R, t, m, ni = siftgpu.solvePnPRansac(c.X[lo:hi], c.xy[lo:hi], c.K[b], c.thr, c.iters, c.conf, c.mask[lo:hi])
        pose = np.zeros(12) if R is None else np.c_[R, t].reshape(12)
        assert pose.tobytes() == e["pose"][b].tobytes() and ni == e["n_inliers"][b], c.labels[b]
        assert m.tobytes() == e["mask"][lo:hi].tobytes(), c.labels[b]
