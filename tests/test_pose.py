"""Relative pose and triangulation without a GPU: the entry points are declared,
exported, wrapped and check their arguments; the host sift_recover_pose equals
pose_oracle.py bit for bit on pose_inputs.cpu_cases (pose, E, n_good, every mask
byte, every xyz double); what it recovers is the planted geometry, within a
bound measured against an SVD restatement of cv::recoverPose +
cv::triangulatePoints; sift_triangulate_points equals the oracle bit for bit and
agrees with pose recovery; and the host path runs clean under the address and
undefined-behaviour sanitizers as a stand-alone program.  The calls that need a
context are in test_gpu_pose.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

from conftest import ROOT

import fundamental_inputs as FI
import pose_inputs as I
import pose_oracle as PO

NEW = ["sift_recover_pose", "sift_recover_pose_segmented_device", "sift_recover_pose_segmented",
       "sift_triangulate_points", "sift_triangulate_points_segmented_device"]
PD = ctypes.POINTER(ctypes.c_double)
PF = ctypes.POINTER(ctypes.c_float)


def test_entry_points_declared_exported_and_wrapped(siftgpu):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sift_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert getattr(siftgpu.lib(), name).argtypes is not None, name
    for meth in ["recover_pose_segmented_device", "recoverPoseBatch", "triangulate_points_segmented_device"]:
        assert callable(getattr(siftgpu.Context, meth)), meth
    assert callable(siftgpu.recoverPose) and callable(siftgpu.triangulatePoints)
    blob = open(siftgpu.LIB_PATH, "rb").read()
    assert b"recover_pose_segmented\0" in blob and b"triangulate_segmented\0" in blob     # the stages' names
    # the Jacobi the homography and the fundamental tests pin is still there beside its sibling
    src = open(os.path.join(ROOT, "sift-gpu_amd", "csrc", "homography_math.hpp")).read()
    assert "void smallest_eigvec(" in src and "void sym_eig(" in src


def test_argument_checks(siftgpu):
    L = siftgpu.lib()
    E = siftgpu.SIFT_E_INVALID
    xy = np.zeros(16, np.float32)
    M = np.eye(3).reshape(9)
    out = np.zeros(16)
    ng = ctypes.c_int(0)
    f, m, o = xy.ctypes.data_as(PF), M.ctypes.data_as(PD), out.ctypes.data_as(PD)
    call = lambda F, Ks, Kd, s, d, n, pose, good: L.sift_recover_pose(  # noqa: E731
        F, Ks, Kd, s, d, n, None, 50.0, pose, None, None, None, good)
    g = ctypes.byref(ng)
    for a in ((None, m, m, f, f, 8, o, g), (m, None, m, f, f, 8, o, g), (m, m, None, f, f, 8, o, g),
              (m, m, m, None, f, 8, o, g), (m, m, m, f, None, 8, o, g), (m, m, m, f, f, 8, None, g),
              (m, m, m, f, f, 8, o, None), (m, m, m, f, f, -1, o, g)):
        assert call(*a) == E
    assert L.sift_triangulate_points(None, o, f, f, 2, o) == E and L.sift_triangulate_points(o, None, f, f, 2, o) == E
    assert L.sift_triangulate_points(o, o, None, f, 2, o) == E and L.sift_triangulate_points(o, o, f, f, 2, None) == E
    assert L.sift_triangulate_points(o, o, f, f, -1, o) == E and L.sift_triangulate_points(o, o, None, None, 0, None) == 0
    # a null context, also with nothing to do
    p = out.ctypes.data
    assert L.sift_recover_pose_segmented_device(None, p, p, p, 1, 4, p, p, p, p, 0, None, 50.0, p, None, p, p, None,
                                                None) == E
    assert L.sift_recover_pose_segmented_device(None, None, None, None, 0, 0, None, None, None, None, 0, None, 50.0,
                                                None, None, None, None, None, None) == E
    assert L.sift_recover_pose_segmented(None, None, None, None, 0, 0, None, None, None, None, 0, None, 50.0, None,
                                         None, None, None, None, None) == E
    assert L.sift_triangulate_points_segmented_device(None, p, p, p, 1, 4, p, p, p) == E
    assert L.sift_triangulate_points_segmented_device(None, None, None, None, 0, 0, None, None, None) == E


def _host(siftgpu, c):
    """sift_recover_pose into sentinel-filled outputs -> (rc, pose, E, mask, xyz, n_good)."""
    n = len(c.src)
    pose, E = np.full(12, 5.0), np.full(9, 5.0)
    mask, xyz = np.full(n + 1, 7, np.uint8), np.full((n + 1, 3), 5.0)
    ng = ctypes.c_int(-9)
    rc = siftgpu.lib().sift_recover_pose(
        np.ascontiguousarray(c.F).ctypes.data_as(PD), np.ascontiguousarray(c.K_src).ctypes.data_as(PD),
        np.ascontiguousarray(c.K_dst).ctypes.data_as(PD), c.src.ctypes.data_as(PF), c.dst.ctypes.data_as(PF), n,
        None if c.mask is None else c.mask.ctypes.data, c.thresh, pose.ctypes.data_as(PD), E.ctypes.data_as(PD),
        mask.ctypes.data, xyz.ctypes.data, ctypes.byref(ng))
    assert mask[n] == 7 and (xyz[n] == 5.0).all(), c.label + ": a write past n"
    return rc, pose, E, mask[:n], xyz[:n], ng.value


def test_host_matches_oracle_bitexact(siftgpu):
    """pose (twelve doubles), E, n_good, every mask byte and every xyz double on every case of
    pose_inputs.cpu_cases; no pose is SIFT_E_INVALID with every output zeroed."""
    got = {}
    assert [c.label for c in I.cpu_cases()] == I.CENSUS
    for c in I.cpu_cases():
        o = c.oracle()
        rc, pose, E, mask, xyz, ng = _host(siftgpu, c)
        print(f"{c.label:16s} n={len(c.src):3d} found={o.found} slot={o.slot} counts={o.counts}")
        assert (rc == 0) == bool(o.found) and (rc in (0, siftgpu.SIFT_E_INVALID)), c.label
        assert pose.tobytes() == o.pose.tobytes(), f"{c.label}: pose {pose} != {o.pose}"
        assert E.tobytes() == o.E.tobytes(), f"{c.label}: E"
        assert ng == o.n_good and mask.tobytes() == o.mask.tobytes(), f"{c.label}: n_good / mask"
        assert xyz.tobytes() == o.xyz.tobytes(), f"{c.label}: xyz"
        if not o.found:
            assert not pose.any() and not E.any() and ng == 0 and not mask.any() and not xyz.any(), c.label
        got[c.label] = o
    # what the cases are there for
    assert {got["scene%d" % k].slot for k in range(I.N_SCENES)} == {0, 1, 2, 3}
    assert all(got["scene%d" % k].n_good == 40 for k in range(I.N_SCENES))
    tie = got["tie"]
    assert sorted(tie.counts)[-2:] == [30, 30] and tie.slot == tie.counts.index(30) and tie.n_good == 30
    ref = got["mask_ones"]
    for label in ("F_1e6", "F_1e-6"):
        assert got[label].slot == ref.slot and got[label].n_good == 60
        assert np.abs(got[label].pose - ref.pose).max() < 1e-9
    assert ref.n_good == 60 and 0 < got["mask_partial"].n_good < 60 and not got["mask_zero"].found
    assert got["same_K"].n_good == 60
    assert got["behind_and_far"].n_good == 60 and sorted(got["behind_and_far"].counts)[-2] == 20
    assert got["thresh_inf"].n_good == 75
    assert got["nan_row"].n_good == 59 and got["nan_row"].mask[7] == 0 and got["inf_row"].n_good == 58
    assert not got["n0"].found and got["n1"].n_good == 1
    for label in ("K_src_singular", "K_dst_singular", "K_nan", "F_zero", "F_nan", "F_inf", "thresh_0", "thresh_neg",
                  "thresh_nan"):
        assert not got[label].found, label
    # the module-level wrapper returns the same
    c = I.cpu_cases()[0]
    R, t, E, mask, xyz, ng = siftgpu.recoverPose(c.F, c.K_src, c.K_dst, c.src, c.dst)
    assert np.c_[R, t].tobytes() == got[c.label].pose.tobytes() and ng == 40
    assert siftgpu.recoverPose(np.zeros((3, 3)), c.K_src, c.K_dst, c.src, c.dst)[0] is None


# ---- planted geometry against an SVD restatement of OpenCV --------------------
def _svd_reference(F, K_src, K_dst, src, dst, mask, thresh):
    """cv::recoverPose + cv::triangulatePoints in numpy (np.linalg.svd for the decomposition and for
    each DLT) -> the four candidates in OpenCV's order, each (count, R, t, good, xyz)."""
    E = K_dst.T @ F @ K_src
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    R1, R2, t = U @ W @ Vt, U @ W.T @ Vt, U[:, 2]
    xs = np.c_[src.astype(np.float64), np.ones(len(src))] @ np.linalg.inv(K_src).T
    xd = np.c_[dst.astype(np.float64), np.ones(len(dst))] @ np.linalg.inv(K_dst).T
    xs, xd = xs[:, :2] / xs[:, 2:], xd[:, :2] / xd[:, 2:]
    P0 = np.c_[np.eye(3), np.zeros(3)]
    rows = np.ones(len(src), bool) if mask is None else mask != 0
    res = []
    for R, tt in ((R1, t), (R2, t), (R1, -t), (R2, -t)):
        P1 = np.c_[R, tt]
        Q = np.zeros((len(src), 4))
        for i in range(len(src)):
            A = np.array([xs[i, 0] * P0[2] - P0[0], xs[i, 1] * P0[2] - P0[1],
                          xd[i, 0] * P1[2] - P1[0], xd[i, 1] * P1[2] - P1[1]])
            Q[i] = np.linalg.svd(A)[2][-1]
        Q = Q / Q[:, 3:]
        z2 = (Q @ P1.T)[:, 2]
        good = rows & (Q[:, 2] > 0) & (Q[:, 2] < thresh) & (z2 > 0) & (z2 < thresh)
        res.append((int(good.sum()), R, tt, good, np.where(good[:, None], Q[:, :3], 0.0)))
    return res


def _slot_map(ref, D):
    """Which of the library's slots each candidate of the reference is.  The four poses are the same
    set, but an SVD routine leaves two signs free -- (u1, v1) against (u2, v2), and which of U and V
    takes the sign of det -- and they decide which pose is called R1 and which way t points: the
    reference's slot numbers are those of numpy's SVD, not of OpenCV's, and not the library's.  So
    slots are compared as poses: candidate j of the reference is slot pi[j] of the library, pi a
    permutation, and all four counts must agree through it."""
    lib = [np.array(P).reshape(3, 4) for P in D["P"]]
    pi = [int(np.argmin([np.abs(np.c_[r[1], r[2]] - P).max() for P in lib])) for r in ref]
    assert sorted(pi) == [0, 1, 2, 3], pi
    return pi


def _planted_inputs():
    """(label, F, K_src, K_dst, src, dst, mask, scene): F exact from the geometry, and F from
    sift_find_fundamental (RANSAC) on pixels with 0.25 px of noise and 30 % outliers."""
    out = []
    for seed in range(300, 308):
        sc = I.scene(seed, 80)
        out.append((f"exact{seed}", sc["F"], sc["K_src"], sc["K_dst"], sc["src"], sc["dst"], None, sc))
    return out


# The largest difference between the host path and the SVD reference over the
# inputs of test_planted_geometry (eight exact scenes, three RANSAC estimates),
# measured on the CPU: R 5.6e-16, t 3.4e-16, xyz 6.1e-14 (the largest coordinate
# difference of a point over max(1, its norm); the points lie 4 to 10 units
# away), |R^T R - I| 6.7e-16.  One bound for all of them: 16 x the largest, the
# margin for seeds not tried (test_rank_two's).  The kernels are bit-equal to the
# host path (test_gpu_pose.py), so the bound binds them too.
MEASURED = 6.1e-14
BOUND = 16 * MEASURED


def test_planted_geometry(siftgpu):
    """Against the SVD restatement of cv::recoverPose + cv::triangulatePoints fed the same F, K,
    points and mask: the winner slot, n_good and the mask are equal; R, t and xyz agree within BOUND;
    det R > 0 and R^T R = I within BOUND; and the pose is the planted one."""
    inputs = _planted_inputs()
    for seed in (60, 61, 62):          # F by RANSAC on noisy pixels with 30 % outliers, K of that scene
        s, d, good = FI.data(seed, 200, 0.3, 0.25)
        F, m = siftgpu.findFundamentalMat(s, d)
        assert F is not None
        inputs.append((f"ransac{seed}", F, FI.K, FI.K, s, d, m,
                       {"R": FI.R_TRUE, "t": FI.T_TRUE / np.linalg.norm(FI.T_TRUE)}))
    worst = {"R": 0.0, "t": 0.0, "xyz": 0.0, "orth": 0.0}
    for label, F, Ks, Kd, s, d, mask, sc in inputs:
        o = PO.recover_pose(F, Ks, Kd, s, d, mask)
        R, t, E, mk, xyz, ng = siftgpu.recoverPose(F, Ks, Kd, s, d, mask)
        assert R is not None and np.c_[R, t].tobytes() == o.pose.tobytes(), label
        ref = _svd_reference(F, Ks, Kd, s, d, mask, 50.0)
        pi = _slot_map(ref, PO.decompose(F, Ks, Kd))
        assert [o.counts[pi[j]] for j in range(4)] == [r[0] for r in ref], label     # all four votes
        rcounts = [r[0] for r in ref]
        assert rcounts.count(max(rcounts)) == 1, label                                 # no tie on these inputs
        slot = pi[rcounts.index(max(rcounts))]
        _, rR, rt, rmask, rxyz = ref[rcounts.index(max(rcounts))]
        assert slot == o.slot and ng == max(rcounts) and mk.astype(bool).tolist() == rmask.tolist(), label
        norm = np.maximum(np.linalg.norm(rxyz, axis=1), 1.0)
        diffs = {"R": np.abs(R - rR).max(), "t": np.abs(t - rt).max(),
                 "xyz": (np.abs(xyz - rxyz).max(axis=1) / norm).max(), "orth": np.abs(R.T @ R - np.eye(3)).max()}
        print(label, "slot", slot, "n_good", ng, {k: f"{v:.3g}" for k, v in diffs.items()},
              "planted R", f"{np.abs(R - sc['R']).max():.3g}", "t", f"{np.abs(t - sc['t']).max():.3g}")
        for k, v in diffs.items():
            worst[k] = max(worst[k], float(v))
            assert v <= BOUND, (label, k, v)
        assert np.linalg.det(R) > 0
        exact = label.startswith("exact")
        assert np.abs(R - sc["R"]).max() < (1e-12 if exact else 2e-2), label
        assert np.abs(t - sc["t"]).max() < (1e-12 if exact else 5e-2), label
        if exact:     # the structure, to the float32 pixel quantum (2^-15 px at 300 px, depth / focal ~ 1e-2)
            assert ng == len(s) and np.abs(xyz - sc["X"]).max() < 5e-3, label
    print("worst", worst, "bound", BOUND)


def test_triangulation(siftgpu):
    """sift_triangulate_points against the oracle bit for bit with cameras that are not [I | 0];
    and against pose recovery: with identity calibrations (normalised points are the float points
    themselves) xyz of a good row is xyzw[:3] / xyzw[3] under [I | 0] and the returned pose."""
    c = I.gpu_call()
    for b in (c.index("n8"), c.index("good_a"), c.index("nan")):
        lo, hi = c.bounds(b)
        got = siftgpu.triangulatePoints(c.P_src[b], c.P_dst[b], c.src[lo:hi], c.dst[lo:hi])
        exp = PO.triangulate_points(c.P_src[b], c.P_dst[b], c.src[lo:hi], c.dst[lo:hi])
        assert got.shape == (hi - lo, 4) and got.tobytes() == exp.tobytes(), c.labels[b]
    assert siftgpu.triangulatePoints(c.P_src[0], c.P_dst[0], c.src[:0], c.dst[:0]).shape == (0, 4)
    eye = np.eye(3)
    sc = I.scene(400, 50, eye, eye)
    R, t, E, mask, xyz, ng = siftgpu.recoverPose(sc["F"], eye, eye, sc["src"], sc["dst"])
    assert ng == 50 and mask.all()
    Q = siftgpu.triangulatePoints(PO.IDENTITY_CAMERA, np.c_[R, t], sc["src"], sc["dst"])
    assert (Q[:, :3] / Q[:, 3:]).tobytes() == xyz.tobytes()
    # a true scene: the points reproject onto their pixels under the cameras that made them
    Ps, Pd = np.c_[sc["K_src"], np.zeros(3)], sc["K_dst"] @ np.c_[sc["R"], sc["t"]]
    Q = siftgpu.triangulatePoints(Ps, Pd, sc["src"], sc["dst"])
    assert np.abs(Q[:, :3] / Q[:, 3:] - sc["X"]).max() < 1e-4


def test_pose_rule_program(tmp_path):
    """tests/cpp/pose_rule.cpp linked with pose.hip alone (host code only), with the address and
    undefined-behaviour sanitizers where the compiler has their runtimes: the sanitizer check of
    the host path, as a program of its own."""
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
    exe = tmp_path / "pose_rule"
    base = [hipcc, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "--offload-host-only", "-x", "hip",
            os.path.join(ROOT, "tests", "cpp", "pose_rule.cpp"),
            os.path.join(ROOT, "sift-gpu_amd", "csrc", "pose.hip"), "-o", str(exe)]
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "pose rule ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_gpu_inputs_census():
    """The committed inputs of the GPU test are what that test needs, counted on the oracle alone."""
    c = I.gpu_call()
    e = I.expected()
    sizes = [c.size(b) for b in range(len(c.labels))]
    assert {0, 1, 8, 255, 256, 257, 600} <= set(sizes)
    assert c.size(c.index("backwards")) == 0 and c.moff[c.index("backwards") + 1] < c.moff[c.index("backwards")]
    assert c.moff[-1] > c.m_cap > c.moff[-2] and len(c.src) == c.moff[-1]
    for bad in ("not_found", "nan", "singular_K"):
        b = c.index(bad)
        assert e["found"][b - 1] == 1 and e["found"][b + 1] == 1, bad
    assert e["found"][c.index("not_found")] == 0 and e["found"][c.index("singular_K")] == 0
    assert np.isnan(c.src[slice(*c.bounds(c.index("nan")))]).any() and e["found"][c.index("nan")] == 1
    assert set(e["slot"]) == {-1, 0, 1, 2, 3}
    assert 0 < e["n_good"][c.index("n600")] < 600          # the mask takes rows out
    assert I.expected(False, 1)["n_good"][c.index("n600")] > e["n_good"][c.index("n600")]
    assert I.expected(True, 0)["found"][c.index("singular_K")] == 1     # segment 0's K serves every segment
