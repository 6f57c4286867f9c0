"""CPU tests of lens undistortion (sift_undistort*, sift_undistort_points*): the rule's header
csrc/undistort_math.hpp compiled on the host (tests/cpp/undistort_rule.cpp, plain and under the
address / undefined-behaviour sanitizers) and the library's host point path, both against the
numpy restatement (tests/undistort_oracle.py) bit for bit over the case tables of
tests/undistort_inputs.py; anchors that need no oracle; planted geometry; the chain undistort ->
fundamental matrix -> pose on the host; and the argument errors that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pose_inputs as PI
import undistort_inputs as I
import undistort_oracle as UO
from conftest import ROOT, assert_bits_equal
from test_abi import HEADER, declared_symbols

f32, f64 = np.float32, np.float64
pdbl = ctypes.POINTER(ctypes.c_double)


def _dp(a):
    return None if a is None else a.ctypes.data_as(pdbl)


def host_points(S, case_or_xy, K, dist, P, iters, stride=8, in_place=False):
    """sift_undistort_points on rows of `stride` bytes -> (rc, rows uint8 [n, stride])."""
    src = I.as_rows(case_or_xy, stride)
    dst = src if in_place else np.full_like(src, 0xCD)
    Kd, dd = np.ascontiguousarray(K, f64).reshape(9), np.ascontiguousarray(dist, f64).reshape(8)
    Pd = None if P is None else np.ascontiguousarray(P, f64).reshape(9)
    n = len(src)
    rc = S.lib().sift_undistort_points(_dp(Kd), _dp(dd), _dp(Pd), iters, src.ctypes.data if n else None,
                                       dst.ctypes.data if n else None, stride, n)
    return rc, dst


# ---- the restatement on hand-written cases ----------------------------------------------------
def test_oracle_forward_then_inverse_is_the_identity_without_distortion():
    xy = I.point_rows(50, 3, special=False)
    out, ok = UO.undistort_points_ref(xy, I.PT_K, I.ZERO, I.PT_K, 5)
    assert ok
    assert_bits_equal(out, xy, "zero distortion, P = K")
    src = I.W.pixels("u8x3", (9, 13), 1)
    assert_bits_equal(UO.undistort_ref(src, I.camera(9, 13), I.ZERO), src, "zero distortion image")


def test_the_case_tables_cover_what_they_should():
    names = [c["name"] for c in I.IMAGE_CASES]
    assert len(names) == len(set(names))
    for kind in I.PIXELS:
        for cam in I.image_cameras(17, 31):
            assert f"{kind}-17x31to17x31-{cam}" in names
    by = {c["name"]: c for c in I.IMAGE_CASES}
    # the denominator is exactly zero on a pixel, and W is exactly zero on a column
    cam = UO.image_camera(*I.image_cameras(17, 31)["den_zero"])
    x, y = UO.project(cam[0], np.arange(31.0)[None, :], np.arange(17.0)[:, None])
    assert (UO.terms(cam[2], x + 0 * y, y + 0 * x)[1] == 0).any()
    Ni = UO.image_camera(*I.image_cameras(17, 31)["w_zero"])[0]
    assert ((Ni[6] * np.arange(31.0) + Ni[8]) == 0).sum() == 1
    # partly and wholly outside, and the cameras with no rule
    part = I.expected_image(by["u8-17x31to17x31-partly_outside"])
    assert part.any() and not part[:, -8:].any()
    assert not I.expected_image(by["u8-17x31to17x31-wholly_outside"]).any()
    for cam in I.NO_RULE:
        assert UO.image_camera(*I.image_cameras(17, 31)[cam]) is None, cam
        assert not I.expected_image(by[f"f32-17x31to17x31-{cam}"]).any()
    assert any(c["out_shape"] != c["src"].shape[:2] for c in I.IMAGE_CASES)
    drawn = sum(bool(np.any(I.expected_image(c).view(np.uint8))) for c in I.IMAGE_CASES)
    assert drawn > len(I.IMAGE_CASES) * 0.6
    # points: every iteration count, P absent / K / general, n = 0 and 1, NaN and infinite rows
    pn = [c["name"] for c in I.POINT_CASES]
    assert {f"barrel-it{k}" for k in I.ITERS} <= set(pn) and {"n0", "n1"} <= set(pn)
    assert any(c["P"] is None for c in I.POINT_CASES) and any(c["P"] is I.GENERAL_P for c in I.POINT_CASES)
    xy = I.POINT_CASES[0]["xy"]
    assert np.isnan(xy).any() and np.isinf(xy).any()
    for cam in I.PT_NO_RULE:
        e, ok = I.expected_points(next(c for c in I.POINT_CASES if c["name"].startswith(cam)))
        assert not ok and not e.any()
    e, ok = I.expected_points(next(c for c in I.POINT_CASES if c["name"] == "barrel-it5"))
    assert ok and np.isnan(e[1]).all() and np.isfinite(e[8:]).all()       # a NaN row harms no other


# ---- the header on the host against the restatement ------------------------------------------
def _build_rule(tmp_path, sanitize):
    src = os.path.join(ROOT, "tests", "cpp", "undistort_rule.cpp")
    exe = tmp_path / ("undistort_rule_san" if sanitize else "undistort_rule")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", src,
           "-o", str(exe)]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    return exe if r.returncode == 0 else None, r.stderr


_TABLE = I.rule_table()


def _run_rule(exe, tmp_path):
    cases, results = tmp_path / "cases.bin", tmp_path / "results.bin"
    I.write_cases(cases, _TABLE)
    r = subprocess.run([str(exe), str(cases), str(results)], capture_output=True, text=True)
    assert r.returncode == 0 and f"undistort rule ok: {len(_TABLE)} cases" in r.stdout, \
        r.stdout[-2000:] + r.stderr[-2000:]
    return I.read_results(results, _TABLE)


def _compare(results):
    for e, (ok, got) in zip(_TABLE, results):
        if e[0] == "image":
            c = e[1]
            assert ok == int(UO.image_camera(c["K"], c["dist"], c["newK"]) is not None), c["name"]
            assert_bits_equal(UO.canonical(got), UO.canonical(I.expected_image(c)), c["name"])
        else:
            _, c, stride, in_place = e
            what = f"{c['name']} stride {stride} in_place {in_place}"
            assert ok == int(I.expected_points(c)[1]), what
            want = I.expected_rows(c, stride, in_place)
            assert_bits_equal(UO.canonical(I.rows_xy(got)), UO.canonical(I.rows_xy(want)), what)
            assert_bits_equal(got[:, 8:], want[:, 8:], what + ": the other bytes of a row")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitized"])
def test_header_on_the_host_equals_the_restatement(tmp_path, sanitize):
    """Fails to build before csrc/undistort_math.hpp exists.  The sanitized build links the address
    and undefined-behaviour runtimes statically into the stand-alone program (nothing sanitised is
    loaded into Python); where the host compiler lacks them it is the plain build again."""
    exe, err = _build_rule(tmp_path, sanitize)
    if exe is None and sanitize:
        exe, err = _build_rule(tmp_path, False)
    assert exe is not None, err[-3000:]
    _compare(_run_rule(exe, tmp_path))


def test_the_warp_keeps_its_split(tmp_path):
    """source_coord of warp_math.hpp now ends in split_coord, which undistortion shares."""
    text = open(os.path.join(ROOT, "sift-gpu_amd", "csrc", "warp_math.hpp")).read()
    assert "return split_coord(fX, fY);" in text and "32.0 / Wd" in text


# ---- the library's host point path against the restatement ---------------------------------
@pytest.mark.parametrize("stride,in_place", [(8, False), (8, True), (I.KP_STRIDE, False), (I.KP_STRIDE, True)])
def test_host_point_path_equals_the_restatement(siftgpu, stride, in_place):
    for c in I.POINT_CASES:
        rc, rows = host_points(siftgpu, c["xy"], c["K"], c["dist"], c["P"], c["iters"], stride, in_place)
        want, ok = I.expected_points(c)
        assert rc == (siftgpu.SIFT_OK if ok else siftgpu.SIFT_E_INVALID), c["name"]
        assert_bits_equal(UO.canonical(I.rows_xy(rows)), UO.canonical(want), c["name"])
        assert (rows[:, 8:] == (0x5A if in_place else 0xCD)).all(), c["name"]


# ---- anchors that need no oracle ---------------------------------------------------------------
def test_zero_distortion_with_P_equal_K_reproduces_the_input_floats(siftgpu):
    xy = I.point_rows(300, 8, special=False)
    for iters in I.ITERS:
        assert_bits_equal(siftgpu.undistortPoints(xy, I.PT_K, I.ZERO, I.PT_K, iters), xy, f"iters {iters}")
    kp = np.zeros(300, siftgpu.KEYPOINT_DTYPE)
    kp["x"], kp["y"], kp["size"], kp["octave"] = xy[:, 0], xy[:, 1], 3.5, 7
    out = siftgpu.undistortPoints(kp, I.PT_K, np.zeros(4), I.PT_K)
    assert out.tobytes() == kp.tobytes()


def test_zero_distortion_with_newK_equal_K_reproduces_the_source_bytes(tmp_path):
    table = [("image", c) for c in I.IMAGE_CASES
             if c["name"] in ("f32-17x31to17x31-zero_newK_is_K", "u8x3-17x31to17x31-zero_newK_is_K",
                              "f32-17x31to17x31-zero", "u8x3-17x31to17x31-zero")]
    assert len(table) == 4
    exe, err = _build_rule(tmp_path, False)
    assert exe is not None, err[-3000:]
    cases, results = tmp_path / "anchor.bin", tmp_path / "anchor_out.bin"
    I.write_cases(cases, table)
    subprocess.run([str(exe), str(cases), str(results)], check=True, capture_output=True)
    for (_, c), (ok, img) in zip(table, I.read_results(results, table)):
        assert ok == 1
        assert_bits_equal(img, c["src"], c["name"])


# ---- planted geometry ------------------------------------------------------------------------
# The largest distance, in pixels, between a planted ideal point and what five iterations give
# back from its distorted float pixel (400 points over a 640 x 480 frame, f = 576; the distorted
# pixel's rounding to float, about 3e-5 pixels, is part of it), measured on this code, and the
# bound asserted: 16 x that.
#   mild   (|k1| = 0.1, points moved by up to 13.5 px): 5.3e-5 px (barrel), 5.8e-5 px (pincushion)
#   strong (|k1| = 0.3, points moved by up to 39.3 px): 3.6e-2 px (barrel), 1.2e-2 px (pincushion)
PLANTED = {"mild": (0.1, 5.84e-5, 16 * 5.84e-5), "strong": (0.3, 3.61e-2, 16 * 3.61e-2)}


@pytest.mark.parametrize("sign", [-1, 1], ids=["barrel", "pincushion"])
@pytest.mark.parametrize("level", ["mild", "strong"])
def test_planted_points_come_back(siftgpu, level, sign):
    k1, _, bound = PLANTED[level]
    ideal, distorted, d = I.planted(sign * k1)
    back = siftgpu.undistortPoints(distorted, I.PT_K, d, I.PT_K, 5)
    err = float(np.abs(back.astype(f64) - ideal).max())
    moved = float(np.abs(distorted.astype(f64) - ideal).max())
    print(f"planted {level} k1 {sign * k1:+}: moved by up to {moved:.3g} px, error after 5 iterations {err:.3g} px")
    assert moved > 5.0 and err < bound
    # more iterations do not make it worse, and none at all leaves the distortion in
    e0 = float(np.abs(siftgpu.undistortPoints(distorted, I.PT_K, d, I.PT_K, 0).astype(f64) - ideal).max())
    e100 = float(np.abs(siftgpu.undistortPoints(distorted, I.PT_K, d, I.PT_K, 100).astype(f64) - ideal).max())
    assert e0 == pytest.approx(moved, rel=1e-6) and e100 <= err * 1.0001 + 1e-4


# ---- the chain on the host --------------------------------------------------------------------
def _angle(a, b):
    return float(np.degrees(np.arccos(np.clip(np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b)), -1, 1))))


def _rot_angle(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1) / 2, -1, 1))))


def chain_scene(n=300, seed=3):
    """Two views of a planted scene through one distorting lens (k1 = -0.12): the distorted pixel rows."""
    rng = np.random.default_rng(seed)
    R = PI._rotation(np.array([0.2, 1.0, 0.1]), np.deg2rad(8.0))
    t = np.array([-1.0, 0.05, 0.1])
    t /= np.linalg.norm(t)
    X = PI._box_under(rng, n, R, t)
    d = I.dist8(k1=-0.12, k2=0.02, p1=5e-4, p2=-3e-4)
    rows = []
    for Xc in (X, X @ R.T + t):
        xd, yd = UO.distort(d, Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2])
        p = np.c_[xd, yd, np.ones(n)] @ I.PT_K.T
        rows.append((p[:, :2] / p[:, 2:]).astype(f32))
    return dict(R=R, t=t, d=d, src=rows[0], dst=rows[1])


def run_chain(siftgpu, src, dst):
    """-> (n_good, degrees to the planted R, degrees to the planted t) of estimate + pose on these rows."""
    sc = chain_scene()
    F, mask = siftgpu.findFundamentalMat(src, dst, 3.0, 1000, 0.99)
    assert F is not None
    R, t, _, _, _, n_good = siftgpu.recoverPose(F, I.PT_K, I.PT_K, src, dst, mask)
    assert R is not None
    return n_good, _rot_angle(R, sc["R"]), _angle(t, sc["t"])


def test_chain_on_the_host_is_at_least_as_good_with_undistortion(siftgpu):
    sc = chain_scene()
    raw = run_chain(siftgpu, sc["src"], sc["dst"])
    und = run_chain(siftgpu, siftgpu.undistortPoints(sc["src"], I.PT_K, sc["d"], I.PT_K),
                    siftgpu.undistortPoints(sc["dst"], I.PT_K, sc["d"], I.PT_K))
    print(f"chain: distorted rows n_good {raw[0]}, R off {raw[1]:.4f} deg, t off {raw[2]:.4f} deg; "
          f"undistorted rows n_good {und[0]}, R off {und[1]:.4f} deg, t off {und[2]:.4f} deg")
    assert raw[0] > 0                                    # the distorted run still finds a pose
    assert und[0] >= raw[0] and und[1] <= raw[1] and und[2] <= raw[2]
    assert und[0] == len(sc["src"]) and und[1] < 0.05 and und[2] < 0.5


# ---- the entry points ---------------------------------------------------------------------------
NEW = ["sift_undistort_batch_device", "sift_undistort", "sift_undistort_points",
       "sift_undistort_points_segmented_device", "sift_undistort_points_segmented"]


def test_header_declares_the_entry_points_and_states_the_rule():
    assert set(NEW) <= set(declared_symbols())
    text = open(HEADER).read()
    for phrase in ("num = 1 + ((k3 r2 + k2) r2 + k1) r2", "den = 1 + ((k6 r2 + k5) r2 + k4) r2",
                   "dx = ((2 p1) x) y + p2 (r2 + 2 xx)", "icd = den / num", "not bit-compatible with OpenCV",
                   "k_per_segment"):
        assert phrase in text, phrase
    rule = open(os.path.join(ROOT, "sift-gpu_amd", "csrc", "undistort_math.hpp")).read()
    assert "not bit-compatible with OpenCV" in rule and not re.search(r"\b(sqrt|pow|exp|log|sin|cos|atan)\s*\(", rule)


def test_library_exports_the_entry_points_and_rejects_bad_arguments(siftgpu):
    L = siftgpu.lib()
    assert all(hasattr(L, s) for s in NEW)
    E = siftgpu.SIFT_E_INVALID
    src, dst = np.zeros((2, 2), f32), np.full((2, 2), 5.0, f32)
    K, d = np.eye(3), np.zeros(8)
    # a NULL context is SIFT_E_INVALID whatever else is passed (no device needed), and nothing is written
    assert L.sift_undistort(None, 0, 1, src.ctypes.data, 2, 2, 0, _dp(K), _dp(d), None, dst.ctypes.data, 2, 2) == E
    assert L.sift_undistort_batch_device(None, 0, 1, None, 2, 2, 0, 0, None, None, None, 0, 1, None, 2, 2, 0, 0) == E
    assert L.sift_undistort_batch_device(None, 0, 1, None, 2, 2, 0, 0, None, None, None, 0, 0, None, 2, 2, 0, 0) == E
    assert L.sift_undistort_points_segmented_device(None, None, None, 8, None, 1, 1, None, None, None, 0, 5, None) == E
    assert L.sift_undistort_points_segmented(None, None, None, 8, None, 1, 1, None, None, None, 0, 5, None) == E
    assert (dst == 5.0).all()
    # the host point call: iters, strides, NULL buffers; nothing is written
    xy = I.point_rows(4, 1, special=False)
    for iters in (-1, 101):
        rc, rows = host_points(siftgpu, xy, I.PT_K, I.ZERO, None, iters)
        assert rc == E and (rows == 0xCD).all(), iters
    buf = np.full((4, 8), 0xCD, np.uint8)
    for stride in (4, 0, 10, 7):
        assert L.sift_undistort_points(_dp(np.eye(3)), _dp(d), None, 5, xy.ctypes.data, buf.ctypes.data, stride, 4) == E
    assert L.sift_undistort_points(None, _dp(d), None, 5, xy.ctypes.data, buf.ctypes.data, 8, 4) == E
    assert L.sift_undistort_points(_dp(np.eye(3)), None, None, 5, xy.ctypes.data, buf.ctypes.data, 8, 4) == E
    assert L.sift_undistort_points(_dp(np.eye(3)), _dp(d), None, 5, None, buf.ctypes.data, 8, 4) == E
    assert L.sift_undistort_points(_dp(np.eye(3)), _dp(d), None, 5, xy.ctypes.data, buf.ctypes.data, 8, -1) == E
    assert (buf == 0xCD).all()
    assert L.sift_undistort_points(_dp(np.eye(3)), _dp(d), None, 5, None, None, 8, 0) == siftgpu.SIFT_OK


def test_python_interface(siftgpu):
    for name in ("undistort", "undistort_batch_device", "undistort_points_segmented_device", "undistortPointsSegmented"):
        assert callable(getattr(siftgpu.Context, name, None)), name
    assert callable(siftgpu.undistort) and callable(siftgpu.undistortPoints)
    # argument errors raised before any library call (no device needed)
    with pytest.raises(ValueError):
        siftgpu.undistortPoints(np.zeros((2, 2), f32), np.eye(3), np.zeros(9))
    with pytest.raises(ValueError):
        siftgpu.undistortPoints(np.zeros((2, 2), f32), np.eye(3), np.zeros(5), iters=101)
    with pytest.raises(siftgpu.SiftError):
        siftgpu.undistortPoints(np.zeros((2, 2), f32), np.zeros((3, 3)), np.zeros(5))
    # fewer than eight coefficients are padded with zeros; normalised output with P absent
    out = siftgpu.undistortPoints(np.array([[I.PT_K[0, 2], I.PT_K[1, 2]]], f32), I.PT_K, [-0.2, 0.05])
    assert np.abs(out).max() < 1e-6
