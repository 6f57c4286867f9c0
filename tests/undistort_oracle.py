"""The rule of sift_undistort[_batch_device] and sift_undistort_points[_segmented[_device]]
(include/sift_hip.h, csrc/undistort_math.hpp) restated in numpy: float64 element by element in the
header's operation order (numpy fuses nothing), np.rint for the ties, and the warp's own second
half (tests/warp_inputs.py: samples outside are 0, the float32 blend as four products and three
sums, the uint8 blend in integers).  The calibration inverse is tests/pose_oracle.py's invert3.
Every comparison made with it is bit for bit; NaN is compared as "a NaN, here".

It is the library's own statement of cv::undistort / cv::undistortPoints for the 8-coefficient
rational model (k1 k2 p1 p2 k3 k4 k5 k6), not OpenCV's bits."""
import numpy as np

import pose_oracle as PO
import warp_inputs as W

f32, f64 = np.float32, np.float64
INT_MIN, INT_MAX = -2147483648.0, 2147483647.0


def _finite(a):
    return bool(np.all(np.isfinite(np.asarray(a, f64))))


def terms(d, x, y):
    """(num, den, dx, dy) at normalised (x, y) arrays."""
    d = [f64(v) for v in d]
    two = f64(2.0)
    with np.errstate(all="ignore"):
        xx, yy = x * x, y * y
        r2 = xx + yy
        num = f64(1.0) + ((d[4] * r2 + d[1]) * r2 + d[0]) * r2
        den = f64(1.0) + ((d[7] * r2 + d[6]) * r2 + d[5]) * r2
        dx = ((two * d[2]) * x) * y + d[3] * (r2 + two * xx)
        dy = d[2] * (r2 + two * yy) + ((two * d[3]) * x) * y
    return num, den, dx, dy


def distort(d, x, y):
    """The forward model: normalised ideal (x, y) -> normalised distorted (xd, yd)."""
    num, den, dx, dy = terms(d, x, y)
    with np.errstate(all="ignore"):
        s = num / den
        return x * s + dx, y * s + dy


def project(A, u, v):
    A = [f64(a) for a in np.asarray(A, f64).reshape(9)]
    with np.errstate(all="ignore"):
        X = (A[0] * u + A[1] * v) + A[2]
        Y = (A[3] * u + A[4] * v) + A[5]
        Wh = (A[6] * u + A[7] * v) + A[8]
        return X / Wh, Y / Wh


def image_camera(K, dist, newK=None):
    """(newK^-1, K, dist) as lists, or None where the image undistorts to zeros."""
    if not _finite(K) or not _finite(dist):
        return None
    Ki = PO.invert3(K)
    if Ki is None:
        return None
    Ni = Ki
    if newK is not None:
        if not _finite(newK):
            return None
        Ni = PO.invert3(newK)
        if Ni is None:
            return None
    return Ni, [f64(v) for v in np.asarray(K, f64).reshape(9)], [f64(v) for v in np.asarray(dist, f64).reshape(8)]


def source_coords(cam, out_rows, out_cols):
    """(sx, ax, sy, ay, valid) of every destination pixel, [out_rows, out_cols] each."""
    Ni, K, d = cam
    u = np.broadcast_to(np.arange(out_cols, dtype=f64)[None, :], (out_rows, out_cols))
    v = np.broadcast_to(np.arange(out_rows, dtype=f64)[:, None], (out_rows, out_cols))
    x, y = project(Ni, u, v)
    xd, yd = distort(d, x, y)
    with np.errstate(all="ignore"):
        Wd = (K[6] * xd + K[7] * yd) + K[8]
        fX = (f64(32.0) * ((K[0] * xd + K[1] * yd) + K[2])) / Wd
        fY = (f64(32.0) * ((K[3] * xd + K[4] * yd) + K[5])) / Wd
    valid = ~(np.isnan(fX) | np.isnan(fY))
    X = np.rint(np.clip(np.where(valid, fX, 0.0), INT_MIN, INT_MAX)).astype(np.int64)
    Y = np.rint(np.clip(np.where(valid, fY, 0.0), INT_MIN, INT_MAX)).astype(np.int64)
    return X >> 5, X & 31, Y >> 5, Y & 31, valid


def undistort_ref(src, K, dist, newK=None, out_shape=None):
    """src float32 [rows, cols] or uint8 [rows, cols] / [rows, cols, 3] -> [out_rows, out_cols(, 3)]."""
    src = np.asarray(src)
    out_rows, out_cols = src.shape[:2] if out_shape is None else out_shape
    out = np.zeros((out_rows, out_cols) + src.shape[2:], src.dtype)
    cam = image_camera(K, dist, newK)
    if cam is None:
        return out
    sx, ax, sy, ay, valid = source_coords(cam, out_rows, out_cols)
    v00, v01 = W._sample(src, sy, sx), W._sample(src, sy, sx + 1)
    v10, v11 = W._sample(src, sy + 1, sx), W._sample(src, sy + 1, sx + 1)
    if src.dtype == f32:
        fx, fy = ax.astype(f32) * f32(0.03125), ay.astype(f32) * f32(0.03125)
        one = f32(1.0)
        w00, w01, w10, w11 = (one - fy) * (one - fx), (one - fy) * fx, fy * (one - fx), fy * fx
        with np.errstate(all="ignore"):
            val = ((v00 * w00 + v01 * w01) + v10 * w10) + v11 * w11
        assert val.dtype == f32
        return np.where(valid, val, f32(0.0))
    assert src.dtype == np.uint8
    if src.ndim == 3:
        ax, ay, valid = ax[..., None], ay[..., None], valid[..., None]
    k00, k01, k10, k11 = (32 - ay) * (32 - ax), (32 - ay) * ax, ay * (32 - ax), ay * ax
    val = (v00.astype(np.int64) * k00 + v01.astype(np.int64) * k01 + v10.astype(np.int64) * k10 +
           v11.astype(np.int64) * k11 + 512) >> 10
    return np.where(valid, val, 0).astype(np.uint8)


def undistort_points_ref(xy, K, dist, P=None, iters=5):
    """xy float32 [n, 2] -> (float32 [n, 2], ok).  ok False: zeros."""
    xy = np.ascontiguousarray(xy, f32).reshape(-1, 2)
    bad = np.zeros_like(xy), False
    if not _finite(K) or not _finite(dist) or (P is not None and not _finite(P)):
        return bad
    Ki = PO.invert3(K)
    if Ki is None:
        return bad
    d = [f64(v) for v in np.asarray(dist, f64).reshape(8)]
    x0, y0 = project(Ki, xy[:, 0].astype(f64), xy[:, 1].astype(f64))
    x, y = x0, y0
    for _ in range(iters):
        num, den, dx, dy = terms(d, x, y)
        with np.errstate(all="ignore"):
            icd = den / num
            x, y = (x0 - dx) * icd, (y0 - dy) * icd
    if P is not None:
        x, y = project(P, x, y)
    with np.errstate(all="ignore"):
        return np.stack([x.astype(f32), y.astype(f32)], axis=1), True


def canonical(a):
    """a with every float32 NaN replaced by one NaN (tests/warp_inputs.py canonical: the sign and
    payload of a NaN result are open in IEEE 754)."""
    return W.canonical(a)
