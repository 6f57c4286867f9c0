"""CPU restatement of sift_estimate_affine (estimateAffine2D /
estimateAffinePartial2D by RANSAC) as sift-gpu_amd/csrc/affine_math.hpp states
it, for checking the host path and the kernel value for value.

TEST INFRASTRUCTURE ONLY (tests import it; the product never does).  It lives
under tests/ because oracle/ is frozen; RNG, update_num_iters and the constants
are oracle/homography.py's.

The rule is RANSACPointSetRegistrator::run with m model points in place of 4
(AFFINE m = 3, SIMILARITY m = 2): n < m none; n == m a direct fit, no subset
check, a mask of ones; else RNG(~0), subsets of m distinct rows until the
subset check accepts one (10000 attempts), a closed-form minimal solve in
double, the float inlier test of Affine2DEstimatorCallback::computeError, a win
iff good > max(max_good, m - 1), update_num_iters after each win; then the
ordinary least-squares refit on the best hypothesis's inliers (centred double
sums in pair order, closed form), which stands in for OpenCV's 10 LMSolver
iterations because the residual is linear in the parameters.  Not
bit-compatible with OpenCV.  Python floats are IEEE doubles without fusing and
numpy float32 element-wise ops are unfused floats, so results compare bit for
bit.
"""
from __future__ import annotations

import math

import numpy as np

import homography as HO

AFFINE, SIMILARITY = 0, 1
DBL_MAX = float(np.finfo(np.float64).max)
MAX_ATTEMPTS = 10000


def model_points(model):
    return 3 if model == AFFINE else 2


def _finite6(A):
    return all(abs(a) <= DBL_MAX for a in A)      # False for NaN and inf


def _collinear3(p):
    dx1, dy1 = p[1][0] - p[2][0], p[1][1] - p[2][1]
    dx2, dy2 = p[0][0] - p[2][0], p[0][1] - p[2][1]
    return abs(dx2 * dy1 - dy2 * dx1) <= HO.FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2))


def check_subset(model, s, d):
    if model == AFFINE:
        return not _collinear3(s) and not _collinear3(d)
    return not (s[0][0] == s[1][0] and s[0][1] == s[1][1])


def _det3c(a0, a1, a2, b0, b1, b2, c0, c1, c2):
    return a0 * (b1 * c2 - c1 * b2) - a1 * (b0 * c2 - c0 * b2) + a2 * (b0 * c1 - b1 * c0)


def solve_minimal(model, s, d):
    """The six coefficients from the first m points, or None."""
    if model == AFFINE:
        (x0, y0), (x1, y1), (x2, y2) = s[0], s[1], s[2]
        (X0, Y0), (X1, Y1), (X2, Y2) = d[0], d[1], d[2]
        det = HO._det3(x0, y0, x1, y1, x2, y2)
        if det == 0:
            return None
        A = [HO._det3(X0, y0, X1, y1, X2, y2) / det, HO._det3(x0, X0, x1, X1, x2, X2) / det,
             _det3c(x0, y0, X0, x1, y1, X1, x2, y2, X2) / det,
             HO._det3(Y0, y0, Y1, y1, Y2, y2) / det, HO._det3(x0, Y0, x1, Y1, x2, Y2) / det,
             _det3c(x0, y0, Y0, x1, y1, Y1, x2, y2, Y2) / det]
    else:
        (x0, y0), (X0, Y0) = s[0], d[0]
        dx, dy, dX, dY = s[1][0] - x0, s[1][1] - y0, d[1][0] - X0, d[1][1] - Y0
        den = dx * dx + dy * dy
        if den == 0:
            return None
        a, b = (dX * dx + dY * dy) / den, (dY * dx - dX * dy) / den
        A = [a, -b, X0 - (a * x0 - b * y0), b, a, Y0 - (b * x0 + a * y0)]
    return A if _finite6(A) else None


def find_inliers(src, dst, A, thr):
    """computeError + the inlier test in float32 -> (mask, count)."""
    with np.errstate(over="ignore", invalid="ignore"):
        f = [np.float32(a) for a in A]
        x, y, X, Y = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
        a = f[0] * x + f[1] * y + f[2] - X
        b = f[3] * x + f[4] * y + f[5] - Y
        mask = (a * a + b * b <= np.float32(thr * thr)).astype(np.uint8)
    return mask, int(mask.sum())


def refit(model, s, d, mask, A):
    """The least-squares fit on the inliers, or A when it is singular or non-finite."""
    rows = [i for i in range(len(s)) if mask[i]]
    c = [0.0] * 4
    for i in rows:
        c[0] += s[i][0]
        c[1] += s[i][1]
        c[2] += d[i][0]
        c[3] += d[i][1]
    c = [v / len(rows) for v in c]
    S = [0.0] * (7 if model == AFFINE else 3)
    for i in rows:
        u, v, U, V = s[i][0] - c[0], s[i][1] - c[1], d[i][0] - c[2], d[i][1] - c[3]
        if model == AFFINE:
            t = (u * u, u * v, v * v, u * U, v * U, u * V, v * V)
        else:
            t = (u * u + v * v, u * U + v * V, u * V - v * U)
        for k in range(len(S)):
            S[k] += t[k]
    R = [0.0] * 6
    if model == AFFINE:
        det = S[0] * S[2] - S[1] * S[1]
        if det == 0:
            return A
        R[0] = (S[3] * S[2] - S[4] * S[1]) / det
        R[1] = (S[0] * S[4] - S[1] * S[3]) / det
        R[3] = (S[5] * S[2] - S[6] * S[1]) / det
        R[4] = (S[0] * S[6] - S[1] * S[5]) / det
    else:
        if S[0] == 0:
            return A
        a, b = S[1] / S[0], S[2] / S[0]
        R[0], R[1], R[3], R[4] = a, -b, b, a
    R[2] = c[2] - (R[0] * c[0] + R[1] * c[1])
    R[5] = c[3] - (R[3] * c[0] + R[4] * c[1])
    return R if _finite6(R) else A


def estimate_affine(src, dst, model, thr=3.0, max_iters=2000, confidence=0.99):
    """-> (A as 6 floats or None, inlier mask uint8[n])."""
    src = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
    dst = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
    n = len(src)
    none = (None, np.zeros(n, np.uint8))
    if model not in (AFFINE, SIMILARITY):
        return none
    m = model_points(model)
    if n < m or not (0 < confidence < 1) or max_iters < 1:
        return none
    s = [(float(a), float(b)) for a, b in src]
    d = [(float(a), float(b)) for a, b in dst]
    if n == m:
        best = solve_minimal(model, s, d)
        if best is None:
            return none
        return best, np.ones(n, np.uint8)
    rng = HO.RNG()
    niters, max_good, best, best_mask = max_iters, 0, None, np.zeros(n, np.uint8)
    it = 0
    while it < niters:
        idx = [0] * m
        ok_subset = False
        for _attempt in range(MAX_ATTEMPTS):
            ms, md = [], []
            for i in range(m):
                while True:
                    idx[i] = rng.uniform(0, n)
                    if idx[i] not in idx[:i]:
                        break
                ms.append(s[idx[i]])
                md.append(d[idx[i]])
            if check_subset(model, ms, md):
                ok_subset = True
                break
        if not ok_subset:
            break
        A = solve_minimal(model, ms, md)
        it += 1
        if A is None:
            continue
        mask, good = find_inliers(src, dst, A, thr)
        if good > max(max_good, m - 1):
            best_mask, best, max_good = mask, A, good
            niters = HO.update_num_iters(confidence, (n - good) / n, m, niters)
    if max_good <= 0:
        return none
    return refit(model, s, d, best_mask, best), best_mask


def as_h(A):
    """The nine doubles the segmented forms write: A's rows, then 0 0 1 (zeros for none)."""
    return np.zeros(9) if A is None else np.array(list(A) + [0.0, 0.0, 1.0], np.float64)
