"""CPU restatement of sift_recover_pose and sift_triangulate_points (recoverPose
with its cheirality test, triangulatePoints by DLT) as
sift-gpu_amd/csrc/pose_math.hpp states them, for checking the host path and the
kernels value for value.

TEST INFRASTRUCTURE ONLY (tests import it; the product never does).  It lives
under tests/ because oracle/ is frozen.

Convention: src is image 1, dst image 2, [dst; 1]^T F [src; 1] = 0, X_dst = R
X_src + t, E ~ [t]x R; matrices row-major.  The rule:

1. K^-1 = adj(K) / det(K); a zero or non-finite determinant or a non-finite
   entry: no pose.  A pixel becomes K^-1 (x, y, 1)^T divided by its third
   component.
2. E0 = K_dst^T (F K_src); the eigenpairs of E0^T E0 by the cyclic Jacobi of
   homography_math.hpp, ordered sigma_1^2 >= sigma_2^2 >= sigma_3^2 by three
   compare-exchanges; a non-finite sigma^2 or sigma_2^2 <= 0: no pose.  u1 = E0
   v1 / sigma_1, u2 = E0 v2 / sigma_2, u3 = u1 x u2, v3 negated when det [v1 v2
   v3] < 0; E = ((sigma_1 + sigma_2) / 2) (u1 v1^T + u2 v2^T).
3. R1 = U W V^T, R2 = U W^T V^T, t = u3; candidates (R1, +t), (R2, +t), (R1, -t),
   (R2, -t).
4. DLT: rows x P_src[2] - P_src[0], y P_src[2] - P_src[1], X P_dst[2] - P_dst[0],
   Y P_dst[2] - P_dst[1]; Q = the eigenvector of A^T A's smallest eigenvalue.
5. A considered row (mask_in None or non-zero) is good iff 0 < z < thresh for
   Q[2] / Q[3] and for (P_dst Q / Q[3])[2]; the winner is the first candidate with
   the largest count; a pose iff that count >= 1 (and thresh > 0).

The Jacobi runs over a whole batch of matrices at once: numpy float64
element-wise operations are unfused IEEE doubles, a matrix that has left the
sweep loop is frozen by a mask, and a skipped rotation likewise, so every matrix
sees exactly the statements of smallest_eigvec / sym_eig in their order, and
results compare bit for bit.  Not bit-compatible with OpenCV.
"""
from __future__ import annotations

import math

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
SLOTS = 4


def _finite(a):
    return all(abs(v) <= DBL_MAX for v in a)      # False for NaN and inf


def jacobi_batch(A):
    """The sweeps of smallest_eigvec / sym_eig on A [n, N, N] (float64, modified in place) -> V [n, N, N]."""
    n, N = A.shape[0], A.shape[1]
    V = np.tile(np.eye(N), (n, 1, 1))
    active = np.ones(n, bool)
    with np.errstate(all="ignore"):
        for _ in range(60):
            off = np.zeros(n)
            for i in range(N):
                for j in range(i + 1, N):
                    off = off + A[:, i, j] * A[:, i, j]
            active &= ~(off < 1e-300)
            if not active.any():
                break
            for p in range(N):
                for q in range(p + 1, N):
                    apq = A[:, p, q].copy()
                    do = (active & ~(np.abs(apq) < 1e-300))[:, None]
                    th = (A[:, q, q] - A[:, p, p]) / (2 * apq)
                    t = np.where(th >= 0, 1.0, -1.0) / (np.abs(th) + np.sqrt(th * th + 1))
                    c = 1 / np.sqrt(t * t + 1)
                    s = (t * c)[:, None]
                    c = c[:, None]
                    cp, cq = A[:, :, p].copy(), A[:, :, q].copy()
                    A[:, :, p] = np.where(do, c * cp - s * cq, cp)
                    A[:, :, q] = np.where(do, s * cp + c * cq, cq)
                    rp, rq = A[:, p, :].copy(), A[:, q, :].copy()
                    A[:, p, :] = np.where(do, c * rp - s * rq, rp)
                    A[:, q, :] = np.where(do, s * rp + c * rq, rq)
                    vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p] = np.where(do, c * vp - s * vq, vp)
                    V[:, :, q] = np.where(do, s * vp + c * vq, vq)
    return V


def smallest_eigvec_batch(A):
    """-> [n, N]: the column of V at the first smallest diagonal entry."""
    V = jacobi_batch(A)
    N = A.shape[1]
    least, v = A[:, 0, 0].copy(), V[:, :, 0].copy()
    for i in range(1, N):
        less = A[:, i, i] < least
        least = np.where(less, A[:, i, i], least)
        v = np.where(less[:, None], V[:, :, i], v)
    return v


def invert3(K):
    K = [float(v) for v in np.asarray(K, np.float64).reshape(9)]
    c = [K[4] * K[8] - K[5] * K[7], K[2] * K[7] - K[1] * K[8], K[1] * K[5] - K[2] * K[4],
         K[5] * K[6] - K[3] * K[8], K[0] * K[8] - K[2] * K[6], K[2] * K[3] - K[0] * K[5],
         K[3] * K[7] - K[4] * K[6], K[1] * K[6] - K[0] * K[7], K[0] * K[4] - K[1] * K[3]]
    det = K[0] * c[0] + K[1] * c[3] + K[2] * c[6]
    if not (abs(det) > 0 and abs(det) <= DBL_MAX):
        return None
    Ki = [v / det for v in c]
    return Ki if _finite(Ki) else None


def normalise(Ki, pts):
    """pts float32 [n, 2] -> (x, y) float64 arrays."""
    px, py = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        w = Ki[6] * px + Ki[7] * py + Ki[8]
        return (Ki[0] * px + Ki[1] * py + Ki[2]) / w, (Ki[3] * px + Ki[4] * py + Ki[5]) / w


def _mat3mul(a, b):
    return [a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j] for i in range(3) for j in range(3)]


def decompose(F, K_src, K_dst):
    """Steps 1 to 3 -> dict(Kis, Kid, E [9], P [4][12], u3, sigma) or None."""
    Kis, Kid = invert3(K_src), invert3(K_dst)
    if Kis is None or Kid is None:
        return None
    F = [float(v) for v in np.asarray(F, np.float64).reshape(9)]
    Ks = [float(v) for v in np.asarray(K_src, np.float64).reshape(9)]
    Kd = [float(v) for v in np.asarray(K_dst, np.float64).reshape(9)]
    with np.errstate(all="ignore"):
        T = [float(v) for v in np.array(_mat3mul(np.array(F), np.array(Ks)))]
        Tn, Kn = np.array(T), np.array(Kd)
        E0 = [float(Kn[i] * Tn[j] + Kn[3 + i] * Tn[3 + j] + Kn[6 + i] * Tn[6 + j]) for i in range(3) for j in range(3)]
        En = np.array(E0)
        G = np.array([[[En[i] * En[j] + En[3 + i] * En[3 + j] + En[6 + i] * En[6 + j] for j in range(3)]
                       for i in range(3)]])
    V = jacobi_batch(G)[0]
    d = [float(G[0, i, i]) for i in range(3)]
    v = [[float(V[k, i]) for k in range(3)] for i in range(3)]
    for a, b in ((0, 1), (1, 2), (0, 1)):
        if d[b] > d[a]:
            d[a], d[b] = d[b], d[a]
            v[a], v[b] = v[b], v[a]
    if not _finite(d) or not d[1] > 0:
        return None
    v1, v2, v3 = v
    s1, s2 = math.sqrt(d[0]), math.sqrt(d[1])
    with np.errstate(all="ignore"):
        f = np.float64
        u1 = [float((f(E0[i * 3]) * v1[0] + f(E0[i * 3 + 1]) * v1[1] + f(E0[i * 3 + 2]) * v1[2]) / s1) for i in range(3)]
        u2 = [float((f(E0[i * 3]) * v2[0] + f(E0[i * 3 + 1]) * v2[1] + f(E0[i * 3 + 2]) * v2[2]) / s2) for i in range(3)]
        a1, a2 = [f(x) for x in u1], [f(x) for x in u2]
        u3 = [float(a1[1] * a2[2] - a1[2] * a2[1]), float(a1[2] * a2[0] - a1[0] * a2[2]),
              float(a1[0] * a2[1] - a1[1] * a2[0])]
        det = (v1[0] * (v2[1] * v3[2] - v2[2] * v3[1]) - v1[1] * (v2[0] * v3[2] - v2[2] * v3[0]) +
               v1[2] * (v2[0] * v3[1] - v2[1] * v3[0]))
        if det < 0:
            v3 = [-x for x in v3]
        half = (s1 + s2) / 2
        a3 = [f(x) for x in u3]
        E = [float(half * (a1[i] * v1[j] + a2[i] * v2[j])) for i in range(3) for j in range(3)]
        R1 = [float(a2[i] * v1[j] - a1[i] * v2[j] + a3[i] * v3[j]) for i in range(3) for j in range(3)]
        R2 = [float(a1[i] * v2[j] - a2[i] * v1[j] + a3[i] * v3[j]) for i in range(3) for j in range(3)]
    P = []
    for R, sign in ((R1, 1), (R2, 1), (R1, -1), (R2, -1)):
        P.append([R[i * 3 + j] if j < 3 else (u3[i] if sign > 0 else -u3[i]) for i in range(3) for j in range(4)])
    if not (_finite(E) and _finite(P[0]) and _finite(P[1])):
        return None
    return {"Kis": Kis, "Kid": Kid, "E": E, "P": P, "u3": u3, "sigma": (s1, s2, d[2])}


def triangulate(P_src, P_dst, x, y, X, Y):
    """Step 4 for arrays of points (float64) -> Q [n, 4], homogeneous, not divided."""
    Ps = np.asarray(P_src, np.float64).reshape(12)
    Pd = np.asarray(P_dst, np.float64).reshape(12)
    n = len(x)
    with np.errstate(all="ignore"):
        a = [[x * Ps[8 + k] - Ps[k] for k in range(4)], [y * Ps[8 + k] - Ps[4 + k] for k in range(4)],
             [X * Pd[8 + k] - Pd[k] for k in range(4)], [Y * Pd[8 + k] - Pd[4 + k] for k in range(4)]]
        A = np.zeros((n, 4, 4))
        for j in range(4):
            for k in range(j, 4):
                A[:, j, k] = a[0][j] * a[0][k] + a[1][j] * a[1][k] + a[2][j] * a[2][k] + a[3][j] * a[3][k]
                A[:, k, j] = A[:, j, k]
    return smallest_eigvec_batch(A) if n else np.zeros((0, 4))


def triangulate_points(P_src, P_dst, src, dst):
    """sift_triangulate_points: float32 points as given -> xyzw float64 [n, 4]."""
    s = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
    d = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
    f = np.float64
    return triangulate(P_src, P_dst, s[:, 0].astype(f), s[:, 1].astype(f), d[:, 0].astype(f), d[:, 1].astype(f))


IDENTITY_CAMERA = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]


def good_points(D, P, src, dst, thresh):
    """Steps 4 and 5 under the camera P -> (good bool [n], xyz [n, 3])."""
    x, y = normalise(D["Kis"], src)
    X, Y = normalise(D["Kid"], dst)
    Q = triangulate(IDENTITY_CAMERA, P, x, y, X, Y)
    with np.errstate(all="ignore"):
        xyz = np.stack([Q[:, 0] / Q[:, 3], Q[:, 1] / Q[:, 3], Q[:, 2] / Q[:, 3]], axis=1)
        z2 = P[8] * xyz[:, 0] + P[9] * xyz[:, 1] + P[10] * xyz[:, 2] + P[11]
        good = (xyz[:, 2] > 0) & (xyz[:, 2] < thresh) & (z2 > 0) & (z2 < thresh)
    return good, xyz


class Pose:
    """What sift_recover_pose writes, and the slot that won (-1: no pose)."""

    def __init__(self, n):
        self.found, self.slot, self.n_good = 0, -1, 0
        self.pose, self.E = np.zeros(12), np.zeros(9)
        self.mask, self.xyz = np.zeros(n, np.uint8), np.zeros((n, 3))
        self.counts = [0] * SLOTS


def recover_pose(F, K_src, K_dst, src, dst, mask_in=None, thresh=50.0) -> Pose:
    src = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
    dst = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
    n = len(src)
    out = Pose(n)
    if not thresh > 0:
        return out
    D = decompose(F, K_src, K_dst)
    if D is None:
        return out
    rows = np.ones(n, bool) if mask_in is None else np.asarray(mask_in).reshape(-1) != 0
    res = [good_points(D, P, src, dst, thresh) for P in D["P"]]
    out.counts = [int((g & rows).sum()) for g, _ in res]
    w = 0
    for c in range(1, SLOTS):
        if out.counts[c] > out.counts[w]:
            w = c
    if out.counts[w] < 1:
        return out
    good = res[w][0] & rows
    out.found, out.slot, out.n_good = 1, w, out.counts[w]
    out.pose, out.E = np.array(D["P"][w], np.float64), np.array(D["E"], np.float64)
    out.mask = good.astype(np.uint8)
    out.xyz = np.where(good[:, None], res[w][1], 0.0)
    return out
