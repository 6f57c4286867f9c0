"""CPU restatement of sift_solve_p3p and sift_solve_pnp (solvePnPRansac over a
Lambda-Twist P3P, with a Cayley Gauss-Newton refit) as
sift-gpu_amd/csrc/pnp_math.hpp and pnp.hip state them, for checking the host
path and the kernel value for value.

TEST INFRASTRUCTURE ONLY (tests import it; the product never does).  It lives
under tests/ because oracle/ is frozen.

Convention: X_cam = R X + t, a pose is [R | t] by rows (12 doubles).  The rule is
written out in include/sift_hip.h; here every expression is restated in the
order pnp_math.hpp evaluates it.  Scalars are numpy float64 (unfused IEEE
doubles; division by zero and sqrt of a negative give inf / NaN as in C), the
3 x 3 Jacobi is pose_oracle.jacobi_batch at a batch of one, the per-row work
(inlier test, refit terms) runs over all rows at once with the sums taken in row
order by a Python loop, so results compare bit for bit.  Not bit-compatible with
OpenCV.
"""
from __future__ import annotations

import numpy as np

import homography as HO
import pose_oracle as PO

F = np.float64
DBL_MAX = float(np.finfo(np.float64).max)
ZERO, ONE, TWO, THREE, FOUR = F(0), F(1), F(2), F(3), F(4)


def _finite(a):
    return all(abs(v) <= DBL_MAX for v in a)


def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross3(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _adj3(A):
    return [A[4] * A[8] - A[5] * A[7], A[2] * A[7] - A[1] * A[8], A[1] * A[5] - A[2] * A[4],
            A[5] * A[6] - A[3] * A[8], A[0] * A[8] - A[2] * A[6], A[2] * A[3] - A[0] * A[5],
            A[3] * A[7] - A[4] * A[6], A[1] * A[6] - A[0] * A[7], A[0] * A[4] - A[1] * A[3]]


def _det3(A, c):
    return A[0] * c[0] + A[1] * c[3] + A[2] * c[6]


def _trace_product(a, b):
    s = a[0] * b[0]
    for k in range(1, 9):
        s = s + a[k] * b[k]
    return s


def _cubic(g, k2, k1, k0):
    return ((g + k2) * g + k1) * g + k0


def _mat3mul(a, b):
    return [a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j] for i in range(3) for j in range(3)]


def calibrate(K):
    """-> (K [9] float64 scalars, Ki [9]) or None."""
    Ki = PO.invert3(K)
    if Ki is None:
        return None
    return [F(v) for v in np.asarray(K, np.float64).reshape(9)], [F(v) for v in Ki]


def normalise1(Ki, p):
    px, py = F(p[0]), F(p[1])
    w = Ki[6] * px + Ki[7] * py + Ki[8]
    return (Ki[0] * px + Ki[1] * py + Ki[2]) / w, (Ki[3] * px + Ki[4] * py + Ki[5]) / w


def bearing(Ki, p):
    u, v = normalise1(Ki, p)
    nrm = np.sqrt(u * u + v * v + ONE)
    return [u / nrm, v / nrm, ONE / nrm]


def p3p(x, y):
    """x: 9 float64 (three 3-D points), y: 9 (their bearings) -> a list of poses (12 float64 each)."""
    out = []
    d12 = [x[k] - x[3 + k] for k in range(3)]
    d13 = [x[k] - x[6 + k] for k in range(3)]
    d23 = [x[3 + k] - x[6 + k] for k in range(3)]
    a12, a13, a23 = _dot3(d12, d12), _dot3(d13, d13), _dot3(d23, d23)
    b12, b13, b23 = _dot3(y[0:3], y[3:6]), _dot3(y[0:3], y[6:9]), _dot3(y[3:6], y[6:9])
    D1 = [a23, -a23 * b12, ZERO, -a23 * b12, a23 - a12, a12 * b23, ZERO, a12 * b23, -a12]
    D2 = [a23, ZERO, -a23 * b13, ZERO, -a13, a13 * b23, -a23 * b13, a13 * b23, a23 - a13]
    A1, A2 = _adj3(D1), _adj3(D2)
    c0, c3 = _det3(D1, A1), _det3(D2, A2)
    c1, c2 = _trace_product(A1, D2), _trace_product(A2, D1)
    if not abs(c3) > 0:
        return out
    k2, k1, k0 = c2 / c3, c1 / c3, c0 / c3
    big = abs(k2)
    if abs(k1) > big:
        big = abs(k1)
    if abs(k0) > big:
        big = abs(k0)
    lo, hi = -(ONE + big), ONE + big
    for _ in range(64):
        mid = (lo + hi) / TWO
        if _cubic(mid, k2, k1, k0) < 0:
            lo = mid
        else:
            hi = mid
    g = (lo + hi) / TWO
    for _ in range(2):
        f, df = _cubic(g, k2, k1, k0), (THREE * g + TWO * k2) * g + k1
        if abs(df) > 0:
            g = g - f / df
    A = np.array([[[D1[i * 3 + j] + g * D2[i * 3 + j] for j in range(3)] for i in range(3)]], np.float64)
    V = PO.jacobi_batch(A)[0]
    d = [F(A[0, i, i]) for i in range(3)]
    z, least = 0, abs(d[0])
    if abs(d[1]) < least:
        least, z = abs(d[1]), 1
    if abs(d[2]) < least:
        z = 2
    ia, ib = (1 if z == 0 else 0), (1 if z == 2 else 2)
    da, db = d[ia], d[ib]
    ea, eb = [F(V[i, ia]) for i in range(3)], [F(V[i, ib]) for i in range(3)]
    ab, ba = bool(da > 0 and db < 0), bool(db > 0 and da < 0)
    if not ab and not ba:
        return out
    s = np.sqrt(-db / da) if ab else np.sqrt(-da / db)
    e1, e2 = (ea, eb) if ab else (eb, ea)
    cr = _cross3(d12, d13)
    X = [v for i in range(3) for v in (d12[i], d13[i], cr[i])]
    Xa = _adj3(X)
    dx = _det3(X, Xa)
    Xi = [v / dx for v in Xa]
    for line in range(2):
        sg = -s if line else s
        w0, w1, w2 = e1[0] + sg * e2[0], e1[1] + sg * e2[1], e1[2] + sg * e2[2]
        p, q = -w1 / w0, -w2 / w0
        qa = D1[0] * q * q + D1[8]
        qb = TWO * (D1[0] * p * q + D1[1] * q + D1[5])
        qc = D1[0] * p * p + TWO * D1[1] * p + D1[4]
        disc = qb * qb - FOUR * qa * qc
        if not disc >= 0:
            continue
        sq = np.sqrt(disc)
        for root in range(2):
            tau = ((-sq if root else sq) - qb) / (TWO * qa)
            l1r, den = p + q * tau, ONE + tau * tau - TWO * b23 * tau
            if not (tau > 0 and l1r > 0 and den > 0):
                continue
            l2 = np.sqrt(a23 / den)
            l3, l1 = tau * l2, l1r * l2
            for _ in range(5):
                r0 = l1 * l1 + l2 * l2 - TWO * b12 * l1 * l2 - a12
                r1 = l1 * l1 + l3 * l3 - TWO * b13 * l1 * l3 - a13
                r2 = l2 * l2 + l3 * l3 - TWO * b23 * l2 * l3 - a23
                J = [TWO * l1 - TWO * b12 * l2, TWO * l2 - TWO * b12 * l1, ZERO, TWO * l1 - TWO * b13 * l3, ZERO,
                     TWO * l3 - TWO * b13 * l1, ZERO, TWO * l2 - TWO * b23 * l3, TWO * l3 - TWO * b23 * l2]
                Ja = _adj3(J)
                dj = _det3(J, Ja)
                if dj == 0:
                    break
                l1 = l1 - (Ja[0] * r0 + Ja[1] * r1 + Ja[2] * r2) / dj
                l2 = l2 - (Ja[3] * r0 + Ja[4] * r1 + Ja[5] * r2) / dj
                l3 = l3 - (Ja[6] * r0 + Ja[7] * r1 + Ja[8] * r2) / dj
            f1 = [l1 * y[k] - l2 * y[3 + k] for k in range(3)]
            f2 = [l1 * y[k] - l3 * y[6 + k] for k in range(3)]
            fc = _cross3(f1, f2)
            Y = [v for i in range(3) for v in (f1[i], f2[i], fc[i])]
            R = _mat3mul(Y, Xi)
            pose = []
            for i in range(3):
                pose += [R[i * 3], R[i * 3 + 1], R[i * 3 + 2],
                         l1 * y[i] - (R[i * 3] * x[0] + R[i * 3 + 1] * x[1] + R[i * 3 + 2] * x[2])]
            if _finite(pose):
                out.append(pose)
    return out


def _rows(xyz, xy):
    X = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    p = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
    return X, p


def solve_p3p(xyz, xy, K):
    """sift_solve_p3p -> float64 [n_solutions, 12]."""
    X, p = _rows(xyz, xy)
    with np.errstate(all="ignore"):
        cal = calibrate(K)
        if cal is None:
            return np.zeros((0, 12))
        y = [v for i in range(3) for v in bearing(cal[1], p[i])]
        sols = p3p([F(v) for v in X[:3].reshape(9)], y)
    return np.array(sols, np.float64).reshape(-1, 12)


def _transform(P, x):
    return [P[i * 4] * x[0] + P[i * 4 + 1] * x[1] + P[i * 4 + 2] * x[2] + P[i * 4 + 3] for i in range(3)]


def hypothesis(cal, X4, p4):
    """Four rows -> a pose (12 float64 scalars) or None."""
    K, Ki = cal
    x = [F(v) for v in X4.reshape(12)]
    y = [v for i in range(3) for v in bearing(Ki, p4[i])]
    u, v = normalise1(Ki, p4[3])
    best, pose = F(np.inf), None
    for P in p3p(x[:9], y):
        pc = _transform(P, x[9:12])
        ex, ey = pc[0] / pc[2] - u, pc[1] / pc[2] - v
        e = ex * ex + ey * ey
        if pc[2] > 0 and e < best:
            best, pose = e, P
    return pose


def inliers(cal, P, X, p, t2, rows):
    """The inlier test over all rows at once -> bool [n]."""
    K = cal[0]
    x = [X[:, 0], X[:, 1], X[:, 2]]
    pc = _transform(P, x)
    p0 = K[0] * pc[0] + K[1] * pc[1] + K[2] * pc[2]
    p1 = K[3] * pc[0] + K[4] * pc[1] + K[5] * pc[2]
    p2 = K[6] * pc[0] + K[7] * pc[1] + K[8] * pc[2]
    ex, ey = p0 - p[:, 0].astype(np.float64) * p2, p1 - p[:, 1].astype(np.float64) * p2
    return rows & (p2 > 0) & (ex * ex + ey * ey <= t2 * (p2 * p2))


def refit_sums(cal, P, X, p, mask):
    """The 28 sums over the rows of mask, each a chain in row order."""
    Ki = cal[1]
    px, py = p[:, 0].astype(np.float64), p[:, 1].astype(np.float64)
    w = Ki[6] * px + Ki[7] * py + Ki[8]
    u, v = (Ki[0] * px + Ki[1] * py + Ki[2]) / w, (Ki[3] * px + Ki[4] * py + Ki[5]) / w
    x = [X[:, 0], X[:, 1], X[:, 2]]
    pc = _transform(P, x)
    iz = ONE / pc[2]
    qx, qy = pc[0] * iz, pc[1] * iz
    rx, ry = qx - u, qy - v
    Jx, Jy = [None] * 6, [None] * 6
    for j in range(3):
        a, b = (j + 1) % 3, (j + 2) % 3
        g0 = P[b] * x[a] - P[a] * x[b]
        g1 = P[4 + b] * x[a] - P[4 + a] * x[b]
        g2 = P[8 + b] * x[a] - P[8 + a] * x[b]
        Jx[j] = iz * g0 - qx * iz * g2
        Jy[j] = iz * g1 - qy * iz * g2
    zero = np.zeros(len(X))
    Jx[3], Jx[4], Jx[5] = iz, zero, -qx * iz
    Jy[3], Jy[4], Jy[5] = zero, iz, -qy * iz
    terms = [Jx[a] * Jx[b] + Jy[a] * Jy[b] for a in range(6) for b in range(a, 6)]
    terms += [Jx[a] * rx + Jy[a] * ry for a in range(6)]
    terms.append(rx * rx + ry * ry)
    T = np.stack(terms, axis=1)[mask]            # [inliers, 28], row order
    sums = np.zeros(28)
    for row in T:                                 # 0 + t_0 + t_1 + ...: one chain per accumulator
        sums = sums + row
    return [F(s) for s in sums]


def refit_candidate(sums, P):
    A = [[ZERO] * 7 for _ in range(6)]
    t = 0
    for a in range(6):
        for b in range(a, 6):
            A[a][b] = A[b][a] = sums[t]
            t += 1
    for a in range(6):
        A[a][6] = -sums[21 + a]
    for c in range(6):
        piv, most = c, abs(A[c][c])
        for r in range(c + 1, 6):
            if abs(A[r][c]) > most:
                most, piv = abs(A[r][c]), r
        if most < 1e-300:
            return None
        if piv != c:
            A[c], A[piv] = A[piv], A[c]
        for r in range(c + 1, 6):
            f = A[r][c] / A[c][c]
            for k in range(c, 7):
                A[r][k] = A[r][k] - f * A[c][k]
    d = [ZERO] * 6
    for c in range(5, -1, -1):
        v = A[c][6]
        for k in range(c + 1, 6):
            v = v - A[c][k] * d[k]
        d[c] = v / A[c][c]
    a = [d[0] / TWO, d[1] / TWO, d[2] / TWO]
    aa = _dot3(a, a)
    den = ONE + aa
    C = [((ONE - aa) + TWO * a[0] * a[0]) / den, (TWO * a[0] * a[1] - TWO * a[2]) / den,
         (TWO * a[0] * a[2] + TWO * a[1]) / den, (TWO * a[1] * a[0] + TWO * a[2]) / den,
         ((ONE - aa) + TWO * a[1] * a[1]) / den, (TWO * a[1] * a[2] - TWO * a[0]) / den,
         (TWO * a[2] * a[0] - TWO * a[1]) / den, (TWO * a[2] * a[1] + TWO * a[0]) / den,
         ((ONE - aa) + TWO * a[2] * a[2]) / den]
    R = [P[0], P[1], P[2], P[4], P[5], P[6], P[8], P[9], P[10]]
    Rn = _mat3mul(R, C)
    Pn = []
    for i in range(3):
        Pn += [Rn[i * 3], Rn[i * 3 + 1], Rn[i * 3 + 2], P[i * 4 + 3] + d[3 + i]]
    return Pn


class Pnp:
    """What sift_solve_pnp writes, with the RANSAC model before the refit and the iterations run."""

    def __init__(self, n):
        self.found, self.n_inliers, self.iters, self.refit_steps = 0, 0, 0, 0
        self.pose, self.ransac_pose = np.zeros(12), np.zeros(12)
        self.mask = np.zeros(n, np.uint8)


def _draw_subset(rng, n):
    idx = []
    for i in range(4):
        while True:
            v = rng.uniform(0, n)
            if v not in idx:
                break
        idx.append(v)
    return idx


def solve_pnp(xyz, xy, K, row_mask=None, thr=8.0, max_iters=100, confidence=0.99) -> Pnp:
    X, p = _rows(xyz, xy)
    n = len(X)
    out = Pnp(n)
    with np.errstate(all="ignore"):
        cal = calibrate(K)
        if n < 4 or not (confidence > 0 and confidence < 1) or max_iters < 1 or cal is None:
            return out
        rows = np.ones(n, bool) if row_mask is None else np.asarray(row_mask).reshape(-1) != 0

        def fit(idx):
            if not all(rows[i] for i in idx):
                return None
            return hypothesis(cal, X[idx], p[idx])

        if n == 4:
            best = fit([0, 1, 2, 3])
            if best is None:
                return out
            best_mask, max_good = np.ones(n, bool), 4
            out.ransac_pose = np.array(best, np.float64)
        else:
            t2 = F(thr) * F(thr)
            rng = HO.RNG()
            niters, max_good, best, best_mask = int(max_iters), 0, None, None
            it = 0
            while it < niters:
                it += 1
                model = fit(_draw_subset(rng, n))
                if model is None:
                    continue
                mask = inliers(cal, model, X, p, t2, rows)
                good = int(mask.sum())
                if good > max(max_good, 3):
                    best, best_mask, max_good = model, mask, good
                    niters = HO.update_num_iters(confidence, (n - good) / n, 4, niters)
            out.iters = it
            if max_good <= 0:
                return out
            out.ransac_pose = np.array(best, np.float64)
            cur = best
            held = refit_sums(cal, cur, X, p, best_mask)
            for _ in range(5):
                cand = refit_candidate(held, cur)
                if cand is None:
                    break
                sums = refit_sums(cal, cand, X, p, best_mask)
                if not sums[27] < held[27]:
                    break
                cur, held = cand, sums
                out.refit_steps += 1
            if _finite(cur):
                best = cur
        out.found, out.n_inliers = 1, max_good
        out.pose = np.array(best, np.float64)
        out.mask = best_mask.astype(np.uint8)
    return out
