"""Inputs of the fundamental-matrix tests (test_fundamental.py on the CPU,
test_gpu_fundamental.py on the GPU) and their expected values from
fundamental_oracle.py, computed once per process.

The scene is two pinhole cameras with a real baseline and rotation looking at
3-D points in a box with depth spread (not a plane), projected to float32 with
`noise` px of uniform jitter.  An outlier is a pair whose dst point is moved
perpendicular to its true epipolar line by 50 to 300 px (a random direction
could land on the line); the number of outliers is round(n * out_frac) exactly,
at random rows, so that a segment's iteration count does not hang on a binomial
draw.

cpu_cases() are the host cases: each (label, src, dst, thr, max_iters,
confidence).

gpu_call() is the one device call: segments of 0, 1, 7, 8, 9, 63, 64, 65, 300
and 2 * FUND_ROUND + 1 pairs, a NaN-poisoned segment between two clean ones, one
segment stated twice with a non-monotone offset between its statements ([a, b),
[b, a) = empty, [a, b) again: both write the same bytes), and a last segment
that runs past m_cap.  Its confidence is 1 - 1e-6 and the inlier share of the
large segments is INLIER_SHARE, so that they need more than one round of
hypotheses.  The census (iterations per segment, every update_num_iters call) is
taken by wrapping the oracle's functions, never by editing it."""
import functools

import numpy as np

import fundamental_oracle as FO
import homography as HO

SEED = 500            # a seed for which the census of test_fundamental.py holds
ROUND = 256           # siftgpu.FUND_ROUND (test_fundamental.py checks it against scratch.hpp)
INLIER_SHARE = 0.62   # of the segments of 63 pairs and more

K = np.array([[800.0, 0, 320], [0, 800, 240], [0, 0, 1]])
_ay, _ax = np.deg2rad(9.0), np.deg2rad(-3.0)
R_TRUE = (np.array([[np.cos(_ay), 0, np.sin(_ay)], [0, 1, 0], [-np.sin(_ay), 0, np.cos(_ay)]])
          @ np.array([[1, 0, 0], [0, np.cos(_ax), -np.sin(_ax)], [0, np.sin(_ax), np.cos(_ax)]]))
T_TRUE = np.array([-1.0, 0.12, 0.25])
_tx = np.array([[0, -T_TRUE[2], T_TRUE[1]], [T_TRUE[2], 0, -T_TRUE[0]], [-T_TRUE[1], T_TRUE[0], 0]])
F_TRUE = np.linalg.inv(K).T @ _tx @ R_TRUE @ np.linalg.inv(K)     # [dst;1]^T F [src;1] = 0


def epipolar_distances(F, src, dst):
    """(distance of dst to F src, distance of src to F^T dst) in float64, per pair."""
    s = np.c_[np.asarray(src, np.float64), np.ones(len(src))]
    d = np.c_[np.asarray(dst, np.float64), np.ones(len(dst))]
    l2, l1 = s @ np.asarray(F).reshape(3, 3).T, d @ np.asarray(F).reshape(3, 3)
    return (np.abs((d * l2).sum(1)) / np.hypot(l2[:, 0], l2[:, 1]),
            np.abs((s * l1).sum(1)) / np.hypot(l1[:, 0], l1[:, 1]))


def data(seed, n, out_frac, noise=0.0):
    """n pairs of the two views, round(n * out_frac) of them outliers -> (src, dst, planted inlier flags)."""
    rng = np.random.default_rng(seed)
    P = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 10, n)]
    a = P @ K.T
    b = (P @ R_TRUE.T + T_TRUE) @ K.T
    src = a[:, :2] / a[:, 2:]
    dst = b[:, :2] / b[:, 2:]
    if noise:
        src = src + rng.uniform(-noise, noise, src.shape)
        dst = dst + rng.uniform(-noise, noise, dst.shape)
    bad = np.zeros(n, bool)
    bad[rng.permutation(n)[:int(round(n * out_frac))]] = True
    line = np.c_[src, np.ones(n)] @ F_TRUE.T          # dst's true epipolar line
    normal = line[:, :2] / np.hypot(line[:, 0], line[:, 1])[:, None]
    move = rng.uniform(50, 300, n) * rng.choice([-1.0, 1.0], n)
    dst = np.where(bad[:, None], dst + normal * move[:, None], dst)
    return src.astype(np.float32), dst.astype(np.float32), ~bad


def _pair(seed, n, out_frac, noise=0.0):
    s, d, _ = data(seed, n, out_frac, noise)
    return s, d


@functools.lru_cache(maxsize=None)
def cpu_cases():
    D = (3.0, 1000, 0.99)
    cases = [(f"n{n}", *_pair(100 + n, n, 0.0, 0.2), *D) for n in (0, 1, 7, 8, 9)]
    one = np.tile(np.array([[12.5, 40.25]], np.float32), (8, 1))
    cases.append(("identical", one, one + np.float32(3), *D))
    t = np.arange(20, dtype=np.float32)[:, None]
    line = np.c_[10 + 3 * t, 20 + 2 * t].astype(np.float32)
    cases.append(("collinear", line, (line * np.float32(0.5) + np.float32(7)).astype(np.float32), *D))
    cases.append(("outliers40", *_pair(7, 200, 0.4, 0.3), *D))
    cases.append(("noise", *_pair(8, 120, 0.0, 0.5), *D))
    s, d = _pair(9, 80, 0.3, 0.5)
    cases += [("thr-3", s, d, -3.0, 1000, 0.99), ("thr0", s, d, 0.0, 1000, 0.99), ("thr1e30", s, d, 1e30, 1000, 0.99),
              ("max_iters0", s, d, 3.0, 0, 0.99), ("confidence0", s, d, 3.0, 1000, 0.0),
              ("confidence1", s, d, 3.0, 1000, 1.0)]
    sn, dn = s.copy(), d.copy()
    sn[11] = np.nan
    cases.append(("nan_row", sn, dn, *D))
    si, di = s.copy(), d.copy()
    si[5, 0], di[17, 1] = np.inf, -np.inf
    cases += [("inf_row", si, di, *D), ("inf_row_thr1e30", si, di, 1e30, 1000, 0.99)]
    return cases


class Call:
    """One segmented call: src / dst rows (some past m_cap), offsets, m_cap, labels per segment."""

    def __init__(self):
        self.thr, self.max_iters, self.confidence = 3.0, 2000, 1 - 1e-6
        out = 1 - INLIER_SHARE
        segs = [("n0", 0, 0.0), ("n1", 1, 0.0), ("n7", 7, 0.0), ("n8", 8, 0.0), ("n9", 9, 0.0),
                ("n63", 63, out), ("n64", 64, out), ("n65", 65, out), ("n300", 300, out),
                ("two_rounds_plus_1", 2 * ROUND + 1, out), ("clean_a", 70, out), ("nan", 66, out),
                ("clean_b", 72, out), ("last", 90, out)]
        src, dst, offs, self.labels = [], [], [0], []
        for k, (label, n, f) in enumerate(segs):
            s, d = _pair(SEED + k, n, f, 0.25)
            if label == "nan":
                s[3], d[40, 1] = np.nan, np.nan
            src.append(s)
            dst.append(d)
            offs.append(offs[-1] + n)
            self.labels.append(label)
            if label == "n65":   # stated twice around a non-monotone offset
                offs += [offs[-2], offs[-1]]
                self.labels += ["backwards", "n65_again"]
        self.src = np.concatenate(src).astype(np.float32)
        self.dst = np.concatenate(dst).astype(np.float32)
        self.moff = np.array(offs, np.int32)
        self.m_cap = int(self.moff[-1]) - 21      # the last segment straddles m_cap
        self.big = [b for b, lab in enumerate(self.labels) if self.size(b) >= 63 and lab != "nan"]

    def bounds(self, b):
        o = np.clip(self.moff.astype(np.int64), 0, self.m_cap)
        return int(o[b]), int(max(o[b], o[b + 1]))

    def size(self, b):
        lo, hi = self.bounds(b)
        return hi - lo

    def index(self, label):
        return self.labels.index(label)


@functools.lru_cache(maxsize=None)
def gpu_call():
    return Call()


@functools.lru_cache(maxsize=None)
def expected():
    """(F [n_seg, 9], found, mask [m_cap], census) of gpu_call(); census[b] = (iterations, wins,
    [update_num_iters records]).  A segment stated twice is computed once."""
    c = gpu_call()
    nseg = len(c.labels)
    F = np.zeros((nseg, 9), np.float64)
    found = np.zeros(nseg, np.int32)
    mask = np.zeros(c.m_cap, np.uint8)
    census, done = [], {}
    real_hyp, real_up = FO.hypothesis, HO.update_num_iters
    for b in range(nseg):
        lo, hi = c.bounds(b)
        if (lo, hi) not in done:
            seen = {"iters": 0, "updates": []}

            def hyp(ms, md, seen=seen):
                seen["iters"] += 1
                return real_hyp(ms, md)

            def up(p, ep, model_points, max_iters, seen=seen):
                r = real_up(p, ep, model_points, max_iters)
                seen["updates"].append((p, ep, model_points, max_iters, r))
                return r

            FO.hypothesis, HO.update_num_iters = hyp, up
            try:
                f, fnd, m = FO.find_fundamental(c.src[lo:hi], c.dst[lo:hi], c.thr, c.max_iters, c.confidence)
            finally:
                FO.hypothesis, HO.update_num_iters = real_hyp, real_up
            done[(lo, hi)] = (FO.as_f(f), fnd, m, (seen["iters"], len(seen["updates"]), seen["updates"]))
        F[b], found[b], m, cen = done[(lo, hi)]
        mask[lo:hi] = m
        census.append(cen)
    return F, found, mask, census
