"""Inputs of the affine / similarity estimation tests (test_affine.py on the CPU,
test_gpu_affine.py on the GPU) and their expected values from affine_oracle.py,
computed once per process.

cpu_cases(model) are the host cases: each (label, src, dst, thr, max_iters,
confidence), built per model because the model-point count m sets the sizes.

gpu_call(model) is the one device call per model: segments of 0, 1, 2, 3, 4,
63, 64, 65 and 300 pairs, one of 2 * AFFINE_ROUND + 1, a NaN-poisoned segment
between two clean ones, one segment stated twice with a non-monotone offset
between its statements ([a, b), [b, a) = empty, [a, b) again: both write the
same bytes, so the overlap is harmless), and a last segment that runs past
m_cap.  Its confidence is 1 - 1e-6 and most pairs are outliers, so that
segments of 63 pairs and more need more than one round of hypotheses.  The
census (iterations per segment, every update_num_iters call) is taken by
wrapping the oracle's functions, never by editing it."""
import functools

import numpy as np

import affine_oracle as AO
import homography as HO

SEED = {0: 380, 1: 300}   # per model: seeds for which the census of test_affine.py holds
ROUND = 128   # siftgpu.AFFINE_ROUND (test_affine.py checks it against scratch.hpp)
# dyadic coefficients: integer sources below 1024 map to exactly representable floats
A_TRUE = {AO.AFFINE: np.array([[0.875, -0.25, 31.25], [0.125, 1.0625, -12.5]]),
          AO.SIMILARITY: np.array([[0.75, -0.5, 31.25], [0.5, 0.75, -12.5]])}
MODELS = [AO.AFFINE, AO.SIMILARITY]
NAMES = {AO.AFFINE: "affine", AO.SIMILARITY: "similarity"}


def apply(A, p):
    return (np.asarray(p, np.float64) @ A[:, :2].T + A[:, 2]).astype(np.float32)


def data(model, seed, n, out_frac, noise=0.0, integer=False):
    """n pairs of A_TRUE[model]; about out_frac of them gross outliers (dst moved by 50 to 300 px).
    -> (src, dst, planted inlier flags)."""
    rng = np.random.default_rng(seed)
    src = (rng.integers(0, 1024, (n, 2)) if integer else rng.uniform(0, 640, (n, 2))).astype(np.float32)
    dst = apply(A_TRUE[model], src)
    if noise:
        dst = (dst + rng.uniform(-noise, noise, dst.shape)).astype(np.float32)
    bad = rng.random(n) < out_frac
    ang, r = rng.uniform(0, 2 * np.pi, n), rng.uniform(50, 300, n)
    off = np.c_[r * np.cos(ang), r * np.sin(ang)].astype(np.float32)
    dst[bad] = (dst[bad] + off[bad]).astype(np.float32)
    return src, dst, ~bad


def _pair(model, seed, n, out_frac, noise=0.0):
    s, d, _ = data(model, seed, n, out_frac, noise)
    return s, d


@functools.lru_cache(maxsize=None)
def cpu_cases(model):
    m = AO.model_points(model)
    D = (3.0, 2000, 0.99)
    cases = [(f"n{n}", *_pair(model, 100 + n, n, 0.0, 0.2), *D) for n in (0, 1, m - 1, m, m + 1)]
    if model == AO.AFFINE:
        line = np.array([[0, 0], [1, 2], [2, 4]], np.float32)
        cases.append(("degenerate", line, line + np.float32(5), *D))
    else:
        same = np.array([[7, 9], [7, 9]], np.float32)
        cases.append(("degenerate", same, np.array([[1, 2], [3, 4]], np.float32), *D))
    one = np.tile(np.array([[12.5, 40.25]], np.float32), (10, 1))
    cases.append(("identical", one, one + np.float32(3), *D))
    cases.append(("outliers40", *_pair(model, 7, 300, 0.4, 0.3), *D))
    cases.append(("noise", *_pair(model, 8, 120, 0.0, 0.5), *D))
    s, d = _pair(model, 9, 80, 0.3, 0.5)
    cases += [("thr-3", s, d, -3.0, 2000, 0.99), ("thr0", s, d, 0.0, 2000, 0.99), ("thr1e30", s, d, 1e30, 2000, 0.99),
              ("max_iters0", s, d, 3.0, 0, 0.99), ("confidence0", s, d, 3.0, 2000, 0.0),
              ("confidence1", s, d, 3.0, 2000, 1.0)]
    sn, dn = s.copy(), d.copy()
    sn[11] = np.nan
    cases.append(("nan_row", sn, dn, *D))
    si, di = s.copy(), d.copy()
    si[5, 0], di[17, 1] = np.inf, -np.inf
    cases += [("inf_row", si, di, *D), ("inf_row_thr1e30", si, di, 1e30, 2000, 0.99)]
    return cases


class Call:
    """One segmented call: src / dst rows (some past m_cap), offsets, m_cap, labels per segment."""

    def __init__(self, model):
        self.model, self.thr, self.max_iters, self.confidence = model, 3.0, 2000, 1 - 1e-6
        inl = 0.4 if model == AO.AFFINE else 0.25     # inlier share of the large segments
        segs = [("n0", 0, 0.0), ("n1", 1, 0.0), ("n2", 2, 0.0), ("n3", 3, 0.0), ("n4", 4, 0.0),
                ("n63", 63, 1 - inl), ("n64", 64, 1 - inl), ("n65", 65, 1 - inl), ("n300", 300, 1 - inl),
                ("two_rounds_plus_1", 2 * ROUND + 1, 1 - inl), ("clean_a", 70, 1 - inl), ("nan", 66, 1 - inl),
                ("clean_b", 72, 1 - inl), ("last", 90, 1 - inl)]
        src, dst, offs, self.labels = [], [], [0], []
        for k, (label, n, f) in enumerate(segs):
            s, d = _pair(model, SEED[model] + k, n, f, 0.5)
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
def gpu_call(model):
    return Call(model)


def expect_segments(src, dst, moff, m_cap, model, thr, max_iters, confidence):
    """The oracle per clamped segment -> (H [n, 9], found [n], mask [m_cap], rows outside segments 0)."""
    o = np.clip(np.asarray(moff, np.int64), 0, m_cap)
    nseg = len(o) - 1
    H = np.zeros((nseg, 9), np.float64)
    found = np.zeros(nseg, np.int32)
    mask = np.zeros(m_cap, np.uint8)
    for b in range(nseg):
        lo, hi = int(o[b]), int(max(o[b], o[b + 1]))
        A, m = AO.estimate_affine(src[lo:hi], dst[lo:hi], model, thr, max_iters, confidence)
        H[b], found[b] = AO.as_h(A), A is not None
        mask[lo:hi] = m
    return H, found, mask


@functools.lru_cache(maxsize=None)
def expected(model):
    """(H, found, mask, census) of gpu_call(model); census[b] = (iterations, wins, [update_num_iters records])."""
    c = gpu_call(model)
    nseg = len(c.labels)
    H = np.zeros((nseg, 9), np.float64)
    found = np.zeros(nseg, np.int32)
    mask = np.zeros(c.m_cap, np.uint8)
    census = []
    real_solve, real_up = AO.solve_minimal, HO.update_num_iters
    for b in range(nseg):
        lo, hi = c.bounds(b)
        seen = {"solves": 0, "updates": []}

        def solve(model_, s, d, seen=seen):
            seen["solves"] += 1
            return real_solve(model_, s, d)

        def up(p, ep, model_points, max_iters, seen=seen):
            r = real_up(p, ep, model_points, max_iters)
            seen["updates"].append((p, ep, model_points, max_iters, r))
            return r

        AO.solve_minimal, HO.update_num_iters = solve, up
        try:
            A, m = AO.estimate_affine(c.src[lo:hi], c.dst[lo:hi], model, c.thr, c.max_iters, c.confidence)
        finally:
            AO.solve_minimal, HO.update_num_iters = real_solve, real_up
        H[b], found[b] = AO.as_h(A), A is not None
        mask[lo:hi] = m
        # one minimal solve per iteration; n == m is the direct fit, no iteration
        iters = 0 if hi - lo <= AO.model_points(model) else seen["solves"]
        census.append((iters, len(seen["updates"]), seen["updates"]))
    return H, found, mask, census
