"""Inputs of the segmented-homography tests (test_homography_batch.py on the CPU,
test_gpu_homography_batch.py on the GPU) and their expected values from
oracle/homography.py, computed once per process.

Three calls, because threshold and max_iters are per call:
  MAIN     thr 3, max_iters 2000: segments of 0, 3, 4 and 5 pairs, the five
           (seed, n, out_frac, noise) sets of test_matches_oracle_bitexact, an
           all-collinear segment (the 10000-attempt exit at iteration 0), 300
           pairs at 30 % outliers, and a segment that ends in the second round
           (the five sets already end in the first round -- 22 iterations --, in
           the third -- 139 -- and at max_iters = 2000 with a model);
  CAPPED   thr 3, max_iters 200: 75 % outliers, so niters never drops below
           max_iters -- the loop reaches max_iters with a model;
  NONE     thr 1e-6, max_iters 200, pure outliers: even a hypothesis's own four
           points miss a 1e-6 px threshold in float arithmetic, so no hypothesis
           ever has more than 3 inliers -- the loop reaches max_iters with none.
The census (how many iterations each segment ran, every update_num_iters call)
is taken by wrapping the oracle's functions, never by editing it."""
import functools

import numpy as np

import homography as HO

H_TRUE = np.array([[0.9, -0.12, 31.0], [0.08, 1.05, -12.5], [2e-4, -1e-4, 1.0]])
BITEXACT_SETS = [(10, 60, 0.3, 0.5), (11, 150, 0.5, 1.0), (12, 40, 0.1, 0.0), (13, 200, 0.6, 2.0), (14, 5, 0.0, 0.3)]


def project(H, p):
    q = np.c_[p, np.ones(len(p))] @ H.T
    return (q[:, :2] / q[:, 2:]).astype(np.float32)


def data(seed, n, out_frac, noise=0.0):
    """test_homography.py's _data on default_rng(seed)."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(0, 640, (n, 2)).astype(np.float32)
    dst = project(H_TRUE, src.astype(np.float64))
    if noise:
        dst = (dst + rng.normal(0, noise, dst.shape)).astype(np.float32)
    bad = rng.random(n) < out_frac
    dst[bad] = rng.uniform(0, 640, (int(bad.sum()), 2)).astype(np.float32)
    return src, dst


def _line(n):
    p = np.c_[np.arange(n), 2 * np.arange(n)].astype(np.float32)
    return p, p.copy()


class Call:
    def __init__(self, name, segments, thr=3.0, max_iters=2000, confidence=0.995):
        self.name, self.thr, self.max_iters, self.confidence = name, thr, max_iters, confidence
        self.labels = [s[0] for s in segments]
        self.sizes = [len(s[1]) for s in segments]
        self.src = np.concatenate([s[1] for s in segments]).astype(np.float32).reshape(-1, 2)
        self.dst = np.concatenate([s[2] for s in segments]).astype(np.float32).reshape(-1, 2)
        self.moff = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int32)

    def index(self, label):
        return self.labels.index(label)


def _seg(label, pair):
    return (label, pair[0], pair[1])


@functools.lru_cache(maxsize=None)
def calls():
    main = [_seg("empty", data(1, 0, 0)), _seg("three", data(2, 3, 0)), _seg("four", data(3, 4, 0)),
            _seg("five", data(4, 5, 0))]
    main += [_seg(f"set{seed}", data(seed, n, f, nz)) for seed, n, f, nz in BITEXACT_SETS]
    main += [_seg("collinear", _line(10)), _seg("empty_between", data(1, 0, 0)),
             _seg("n300", data(0, 300, 0.3)), _seg("second_round", data(21, 120, 0.5, 0.5))]
    capped = [_seg("capped", data(30, 100, 0.75, 0.5)), _seg("clean", data(31, 30, 0.1, 0.2))]
    none = [_seg("outliers", data(40, 30, 1.0)), _seg("clean", data(31, 30, 0.1, 0.2))]
    return (Call("MAIN", main), Call("CAPPED", capped, max_iters=200), Call("NONE", none, thr=1e-6, max_iters=200))


def expect_segments(src, dst, moff, m_cap, thr, max_iters, confidence):
    """The oracle per clamped segment -> (H [n, 9] zeros for none, found [n], mask [m_cap] or rows untouched = 0)."""
    o = np.clip(np.asarray(moff, np.int64), 0, m_cap)
    nseg = len(o) - 1
    H = np.zeros((nseg, 9), np.float64)
    found = np.zeros(nseg, np.int32)
    mask = np.zeros(m_cap, np.uint8)
    for b in range(nseg):
        lo, hi = int(o[b]), int(max(o[b], o[b + 1]))
        h, m = HO.find_homography(src[lo:hi], dst[lo:hi], thr, max_iters, confidence)
        if h is not None:
            H[b], found[b] = np.array(h, np.float64), 1
        mask[lo:hi] = m
    return H, found, mask


@functools.lru_cache(maxsize=None)
def expected():
    """{call name: (H, found, mask, census)}; census[b] = (iterations, [update_num_iters records])."""
    out = {}
    real_rk, real_up = HO.run_kernel, HO.update_num_iters
    for c in calls():
        H = np.zeros((len(c.sizes), 9), np.float64)
        found = np.zeros(len(c.sizes), np.int32)
        mask = np.zeros(len(c.src), np.uint8)
        census = []
        for b in range(len(c.sizes)):
            lo, hi = int(c.moff[b]), int(c.moff[b + 1])
            seen = {"four": 0, "updates": []}  # "four": run_kernel calls

            def rk(M, m, seen=seen):
                seen["four"] += 1
                return real_rk(M, m)

            def up(p, ep, model_points, max_iters, seen=seen):
                r = real_up(p, ep, model_points, max_iters)
                seen["updates"].append((p, ep, model_points, max_iters, r))
                return r

            HO.run_kernel, HO.update_num_iters = rk, up
            try:
                h, m = HO.find_homography(c.src[lo:hi], c.dst[lo:hi], c.thr, c.max_iters, c.confidence)
            finally:
                HO.run_kernel, HO.update_num_iters = real_rk, real_up
            if h is not None:
                H[b], found[b] = np.array(h, np.float64), 1
            mask[lo:hi] = m
            # run_kernel runs once per iteration, and once more for the refit (n > 4 with a model);
            # n == 4 is the direct fit, no iteration
            iters = 0 if hi - lo <= 4 else seen["four"] - (1 if h is not None else 0)
            census.append((iters, seen["updates"]))
        out[c.name] = (H, found, mask, census)
    return out
