"""Crafted inputs of the homography edge tests (test_homography_edges.py on the
CPU, test_gpu_homography_edges.py on the GPU) and their expected values from
oracle/homography.py, computed once per process.  The pattern is
homography_batch_inputs.py's: pair sets, one Call per (thr, max_iters,
confidence), a census taken by wrapping the oracle's functions.

  SEAMS      segment sizes on the seams of the kernels (the 64-pair ballot loop,
             the 64-pair term staging of the refit, the 128- and 256-thread
             mask strides), 10 % outliers; 257 is last so that m_cap can cut it;
  PLACED     inliers placed against the refit's 64-pair chunks, by row order;
  SCALE      an 8K frame's coordinates, the same shifted negative, and an H
             whose w crosses zero inside the point cloud;
  DUPS       repeated pairs, a shared src point, a shared dst point, and 12 rows
             on three positions (get_subset exhausts its attempts at iteration 0);
  FOUR       the direct fit (n == 4 skips check_subset) on degenerate quadruples;
  THR0 / THRNEG / THRBIG   a clean and a 30 %-outlier set under thr 0, -3, 1e30;
  CAP1 / CAP63 / CAP64 / CAP65   max_iters before, on and after a round boundary;
  DEGEN      built from the oracle's own first hypothesis: a winning model whose
             inliers are four copies of one pair, so the refit fails
             (spread_finish) and, with that pair's src.x == 0, lm_solve fails;
  NONFINITE  a NaN row, a +inf row and an all-NaN segment, each between two
             ordinary segments (no oracle values for those three: x86 and gfx950
             generate different NaN bit patterns, and a NaN Jacobi in Python
             takes seconds per hypothesis)."""
import functools

import numpy as np

import homography as HO
from homography_batch_inputs import H_TRUE, Call, data, project

SEAM_SIZES = [63, 64, 65, 127, 128, 129, 255, 256, 511, 512, 513, 2048, 257]
H_8K = np.array([[1.02, 0.03, -40.0], [-0.02, 0.98, 25.0], [1e-5, -5e-6, 1.0]])
H_PROJ = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0 / 320, 0.0, 1.0]])   # w = 0 on x = 320
SQUARE = np.array([[0, 0], [100, 0], [100, 100], [0, 100]], np.float32)


def pairs(seed, n_in, n_out, H=H_TRUE, box=(0, 0, 640, 640), noise=0.0):
    """n_in rows consistent with H, then n_out rows whose dst is uniform in the box."""
    rng = np.random.default_rng(seed)
    lo, hi = box[:2], box[2:]
    src = rng.uniform(lo, hi, (n_in + n_out, 2)).astype(np.float32)
    dst = project(H, src.astype(np.float64))
    if noise:
        dst = (dst + rng.normal(0, noise, dst.shape)).astype(np.float32)
    dst[n_in:] = rng.uniform(lo, hi, (n_out, 2)).astype(np.float32)
    return src, dst


def _rows(pair, order):
    order = np.asarray(order)
    return pair[0][order], pair[1][order]


def _seam(n):
    """n pairs, 10 % outliers, the first and the last row consistent with H_TRUE."""
    s, d = data(100 + n, n, 0.1, 0.3)
    d[[0, -1]] = project(H_TRUE, s[[0, -1]].astype(np.float64))
    return s, d


def _placed():
    """{label: (src, dst)}: orderings of generated rows (pairs(): inliers first)."""
    out = {}
    out["first64_out"] = _rows(pairs(200, 136, 64), np.r_[136:200, 0:136])
    out["tail_only"] = _rows(pairs(201, 40, 64), np.r_[40:104, 0:40])          # n = 104: chunk 1 holds rows 64..103
    perm = np.random.default_rng(202).permutation(128) + 1                     # n = 129: row 0 (an inlier) goes last
    out["last_row_in"] = _rows(pairs(202, 100, 29), np.r_[perm, 0])
    out["in64"] = _rows(pairs(203, 64, 16), np.random.default_rng(203).permutation(80))
    out["in65"] = _rows(pairs(204, 65, 16), np.random.default_rng(204).permutation(81))
    return out


def _scale():
    box = (0, 0, 7680, 4320)
    s, d = pairs(210, 180, 20, H_8K, box, 0.5)
    shift = np.array([9000, 5000], np.float32)
    ps, pd = pairs(211, 72, 8, H_PROJ, (0, 0, 640, 480))
    ps[-1], pd[-1] = (320.0, 100.0), (17.0, 23.0)     # a row exactly on the true H's line at infinity
    return {"frame8k": (s, d), "negative": (s - shift, d - shift), "w_crosses_zero": (ps, pd)}


def _dups():
    s, d = pairs(220, 30, 10, noise=0.3)
    triple = (np.repeat(s, 3, axis=0), np.repeat(d, 3, axis=0))
    ss, sd = pairs(221, 40, 20, noise=0.2)
    ss[40:] = (100.0, 100.0)                          # 20 rows share one src point, dst differs
    ds, dd = pairs(222, 40, 20, noise=0.2)
    dd[40:] = (300.0, 200.0)                          # 20 rows share one dst point, src differs
    pos = np.array([[10, 10], [200, 50], [90, 300]], np.float32)
    three = pos[np.arange(12) % 3]
    return {"triple": triple, "shared_src": (ss, sd), "shared_dst": (ds, dd),
            "three_positions": (three, project(H_TRUE, three.astype(np.float64)))}


def _four():
    f = lambda *rows: np.array(rows, np.float32)  # noqa: E731
    quad = f([31, 12], [410, 55], [380, 290], [20, 260])
    line = np.c_[np.arange(4), 2 * np.arange(4)].astype(np.float32)
    sim = np.c_[-2 * SQUARE[:, 1] + 10, 2 * SQUARE[:, 0] + 20].astype(np.float32)    # rotate 90, scale 2, shift
    return {"identical": (np.tile(f([10, 20]), (4, 1)), np.tile(f([30, 40]), (4, 1))),
            "common_dst": (SQUARE, np.tile(f([5, 5]), (4, 1))),
            "common_x": (f([50, 0], [50, 10], [50, 30], [50, 70]), quad),
            "collinear": (line, line.copy()),
            "two_identical": (SQUARE[[0, 1, 2, 0]], quad[[0, 1, 2, 0]]),
            "swapped": (SQUARE, quad[[0, 2, 1, 3]]),
            "similarity": (SQUARE, sim)}


SIMILARITY_H = [0.0, -2.0, 10.0, 2.0, 0.0, 20.0, 0.0, 0.0, 1.0]


def transform_limit_case():
    """(H, points) for perspectiveTransform's |w| <= FLT_EPSILON rule: H's last row is
    (1, 0, 0), so w = x.  The first four points (w = 0, +-FLT_EPSILON, one float
    under it) give (0, 0); the rest (one float over it, its negative, 1) are transformed."""
    eps = np.float32(HO.FLT_EPSILON)
    H = np.array([3.0, 0.5, 1.0, -0.25, 2.0, 7.0, 1.0, 0.0, 0.0])          # w = x
    x = [0.0, eps, -eps, np.nextafter(eps, np.float32(0)), np.nextafter(eps, np.float32(1)),
         -np.nextafter(eps, np.float32(1)), 1.0]
    return H, np.c_[np.array(x, np.float32), np.full(len(x), 5.0, np.float32)]


def first_hypothesis(src, dst):
    """The oracle's first accepted subset of (src, dst) and its model (None: no subset or no model)."""
    s = [(float(a), float(b)) for a, b in src]
    d = [(float(a), float(b)) for a, b in dst]
    rng, n = HO.RNG(), len(s)
    for _ in range(10000):
        idx = []
        while len(idx) < 4:
            r = rng.uniform(0, n)
            if r not in idx:
                idx.append(r)
        if HO.check_subset([s[i] for i in idx], [d[i] for i in idx]):
            return idx, HO.run_kernel([s[i] for i in idx], [d[i] for i in idx])
    return None, None


def _degenerate(seed, point):
    """12 generic rows; then four rows outside the first hypothesis's subset become
    copies of `point` with exactly the dst that hypothesis's model gives it in
    is_inlier's own float arithmetic (error 0).  Under thr 1e-6 the subset's own
    rows miss the limit, so the winning model's inliers are the four copies."""
    s, d = pairs(seed, 12, 0)
    idx, model = first_hypothesis(s, d)
    free = [i for i in range(12) if i not in idx][:4]
    x, y = np.float64(np.float32(point[0])), np.float64(np.float32(point[1]))
    ww = np.float64(np.float32(1.0 / (model[6] * x + model[7] * y + 1.0)))
    s[free] = point
    d[free] = (np.float32((model[0] * x + model[1] * y + model[2]) * ww),
               np.float32((model[3] * x + model[4] * y + model[5]) * ww))
    return s, d


def _nonfinite():
    nan_row = data(74, 40, 0.1, 0.2)
    nan_row[0][17, 0] = np.nan
    inf_row = data(75, 40, 0.1, 0.2)
    inf_row[0][5, 1] = np.inf
    all_nan = (np.full((20, 2), np.nan, np.float32), np.full((20, 2), np.nan, np.float32))
    return [("before", *data(70, 30, 0.1, 0.2)), ("nan_row", *nan_row), ("between0", *data(71, 31, 0.1, 0.2)),
            ("inf_row", *inf_row), ("between1", *data(72, 32, 0.1, 0.2)), ("all_nan", *all_nan),
            ("after", *data(73, 33, 0.1, 0.2))]


NONFINITE_LABELS = ("nan_row", "inf_row", "all_nan")


@functools.lru_cache(maxsize=None)
def calls():
    seg = lambda sets: [(k, v[0], v[1]) for k, v in sets.items()]  # noqa: E731
    clean, out30 = data(60, 50, 0.0, 0.2), data(61, 80, 0.3, 0.5)
    thr_sets = [("clean", *clean), ("out30", *out30)]
    long_run = [("long", *data(30, 100, 0.75, 0.5))]          # reaches max_iters = 200 with a model
    out = [Call("SEAMS", [(f"n{n}", *_seam(n)) for n in SEAM_SIZES]),
           Call("PLACED", seg(_placed())), Call("SCALE", seg(_scale())), Call("DUPS", seg(_dups())),
           Call("FOUR", seg(_four())),
           Call("THR0", thr_sets, thr=0.0, max_iters=100), Call("THRNEG", thr_sets, thr=-3.0),
           Call("THRBIG", thr_sets, thr=1e30)]
    out += [Call(f"CAP{m}", long_run, max_iters=m) for m in (1, 63, 64, 65)]
    out.append(Call("DEGEN", [("refit_fails", *_degenerate(230, (123.0, 77.0))),
                              ("lm_fails", *_degenerate(233, (0.0, 77.0)))], thr=1e-6, max_iters=10))
    out.append(Call("NONFINITE", _nonfinite(), max_iters=200))
    return tuple(out)


def call(name):
    return next(c for c in calls() if c.name == name)


class _H(list):
    """refine_lm's H argument, counting what refine_lm does to it: a slice
    assignment is an accepted step (H[:] = Hn), and entry 6 is read once per pair
    by cost(H) at the start and by each step's Jacobian, and once more when a
    step's candidate is formed (after lm's solve succeeded)."""
    accepts = reads6 = 0

    def __setitem__(self, k, v):
        self.accepts += isinstance(k, slice)
        list.__setitem__(self, k, v)

    def __getitem__(self, k):
        self.reads6 += k == 6
        return list.__getitem__(self, k)


def census_run(src, dst, thr, max_iters, confidence):
    """HO.find_homography under wrappers -> (H or None, mask, census dict):
    iterations, updates [(p, ep, model_points, max_iters, result)], rejects
    {reason: [iteration]}, kernel_failures (run_kernel None inside the loop),
    refit_failed, lm_accepted / lm_rejected / lm_solve_failed."""
    real = {k: getattr(HO, k) for k in ("run_kernel", "update_num_iters", "check_subset", "refine_lm")}
    seen = {"kernels": [], "updates": [], "rejects": {"src": [], "dst": [], "flip": []}, "lm": None}

    def rk(M, m):
        r = real["run_kernel"](M, m)
        seen["kernels"].append((len(M), r is None))
        return r

    def up(p, ep, model_points, mi):
        r = real["update_num_iters"](p, ep, model_points, mi)
        seen["updates"].append((p, ep, model_points, mi, r))
        return r

    def cs(s, d):
        ok = real["check_subset"](s, d)
        if not ok:
            why = "src" if HO._collinear_last(s) else "dst" if HO._collinear_last(d) else "flip"
            seen["rejects"][why].append(len(seen["kernels"]))     # the iteration this subset was drawn for
        return ok

    def lm(s, d, H):
        h = _H(H)
        r = real["refine_lm"](s, d, h)
        # reads6 = n + n * steps + candidates, candidates = steps or (a failed solve) steps - 1
        steps = -((len(s) - h.reads6) // (len(s) + 1))
        failed = (h.reads6 - len(s)) % (len(s) + 1) != 0
        seen["lm"] = (h.accepts, steps - failed - h.accepts, failed)
        return list(r)

    HO.run_kernel, HO.update_num_iters, HO.check_subset, HO.refine_lm = rk, up, cs, lm
    try:
        with np.errstate(all="ignore"):      # 1 / 0 and inf - inf in find_inliers are part of the inputs
            h, m = HO.find_homography(src, dst, thr, max_iters, confidence)
    finally:
        for k, v in real.items():
            setattr(HO, k, v)
    n = len(src)
    refit = n > 4 and h is not None          # then the last run_kernel call is the refit
    loop = seen["kernels"][:-1] if refit else seen["kernels"]
    acc, rej, failed = seen["lm"] or (0, 0, False)
    return h, m, {"iterations": len(loop) if n > 4 else 0, "updates": seen["updates"], "rejects": seen["rejects"],
                  "kernel_failures": sum(f for _, f in loop) if n > 4 else 0,
                  "refit_failed": bool(refit and seen["kernels"][-1][1]),
                  "lm_accepted": acc, "lm_rejected": rej, "lm_solve_failed": failed}


_memo = {}


def oracle(src, dst, thr, max_iters, confidence):
    """HO.find_homography, each distinct input computed once per process -> (H or None, mask, census)."""
    src, dst = np.ascontiguousarray(src, np.float32), np.ascontiguousarray(dst, np.float32)
    key = (src.tobytes(), dst.tobytes(), thr, max_iters, confidence)
    if key not in _memo:
        _memo[key] = census_run(src, dst, thr, max_iters, confidence)
    return _memo[key]


def expect_segments(src, dst, moff, m_cap, thr, max_iters, confidence):
    """homography_batch_inputs.expect_segments through the memo: the oracle per clamped segment."""
    o = np.clip(np.asarray(moff, np.int64), 0, m_cap)
    nseg = len(o) - 1
    H, found, mask = np.zeros((nseg, 9), np.float64), np.zeros(nseg, np.int32), np.zeros(m_cap, np.uint8)
    for b in range(nseg):
        lo, hi = int(o[b]), int(max(o[b], o[b + 1]))
        h, m, _ = oracle(src[lo:hi], dst[lo:hi], thr, max_iters, confidence)
        if h is not None:
            H[b], found[b] = np.array(h, np.float64), 1
        mask[lo:hi] = m
    return H, found, mask


SWEEP_PARAMS = ((0.995, 2000), (0.99, 200), (0.5, 2000))     # (confidence, max_iters) of the update_num_iters sweep


@functools.lru_cache(maxsize=None)
def sweep():
    """(good, n) int arrays: n = 5..512, good = 4..n -- every (n - good) / n a winner can hand update_num_iters."""
    n = np.concatenate([np.full(k - 3, k) for k in range(5, 513)])
    good = np.concatenate([np.arange(4, k + 1) for k in range(5, 513)])
    return good, n


def finite_segment(c, b):
    return c.name != "NONFINITE" or c.labels[b] not in NONFINITE_LABELS


@functools.lru_cache(maxsize=None)
def expected():
    """{call name: (H, found, mask, census)}; census[b] is census_run's dict, None for a non-finite segment
    (whose H / found / mask entries here are zeros and mean nothing)."""
    out = {}
    for c in calls():
        H = np.zeros((len(c.sizes), 9), np.float64)
        found = np.zeros(len(c.sizes), np.int32)
        mask = np.zeros(len(c.src), np.uint8)
        census = []
        for b in range(len(c.sizes)):
            lo, hi = int(c.moff[b]), int(c.moff[b + 1])
            if not finite_segment(c, b):
                census.append(None)
                continue
            h, m, cen = oracle(c.src[lo:hi], c.dst[lo:hi], c.thr, c.max_iters, c.confidence)
            if h is not None:
                H[b], found[b] = np.array(h, np.float64), 1
            mask[lo:hi] = m
            census.append(cen)
        out[c.name] = (H, found, mask, census)
    return out
