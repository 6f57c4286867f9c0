"""Inputs of the PnP tests (test_pnp.py on the CPU, test_gpu_pnp.py on the GPU)
and their expected values from pnp_oracle.py, computed once per process.

view(seed, n) is a calibrated view of n 3-D points: a uniform random rotation,
points in a box 2 to 10 units in front of the camera (a plane for coplanar=True),
expressed in a world frame by the inverse pose, projected through K to float32
pixels; `outliers` of the rows get a pixel at least 30 px from the true one.

p3p_cases() is the census of sift_solve_p3p; cpu_cases() that of sift_solve_pnp;
gpu_call() the one device call of 16 segments (CENSUS / GPU_LABELS name what
must be among them; test_pnp.py asserts it on the oracle's results)."""
import functools

import numpy as np

import pnp_oracle as NO

K_A = np.array([[820.0, 1.5, 330.0], [0, 790.0, 235.0], [0, 0, 1]])      # with skew
K_B = np.array([[640.0, 0, 300.5], [0, 655.0, 260.0], [0, 0, 1]])
K_SINGULAR = np.array([[800.0, 0, 320.0], [0, 800.0, 240.0], [1600.0, 0, 640.0]])   # row 2 = 2 x row 0
THRESH, ITERS, CONF = 8.0, 100, 0.99


def _rotation_uniform(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def project(K, Xc):
    p = Xc @ K.T
    return p[:, :2] / p[:, 2:]


def view(seed, n, K=K_A, coplanar=False, outliers=0.0, depth=(2, 10)):
    """-> dict(X [n, 3] world, xy float32 [n, 2], R, t, K, good bool [n]); X_cam = R X + t."""
    rng = np.random.default_rng(11000 + seed)
    R = _rotation_uniform(rng)
    t = rng.uniform(-3, 3, 3)
    Xc = np.c_[rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(*depth, n)]
    if coplanar:       # a tilted plane in the camera frame
        Xc[:, 2] = 6 + 0.4 * Xc[:, 0] - 0.3 * Xc[:, 1]
    X = (Xc - t) @ R                       # R^T (Xc - t)
    xy = project(K, X @ R.T + t)
    good = np.ones(n, bool)
    bad = rng.permutation(n)[:int(round(outliers * n))]
    good[bad] = False
    for i in bad:
        while True:
            p = rng.uniform((0, 0), (640, 480))
            if np.abs(p - xy[i]).max() >= 30:
                break
        xy[i] = p
    return {"X": X, "xy": xy.astype(np.float32), "R": R, "t": t, "K": K, "good": good}


# ---- sift_solve_p3p -----------------------------------------------------------
N_GENERAL = 48
ABOVE = [1, 3, 5, 7, 9, 107, 153]     # seeds of triangle_above; 107 has three solutions, 1 four
P3P_CENSUS = (["general%d" % k for k in range(N_GENERAL)] + ["above%d" % k for k in ABOVE] +
              ["equal_points", "collinear", "at_centre", "same_bearing", "skew_K", "K_singular", "K_nan", "xyz_nan",
               "xyz_inf", "xy_nan", "xy_inf"])


def triangle_above(seed, K=K_B):
    """A roughly equilateral triangle seen from 1 to 3 units above its middle: where P3P has three
    and four solutions.  -> (X [3, 3] world, xy float32 [3, 2], R, t)."""
    rng = np.random.default_rng(seed)
    R = _rotation_uniform(rng)
    t = rng.uniform(-3, 3, 3)
    ang = rng.uniform(0, 2 * np.pi) + np.array([0, 2.1, 4.2]) + rng.uniform(-0.3, 0.3, 3)
    Xc = np.c_[np.cos(ang), np.sin(ang), np.full(3, rng.uniform(1.0, 3.0))] + rng.uniform(-0.15, 0.15, (3, 3))
    X = (Xc - t) @ R
    return X, project(K, X @ R.T + t).astype(np.float32), R, t


@functools.lru_cache(maxsize=None)
def p3p_cases():
    """-> list of (label, xyz [3, 3], xy float32 [3, 2], K)."""
    cases = []
    for k in range(N_GENERAL):
        v = view(500 + k, 3, K_B if k % 2 else K_A)
        cases.append(("general%d" % k, v["X"], v["xy"], v["K"]))
    for k in ABOVE:
        X, xy, _, _ = triangle_above(k)
        cases.append(("above%d" % k, X, xy, K_B))
    v = view(600, 3, K_B)
    X = v["X"].copy()
    X[2] = X[1]
    cases.append(("equal_points", X, v["xy"], K_B))
    X = v["X"].copy()
    X[2] = X[0] + 2.5 * (X[1] - X[0])
    xy = project(K_B, X @ v["R"].T + v["t"]).astype(np.float32)
    cases.append(("collinear", X, xy, K_B))
    X = v["X"].copy()
    X[0] = -v["R"].T @ v["t"]                  # the camera centre: R X + t = 0
    cases.append(("at_centre", X, v["xy"], K_B))
    xy = v["xy"].copy()
    xy[1] = xy[0]
    cases.append(("same_bearing", v["X"], xy, K_B))
    v2 = view(601, 3, K_A)
    cases.append(("skew_K", v2["X"], v2["xy"], K_A))
    cases.append(("K_singular", v["X"], v["xy"], K_SINGULAR))
    kn = K_B.copy()
    kn[0, 0] = np.nan
    cases.append(("K_nan", v["X"], v["xy"], kn))
    for label, which, val in (("xyz_nan", 0, np.nan), ("xyz_inf", 0, np.inf), ("xy_nan", 1, np.nan),
                              ("xy_inf", 1, np.inf)):
        X, xy = v["X"].copy(), v["xy"].copy()
        (X if which == 0 else xy)[1, 0] = val
        cases.append((label, X, xy, K_B))
    assert [c[0] for c in cases] == P3P_CENSUS
    return cases


# ---- sift_solve_pnp -----------------------------------------------------------
class Case:
    def __init__(self, label, v, X=None, xy=None, K=None, mask=None, thr=THRESH, iters=ITERS, conf=CONF):
        self.label = label
        self.X = np.ascontiguousarray(v["X"] if X is None else X, np.float64).reshape(-1, 3)
        self.xy = np.ascontiguousarray(v["xy"] if xy is None else xy, np.float32).reshape(-1, 2)
        self.K = np.array(v["K"] if K is None else K, np.float64)
        self.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.thr, self.iters, self.conf = thr, iters, conf
        self.view = v

    def oracle(self):
        return NO.solve_pnp(self.X, self.xy, self.K, self.mask, self.thr, self.iters, self.conf)


CENSUS = ["n0", "n3", "n4", "n4_masked", "n5", "coplanar", "out30", "out50", "behind", "zero_rows", "mask_ones",
          "mask_some", "mask_zero", "thr_0", "thr_neg8", "thr_inf", "thr_nan", "iters_0", "iters_1", "conf_0",
          "conf_1", "nan_rows", "inf_rows", "K_singular", "K_nan"]


@functools.lru_cache(maxsize=None)
def cpu_cases():
    v = view(1, 120, K_A, outliers=0.3)
    clean = view(2, 60, K_B)
    cases = [Case("n0", clean, clean["X"][:0], clean["xy"][:0]), Case("n3", clean, clean["X"][:3], clean["xy"][:3]),
             Case("n4", clean, clean["X"][:4], clean["xy"][:4]),
             Case("n4_masked", clean, clean["X"][:4], clean["xy"][:4], mask=[1, 1, 0, 1]),
             Case("n5", clean, clean["X"][:5], clean["xy"][:5]),
             Case("coplanar", view(3, 100, K_B, coplanar=True, outliers=0.2)),
             Case("out30", v), Case("out50", view(4, 200, K_B, outliers=0.5))]
    # 20 rows behind the camera, at the pixels their mirror images would have
    b = view(5, 80, K_A)
    X = b["X"].copy()
    Xc = X[:20] @ b["R"].T + b["t"]
    X[:20] = (-Xc - b["t"]) @ b["R"]
    cases.append(Case("behind", b, X))
    z = view(6, 80, K_B)
    X = z["X"].copy()
    X[::4] = 0
    cases.append(Case("zero_rows", z, X))
    rng = np.random.default_rng(5)
    cases.append(Case("mask_ones", v, mask=np.ones(120, np.uint8)))
    cases.append(Case("mask_some", v, mask=(rng.uniform(size=120) < 0.7).astype(np.uint8) * 255))
    cases.append(Case("mask_zero", v, mask=np.zeros(120, np.uint8)))
    cases += [Case("thr_0", clean, thr=0.0), Case("thr_neg8", v, thr=-8.0), Case("thr_inf", b, X=cases[8].X,
                                                                                 thr=float("inf")),
              Case("thr_nan", v, thr=float("nan")), Case("iters_0", v, iters=0), Case("iters_1", clean, iters=1),
              Case("conf_0", v, conf=0.0), Case("conf_1", v, conf=1.0)]
    X, xy = v["X"].copy(), v["xy"].copy()
    X[3, 1], xy[10, 0], X[40], xy[41] = np.nan, np.nan, np.nan, np.nan
    cases.append(Case("nan_rows", v, X, xy))
    X, xy = v["X"].copy(), v["xy"].copy()
    X[5, 2], xy[12, 1], X[50, 0] = np.inf, -np.inf, -np.inf
    cases.append(Case("inf_rows", v, X, xy))
    cases.append(Case("K_singular", v, K=K_SINGULAR))
    kn = K_A.copy()
    kn[1, 1] = np.nan
    cases.append(Case("K_nan", v, K=kn))
    assert [c.label for c in cases] == CENSUS
    return cases


# ---- the planted scenes of test_planted_geometry -------------------------------
def planted(k, outliers):
    """Scene k of eight: 300 points; scene 3 is coplanar, scenes 1, 3, 5, 7 use the skewed K_A."""
    return view(2000 + k, 300, K_A if k % 2 else K_B, coplanar=(k == 3), outliers=outliers)


# ---- the device call -----------------------------------------------------------
GPU_ITERS = 513          # two rounds of 256 and one more hypothesis
GPU_LABELS = ["n0", "n3", "n4", "n5", "n255", "n256", "n257", "backwards", "n257_again", "n600", "nan", "good_a",
              "singular_K", "good_b", "all_masked", "long"]


class Call:
    """One segmented call: rows (some past m_cap), offsets, a row mask and a K per segment."""

    def __init__(self):
        segs = [("n0", 0, 0.0), ("n3", 3, 0.0), ("n4", 4, 0.0), ("n5", 5, 0.0), ("n255", 255, 0.3),
                ("n256", 256, 0.3), ("n257", 257, 0.3), ("n600", 600, 0.3), ("nan", 60, 0.2), ("good_a", 50, 0.2),
                ("singular_K", 40, 0.0), ("good_b", 45, 0.2), ("all_masked", 40, 0.0), ("long", 140, 0.75)]
        X, xy, mask, offs, self.labels, Ks, self.views = [], [], [], [0], [], [], []
        rng = np.random.default_rng(78)
        for k, (label, n, out) in enumerate(segs):
            v = view(3000 + k, max(n, 1), K_A if k % 2 else K_B, outliers=out)
            x, p = v["X"][:n].copy(), v["xy"][:n].copy()
            if label == "nan":
                x[3], p[20, 1], x[31, 2] = np.nan, np.nan, np.inf
            m = (rng.uniform(size=n) < 0.9).astype(np.uint8)
            if n <= 5:
                m[:] = 1
            if label == "all_masked":
                m[:] = 0
            X.append(x), xy.append(p), mask.append(m)
            offs.append(offs[-1] + n)
            labs = [label]
            if label == "n257":     # stated twice around a non-monotone offset
                offs += [offs[-2], offs[-1]]
                labs += ["backwards", "n257_again"]
            for lab in labs:
                self.labels.append(lab)
                Ks.append((K_SINGULAR if lab == "singular_K" else v["K"]).reshape(9))
                self.views.append(v)
        assert self.labels == GPU_LABELS
        self.X = np.concatenate(X).astype(np.float64)
        self.xy = np.concatenate(xy).astype(np.float32)
        self.mask = np.concatenate(mask).astype(np.uint8)
        self.moff = np.array(offs, np.int32)
        self.m_cap = int(self.moff[-1]) - 20      # the last segment straddles m_cap
        self.K = np.array(Ks)
        self.thr, self.iters, self.conf = THRESH, GPU_ITERS, CONF

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
    """-> dict(pose [n_seg, 12], found, n_inliers, mask [m_cap], iters, written bool [m_cap]) of gpu_call()
    with its row mask and a K per segment, from the oracle."""
    c = gpu_call()
    nseg = len(c.labels)
    out = {"pose": np.zeros((nseg, 12)), "found": np.zeros(nseg, np.int32), "n_inliers": np.zeros(nseg, np.int32),
           "mask": np.zeros(c.m_cap, np.uint8), "iters": [0] * nseg, "written": np.zeros(c.m_cap, bool)}
    for b in range(nseg):
        lo, hi = c.bounds(b)
        r = NO.solve_pnp(c.X[lo:hi], c.xy[lo:hi], c.K[b], c.mask[lo:hi], c.thr, c.iters, c.conf)
        out["pose"][b], out["found"][b], out["n_inliers"][b], out["iters"][b] = r.pose, r.found, r.n_inliers, r.iters
        out["mask"][lo:hi] = r.mask
        out["written"][lo:hi] = True
    return out
