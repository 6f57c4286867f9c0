"""Inputs of the pose tests (test_pose.py on the CPU, test_gpu_pose.py on the GPU)
and their expected values from pose_oracle.py, computed once per process.

scene(seed, n) is a calibrated two-view scene: a rotation of up to 20 degrees
about a random axis, a unit baseline in a random direction, 3-D points in a box
4 to 10 units in front of the src camera that are also in front of the dst
camera, projected to float32 pixels through K_SRC (which has skew) and K_DST
(another focal length and centre); F is exact from the geometry, negated on odd
seeds.  twin_rows() makes rows that satisfy the same F but lie in front of both
cameras only under ANOTHER of the four candidate poses, which is how a tie and
rows "behind a camera" are planted.

cpu_cases() are the host cases, each a Case; CENSUS names what must be among
them (test_pose.py asserts it on the oracle's results).

gpu_call() is the one device call: segments of 0, 1, 8, 255, 256, 257 and 600
rows, a d_found = 0 segment, a NaN-poisoned segment and a singular-K segment each
between two good ones, one segment stated twice around a non-monotone offset,
and a last segment that runs past m_cap; a calibration pair per segment."""
import functools

import numpy as np

import pose_oracle as PO

K_SRC = np.array([[820.0, 1.5, 330.0], [0, 790.0, 235.0], [0, 0, 1]])
K_DST = np.array([[640.0, 0, 300.5], [0, 655.0, 260.0], [0, 0, 1]])
K_SINGULAR = np.array([[800.0, 0, 320.0], [0, 800.0, 240.0], [1600.0, 0, 640.0]])   # row 2 = 2 x row 0
THRESH = 50.0


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def _rotation(axis, angle):
    a = axis / np.linalg.norm(axis)
    S = _skew(a)
    return np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * (S @ S)


def _project(K, X):
    p = X @ K.T
    return (p[:, :2] / p[:, 2:]).astype(np.float32)


def _box_under(rng, n, R, t, depth=(4, 10)):
    """n points `depth` units in front of the src camera and at least 1 unit in front of the dst camera."""
    out = np.zeros((0, 3))
    for _ in range(100):
        X = np.c_[rng.uniform(-2, 2, 4 * n), rng.uniform(-1.5, 1.5, 4 * n), rng.uniform(*depth, 4 * n)]
        out = np.r_[out, X[(X @ R.T + t)[:, 2] > 1.0]]
        if len(out) >= n:
            return out[:n]
    raise ValueError("no points in front of both cameras")


def scene(seed, n, K_src=K_SRC, K_dst=K_DST, noise=0.0):
    """-> dict(F, R, t, X, src, dst, K_src, K_dst); X_dst = R X + t, |t| = 1."""
    rng = np.random.default_rng(7000 + seed)
    R = _rotation(rng.normal(size=3), np.deg2rad(rng.uniform(3, 20)))
    t = rng.normal(size=3)
    t /= np.linalg.norm(t)
    X = _box_under(rng, n, R, t)
    F = np.linalg.inv(K_dst).T @ _skew(t) @ R @ np.linalg.inv(K_src)
    F /= np.abs(F).max()
    if seed % 2:
        F = -F
    src, dst = X @ K_src.T, (X @ R.T + t) @ K_dst.T
    src, dst = src[:, :2] / src[:, 2:], dst[:, :2] / dst[:, 2:]
    if noise:
        src = src + rng.uniform(-noise, noise, src.shape)
        dst = dst + rng.uniform(-noise, noise, dst.shape)
    return {"F": F, "R": R, "t": t, "X": X, "src": src.astype(np.float32), "dst": dst.astype(np.float32),
            "K_src": K_src, "K_dst": K_dst}


def twin_rows(sc, slot, n, seed=0, depth=(4, 10)):
    """n rows of sc's epipolar geometry that are in front of both cameras under candidate `slot`
    of the oracle's decomposition: the scene's own slot, or the one with the baseline reversed
    (slot ^ 2), under which rows lie behind a camera of the scene's own pose.  (The twisted
    pairs look away from each other: no box in front of the src camera is in front of both.)"""
    D = PO.decompose(sc["F"], sc["K_src"], sc["K_dst"])
    P = np.array(D["P"][slot]).reshape(3, 4)
    rng = np.random.default_rng(9000 + seed)
    X = _box_under(rng, n, P[:, :3], P[:, 3], depth)
    return _project(sc["K_src"], X), _project(sc["K_dst"], X @ P[:, :3].T + P[:, 3])


class Case:
    def __init__(self, label, sc, src=None, dst=None, mask=None, thresh=THRESH, F=None, K_src=None, K_dst=None):
        self.label = label
        self.F = np.array(sc["F"] if F is None else F, np.float64)
        self.K_src = np.array(sc["K_src"] if K_src is None else K_src, np.float64)
        self.K_dst = np.array(sc["K_dst"] if K_dst is None else K_dst, np.float64)
        self.src = np.ascontiguousarray(sc["src"] if src is None else src, np.float32).reshape(-1, 2)
        self.dst = np.ascontiguousarray(sc["dst"] if dst is None else dst, np.float32).reshape(-1, 2)
        self.mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        self.thresh = thresh
        self.scene = sc

    def oracle(self):
        return PO.recover_pose(self.F, self.K_src, self.K_dst, self.src, self.dst, self.mask, self.thresh)


N_SCENES = 12
CENSUS = (["scene%d" % k for k in range(N_SCENES)] +
          ["tie", "F_1e6", "F_1e-6", "same_K", "mask_ones", "mask_partial", "mask_zero", "behind_and_far",
           "thresh_inf", "nan_row", "inf_row", "n0", "n1", "K_src_singular", "K_dst_singular", "K_nan", "F_zero",
           "F_rank1", "F_nan", "F_inf", "thresh_0", "thresh_neg", "thresh_nan"])


@functools.lru_cache(maxsize=None)
def cpu_cases():
    cases = [Case("scene%d" % k, scene(k, 40)) for k in range(N_SCENES)]
    sc = scene(100, 60)
    own = PO.recover_pose(sc["F"], sc["K_src"], sc["K_dst"], sc["src"], sc["dst"]).slot
    other = own ^ 2
    ts, td = twin_rows(sc, other, 30)
    cases.append(Case("tie", sc, np.r_[sc["src"][:30], ts], np.r_[sc["dst"][:30], td]))
    cases.append(Case("F_1e6", sc, F=sc["F"] * 1e6))
    cases.append(Case("F_1e-6", sc, F=sc["F"] * 1e-6))
    cases.append(Case("same_K", scene(101, 60, K_DST, K_DST)))
    rng = np.random.default_rng(5)
    cases.append(Case("mask_ones", sc, mask=np.ones(60, np.uint8)))
    cases.append(Case("mask_partial", sc, mask=(rng.uniform(size=60) < 0.6).astype(np.uint8) * 255))
    cases.append(Case("mask_zero", sc, mask=np.zeros(60, np.uint8)))
    # 20 rows behind a camera (good only under another candidate), 15 rows 80 to 200 units away
    fs, fd = twin_rows(sc, own, 15, seed=1, depth=(80, 200))
    bs, bd = twin_rows(sc, own ^ 2, 20, seed=2)
    mixed = (np.r_[sc["src"], bs, fs], np.r_[sc["dst"], bd, fd])
    cases.append(Case("behind_and_far", sc, *mixed))
    cases.append(Case("thresh_inf", sc, *mixed, thresh=float("inf")))
    s, d = sc["src"].copy(), sc["dst"].copy()
    s[7, 1] = np.nan
    cases.append(Case("nan_row", sc, s, d))
    s, d = sc["src"].copy(), sc["dst"].copy()
    s[3, 0], d[9, 1] = np.inf, -np.inf
    cases.append(Case("inf_row", sc, s, d))
    cases.append(Case("n0", sc, sc["src"][:0], sc["dst"][:0]))
    cases.append(Case("n1", sc, sc["src"][:1], sc["dst"][:1]))
    cases.append(Case("K_src_singular", sc, K_src=K_SINGULAR))
    cases.append(Case("K_dst_singular", sc, K_dst=np.zeros((3, 3))))
    kn = K_SRC.copy()
    kn[1, 1] = np.nan
    cases.append(Case("K_nan", sc, K_src=kn))
    cases.append(Case("F_zero", sc, F=np.zeros((3, 3))))
    cases.append(Case("F_rank1", sc, F=np.outer([1.0, 2, 3], [0.5, -1, 2])))
    fn = sc["F"].copy()
    fn[1, 2] = np.nan
    cases.append(Case("F_nan", sc, F=fn))
    fi = sc["F"].copy()
    fi[0, 0] = np.inf
    cases.append(Case("F_inf", sc, F=fi))
    cases += [Case("thresh_0", sc, thresh=0.0), Case("thresh_neg", sc, thresh=-1.0),
              Case("thresh_nan", sc, thresh=float("nan"))]
    assert [c.label for c in cases] == CENSUS
    return cases


def camera(R, t):
    return np.c_[R, t].reshape(12)


class Call:
    """One segmented call: rows (some past m_cap), offsets, per-segment F / found / K / cameras."""

    def __init__(self):
        segs = [("n0", 0), ("n1", 1), ("n8", 8), ("n255", 255), ("n256", 256), ("n257", 257), ("n600", 600),
                ("good_a", 40), ("not_found", 30), ("good_b", 41), ("nan", 50), ("good_c", 42), ("singular_K", 30),
                ("last", 90)]
        src, dst, mask, offs, self.labels = [], [], [], [0], []
        F, found, Ks, Kd, Ps, Pd = [], [], [], [], [], []
        rng = np.random.default_rng(77)
        for k, (label, n) in enumerate(segs):
            sc = scene(200 + k, max(n, 1), noise=0.2)
            s, d = sc["src"][:n].copy(), sc["dst"][:n].copy()
            if label == "nan":
                s[3], d[20, 1] = np.nan, np.nan
            m = (rng.uniform(size=n) < 0.8).astype(np.uint8)
            if label == "n1":
                m[:] = 1
            src.append(s), dst.append(d), mask.append(m)
            offs.append(offs[-1] + n)
            rows = [(label, sc)]
            if label == "n257":     # stated twice around a non-monotone offset
                offs += [offs[-2], offs[-1]]
                rows += [("backwards", sc), ("n257_again", sc)]
            for lab, sc_ in rows:
                self.labels.append(lab)
                F.append(sc_["F"].reshape(9))
                found.append(0 if lab == "not_found" else 1)
                Ks.append((K_SINGULAR if lab == "singular_K" else sc_["K_src"]).reshape(9))
                Kd.append(sc_["K_dst"].reshape(9))
                # cameras for the triangulation call: neither is [I | 0]
                Rs = _rotation(np.array([0.2, 1.0, -0.3]), 0.05 * (k + 1))
                ts = np.array([0.1 * k, -0.2, 0.05])
                Ps.append((sc_["K_src"] @ np.c_[Rs, ts]).reshape(12))
                Pd.append((sc_["K_dst"] @ np.c_[sc_["R"] @ Rs, sc_["R"] @ ts + sc_["t"]]).reshape(12))
        self.src, self.dst = np.concatenate(src).astype(np.float32), np.concatenate(dst).astype(np.float32)
        self.mask = np.concatenate(mask).astype(np.uint8)
        self.moff = np.array(offs, np.int32)
        self.m_cap = int(self.moff[-1]) - 21      # the last segment straddles m_cap
        self.F, self.found = np.array(F), np.array(found, np.int32)
        self.K_src, self.K_dst = np.array(Ks), np.array(Kd)
        self.P_src, self.P_dst = np.array(Ps), np.array(Pd)
        self.thresh = THRESH

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
def expected(with_mask=True, k_per_segment=1):
    """-> dict(pose [n_seg, 12], E [n_seg, 9], found, n_good, mask [m_cap], xyz [m_cap, 3], slot) of
    gpu_call(); k_per_segment 0 uses segment 0's calibrations for every segment."""
    c = gpu_call()
    nseg = len(c.labels)
    out = {"pose": np.zeros((nseg, 12)), "E": np.zeros((nseg, 9)), "found": np.zeros(nseg, np.int32),
           "n_good": np.zeros(nseg, np.int32), "mask": np.zeros(c.m_cap, np.uint8), "xyz": np.zeros((c.m_cap, 3)),
           "slot": [-1] * nseg}
    for b in range(nseg):
        lo, hi = c.bounds(b)
        kb = b if k_per_segment else 0
        if c.found[b]:
            r = PO.recover_pose(c.F[b], c.K_src[kb], c.K_dst[kb], c.src[lo:hi], c.dst[lo:hi],
                                c.mask[lo:hi] if with_mask else None, c.thresh)
        else:
            r = PO.Pose(hi - lo)
        out["pose"][b], out["E"][b], out["found"][b], out["n_good"][b] = r.pose, r.E, r.found, r.n_good
        out["mask"][lo:hi], out["xyz"][lo:hi], out["slot"][b] = r.mask, r.xyz, r.slot
    return out


@functools.lru_cache(maxsize=None)
def expected_xyzw():
    """-> (xyzw [m_cap, 4], written bool [m_cap]) of the triangulation call over gpu_call()'s offsets."""
    c = gpu_call()
    out, written = np.zeros((c.m_cap, 4)), np.zeros(c.m_cap, bool)
    for b in range(len(c.labels)):
        lo, hi = c.bounds(b)
        out[lo:hi] = PO.triangulate_points(c.P_src[b], c.P_dst[b], c.src[lo:hi], c.dst[lo:hi])
        written[lo:hi] = True
    return out, written
