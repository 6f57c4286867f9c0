"""The case tables of the undistortion tests: images and point rows, the cameras they go through,
the file format of tests/cpp/undistort_rule.cpp, and the one segmented call of the GPU test.
The expected results are tests/undistort_oracle.py's, computed once and kept read-only."""
import numpy as np

import undistort_oracle as UO
import warp_inputs as W

f32, f64 = np.float32, np.float64
PIXELS = W.PIXELS
KP_STRIDE = 28          # sizeof(sift_keypoint)
ZERO = np.zeros(8, f64)


def camera(rows, cols, f_scale=0.9, skew=0.0):
    f = f_scale * cols
    return np.array([[f, skew, (cols - 1) / 2], [0, f * 1.02, (rows - 1) / 2], [0, 0, 1]], f64)


def dist8(k1=0.0, k2=0.0, p1=0.0, p2=0.0, k3=0.0, k4=0.0, k5=0.0, k6=0.0):
    return np.array([k1, k2, p1, p2, k3, k4, k5, k6], f64)


ALL_EIGHT = dist8(0.2, -0.1, 0.003, -0.002, 0.05, 0.15, -0.05, 0.01)
# W = u - 4 exactly: the inverse of [[1, 0, 0], [0, 1, 0], [1, 0, -4]] (det -4, every entry exact)
NEWK_W0 = np.array([[1, 0, 0], [0, 1, 0], [0.25, 0, -0.25]], f64)
# x = u / 16, y = v / 16 exactly; with k4 = -1 the denominator is exactly 0 on r2 = 1 (pixel (16, 0))
K_POW2 = np.array([[16, 0, 0], [0, 16, 0], [0, 0, 1]], f64)


def image_cameras(rows, cols):
    """name -> (K, dist, newK or None)."""
    K = camera(rows, cols)
    nan_K, inf_d, nan_d, nan_N = K.copy(), dist8(k1=-0.1), dist8(k1=-0.1), K.copy()
    nan_K[1, 1], inf_d[4], nan_d[2], nan_N[0, 2] = np.nan, np.inf, np.nan, np.nan
    sing = np.array([[1, 2, 3], [2, 4, 6], [1, 1, 1]], f64)
    shift = K.copy()
    shift[0, 2] -= cols / 2                       # the destination's right half sees nothing
    far = K.copy()
    far[0, 2] += 10 * cols                        # wholly outside
    zoom = K.copy()
    zoom[0, 0] *= 0.8
    zoom[1, 1] *= 0.7
    zoom[0, 2] += 1.25
    return {
        "zero": (K, ZERO, None),
        "zero_newK_is_K": (K, ZERO, K),
        "barrel": (K, dist8(k1=-0.3), None),
        "pincushion": (K, dist8(k1=0.3), None),
        "tangential": (K, dist8(p1=0.01, p2=-0.02), None),
        "all_eight": (K, ALL_EIGHT, None),
        "skew": (camera(rows, cols, skew=3.0), dist8(k1=-0.2, p1=0.004), None),
        "newK_zoom": (K, dist8(k1=-0.2), zoom),
        "partly_outside": (K, dist8(k1=-0.1), shift),
        "wholly_outside": (K, dist8(k1=-0.1), far),
        "den_zero": (K_POW2, dist8(k4=-1.0), None),
        "w_zero": (K, ZERO, NEWK_W0),
        "singular_K": (sing, dist8(k1=-0.1), None),
        "nan_K": (nan_K, dist8(k1=-0.1), None),
        "singular_newK": (K, dist8(k1=-0.1), sing),
        "nan_newK": (K, dist8(k1=-0.1), nan_N),
        "nan_dist": (K, nan_d, None),
        "inf_dist": (K, inf_d, None),
    }


NO_RULE = ("singular_K", "nan_K", "singular_newK", "nan_newK", "nan_dist", "inf_dist")
# source shape, destination shape
SHAPES = [((1, 1), (1, 1)), ((5, 3), (9, 2)), ((17, 31), (17, 31)), ((17, 31), (31, 17)), ((67, 131), (70, 259))]
FULL_SHAPE = ((17, 31), (17, 31))      # every camera on this one
ELSEWHERE = ("zero", "barrel", "all_eight", "newK_zoom", "partly_outside", "singular_K")


def image_cases():
    """dicts with name, kind, src, K, dist, newK, out_shape."""
    out = []
    for si, (src_shape, out_shape) in enumerate(SHAPES):
        cams = image_cameras(*src_shape)
        names = list(cams) if (src_shape, out_shape) == FULL_SHAPE else ELSEWHERE
        for ki, kind in enumerate(PIXELS):
            src = W.pixels(kind, src_shape, 500 + 10 * si + ki)
            for name in names:
                K, d, N = cams[name]
                out.append(dict(name=f"{kind}-{src_shape[0]}x{src_shape[1]}to{out_shape[0]}x{out_shape[1]}-{name}",
                                kind=kind, src=src, K=K, dist=d, newK=N, out_shape=out_shape))
    # NaN and infinite samples inside the image propagate, even at weight 0
    src = W.pixels("f32", (17, 31), 577, nonfinite=True)
    K, d, N = image_cameras(17, 31)["barrel"]
    out.append(dict(name="f32-nonfinite-barrel", kind="f32", src=src, K=K, dist=d, newK=N, out_shape=(17, 31)))
    return out


IMAGE_CASES = image_cases()
_EXPECTED = {}


def expected_image(case):
    if case["name"] not in _EXPECTED:
        e = UO.undistort_ref(case["src"], case["K"], case["dist"], case["newK"], case["out_shape"])
        e.setflags(write=False)
        _EXPECTED[case["name"]] = e
    return _EXPECTED[case["name"]]


# ---- points -----------------------------------------------------------------------------------
PT_ROWS, PT_COLS = 480, 640
PT_K = camera(PT_ROWS, PT_COLS)
GENERAL_P = np.array([[500, 2, 300], [-1, 510, 250], [1e-4, -2e-4, 1.0]], f64)


def point_rows(n, seed, special=True):
    """Pixel positions over the frame; with special, a NaN row, an infinite row and the principal point."""
    r = np.random.default_rng(seed)
    xy = np.stack([r.uniform(0, PT_COLS - 1, n), r.uniform(0, PT_ROWS - 1, n)], axis=1).astype(f32)
    if special and n >= 8:
        xy[1] = (np.nan, 10.0)
        xy[3] = (20.0, np.nan)
        xy[5] = (np.inf, 7.0)
        xy[6] = (-np.inf, np.inf)
        xy[7] = (PT_K[0, 2], PT_K[1, 2])
    return xy


def point_cameras():
    """name -> (K, dist, P or None)."""
    K = PT_K
    sing = np.array([[1, 2, 3], [2, 4, 6], [1, 1, 1]], f64)
    nan_K, nan_d, nan_P = K.copy(), dist8(k1=-0.1), K.copy()
    nan_K[0, 0], nan_d[7], nan_P[2, 2] = np.nan, np.nan, np.inf
    return {
        "zero_P_is_K": (K, ZERO, K),
        "zero_normalised": (K, ZERO, None),
        "barrel": (K, dist8(k1=-0.3), K),
        "pincushion": (K, dist8(k1=0.3), K),
        "tangential": (K, dist8(p1=0.01, p2=-0.02), None),
        "all_eight": (K, ALL_EIGHT, GENERAL_P),
        "skew": (camera(PT_ROWS, PT_COLS, skew=3.0), dist8(k1=-0.2, p1=0.004), K),
        # 1 + k1 r2 = 0 inside the frame (r2 = 2.5 is beyond it for this K; k1 = -8 brings it in)
        "num_zero_ring": (K, dist8(k1=-8.0), K),
        "singular_K": (sing, dist8(k1=-0.1), K),
        "nan_K": (nan_K, dist8(k1=-0.1), K),
        "nan_dist": (K, nan_d, None),
        "inf_P": (K, dist8(k1=-0.1), nan_P),
    }


PT_NO_RULE = ("singular_K", "nan_K", "nan_dist", "inf_P")
ITERS = (0, 1, 5, 100)


def point_cases():
    """dicts with name, xy, K, dist, P, iters."""
    out = []
    xy = point_rows(97, 11)
    for name, (K, d, P) in point_cameras().items():
        for it in (ITERS if name in ("barrel", "all_eight", "zero_P_is_K", "singular_K") else (5,)):
            out.append(dict(name=f"{name}-it{it}", xy=xy, K=K, dist=d, P=P, iters=it))
    K, d, P = point_cameras()["all_eight"]
    out.append(dict(name="n0", xy=np.zeros((0, 2), f32), K=K, dist=d, P=P, iters=5))
    out.append(dict(name="n1", xy=point_rows(1, 12), K=K, dist=d, P=P, iters=5))
    return out


POINT_CASES = point_cases()


def expected_points(case):
    key = "pt-" + case["name"]
    if key not in _EXPECTED:
        e, ok = UO.undistort_points_ref(case["xy"], case["K"], case["dist"], case["P"], case["iters"])
        e.setflags(write=False)
        _EXPECTED[key] = (e, ok)
    return _EXPECTED[key]


def as_rows(xy, stride, fill=0x5A):
    """xy [n, 2] float32 inside rows of stride bytes, the other bytes fill: uint8 [n, stride]."""
    rows = np.full((len(xy), stride), fill, np.uint8)
    rows[:, :8] = np.ascontiguousarray(xy, f32).view(np.uint8).reshape(len(xy), 8)
    return rows


def rows_xy(rows):
    return np.ascontiguousarray(rows[:, :8]).view(f32).reshape(len(rows), 2)


# ---- the rule program's files ---------------------------------------------------------------
def _cam26(K, d, third):
    t = np.zeros(9, f64) if third is None else np.asarray(third, f64).reshape(9)
    return np.concatenate([np.asarray(K, f64).reshape(9), np.asarray(d, f64).reshape(8), t]).tobytes()


def rule_table():
    """What the rule program is given: every image case, and every point case at both strides, out of
    place and in place.  Entries: ("image", case) or ("points", case, stride, in_place)."""
    t = [("image", c) for c in IMAGE_CASES]
    for c in POINT_CASES:
        for stride in (8, KP_STRIDE):
            for in_place in (0, 1):
                t.append(("points", c, stride, in_place))
    return t


def write_cases(path, table):
    with open(path, "wb") as f:
        for e in table:
            if e[0] == "image":
                c = e[1]
                pixel, ch, _ = W.pixel_args(c["kind"])
                r, cl = c["src"].shape[:2]
                f.write(np.array([0, pixel, ch, r, cl, c["out_shape"][0], c["out_shape"][1],
                                  int(c["newK"] is not None)], np.int32).tobytes())
                f.write(_cam26(c["K"], c["dist"], c["newK"]))
                f.write(np.ascontiguousarray(c["src"]).tobytes())
            else:
                _, c, stride, in_place = e
                f.write(np.array([1, len(c["xy"]), stride, c["iters"], int(c["P"] is not None), in_place, 0, 0],
                                 np.int32).tobytes())
                f.write(_cam26(c["K"], c["dist"], c["P"]))
                f.write(as_rows(c["xy"], stride).tobytes())


def read_results(path, table):
    """Per entry (ok, array): the image, or the rows as uint8 [n, stride]."""
    data = open(path, "rb").read()
    out, at = [], 0
    for e in table:
        ok = int(np.frombuffer(data, np.int32, 1, at)[0])
        at += 4
        if e[0] == "image":
            c = e[1]
            _, ch, bpp = W.pixel_args(c["kind"])
            n = c["out_shape"][0] * c["out_shape"][1] * bpp
            img = np.frombuffer(data, np.uint8, n, at)
            at += n
            shape = c["out_shape"] + ((3,) if ch == 3 else ())
            out.append((ok, img.view(f32 if c["kind"] == "f32" else np.uint8).reshape(shape)))
        else:
            _, c, stride, _ = e
            n = len(c["xy"]) * stride
            out.append((ok, np.frombuffer(data, np.uint8, n, at).reshape(len(c["xy"]), stride)))
            at += n
    assert at == len(data), "trailing bytes in the result file"
    return out


def expected_rows(case, stride, in_place):
    """The rows the rule leaves: the (x, y) floats replaced; the other bytes 0x5A in place, 0xCD otherwise."""
    e, _ = expected_points(case)
    return as_rows(e, stride, 0x5A if in_place else 0xCD)


# ---- planted geometry -------------------------------------------------------------------------
def planted(k1, n=400, seed=5, dist=None):
    """Ideal pixels over the frame pushed through the forward model in numpy: (ideal float64 [n, 2],
    distorted float32 [n, 2], dist).  The distorted pixels are rounded to float, as a detector's are."""
    r = np.random.default_rng(seed)
    ideal = np.stack([r.uniform(0, PT_COLS - 1, n), r.uniform(0, PT_ROWS - 1, n)], axis=1)
    d = dist8(k1=k1, k2=-k1 / 5, p1=1e-3, p2=-5e-4) if dist is None else dist
    Ki = np.linalg.inv(PT_K)
    h = np.c_[ideal, np.ones(n)] @ Ki.T
    xd, yd = UO.distort(d, h[:, 0] / h[:, 2], h[:, 1] / h[:, 2])
    pix = np.c_[xd, yd, np.ones(n)] @ PT_K.T
    return ideal, (pix[:, :2] / pix[:, 2:]).astype(f32), d


# ---- the GPU test's one segmented call --------------------------------------------------------
class PointCall:
    """16 segments on the list of test_gpu_pose.py: 0, 1, 8, 255, 256, 257 and 600 rows, a backwards
    offset, offsets past m_cap, and a NaN row and a singular K, each between two good segments."""
    labels = ["n257", "n0", "n1", "good_a", "nan_row", "good_b", "singular_K", "good_c", "n255", "n256",
              "backwards", "n8", "n600", "all_eight", "pincushion", "past_cap"]
    sizes = [257, 0, 1, 40, 30, 40, 25, 40, 255, 256, -20, 8, 600, 50, 33, 500]

    def __init__(self):
        off = [0]
        for s in self.sizes:
            off.append(off[-1] + s)
        # "backwards" ends 20 rows before it starts, so the segments after it ("n8", and the first 12
        # rows of "n600") share rows with the tail of "n256"
        self.moff = np.array(off, np.int32)
        self.m_cap = int(self.moff[-2]) + 100          # the last segment runs past m_cap
        assert self.moff[-1] > self.m_cap > self.moff[-2]
        n = int(self.moff.max())
        self.xy = point_rows(n, 21, special=False)
        lo, _ = self.bounds(self.index("nan_row"))
        self.xy[lo + 3] = (np.nan, 5.0)
        cams = point_cameras()
        good = cams["barrel"]
        self.K = np.stack([good[0]] * 16)
        self.dist = np.stack([good[1]] * 16)
        self.P = np.stack([good[0]] * 16)
        for label, cam in (("singular_K", "singular_K"), ("all_eight", "all_eight"), ("pincushion", "pincushion"),
                           ("n600", "skew")):
            K, d, P = cams[cam]
            b = self.index(label)
            self.K[b], self.dist[b], self.P[b] = K, d, (K if P is None else P)

    def index(self, label):
        return self.labels.index(label)

    def bounds(self, b):
        lo, hi = (int(np.clip(v, 0, self.m_cap)) for v in self.moff[b:b + 2])
        return lo, max(lo, hi)

    def size(self, b):
        lo, hi = self.bounds(b)
        return hi - lo

    def expected(self, per=True, with_P=True, iters=5):
        """(xy float32 [m_cap, 2], written bool [m_cap], ok int32 [16], twice bool [m_cap]): rows that two
        segments own (twice) are left out of comparisons where the cameras differ or the call is in place."""
        out = np.full((self.m_cap, 2), np.nan, f32)
        written, twice = np.zeros(self.m_cap, bool), np.zeros(self.m_cap, bool)
        ok = np.zeros(16, np.int32)
        for b in range(16):
            c = b if per else 0
            lo, hi = self.bounds(b)
            e, k = UO.undistort_points_ref(self.xy[lo:hi], self.K[c], self.dist[c], self.P[c] if with_P else None,
                                           iters)
            twice[lo:hi] |= written[lo:hi]
            out[lo:hi], written[lo:hi], ok[b] = e, True, int(k)
        return out, written, ok, twice


_CALL = []


def gpu_call():
    if not _CALL:
        _CALL.append(PointCall())
    return _CALL[0]
