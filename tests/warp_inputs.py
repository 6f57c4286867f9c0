"""The rule of sift_warp_perspective[_segmented_device] (include/sift_hip.h,
csrc/warp_math.hpp) restated in numpy, and the case table the CPU test
(test_warp.py, through tests/cpp/warp_rule.cpp) and the GPU test
(test_gpu_warp.py) share.

The rule is the library's own statement of cv::warpPerspective(src, dst, H,
dsize, INTER_LINEAR [| WARP_INVERSE_MAP], BORDER_CONSTANT, 0): coordinates in
float64 with np.rint (ties to even), the float32 blend as four products and
three sums in the written order, the uint8 blend in integers.  Every comparison
made with it is bit for bit."""
import numpy as np

f32, f64 = np.float32, np.float64
INT_MIN, INT_MAX = -2147483648.0, 2147483647.0


def warp_matrix(H, inverse=False):
    """(M [9] float64, ok): M = H with inverse, else adj(H) * (1 / det(H)) with the cofactors in
    the header's order.  ok False (M zeros): a non-finite entry of H or M, det 0 or non-finite."""
    h = [f64(v) for v in np.asarray(H, f64).reshape(9)]
    ok = bool(np.all(np.isfinite(h)))
    with np.errstate(all="ignore"):
        if inverse:
            M = np.array(h, f64)
        else:
            c0 = h[4] * h[8] - h[5] * h[7]
            c1 = h[5] * h[6] - h[3] * h[8]
            c2 = h[3] * h[7] - h[4] * h[6]
            det = (h[0] * c0 + h[1] * c1) + h[2] * c2
            r = f64(1.0) / det
            M = np.array([c0 * r, (h[2] * h[7] - h[1] * h[8]) * r, (h[1] * h[5] - h[2] * h[4]) * r,
                          c1 * r, (h[0] * h[8] - h[2] * h[6]) * r, (h[2] * h[3] - h[0] * h[5]) * r,
                          c2 * r, (h[1] * h[6] - h[0] * h[7]) * r, (h[0] * h[4] - h[1] * h[3]) * r], f64)
            ok = ok and det != 0 and bool(np.isfinite(det)) and bool(np.all(np.isfinite(M)))
    return (M, True) if ok else (np.zeros(9, f64), False)


def inverse_rule(H):
    """The rule's own inverse of H, as a 3 x 3 matrix (for the WARP_INVERSE_MAP form of a call)."""
    M, ok = warp_matrix(H, False)
    assert ok
    return M.reshape(3, 3)


def source_coords(M, out_rows, out_cols):
    """(sx, ax, sy, ay, valid) of every destination pixel, [out_rows, out_cols] each."""
    M = [f64(v) for v in M]
    x = np.arange(out_cols, dtype=f64)[None, :]
    y = np.arange(out_rows, dtype=f64)[:, None]
    with np.errstate(all="ignore"):
        Wd = (M[6] * x + M[7] * y) + M[8]
        W = np.where(Wd != 0, f64(32.0) / Wd, f64(0.0))
        fX = ((M[0] * x + M[1] * y) + M[2]) * W
        fY = ((M[3] * x + M[4] * y) + M[5]) * W
    valid = ~(np.isnan(fX) | np.isnan(fY))
    X = np.rint(np.clip(np.where(valid, fX, 0.0), INT_MIN, INT_MAX)).astype(np.int64)
    Y = np.rint(np.clip(np.where(valid, fY, 0.0), INT_MIN, INT_MAX)).astype(np.int64)
    return X >> 5, X & 31, Y >> 5, Y & 31, valid


def _sample(S, sy, sx):
    """S[sy][sx] ([..., channels] kept), 0 outside the image and never read there."""
    rows, cols = S.shape[:2]
    inside = (sy >= 0) & (sy < rows) & (sx >= 0) & (sx < cols)
    v = S[np.clip(sy, 0, rows - 1), np.clip(sx, 0, cols - 1)]
    return np.where(inside if S.ndim == 2 else inside[..., None], v, S.dtype.type(0))


def warp_ref(src, H, out_shape, inverse=False, found=1):
    """src float32 [rows, cols] or uint8 [rows, cols] / [rows, cols, 3] -> [out_rows, out_cols(, 3)]."""
    src = np.asarray(src)
    out_rows, out_cols = out_shape
    out = np.zeros((out_rows, out_cols) + src.shape[2:], src.dtype)
    M, ok = warp_matrix(H, inverse)
    if not ok or not found:
        return out
    sx, ax, sy, ay, valid = source_coords(M, out_rows, out_cols)
    v00, v01 = _sample(src, sy, sx), _sample(src, sy, sx + 1)
    v10, v11 = _sample(src, sy + 1, sx), _sample(src, sy + 1, sx + 1)
    if src.dtype == f32:
        fx, fy = ax.astype(f32) * f32(0.03125), ay.astype(f32) * f32(0.03125)
        one = f32(1.0)
        w00, w01, w10, w11 = (one - fy) * (one - fx), (one - fy) * fx, fy * (one - fx), fy * fx
        with np.errstate(all="ignore"):
            val = ((v00 * w00 + v01 * w01) + v10 * w10) + v11 * w11
        assert val.dtype == f32
        return np.where(valid, val, f32(0.0))
    assert src.dtype == np.uint8
    if src.ndim == 3:
        ax, ay, valid = ax[..., None], ay[..., None], valid[..., None]
    k00, k01, k10, k11 = (32 - ay) * (32 - ax), (32 - ay) * ax, ay * (32 - ax), ay * ax
    val = (v00.astype(np.int64) * k00 + v01.astype(np.int64) * k01 + v10.astype(np.int64) * k10 +
           v11.astype(np.int64) * k11 + 512) >> 10
    return np.where(valid, val, 0).astype(np.uint8)


def canonical(a):
    """a with every float32 NaN replaced by one NaN.  IEEE 754 leaves the sign and payload of a
    NaN result open (x86 makes 0 * inf a negative quiet NaN, gfx950 a positive one, and which of
    two NaN operands survives depends on the operand order the compiler picked), so a NaN pixel --
    reached only from NaN or infinite source samples -- is pinned as "a NaN, here"; every other
    pixel is compared bit for bit."""
    a = np.ascontiguousarray(a)
    if a.dtype != f32:
        return a
    out = a.copy()
    out[np.isnan(a)] = f32(np.nan)
    return out


# ---- pixels ---------------------------------------------------------------------------------
def values_f32(shape, seed, nonfinite=False):
    """Negatives, large and small magnitudes, denormals and zeros (nonfinite: NaN and infinities too)."""
    r = np.random.default_rng(seed)
    v = (r.standard_normal(shape) * 100).astype(f32)
    flat = v.reshape(-1)
    n = flat.size
    if n >= 3:
        k = max(1, n // 7)
        flat[r.integers(0, n, k)] = f32(2.0 ** -140) * r.integers(-9, 10, k).astype(f32)
        flat[r.integers(0, n, max(1, n // 11))] = f32(1.0) + f32(2.0 ** -23)
    if nonfinite:
        flat[r.integers(0, n, max(1, n // 9))] = f32(np.nan)
        flat[r.integers(0, n, max(1, n // 9))] = f32(np.inf)
        flat[r.integers(0, n, max(1, n // 13))] = f32(-np.inf)
    return v


def values_u8(shape, seed):
    """Every kind of neighbourhood: noise with runs of 0 and 255 next to each other."""
    r = np.random.default_rng(seed)
    v = r.integers(0, 256, shape).astype(np.uint8)
    flat = v.reshape(-1)
    n = flat.size
    if n >= 4:
        k = max(1, n // 6)
        flat[r.integers(0, n, k)] = 255
        flat[r.integers(0, n, k)] = 0
    return v


PIXELS = ("f32", "u8", "u8x3")


def pixels(kind, shape, seed, nonfinite=False):
    if kind == "f32":
        return values_f32(shape, seed, nonfinite)
    return values_u8(shape if kind == "u8" else shape + (3,), seed)


# ---- homographies ------------------------------------------------------------------------
def _shift(tx, ty):
    return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], f64)


def _rotation(deg, rows, cols, orows, ocols):
    """Rotation about the source centre, mapped onto the destination centre."""
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    to_origin = _shift(-(cols - 1) / 2, -(rows - 1) / 2)
    back = _shift((ocols - 1) / 2, (orows - 1) / 2)
    return back @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], f64) @ to_origin


def homographies(rows, cols, orows, ocols):
    """name -> (H 3 x 3, inverse, found).  Those given with inverse = True state M itself, so the
    coordinates they produce are exact by construction (no inversion in between)."""
    nan = np.nan
    return {
        "identity": (np.eye(3), False, 1),
        # sx = -1 on the image's first column, and v01 outside on its last
        "shift_x+1": (_shift(1, 0), False, 1),
        "shift_x-1": (_shift(-1, 0), False, 1),
        "shift_y+2_x-3": (_shift(-3, 2), False, 1),
        "shift_to_last_col": (_shift(-(cols - 1), -(rows - 1)), True, 1),   # S[0][0] lands on pixel (cols - 1, rows - 1)
        "shift_from_last_col": (_shift(cols - 1, rows - 1), True, 1),       # pixel (0, 0) samples S[rows - 1][cols - 1] alone
        "shift_5/32_-11/32": (_shift(5 / 32, -11 / 32), True, 1),
        "shift_31/32": (_shift(31 / 32, 31 / 32), True, 1),
        # ties: 32 x + 0.5 -> 32 x (even), 32 y + 1.5 -> 32 y + 2
        "ties_1/64_3/64": (_shift(1 / 64, 3 / 64), True, 1),
        "ties_negative": (_shift(-1 / 64, -3 / 64), True, 1),
        "scale_2": (np.diag([2.0, 2.0, 1.0]), False, 1),
        "scale_0.5": (np.diag([0.5, 0.5, 1.0]), False, 1),
        "rotation_30": (_rotation(30, rows, cols, orows, ocols), False, 1),
        "projective": (np.array([[0.9, 0.12, 1.5], [-0.07, 1.1, -0.8], [1.5e-3, -2.5e-3, 1.0]], f64), False, 1),
        # Wd = x - k is exactly 0 on one destination column (W = 0: the pixel is S[0][0]) and changes sign across it
        "horizon": (np.array([[1, 0, 0], [0, 1, 0], [1, 0, -float(ocols // 2)]], f64), True, 1),
        "horizon_oblique": (np.array([[1.3, 0.1, 2], [0.2, 0.9, 1], [0.25, 0.5, -1.0]], f64), True, 1),
        # |fX| far beyond an int: clamped to INT_MIN (x = 0), 0 (x = 1) and INT_MAX
        "clamp_1e12": (np.array([[1e12, 0, -1e12], [0, 1e12, -1e12], [0, 0, 1]], f64), True, 1),
        # W = 32 / 1e-320 = inf: 0 * inf is a NaN coordinate (pixel 0) on column 0 and row 0
        "zero_times_inf": (np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1e-320]], f64), True, 1),
        "singular": (np.array([[1, 2, 3], [2, 4, 6], [1, 1, 1]], f64), False, 1),
        "nan_entry": (np.array([[1, 0, 0], [0, nan, 0], [0, 0, 1]], f64), False, 1),
        "nan_entry_inverse": (np.array([[1, 0, 0], [0, 1, 0], [0, nan, 1]], f64), True, 1),
        "inf_entry": (np.array([[1, 0, np.inf], [0, 1, 0], [0, 0, 1]], f64), False, 1),
        "overflowing_inverse": (np.diag([1e-310, 1e10, 1e10]), False, 1),   # finite H and det, an infinite entry of M
        "not_found": (_shift(0.25, 0.5), False, 0),
    }


# source shape, destination shape
SHAPES = [((1, 1), (1, 1)), ((1, 7), (3, 5)), ((5, 3), (9, 2)), ((17, 31), (31, 17)), ((67, 131), (64, 128)),
          ((67, 131), (70, 259)), ((203, 157), (203, 157))]
FULL_SHAPE = ((17, 31), (31, 17))     # every homography on this one
ELSEWHERE = ("identity", "shift_x+1", "shift_5/32_-11/32", "ties_1/64_3/64", "rotation_30", "projective", "horizon")


def cases():
    """The table: dicts with name, kind, src, H, inverse, found, out_shape."""
    out = []
    for si, (src_shape, out_shape) in enumerate(SHAPES):
        hs = homographies(*src_shape, *out_shape)
        names = list(hs) if (src_shape, out_shape) == FULL_SHAPE else ELSEWHERE
        for ki, kind in enumerate(PIXELS):
            src = pixels(kind, src_shape, 100 * si + ki)
            for name in names:
                H, inverse, found = hs[name]
                out.append(dict(name=f"{kind}-{src_shape[0]}x{src_shape[1]}to{out_shape[0]}x{out_shape[1]}-{name}",
                                kind=kind, src=src, H=np.ascontiguousarray(H, f64), inverse=inverse, found=found,
                                out_shape=out_shape))
    # NaN and infinite samples inside the image propagate, even at weight 0
    src = pixels("f32", (17, 31), 77, nonfinite=True)
    hs = homographies(17, 31, 31, 17)
    for name in ("identity", "shift_5/32_-11/32", "rotation_30"):
        H, inverse, found = hs[name]
        out.append(dict(name=f"f32-nonfinite-{name}", kind="f32", src=src, H=np.ascontiguousarray(H, f64),
                        inverse=inverse, found=found, out_shape=(31, 17)))
    return out


CASES = cases()
_EXPECTED = {}


def expected(case):
    """warp_ref of a case, computed once."""
    if case["name"] not in _EXPECTED:
        e = warp_ref(case["src"], case["H"], case["out_shape"], case["inverse"], case["found"])
        e.setflags(write=False)
        _EXPECTED[case["name"]] = e
    return _EXPECTED[case["name"]]


def pixel_args(kind):
    """(SIFT_PIXEL_*, channels, bytes per pixel)."""
    return {"f32": (0, 1, 4), "u8": (1, 1, 1), "u8x3": (1, 3, 3)}[kind]


def write_cases(path, table):
    """The file tests/cpp/warp_rule.cpp reads: per case eight int32 (pixel, channels, rows, cols,
    out_rows, out_cols, inverse, found), nine float64 (H), then the packed source bytes."""
    with open(path, "wb") as f:
        for c in table:
            pixel, ch, _ = pixel_args(c["kind"])
            r, cl = c["src"].shape[:2]
            f.write(np.array([pixel, ch, r, cl, c["out_shape"][0], c["out_shape"][1], int(c["inverse"]), c["found"]],
                             np.int32).tobytes())
            f.write(c["H"].tobytes())
            f.write(np.ascontiguousarray(c["src"]).tobytes())


def read_results(path, table):
    """What warp_rule.cpp writes: per case nine float64 (M), one int32 (ok), then the packed warped bytes."""
    data = open(path, "rb").read()
    out, at = [], 0
    for c in table:
        _, ch, bpp = pixel_args(c["kind"])
        M = np.frombuffer(data, f64, 9, at)
        ok = int(np.frombuffer(data, np.int32, 1, at + 72)[0])
        at += 76
        n = c["out_shape"][0] * c["out_shape"][1] * bpp
        img = np.frombuffer(data, np.uint8, n, at)
        at += n
        shape = c["out_shape"] + ((3,) if ch == 3 else ())
        out.append((M, ok, img.view(f32 if c["kind"] == "f32" else np.uint8).reshape(shape)))
    assert at == len(data), "trailing bytes in the result file"
    return out
