"""Inputs of the provided-keypoint tests (sift_compute_batch / sift_compute):
crafted keypoint rows, the dense grid, the invalid rows, and a numpy restatement
of the two quantities the device prep stage derives from a row -- the window
radius and the keypoint's pixel (descriptor.hip's setup, float32 step by step) --
so the tests can assert from the inputs which descriptor form each row takes."""
import numpy as np

KEYPOINT_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

SHAPES = [(203, 157), (160, 128)]   # rows x cols; 203 x 157: the 5th octave is 12 x 9
N_OCT = 5
DET_RADIUS = 40                     # descriptor.hip: windows with a row table


def rows_of(spec):
    """spec: (x, y, size, angle, octave, layer) tuples -> KEYPOINT_DTYPE rows."""
    k = np.zeros(len(spec), KEYPOINT_DTYPE)
    for i, (x, y, size, angle, octave, layer) in enumerate(spec):
        k[i] = (x, y, size, angle, 0.5, (octave & 255) | (layer << 8), -1)
    return k


def unpack(kps):
    o = kps["octave"] & 255
    o = np.where(o < 128, o, o - 256)
    return o, (kps["octave"] >> 8) & 255


def valid(kps, max_layer=4, n_oct=N_OCT):
    o, layer = unpack(kps)
    return (o >= 0) & (o < n_oct) & (layer <= 4) & (layer <= max_layer)


def window(kps, shape):
    """(radius, px, py, octave rows, octave cols) of valid rows, as the kernel forms them."""
    f = np.float32
    o, _ = unpack(kps)
    o = np.clip(o, 0, N_OCT - 1)
    scale = (f(1) / (1 << o).astype(f)).astype(f)
    size = (kps["size"] * scale).astype(f)
    hw = (f(3) * (size * f(0.5)).astype(f)).astype(f)
    v = ((hw * f(1.4142135623730951)).astype(f) * f(5)).astype(f) * f(0.5)
    radius = np.rint(v.astype(f)).astype(np.int64)          # cvRound: to nearest, ties to even
    rows, cols = shape[0] >> o, shape[1] >> o
    diag = np.floor(np.sqrt(cols.astype(np.float64) ** 2 + rows.astype(np.float64) ** 2)).astype(np.int64)
    px = np.rint((kps["x"] * scale).astype(f)).astype(np.int64)
    py = np.rint((kps["y"] * scale).astype(f)).astype(np.int64)
    return np.minimum(radius, diag), px, py, rows, cols, radius > diag


def takes_det(kps, shape):
    """Rows the detected-keypoint form of the descriptor kernel can take."""
    r, px, py, rows, cols, _ = window(kps, shape)
    return (kps["size"] > 0) & (r <= DET_RADIUS) & (px >= 1) & (px <= cols - 2) & (py >= 1) & (py <= rows - 2)


def crafted(shape, variant=0):
    """Valid rows that reach every branch: layers 0 and 4, octave 4, radius 40 and 41
    and one clamped to the image diagonal, points on and outside the border, the
    angles 0, 360 and the float below it."""
    R, C = shape
    v = float(variant)
    below360 = float(np.nextafter(np.float32(360), np.float32(0)))   # 359.99997
    spec = [
        (C / 2 + v, R / 2, 3.2, 0.0, 0, 1),
        (C / 2, R / 2 + v, 4.1, 360.0, 0, 2),
        (C / 3, R / 3, 5.0, below360, 0, 3),
        (40.25 + v, 50.5, 2.5, 77.0, 0, 0),                 # layer 0
        (60.0, 70.75 + v, 6.0, 191.5, 0, 4),                # layer 4
        (C / 2, R / 2, 7.54, 33.0, 0, 2),                   # radius 40
        (C / 2, R / 2, 7.73, 33.0, 0, 2),                   # radius 41
        (C / 2, R / 2, 2 * 7.54, 120.0, 1, 1),              # radius 40 in octave 1
        (C / 2, R / 2, 2 * 7.73, 120.0, 1, 2),              # radius 41 in octave 1
        (C / 2, R / 2, 100.0, 250.0, 0, 1),                 # clamped to the diagonal
        (80.0 + v, 100.0, 20.0, 10.0, 4, 1),                # octave 4
        (70.0, 90.0 + v, 300.0, 300.0, 4, 3),               # octave 4, clamped
        (30.0, 45.0, 9.0, 45.0, 2, 2),
        (100.0, 120.0, 14.0, 135.0, 3, 1),
        (0.0, 0.0, 4.0, 20.0, 0, 1),                        # on the corner
        (C - 1.0, R - 1.0, 4.0, 200.0, 0, 2),               # on the far corner
        (0.4, R / 2, 3.0, 90.0, 0, 1),                      # rounds onto the border column
        (1.0, 1.0, 3.0, 0.0, 0, 1),                         # first interior pixel
        (C - 2.0, R - 2.0, 3.0, 360.0, 0, 1),               # last interior pixel
        (-5.0, 10.0, 6.0, 15.0, 0, 2),                      # outside, left
        (C + 3.0, R + 2.0, 8.0, 15.0, 0, 2),                # outside, beyond the far corner
        (C / 2, -30.0, 3.0, 15.0, 1, 1),                    # outside, window misses the image
    ]
    return rows_of(spec)


INVALID = [("octave 254 (-2)", 254, 1, 4), ("octave = n_octaves", N_OCT, 1, 4), ("layer 5", 0, 5, 4),
           ("layer 4 under max_layer 3", 0, 4, 3)]


def invalid_row(octave, layer):
    return rows_of([(50.0, 60.0, 4.0, 30.0, octave, layer)])


def dense_grid(shape, step=4, size=4.0):
    """One keypoint per step pixels, one size, octave 0 layer 1, angles that vary."""
    R, C = shape
    ys, xs = np.mgrid[step // 2:R:step, step // 2:C:step]
    k = np.zeros(xs.size, KEYPOINT_DTYPE)
    k["x"], k["y"] = xs.reshape(-1), ys.reshape(-1)
    k["size"] = size
    k["angle"] = (np.arange(xs.size) * 37) % 360
    k["response"] = 1.0
    k["octave"] = 0 | (1 << 8)
    k["class_id"] = -1
    return k


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
