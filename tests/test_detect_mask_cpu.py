"""CPU tests of the detection mask: the numpy rule of tests/detect_mask_inputs.py
on hand-written cases, that the inputs of the GPU tests can tell the rounding
rule from its near misses, and that the Python wrappers refuse a bad mask before
any library call."""
import numpy as np
import pytest

import detect_mask_inputs as M
import retain_best_inputs as R


def _keep(x, y, mask):
    return M.keep_mask(np.array([x], np.float32), np.array([y], np.float32), mask).tolist()[0]


def test_half_rounds_up_and_just_below_rounds_down():
    # 0.49999997f + 0.5f rounds to 1.0f: the float sum decides, not the real one
    idx, ok = M.pixel_index(np.array([3.5, 3.4999998, 0.0, 0.49999997, 0.25, 0.5], np.float32), 10)
    assert ok.all() and idx.tolist() == [4, 3, 0, 1, 0, 1]
    mask = np.zeros((2, 10), np.uint8)
    mask[0, 4] = 1
    assert _keep(3.5, 0.0, mask) and not _keep(3.4999998, 0.0, mask)
    mask = np.zeros((2, 10), np.uint8)
    mask[0, 3] = 9      # any non-zero value keeps
    assert _keep(3.4999998, 0.0, mask) and not _keep(3.5, 0.0, mask)


def test_x_is_the_column_and_y_the_row_on_a_non_square_mask():
    mask = np.zeros((4, 9), np.uint8)
    mask[1, 7] = 255
    assert _keep(7.0, 1.0, mask)          # x = 7: column 7, y = 1: row 1
    assert not _keep(1.0, 7.0, mask)      # exchanged: row 7 does not exist
    mask = np.zeros((9, 4), np.uint8)
    mask[7, 1] = 255
    assert _keep(1.0, 7.0, mask) and not _keep(7.0, 1.0, mask)


def test_outside_and_nan_are_dropped():
    rows, cols = 5, 8
    ones = M.full((rows, cols), 255)
    assert _keep(cols - 0.75, rows - 0.75, ones)                  # the last pixel
    assert not _keep(cols - 0.5, 1.0, ones)                       # rounds to column `cols`
    assert not _keep(1.0, rows - 0.5, ones)
    assert _keep(-0.5, -0.5, ones) and _keep(-1.25, 0.0, ones)    # sums in (-1, 0] truncate to index 0
    assert not _keep(-1.5, 0.0, ones) and not _keep(0.0, -1.5, ones)
    for bad in (np.nan, np.inf, -np.inf, 3e9, -3e9, 1e30):
        assert not _keep(bad, 1.0, ones) and not _keep(1.0, bad, ones), bad
    idx, ok = M.pixel_index(np.array([np.nan, 1e30, -1e30], np.float32), cols)
    assert not ok.any() and idx.tolist() == [0, 0, 0]             # nothing out of range was converted


def test_the_sum_is_formed_in_float32():
    # 2^23 + 0.5 is not a float32: the float sum rounds to even, 8388608 + 0.5 -> 8388608
    idx, ok = M.pixel_index(np.array([8388608.0, 8388609.0], np.float32), 1 << 24)
    assert ok.all() and idx.tolist() == [8388608, 8388610]


def test_filter_keeps_order_and_rows():
    kps = np.zeros(4, [("x", "<f4"), ("y", "<f4"), ("octave", "<i4")])
    kps["x"] = [1.0, 5.0, 1.2, 6.0]
    kps["y"] = [1.0, 1.0, 0.6, 0.0]
    desc = np.arange(8, dtype=np.float32).reshape(4, 2)
    k, d = M.filter_keypoints(kps, desc, M.half_plane((3, 8)))   # columns 0..3 kept
    assert k["x"].tolist() == [1.0, np.float32(1.2)] and d.tolist() == [[0, 1], [4, 5]]


def test_masks():
    s = (6, 5)
    assert M.checkerboard(s)[0].tolist() == [255, 0, 255, 0, 255] and M.checkerboard(s)[1, 0] == 0
    assert M.half_plane(s)[3].tolist() == [1, 1, 0, 0, 0]
    w = M.window((40, 30), 8, 4)
    assert w.sum() == 7 * 256 and w[8, 4] and w[23, 19] and not w[24, 19] and not w[8, 20]
    p = M.padded(M.half_plane(s), 3)
    assert p.shape == (6, 8) and p[2].tolist() == [1, 1, 0, 0, 0, 255, 255, 255]
    p = M.padded(M.full(s), 2)
    assert p[:, 5:].max() == 0


# ---- the inputs of the GPU tests -----------------------------------------------------
def test_one_image_input_can_tell_the_rules_apart(oracle):
    """What tests/test_gpu_detect_mask.py asserts again on its unmasked run: the
    stars-and-blobs image alone has both halves of frac(x) and frac(y), octaves
    >= 1 and more distinct positions than a workgroup of the mark kernel has
    threads; and the checkerboard then separates the rounding rule from
    truncation and from exchanged coordinates."""
    kps, _ = oracle.sift(M.stars_blobs_image())
    for v in (kps["x"], kps["y"]):
        lo, hi = M.fractions(v)
        assert lo > 20 and hi > 20
    assert int(((kps["octave"] & 255) >= 1).sum()) >= 5
    assert M.distinct_positions(kps) > M.MARK_THREADS
    cb = M.checkerboard(M.SHAPE)
    want = M.keep_mask(kps["x"], kps["y"], cb)
    assert 0 < want.sum() < len(kps)
    x, y = kps["x"], kps["y"]
    trunc = cb[y.astype(np.int32), x.astype(np.int32)] != 0
    inb = (x + 0.5 < M.SHAPE[0]) & (y + 0.5 < M.SHAPE[1])
    swapped = np.zeros(len(kps), bool)
    swapped[inb] = cb[(x[inb] + np.float32(0.5)).astype(np.int32), (y[inb] + np.float32(0.5)).astype(np.int32)] != 0
    assert (trunc != want).any() and (swapped != want).any()
    # the named inputs of the same shape have part of this each
    k2, _ = oracle.sift(oracle.synth_image(2, *M.SHAPE))
    assert int(((k2["octave"] & 255) >= 1).sum()) >= 5 and min(M.fractions(k2["x"]) + M.fractions(k2["y"])) > 20
    import adversarial_inputs as A
    ks, _ = oracle.sift(A.img_stars(*M.SHAPE))
    assert M.distinct_positions(ks) > M.MARK_THREADS and min(M.fractions(ks["x"]) + M.fractions(ks["y"])) > 20


def test_budget_and_mask_do_not_commute_on_the_test_input(oracle):
    """n = 40 on synth 0 at 160 x 128 with the left half kept: filter(budget run)
    != budget(filter run), so the GPU test pins the order."""
    kps, desc = oracle.sift(oracle.synth_image(0, *M.BATCH_SHAPE))
    hp = M.half_plane(M.BATCH_SHAPE)
    a = M.filter_keypoints(*R.filter_keypoints(kps, desc, 40), hp)[0]
    b = R.filter_keypoints(*M.filter_keypoints(kps, desc, hp), 40)[0]
    assert 0 < len(a) < 40 <= len(b) and a.tobytes() != b.tobytes()


# ---- the wrappers ----------------------------------------------------------------------
class _NoLibrary:
    """Stands in for a Context: any use of the library or the handle fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper reached for {name} before refusing the mask")


@pytest.mark.parametrize("bad", [np.ones((12, 16), np.float32), np.ones((12, 16), np.int32),
                                 np.ones((16, 12), np.uint8), np.ones((12, 15), bool), np.ones((12 * 16,), np.uint8)])
def test_wrappers_refuse_a_bad_mask_without_a_library_call(monkeypatch, bad):
    import siftgpu
    img = np.zeros((12, 16), np.float32)

    def no_lib(*a, **k):
        raise AssertionError("a library call was made")
    monkeypatch.setattr(siftgpu, "lib", no_lib)
    monkeypatch.setattr(siftgpu, "_ctx", no_lib)
    with pytest.raises(ValueError):
        siftgpu.SIFT_NCL(img, mask=bad)
    with pytest.raises(ValueError):
        siftgpu.Context.SIFT_NCL(_NoLibrary(), img, mask=bad)


def test_wrapper_mask_conversion():
    import siftgpu
    m = siftgpu._detection_mask(np.array([[True, False], [False, True]]), (2, 2))
    assert m.dtype == np.uint8 and m.tolist() == [[1, 0], [0, 1]] and m.flags.c_contiguous
    v = np.arange(12, dtype=np.uint8).reshape(3, 4)[:, ::2]      # a strided view is packed
    m = siftgpu._detection_mask(v, (3, 2))
    assert m.flags.c_contiguous and m.tolist() == v.tolist()
    assert siftgpu._detection_mask(None, (3, 2)) is None
