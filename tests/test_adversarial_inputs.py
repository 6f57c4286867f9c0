"""CPU-side coverage of the crafted inputs (tests/adversarial_inputs.py): which
branches of the extrema stage each committed case reaches, asserted on the
oracle's branch counters alone (oracle.extrema_stats).  No GPU.  This is what
makes the bit-for-bit GPU comparison of tests/test_gpu_adversarial.py
meaningful: a generator change cannot silently lose a branch.

Observed on the oracle (every minimum below is about half of these).  Columns:
n keypoints | raw extrema | kept | rejected: offset > INT_MAX/3, layer range,
border, max-interp, contrast, det <= 0, edge | converged after moving: layer,
r or c | v > 0, v < 0 | clipped orientation windows | largest peak count |
keypoints per octave 0..3 | per layer 1, 2

  white    96x128   6201 |  1861  1781 | 0   27   2   42  0   5  4 |   4  13 |  936  925 |  672 | 9 | 4976 1081 138  6 | 2708 3493
  white    83x117   4465 |  1428  1369 | 0   29   1   27  0   1  1 |   4   5 |  719  709 |  553 | 8 | 3706  669  90  0 | 2004 2461
  smooth   96x128   1826 |   652   569 | 0   56   2   20  0   3  2 |   4   9 |  317  335 |  218 | 7 | 1516  279  27  4 |  774 1052
  smooth   83x117   1373 |   489   420 | 0   37   0   26  0   2  4 |   5  14 |  250  239 |  172 | 8 | 1141  207  25  0 |  614  759
  plateau  96x128    828 |  4722   249 | 0 2016 253 1721 50 401 32 | 105 524 | 2361 2361 |   64 | 7 |  707  113   8  0 |  317  511
  plateau  83x117    734 |  3554   221 | 0 1542 133 1293 52 283 30 | 100 423 | 1784 1770 |   77 | 7 |  585  141   8  0 |  369  365
  flat     96x128      0 |  1834  1757 | 0   26   1   42  2   3  3 |   3   8 |  900  934 |  656 | 0 |    0    0   0  0 |    0    0
  flat     83x117      0 |  1377  1328 | 0   19   1   22  2   2  3 |   4   9 |  699  678 |  518 | 0 |    0    0   0  0 |    0    0
  checker  96x128   7104 |  1836  1776 | 0   26   2   23  2   4  3 |   7  14 |  916  920 |  642 | 4 | 5812 1112 176  4 | 3520 3584
  checker  83x117   5156 |  1352  1289 | 0   27   1   30  1   3  1 |   3  12 |  668  684 |  518 | 4 | 4244  816  96  0 | 2580 2576
  planted  96x128     21 |    45     7 | 2    0   0   10  0  26  0 |   4   4 |   40    5 |    5 | 5 |   21    0   0  0 |   13    8
  planted  83x117     25 |    45     7 | 2    0   0   10  0  26  0 |   4   4 |   40    5 |    5 | 5 |   25    0   0  0 |   21    4
  regrow  256x320  46663 | 14431 13907 | 0  231   3  228 13  27 22 |  32  95 | 7237 7194 | 2207 | 9 | 36060 8375 1887 316 | 20892 25771

Mean peaks per kept candidate: white 3.48 / 3.26, checker exactly 4 (every
histogram has four tied maxima), regrow 3.36.  The largest orientation radius
is 17 in the random families.  Only the planted "huge" neighbourhoods reach the
INT_MAX/3 rejection (see adversarial_inputs.planted_neighbourhoods for why no
first refinement step can), and the planted "half" ones sit exactly on the
0.5f boundary (8 max-interp rejections: the 4 planted centres and their 4
equal neighbours; 2 more from the "nan_offset" pair, whose finite pixels
overflow the 3 x 3 solve to a NaN offset).  Every rejection reason is reachable
with finite inputs.

Images (keypoints at 240x320 / 203x157): noise_u8 52 / 15, fractional 49 / 25,
u16_range 225 / 55, signed 22 / 5, stars 1334 / 544 (1.87 / 1.90 peaks per
kept candidate), constant 0 / 0, constant_bright 4 / 0.
"""
import numpy as np
import pytest

import adversarial_inputs as A

SCALARS = ("raw_extrema", "kept", "rej_offset_huge", "rej_layer", "rej_border", "rej_max_interp", "rej_contrast",
           "rej_det", "rej_edge", "moved_layer", "moved_rc", "positive", "negative", "orient_clipped")


@pytest.fixture(scope="module")
def pyramid_stats(oracle):
    """{(family, rows, cols): (keypoint count, stats)} of every committed pyramid case."""
    out = {}
    for fam, r, c in A.pyramid_cases():
        g, d = A.PYRAMID_FAMILIES[fam](r, c)
        kps = oracle.find_scale_space_extrema(g, d, r, c)
        out[fam, r, c] = (len(kps), oracle.extrema_stats())
    return out


def test_stats_are_consistent_and_change_nothing(oracle):
    """The counters add up, describe the last call only, and counting leaves
    the result untouched (two runs, byte-identical)."""
    g, d = A.pyr_white(96, 128)
    k1 = oracle.find_scale_space_extrema(g, d, 96, 128)
    s = oracle.extrema_stats()
    k2 = oracle.find_scale_space_extrema(g, d, 96, 128)
    s2 = oracle.extrema_stats()
    assert k1.tobytes() == k2.tobytes()
    assert {k: v for k, v in s.items() if k != "keypoints"} == {k: v for k, v in s2.items() if k != "keypoints"}
    assert np.array_equal(s["keypoints"], s2["keypoints"])
    rejected = sum(s[k] for k in s if k.startswith("rej_"))
    assert s["raw_extrema"] == s["positive"] + s["negative"] == s["kept"] + rejected
    assert sum(s["peaks_hist"]) == s["kept"]
    assert sum(i * n for i, n in enumerate(s["peaks_hist"])) == len(k1) == int(s["keypoints"].sum())
    oct_ = k1["octave"] & 255
    lay = (k1["octave"] >> 8) & 255
    for o in range(5):
        for ly in (1, 2):
            assert s["keypoints"][o, ly - 1] == np.count_nonzero((oct_ == o) & (lay == ly))
    oracle.extrema_stats_reset()
    z = oracle.extrema_stats()
    assert z["raw_extrema"] == 0 and not z["keypoints"].any() and not any(z["peaks_hist"])


def test_every_branch_is_reached(pyramid_stats):
    tot = {k: sum(s[k] for _, s in pyramid_stats.values()) for k in SCALARS}
    # about half of the observed totals over the 12 committed cases
    minimum = {"raw_extrema": 9500, "kept": 5400, "rej_offset_huge": 2, "rej_layer": 1900, "rej_border": 190,
               "rej_max_interp": 1600, "rej_contrast": 55, "rej_det": 370, "rej_edge": 40, "moved_layer": 120,
               "moved_rc": 500, "positive": 4800, "negative": 4700, "orient_clipped": 2000}
    for k, m in minimum.items():
        assert tot[k] >= m >= 1, (k, tot[k], m)


@pytest.mark.parametrize("fam,reasons", [
    ("white", {"rej_layer": 25, "rej_max_interp": 30, "moved_rc": 8, "moved_layer": 3}),
    ("smooth", {"rej_layer": 45, "rej_max_interp": 20, "moved_rc": 10, "moved_layer": 4}),
    ("plateau", {"rej_layer": 1700, "rej_border": 190, "rej_max_interp": 1500, "rej_contrast": 50, "rej_det": 340,
                 "rej_edge": 30, "moved_layer": 100, "moved_rc": 470}),
    ("planted", {"rej_offset_huge": 4, "rej_max_interp": 20, "rej_det": 26, "kept": 7}),
])
def test_family_reaches_what_it_is_for(pyramid_stats, fam, reasons):
    """Per family, summed over both shapes (minima about half the observed;
    the planted counts are exact by construction)."""
    for k, m in reasons.items():
        got = sum(s[k] for (f, _, _), (_, s) in pyramid_stats.items() if f == fam)
        assert got >= m, (fam, k, got, m)


def test_layers_octaves_and_peak_counts(pyramid_stats):
    kp = sum(s["keypoints"] for _, s in pyramid_stats.values())
    assert kp[:, 0].sum() >= 6500 and kp[:, 1].sum() >= 7400          # layers 1 and 2
    for o, m in enumerate((11000, 2200, 280, 7)):                      # octaves 0..3
        assert kp[o].sum() >= m, (o, kp[o])
    hist = np.sum([s["peaks_hist"] for _, s in pyramid_stats.values()], axis=0)
    assert hist[6:].sum() >= 170                                       # some candidate has >= 6 peaks
    assert max(i for i, n in enumerate(hist) if n) >= 8                # observed 9
    means = {k: n / s["kept"] for k, (n, s) in pyramid_stats.items() if s["kept"]}
    assert max(means.values()) > 2 and means["white", 96, 128] > 2     # observed 3.48
    assert max(s["max_orient_radius"] for _, s in pyramid_stats.values()) >= 14   # observed 17


def test_flat_planes_keep_candidates_and_emit_nothing(pyramid_stats):
    for shape in A.PYRAMID_SHAPES:
        n, s = pyramid_stats[("flat",) + shape]
        assert n == 0 and s["kept"] >= 600 and s["peaks_hist"][0] == s["kept"]


def test_checker_histograms_tie(pyramid_stats):
    """Every kept candidate of the checkerboard family has exactly 4 peaks."""
    for shape in A.PYRAMID_SHAPES:
        n, s = pyramid_stats[("checker",) + shape]
        assert s["kept"] >= 600 and s["peaks_hist"][4] == s["kept"] and n == 4 * s["kept"]


def test_regrow_case_fits_the_workspace_and_outgrows_the_buffer(oracle):
    """The keypoints exceed a fresh context's internal buffer (so the library
    must grow it and run again) while the raw extrema still fit its candidate
    workspace (so the run is no SIFT_E_WORKSPACE error)."""
    r, c = A.REGROW_SHAPE
    cap = A.default_candidate_capacity(r, c)
    per_slot = A.keypoints_per_candidate_slot()
    g, d = A.regrow_pyramid()
    kps = oracle.find_scale_space_extrema(g, d, r, c)
    s = oracle.extrema_stats()
    assert s["raw_extrema"] <= cap, (s["raw_extrema"], cap)
    assert s["raw_extrema"] >= 7000                                    # observed 14431
    assert len(kps) > per_slot * cap, (len(kps), per_slot, cap)
    assert s["keypoints"][:4].sum(1).min() >= 150                      # octaves 0..3, observed 316 in octave 3


@pytest.mark.parametrize("fam,minimum", [("noise_u8", (26, 7)), ("fractional", (24, 12)), ("u16_range", (110, 27)),
                                         ("signed", (11, 2)), ("stars", (660, 270)), ("constant_bright", (2, 0))])
def test_image_families_yield_keypoints(oracle, fam, minimum):
    for shape, m in zip(A.IMAGE_SHAPES, minimum):
        img = A.IMAGE_FAMILIES[fam](*shape)
        assert img.dtype == np.float32 and np.isfinite(img).all()
        kps, desc = oracle.sift(img)
        assert len(kps) >= m, (fam, shape, len(kps))
        assert np.isfinite(desc).all()


def test_image_value_ranges():
    """The families are what their names say: fractional values, values above
    255, negative values."""
    f = A.img_fractional(*A.IMAGE_SHAPES[0])
    assert np.count_nonzero(f != np.round(f)) > f.size * 0.9 and f.min() >= 0 and f.max() <= 255
    assert A.img_u16_range(*A.IMAGE_SHAPES[0]).max() > 60000
    assert A.img_signed(*A.IMAGE_SHAPES[0]).min() < -200
    u8 = A.img_noise_u8(*A.IMAGE_SHAPES[0])
    assert np.array_equal(u8, np.round(u8)) and u8.min() == 0 and u8.max() == 255


def test_stars_have_multiple_peaks_and_constant_is_empty(oracle):
    for shape in A.IMAGE_SHAPES:
        kps, _ = oracle.sift(A.img_stars(*shape))
        s = oracle.extrema_stats()
        assert len(kps) / s["kept"] > 1.4                              # observed 1.87 / 1.90
        kps, desc = oracle.sift(A.img_constant(*shape))
        assert len(kps) == 0 and desc.shape == (0, 128)
    assert A.BATCH_ORDER[0] == A.BATCH_ORDER[2] == A.BATCH_ORDER[-1] == "constant"


def test_generators_are_deterministic():
    for fam, r, c in A.pyramid_cases():
        g1, d1 = A.PYRAMID_FAMILIES[fam](r, c)
        g2, d2 = A.PYRAMID_FAMILIES[fam](r, c)
        assert g1.tobytes() == g2.tobytes() and d1.tobytes() == d2.tobytes()
        assert np.isfinite(g1).all() and np.isfinite(d1).all()
        n = sum(rr * cc for rr, cc in A.octave_shapes(r, c))
        assert g1.shape == (5 * n,) and d1.shape == (4 * n,) and g1.dtype == d1.dtype == np.float32
    for fam, f in A.IMAGE_FAMILIES.items():
        assert f(*A.IMAGE_SHAPES[1]).tobytes() == f(*A.IMAGE_SHAPES[1]).tobytes(), fam
