"""Shared by the tests that use tests/golden/ref_*.npz (outputs recorded from the
reference's own source) and by tests/golden/make_ref_golden.py, which writes them."""
import numpy as np

import adversarial_inputs as A
from conftest import book_image, load_golden

REF_FIXTURES = ["ref_book", "ref_synth_160x128", "ref_synth_203x157", "ref_synth_240x320",
                "ref_fractional_203x157", "ref_stars_203x157"]


def ref_input(name, oracle):
    """The image a fixture was recorded from."""
    g = load_golden(name)
    if name == "ref_book":
        return book_image()
    if "seed" in g.files:
        return oracle.synth_image(int(g["seed"]), int(g["rows"]), int(g["cols"]))
    return A.IMAGE_FAMILIES[str(g["family"])](int(g["rows"]), int(g["cols"]))


def descriptor_angles(kps):
    """The radians that calcSIFTDescriptor hands to cosf / sinf (src/sift.cpp:748-751, :583)."""
    ang = np.float32(360) - kps["angle"]
    ang = np.where(np.abs(ang - np.float32(360)) < np.finfo(np.float32).eps, np.float32(0), ang)
    return ang.astype(np.float32) * np.float32(np.pi / 180)


def libm_rows(oracle, refsrc, kps):
    """Mask of the keypoints at whose descriptor angle libm's cosf or sinf (refsrc.helper) is not
    (float)cos / sin((double)x) (oracle.helper)."""
    x = descriptor_angles(kps)
    bad = np.zeros(len(kps), bool)
    for op in (3, 4):
        bad |= oracle.helper(op, x).view(np.uint32) != refsrc.helper(op, x).view(np.uint32)
    return bad


def expected_device_descriptors(g):
    """What the oracle's and the device's definition gives for a fixture: the reference's
    descriptors, with the rows at libm-dependent angles (`libm_rows`) taken from `desc_def`,
    their bytes under (float)f((double)x)."""
    d = g["desc"].copy()
    d[g["libm_rows"]] = g["desc_def"]
    return d


def args_image_fixture(key):
    """(g, k) of tests/golden/ref_args_img_<key>.npz: g holds the plane digests, k the keypoints and
    descriptors (another file of the family where the same bytes were recorded for a smaller octave count)."""
    g = load_golden("ref_args_img_" + key)
    return g, (load_golden(str(g["same_as"])) if "same_as" in g.files else g)


def check_fixture_descriptors(desc, k, what):
    """desc against the descriptors of a ref_args_img_* fixture: every byte, or, where the file holds
    only their digest (more than 500 rows), the digest and the rows of octaves 4 and up in full."""
    from conftest import assert_bits_equal, sha
    if "desc" in k.files:
        assert_bits_equal(desc, expected_device_descriptors(k), what)
    else:
        assert_bits_equal(desc[k["desc_rows"]], k["desc_rows_bytes"], what + " (octaves 4 and up)")
        assert sha(desc) == str(k["desc_sha"]), what + ": digest"
