"""Record outputs of the reference's own source as fixtures: tests/golden/ref_*.npz.

Run from the repo root:  python tests/golden/make_ref_golden.py   (--1080p: the
one-off digest set of the headline workload, about a minute of CPU)

Unlike make_golden.py, nothing here comes from the CPU oracle: every array is
what oracle/_ref/libsift_ref.so computed, i.e. the reference's src/sift.cpp
compiled unmodified with its makefile's flags over the stand-in OpenCV headers
of oracle/cvmini/ (oracle/ref_build.py).  It needs the reference tree, and no
test runs it.  Only data is stored (np.load(allow_pickle=False)).

Per input: SHA-256 of every Gaussian and DoG plane, the keypoint records, the
descriptors, `libm_rows`: the keypoints whose descriptor angle is one at
which this machine's libm cosf / sinf (named in `libm`) differ from
(float)cos / sin((double)x), the definition the oracle and the device keep
(DESIGN.md section 3), and `desc_def`: those rows under that definition (the
only bytes here that the oracle computed).  The 1080p set holds digests only,
with the digest of the keypoints less their `size` and the indices of the
sizes and descriptor rows that follow libm.

The synthetic seeds are ones for which every recorded byte equals the oracle's, so that the GPU can be asserted against them byte for
byte: at 160x128 and 203x157 the seeds of make_golden.py (0 and 2) already
are; at 240x320 its seed 1 has 4 descriptor rows that follow libm, and 157 is
the first seed, trying 0, 1, 2, ... in order (--search), that has none and at
most 450 keypoints (which keeps the file under the size of the largest older
fixture; seed 83 agrees too, with 477).
`book` is a fixed image and keeps its one differing row.
"""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import adversarial_inputs as A  # noqa: E402
import reference_inputs as RI  # noqa: E402
import oracle as O  # noqa: E402
import refsrc as R  # noqa: E402
from conftest import book_image  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

# name -> how tests rebuild the input (tests/reference_inputs.py: ref_input)
SYNTH = {"ref_synth_160x128": (0, 160, 128), "ref_synth_203x157": (2, 203, 157),
         "ref_synth_240x320": (157, 240, 320)}
FAMILY = {"ref_fractional_203x157": ("fractional", 203, 157), "ref_stars_203x157": ("stars", 203, 157)}


def libm_name():
    f = ctypes.CDLL(None).gnu_get_libc_version
    f.restype = ctypes.c_char_p
    return "glibc " + f().decode()


def digests(packed, rows, cols, per):
    return np.array([hashlib.sha256(p.tobytes()).hexdigest() for p in O.split_planes(packed, rows, cols, 5, per)])


def record(name, img, store_full=True, **extra):
    img = np.ascontiguousarray(img, np.float32)
    r, c = img.shape
    g = R.build_gaussian_pyramid(img)
    d = R.build_dog_pyramid(g, r, c)
    kps, desc = R.sift(img)
    out = dict(rows=r, cols=c, n=len(kps), libm=libm_name(),
               kp_sha=hashlib.sha256(kps.tobytes()).hexdigest(),
               desc_sha=hashlib.sha256(desc.tobytes()).hexdigest(),
               gpyr_sha=digests(g, r, c, 5), dog_sha=digests(d, r, c, 4), **extra)
    # against the oracle's definition, (float)f((double)x): which bytes follow libm instead
    ko, do = O.sift(img)
    assert len(ko) == len(kps)
    nosize = kps.copy()
    nosize["size"] = 0
    ko_nosize = ko.copy()
    ko_nosize["size"] = 0
    assert nosize.tobytes() == ko_nosize.tobytes()
    out["kp_nosize_sha"] = hashlib.sha256(nosize.tobytes()).hexdigest()
    size_rows = np.flatnonzero(kps["size"].view(np.uint32) != ko["size"].view(np.uint32)).astype(np.int32)
    desc_rows = np.flatnonzero((desc.view(np.uint32) != do.view(np.uint32)).any(axis=1)).astype(np.int32)
    if store_full:
        assert size_rows.size == 0, "pick an input whose keypoint sizes do not depend on powf"
        out["kps"] = kps.view(np.uint8).reshape(len(kps), 28) if len(kps) else np.zeros((0, 28), np.uint8)
        out["desc"] = desc
        rows = np.flatnonzero(RI.libm_rows(O, R, kps)).astype(np.int32)
        assert np.isin(desc_rows, rows).all()
        out["libm_rows"] = rows
        out["desc_def"] = do[rows]          # those rows under the oracle's and the device's definition
    else:
        out["libm_size_rows"] = size_rows   # keypoints whose `size` follows powf
        out["libm_desc_rows"] = desc_rows   # descriptor rows that follow cosf / sinf
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    print(f"{name}: {r}x{c} -> {len(kps)} keypoints, {len(desc_rows)} descriptor rows and {len(size_rows)} sizes "
          f"follow libm")


def first_agreeing_seed(rows, cols, limit=400):
    """How the seeds in SYNTH were found."""
    for b in range(limit):
        img = O.synth_image(b, rows, cols)
        k0, e0 = O.sift(img)
        k1, e1 = R.sift(img)
        if len(k0) <= 450 and k0.tobytes() == k1.tobytes() and e0.tobytes() == e1.tobytes():
            return b
    raise SystemExit(f"no seed below {limit} at {rows}x{cols}")


def main():
    if not R.available():
        raise SystemExit("needs the reference tree (SIFT_REFERENCE_DIR) or a built oracle/_ref/")
    O.build()
    if "--1080p" in sys.argv:
        record("ref_synth0_1080x1920", O.synth_image(0, 1080, 1920), store_full=False)
        return
    if "--search" in sys.argv:
        for name, (_, r, c) in SYNTH.items():
            print(name, first_agreeing_seed(r, c))
        return
    record("ref_book", book_image())
    for name, (b, r, c) in SYNTH.items():
        record(name, O.synth_image(b, r, c), seed=b)
    for name, (fam, r, c) in FAMILY.items():
        record(name, A.IMAGE_FAMILIES[fam](r, c), family=fam)


if __name__ == "__main__":
    main()
