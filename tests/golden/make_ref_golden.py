"""Record outputs of the reference's own source as fixtures: tests/golden/ref_*.npz.

Run from the repo root:  python tests/golden/make_ref_golden.py   (--1080p: the
one-off digest set of the headline workload, about a minute of CPU; --args: only
the ref_args_* family)

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

The family ref_args_*.npz (inputs: tests/module_arg_inputs.py) covers the
arguments the module entry points accept beyond what SIFT_NCL passes:
  ref_args_blur     digests of Gaussian_Blur and Gaussian_Blur_1D per (shape, sigma);
  ref_args_img_<id> per (image, octave count): plane digests, keypoints, descriptors.
                    buildGaussianPyramid is the reference's only with 5 octaves
                    (src/sift.cpp:248); for another count `gpyr_sha` are the digests
                    of the planes the reference's buildDoGPyramid /
                    findScaleSpaceExtrema / calDescriptor were given (`gpyr_from`
                    says which), and everything else is what those returned;
  ref_args_caller_fo<k>   calDescriptor(gpyr, caller keypoints, firstOctave = k), the rows
                    `rows` whose angle is inside the reference's contract, [0, 720].
"""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import adversarial_inputs as A  # noqa: E402
import module_arg_inputs as M  # noqa: E402
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


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _desc_fields(kps, desc, desc_oracle):
    """libm_rows / desc_def as in record(): the rows at libm-dependent angles, under the oracle's definition."""
    rows = np.flatnonzero(RI.libm_rows(O, R, kps)).astype(np.int32) if len(kps) else np.zeros(0, np.int32)
    differ = np.flatnonzero((desc.view(np.uint32) != desc_oracle.view(np.uint32)).any(axis=1))
    assert np.isin(differ, rows).all()
    return dict(desc=desc, libm_rows=rows, desc_def=desc_oracle[rows])


def record_args():
    # ---- blurs: digests only
    cases = M.blur_cases()
    out = dict(ids=np.array([M.blur_id(c) for c in cases]), libm=libm_name())
    out["blur_sha"] = np.array([_sha(R.gaussian_blur(M.blur_image(*c), c[2])) for c in cases])
    out["blur1d_sha"] = np.array([_sha(R.gaussian_blur_1d(M.blur_image(*c), c[2])) for c in cases])
    np.savez_compressed(os.path.join(OUT, "ref_args_blur.npz"), **out)
    print(f"ref_args_blur: {len(cases)} cases")
    # ---- images: octave counts 6 .. 8 and degenerate shapes
    seen = {}
    for case in M.OCTAVE_CASES + M.DEGENERATE_CASES:
        b, r, c, n = case
        key = M.image_id(case)
        img = O.synth_image(b, r, c)
        if n == 5:
            g, src = R.build_gaussian_pyramid(img), "reference"
        else:
            g, src = O.build_gaussian_pyramid(img, n), "oracle"
        d = R.build_dog_pyramid(g, r, c, n)
        kps = R.find_scale_space_extrema(g, d, r, c, n)
        desc = R.calc_descriptors(g, r, c, kps, n)
        ko = O.find_scale_space_extrema(g, d, r, c, n)
        assert kps.tobytes() == ko.tobytes(), "pick an input whose keypoints do not depend on powf"
        if n == 5:
            ks, ds = R.sift(img)
            assert ks.tobytes() == kps.tobytes() and ds.tobytes() == desc.tobytes()
        out = dict(seed=b, rows=r, cols=c, n_octaves=n, n=len(kps), libm=libm_name(), gpyr_from=src,
                   gpyr_sha=np.array([_sha(p) for p in O.split_planes(g, r, c, n, 5)]),
                   dog_sha=np.array([_sha(p) for p in O.split_planes(d, r, c, n, 4)]))
        same = seen.get((kps.tobytes(), desc.tobytes()))
        if same is not None and len(kps):
            out["same_as"] = same       # keypoints and descriptors byte for byte those of that file
        else:
            seen[(kps.tobytes(), desc.tobytes())] = "ref_args_img_" + key
            out["kps"] = kps.view(np.uint8).reshape(len(kps), 28) if len(kps) else np.zeros((0, 28), np.uint8)
            f = _desc_fields(kps, desc, O.calc_descriptors(g, r, c, kps, n))
            if len(kps) > 500:          # too many rows for a small file: the digest of what
                out["desc_sha"] = _sha(RI.expected_device_descriptors(f))    # expected_device_descriptors gives,
                hi = np.flatnonzero((kps["octave"] & 255) >= 4)             # and the rows of octaves 4 and up in full
                out["desc_rows"] = hi.astype(np.int32)
                out["desc_rows_bytes"] = RI.expected_device_descriptors(f)[hi]
            else:
                out.update(f)
        np.savez_compressed(os.path.join(OUT, f"ref_args_img_{key}.npz"), **out)
        print(f"ref_args_img_{key}: {len(kps)} keypoints, Gaussian planes from the {src}")
    # ---- caller keypoints at each firstOctave
    b, r, c = M.CALLER_IMAGE
    g = R.build_gaussian_pyramid(O.synth_image(b, r, c))
    for fo in M.FIRST_OCTAVES:
        kps = M.caller_keypoints(fo, O.KEYPOINT_DTYPE)
        rows = np.flatnonzero(~M.angle_outside_contract(kps)).astype(np.int32)
        kps = kps[rows]     # angle -30 is outside the reference's contract: its bytes there follow its memory layout
        desc = R.calc_descriptors(g, r, c, kps, M.CALLER_OCTAVES, fo)
        out = dict(first_octave=fo, libm=libm_name(), kp_sha=_sha(kps), rows=rows,
                   **_desc_fields(kps, desc, O.calc_descriptors(g, r, c, kps, M.CALLER_OCTAVES, fo)))
        np.savez_compressed(os.path.join(OUT, f"ref_args_caller_fo{fo}.npz"), **out)
        print(f"ref_args_caller_fo{fo}: {len(kps)} keypoints, {len(out['libm_rows'])} at libm-dependent angles")


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
    if "--args" in sys.argv:
        record_args()
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
    record_args()


if __name__ == "__main__":
    main()
