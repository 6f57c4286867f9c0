"""The HIP path against recorded outputs of the reference's own source.

tests/golden/ref_*.npz were written by tests/golden/make_ref_golden.py from
the reference's src/sift.cpp, compiled unmodified over the stand-in OpenCV
headers of oracle/cvmini/ -- not by the CPU oracle.  Nothing here reads the
reference tree or oracle/_ref/.

Every comparison is total and byte for byte.  src/sift.cpp calls libm's
cosf / sinf / powf; the device, like the oracle, takes (float)f((double)x)
(DESIGN.md section 3).  No recorded keypoint byte depends on that.  Of the
descriptors, the rows at libm-dependent angles (`libm_rows`, a few per
fixture) are expected to equal `desc_def`, their bytes under the device's
definition, and every other row the reference's.  The synthetic and crafted
inputs sit at seeds where the two are the same bytes; in `book`, a fixed image,
one row of 128 differs (tests/test_reference_source.py asserts which).
"""
import numpy as np
import pytest

from conftest import assert_bits_equal, kp_bytes, load_golden, sha
from reference_inputs import REF_FIXTURES, expected_device_descriptors, ref_input

pytestmark = pytest.mark.gpu


def _keypoints_equal(name, g, kps):
    assert len(kps) == int(g["n"]) > 0
    assert_bits_equal(kp_bytes(kps), g["kps"], f"{name} keypoints")


def _descriptors_equal(name, g, desc):
    keep = np.ones(int(g["n"]), bool)
    keep[g["libm_rows"]] = False
    assert_bits_equal(desc[keep], g["desc"][keep], f"{name} descriptors, rows that no libm call decides")
    assert_bits_equal(desc[g["libm_rows"]], g["desc_def"], f"{name} descriptors, rows at libm-dependent angles")
    assert_bits_equal(desc, expected_device_descriptors(g), f"{name} descriptors")


# ---- SIFT_NCL ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", REF_FIXTURES)
def test_sift_ncl_keypoints(ctx, oracle, name):
    g = load_golden(name)
    img = ref_input(name, oracle)
    assert max(img.shape) <= 420 and min(img.shape) <= 300
    _keypoints_equal(name, g, ctx.SIFT_NCL(img)[0])


@pytest.mark.parametrize("name", REF_FIXTURES)
def test_sift_ncl_descriptors(ctx, oracle, name):
    _descriptors_equal(name, load_golden(name), ctx.SIFT_NCL(ref_input(name, oracle))[1])


# ---- the module chain -------------------------------------------------------------------------
@pytest.mark.parametrize("name", REF_FIXTURES)
def test_pyramid_plane_digests(ctx, oracle, name):
    g = load_golden(name)
    gp = ctx.buildGaussianPyramid(ref_input(name, oracle), 5)
    assert [sha(p) for p in gp] == list(g["gpyr_sha"])
    assert [sha(p) for p in ctx.buildDoGPyramid(gp, 5)] == list(g["dog_sha"])


def _chain(ctx, img):
    gp = ctx.buildGaussianPyramid(img, 5)
    kps = ctx.findScaleSpaceExtrema(gp, ctx.buildDoGPyramid(gp, 5), 5)
    return kps, ctx.calDescriptor(gp, kps, 0)


@pytest.mark.parametrize("name", REF_FIXTURES)
def test_module_chain_keypoints(ctx, oracle, name):
    _keypoints_equal(name, load_golden(name), _chain(ctx, ref_input(name, oracle))[0])


@pytest.mark.parametrize("name", REF_FIXTURES)
def test_module_chain_descriptors(ctx, oracle, name):
    _descriptors_equal(name, load_golden(name), _chain(ctx, ref_input(name, oracle))[1])


# ---- one batch call over every same-shaped input ------------------------------------------------
def test_detect_compute_batch(ctx, oracle):
    import torch
    names = [n for n in REF_FIXTURES if (int(load_golden(n)["rows"]), int(load_golden(n)["cols"])) == (203, 157)]
    assert len(names) == 3
    B, R, C = len(names), 203, 157
    imgs = torch.from_numpy(np.stack([ref_input(n, oracle) for n in names])).to("cuda")
    cap = 4096
    kpts = torch.empty((cap, 7), dtype=torch.int32, device="cuda")
    dsc = torch.empty((cap, 128), dtype=torch.float32, device="cuda")
    offs = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
    ctx.detect_compute_batch(imgs.data_ptr(), B, R, C, C, R * C, kpts.data_ptr(), dsc.data_ptr(), cap, offs.data_ptr())
    ctx.sync()
    o = offs.cpu().numpy()
    k = kpts.cpu().numpy().view(np.uint8).reshape(cap, 28)
    d = dsc.cpu().numpy()
    assert o[0] == 0
    for b, n in enumerate(names):
        g = load_golden(n)
        assert o[b + 1] - o[b] == int(g["n"])
        assert_bits_equal(k[o[b]:o[b + 1]], g["kps"], f"batch image {n} keypoints")
        _descriptors_equal(f"batch image {n}", g, d[o[b]:o[b + 1]])


# ---- the scatter-form blur, forced (the variables are read when a context is created) ----------------
def _scatter(siftgpu, monkeypatch, img):
    monkeypatch.setenv("SIFT_HIP_SYM_MIN", "0")
    monkeypatch.setenv("SIFT_HIP_SYM_ROWS_MIN", "0")
    with siftgpu.Context(*img.shape, 1, device=0) as c:
        return c.SIFT_NCL(img)


@pytest.mark.parametrize("name", REF_FIXTURES)
def test_scatter_blur_sift_ncl_keypoints(siftgpu, oracle, monkeypatch, name):
    _keypoints_equal(name, load_golden(name), _scatter(siftgpu, monkeypatch, ref_input(name, oracle))[0])


@pytest.mark.parametrize("name", REF_FIXTURES)
def test_scatter_blur_sift_ncl_descriptors(siftgpu, oracle, monkeypatch, name):
    _descriptors_equal(name, load_golden(name), _scatter(siftgpu, monkeypatch, ref_input(name, oracle))[1])
