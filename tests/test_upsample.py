"""CPU tests of the upsampled first octave (sift_set_upsample): the numpy rule of
tests/upsample_inputs.py on hand-written cases, the round trip that lets the
CPU oracle stand for the upsampled run as it is, the properties of the inputs
the GPU tests (test_gpu_upsample.py) rely on, and the new entry points at the
ABI and in the Python binding."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import upsample_inputs as U
from conftest import assert_bits_equal, kp_bytes
from test_abi import HEADER, declared_symbols

f32 = np.float32


def _mix(a, wa, b, wb):
    """a * wa + b * wb in float32: two products, one sum."""
    return f32(f32(a) * f32(wa)) + f32(f32(b) * f32(wb))


# ---- the doubling rule on hand-written cases --------------------------------------------
def test_1x1_gives_four_copies():
    v = f32(1.0) + f32(2.0 ** -23)
    assert_bits_equal(U.upsample2x_ref(np.array([[v]], f32)), np.full((2, 2), v, f32), "1x1")


def test_1x3_every_value():
    a, b, c = f32(1.0), f32(5.0), f32(-3.0)
    row = [a, _mix(a, .75, b, .25), _mix(a, .25, b, .75), _mix(b, .75, c, .25), _mix(b, .25, c, .75), c]
    assert [float(v) for v in row] == [1.0, 2.0, 4.0, 3.0, -1.0, -3.0]
    assert_bits_equal(U.upsample2x_ref(np.array([[a, b, c]], f32)), np.array([row, row], f32), "1x3")


def test_3x1_every_value():
    a, b, c = f32(1.0), f32(5.0), f32(-3.0)
    col = np.array([[1.0], [2.0], [4.0], [3.0], [-1.0], [-3.0]], f32)
    assert_bits_equal(U.upsample2x_ref(np.array([[a], [b], [c]], f32)), np.repeat(col, 2, axis=1), "3x1")


def test_2x2_every_value():
    got = U.upsample2x_ref(np.array([[0.0, 8.0], [16.0, 40.0]], f32))
    # rows: [0, 2, 6, 8] and [16, 22, 34, 40] after the horizontal pass; the vertical pass mixes them
    want = np.array([[0.0, 2.0, 6.0, 8.0],
                     [4.0, 7.0, 13.0, 16.0],
                     [12.0, 17.0, 27.0, 32.0],
                     [16.0, 22.0, 34.0, 40.0]], f32)
    assert_bits_equal(got, want, "2x2")


def test_edges_are_copies_of_the_source():
    """Edge outputs are bit-equal to the source sample, on s = 1 + 2^-23 among others.
    (The rule says "copied, with no multiply".  No finite float32 tells a copy from the
    interior expression with both taps on the edge sample: s * 0.25f is exact or rounds
    the opposite way to s * 0.75f, and the sum rounds back to s -- checked below on
    values of every kind -- so the copy is pinned through bit equality with the source,
    and through the corner of a 1 x 1 image holding a NaN payload, which a product
    would be free to change and a copy is not.)"""
    s = f32(1.0) + f32(2.0 ** -23)
    r = np.random.default_rng(5)
    vals = np.concatenate([r.integers(0, 2 ** 31 - 2 ** 23 - 1, 20000).astype(np.uint32).view(f32),
                           np.arange(1, 64, dtype=np.uint32).view(f32), np.array([s, 1.1, 3.3, -0.0], f32)])
    with np.errstate(all="ignore"):
        assert_bits_equal(vals * f32(.75) + vals * f32(.25), vals, "s * 0.75f + s * 0.25f == s")
    nan = np.array([0x7fc12345], np.uint32).view(f32).reshape(1, 1)
    assert_bits_equal(U.upsample2x_ref(nan), np.repeat(np.repeat(nan, 2, 0), 2, 1), "1x1 NaN payload")
    img = np.full((3, 4), s, f32)
    img[1, 1:3] = f32(7.0)   # an interior that is not constant
    out = U.upsample2x_ref(img)
    assert out.shape == (6, 8)
    for edge, src in ((out[0], img[0]), (out[-1], img[-1])):
        assert_bits_equal(edge[[0, -1]], src[[0, -1]], "corner copies")
    assert_bits_equal(out[[0, -1]][:, [0, -1]], np.full((2, 2), s, f32), "the four corners")
    assert_bits_equal(out[:, 0], U.upsample2x_ref(img[:, :1])[:, 0], "first column = the column doubled alone")
    assert out[0, 0] == s and out[1, 0] == _mix(s, .75, s, .25)   # row 1 mixes rows 0 and 1: a product


def test_separable_and_denormal_values_survive():
    tiny = f32(2.0 ** -140)
    img = np.array([[tiny, -tiny, 0.0], [4 * tiny, 1.0, -1.0]], f32)
    out = U.upsample2x_ref(img)
    assert out[0, 0] == tiny and out[0, 1] == _mix(tiny, .75, -tiny, .25) == f32(2.0 ** -141)
    assert out.dtype == f32 and out.shape == (4, 6)


# ---- the round trip: the oracle as it stands defines the upsampled run ------------------
@pytest.mark.parametrize("n_oct", U.OCTAVES)
def test_round_trip_descriptors_at_half_scale(oracle, n_oct):
    img = U.image("128x160")
    big = U.upsample2x_ref(img)
    kps, desc = oracle.sift(big, n_oct)
    half = U.half_scale(kps)
    assert_bits_equal(kp_bytes(U.double_scale(half)), kp_bytes(kps), "half_scale is undone exactly")
    g = oracle.build_gaussian_pyramid(big, n_oct)
    again = oracle.calc_descriptors(g, big.shape[0], big.shape[1], half, n_oct, first_octave=-1)
    assert_bits_equal(again, desc, f"{n_oct} octaves: calc_descriptors(first_octave=-1) at the half-scaled keypoints")
    ek, ed = U.expected(img, n_oct)
    assert_bits_equal(kp_bytes(ek), kp_bytes(half), "expected() keypoints")
    assert_bits_equal(ed, desc, "expected() descriptors")


@pytest.mark.parametrize("name,plain,up,first", [("128x160", 99, 257, 160), ("157x203", 165, 414, 247),
                                                 ("96x64", 19, 56, 36)])
def test_expected_list_has_an_octave_below_zero(oracle, name, plain, up, first):
    img = U.image(name)
    kps, _ = oracle.sift(img, 5)
    ek, ed = U.expected(img, 5)
    assert (len(kps), len(ek), int(((ek["octave"] & 255) == 255).sum())) == (plain, up, first)
    assert ed.shape == (up, 128)
    # angle, response and class_id are the doubled run's own
    dk, _ = oracle.sift(U.upsample2x_ref(img), 5)
    for f in ("angle", "response", "class_id"):
        assert_bits_equal(ek[f], dk[f], f)
    assert np.array_equal(ek["octave"] >> 8, dk["octave"] >> 8)


# ---- the entry points ---------------------------------------------------------------------
NEW = ["sift_set_upsample", "sift_upsample2x", "sift_upsample2x_device"]


def test_header_declares_the_entry_points():
    assert set(NEW) <= set(declared_symbols())
    text = open(HEADER).read()
    assert re.search(r"int\s+sift_set_upsample\(sift_ctx\*\s*\w*,\s*int\s+on\);", text)
    assert re.search(r"int\s+sift_upsample2x\(sift_ctx\*\s*\w*,\s*const\s+float\*\s*src,\s*int\s+rows,\s*int\s+cols,"
                     r"\s*size_t\s+row_stride_bytes,\s*float\*\s*dst\);", text)
    assert re.search(r"int\s+sift_upsample2x_device\(sift_ctx\*\s*\w*,\s*const\s+float\*\s*d_src,\s*int\s+batch,", text)
    assert "never upsamples, so unless" in text   # the compute section no longer rejects the case outright


def test_library_exports_the_entry_points(siftgpu):
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    assert all(hasattr(L, s) for s in NEW)
    # a NULL context is SIFT_E_INVALID (no device needed)
    L.sift_set_upsample.restype, L.sift_set_upsample.argtypes = ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]
    assert L.sift_set_upsample(None, 1) == siftgpu.SIFT_E_INVALID
    fp, sz = ctypes.POINTER(ctypes.c_float), ctypes.c_size_t
    L.sift_upsample2x.restype = ctypes.c_int
    L.sift_upsample2x.argtypes = [ctypes.c_void_p, fp, ctypes.c_int, ctypes.c_int, sz, fp]
    src, dst = np.zeros((2, 2), f32), np.zeros((4, 4), f32)
    assert L.sift_upsample2x(None, src.ctypes.data_as(fp), 2, 2, 0, dst.ctypes.data_as(fp)) == siftgpu.SIFT_E_INVALID
    L.sift_upsample2x_device.restype = ctypes.c_int
    L.sift_upsample2x_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         sz, sz, ctypes.c_void_p, sz, sz]
    assert L.sift_upsample2x_device(None, None, 1, 2, 2, 2, 4, None, 4, 16) == siftgpu.SIFT_E_INVALID


def test_python_interface(siftgpu):
    """SIFT_NCL's own parameter lists are pinned (tests/test_compute.py), so the one-call form of
    the setting is a sibling, SIFT_NCL_upsampled, with the same arguments; compute takes upsample."""
    for name in ("set_upsample", "upsample2x", "upsample2x_device", "SIFT_NCL_upsampled"):
        assert callable(getattr(siftgpu.Context, name, None)), name
    for fn in (siftgpu.compute, siftgpu.Context.compute):
        p = inspect.signature(fn).parameters
        assert "upsample" in p and p["upsample"].default is False, fn
    assert list(inspect.signature(siftgpu.SIFT_NCL_upsampled).parameters) == \
        list(inspect.signature(siftgpu.SIFT_NCL).parameters)
    assert list(inspect.signature(siftgpu.Context.SIFT_NCL_upsampled).parameters) == \
        list(inspect.signature(siftgpu.Context.SIFT_NCL).parameters)
