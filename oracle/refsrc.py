"""ctypes binding for oracle/_ref/libsift_ref.so: the reference's own
src/sift.cpp compiled over the stand-in headers of oracle/cvmini/ (recipe:
oracle/ref_build.py, entry points: oracle/ref_wrap.cpp).

TEST INFRASTRUCTURE ONLY.  Same function names and packed layouts as
oracle/oracle.py, so the two are interchangeable in a test.  build_gaussian_pyramid
and sift with five octaves only (src/sift.cpp:248 is right only when
nOctaves == nScales); the DoG, extrema and descriptor functions index by
nScales and take any octave count.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

import ref_build
from oracle import KEYPOINT_DTYPE, octave_shapes, split_planes  # noqa: F401  (same layouts)

LIB_PATH = ref_build.LIB_PATH

_lib = None


def reference_present() -> bool:
    return ref_build.reference_present()


def available() -> bool:
    """True when the library exists or can be built from the reference tree."""
    return os.path.exists(LIB_PATH) or reference_present()


def build():
    return ref_build.build()


def lib():
    global _lib
    if _lib is None:
        build()  # rebuilds when stale; nothing without a reference tree
        L = ctypes.CDLL(LIB_PATH)
        fp = ctypes.POINTER(ctypes.c_float)
        i = ctypes.c_int
        L.rs_gaussian_blur.argtypes = [fp, i, i, ctypes.c_double, fp]
        L.rs_gaussian_blur_1d.argtypes = [fp, i, i, ctypes.c_double, fp]
        L.rs_build_gaussian_pyramid.restype = i
        L.rs_build_gaussian_pyramid.argtypes = [fp, i, i, i, fp]
        L.rs_build_dog_pyramid.restype = i
        L.rs_build_dog_pyramid.argtypes = [fp, i, i, i, fp]
        L.rs_find_scale_space_extrema.restype = i
        L.rs_find_scale_space_extrema.argtypes = [fp, fp, i, i, i, ctypes.c_void_p, i]
        L.rs_calc_descriptors.restype = i
        L.rs_calc_descriptors.argtypes = [fp, i, i, i, ctypes.c_void_p, i, fp, i]
        L.rs_sift.restype = i
        L.rs_sift.argtypes = [fp, i, i, i, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]
        L.rs_free.argtypes = [ctypes.c_void_p]
        L.rs_solve3.argtypes = [fp, fp, fp]
        L.rs_helper.argtypes = [i, fp, fp, fp, i]
        L.rs_saturate_u8.argtypes = [fp, fp, i]
        L.rs_resize_nn.argtypes = [fp, i, i, fp, i, i]
        _lib = L
    return _lib


def _fp(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _five(n_octaves):
    if n_octaves != 5:
        raise ValueError("the reference source is called with 5 octaves only (src/sift.cpp:248)")


def _plane_total(rows, cols, n_octaves, per):
    return sum(r * c for (r, c) in octave_shapes(rows, cols, n_octaves)) * per


def gaussian_blur(img: np.ndarray, sigma: float) -> np.ndarray:
    img = np.ascontiguousarray(img, np.float32)
    out = np.empty_like(img)
    lib().rs_gaussian_blur(_fp(img), img.shape[0], img.shape[1], float(sigma), _fp(out))
    return out


def gaussian_blur_1d(img: np.ndarray, sigma: float) -> np.ndarray:
    img = np.ascontiguousarray(img, np.float32)
    out = np.empty_like(img)
    lib().rs_gaussian_blur_1d(_fp(img), img.shape[0], img.shape[1], float(sigma), _fp(out))
    return out


def resize_nn(img: np.ndarray, drows: int, dcols: int) -> np.ndarray:
    img = np.ascontiguousarray(img, np.float32)
    out = np.empty((drows, dcols), np.float32)
    lib().rs_resize_nn(_fp(img), img.shape[0], img.shape[1], _fp(out), drows, dcols)
    return out


def build_gaussian_pyramid(img: np.ndarray, n_octaves: int = 5) -> np.ndarray:
    _five(n_octaves)
    img = np.ascontiguousarray(img, np.float32)
    r, c = img.shape
    out = np.empty(_plane_total(r, c, n_octaves, 5), np.float32)
    assert lib().rs_build_gaussian_pyramid(_fp(img), r, c, n_octaves, _fp(out)) == 0
    return out


def build_dog_pyramid(gpyr: np.ndarray, rows: int, cols: int, n_octaves: int = 5) -> np.ndarray:
    out = np.empty(_plane_total(rows, cols, n_octaves, 4), np.float32)
    assert lib().rs_build_dog_pyramid(_fp(gpyr), rows, cols, n_octaves, _fp(out)) == 0
    return out


def find_scale_space_extrema(gpyr, dog, rows, cols, n_octaves=5) -> np.ndarray:
    cap = 1 << 14
    while True:
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        n = lib().rs_find_scale_space_extrema(_fp(gpyr), _fp(dog), rows, cols, n_octaves, kps.ctypes.data, cap)
        assert n >= 0
        if n <= cap:
            return kps[:n].copy()
        cap = n


def calc_descriptors(gpyr, rows, cols, kps: np.ndarray, n_octaves=5, first_octave=0) -> np.ndarray:
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    out = np.zeros((len(kps), 128), np.float32)
    if len(kps):
        assert lib().rs_calc_descriptors(_fp(gpyr), rows, cols, n_octaves, kps.ctypes.data, len(kps),
                                         _fp(out), first_octave) == 0
    return out


def sift(img: np.ndarray, n_octaves: int = 5):
    """SIFT_NCL itself: returns (keypoints structured array, N x 128 float32)."""
    _five(n_octaves)
    img = np.ascontiguousarray(img, np.float32)
    kp_p, d_p = ctypes.c_void_p(), ctypes.c_void_p()
    n = lib().rs_sift(_fp(img), img.shape[0], img.shape[1], n_octaves, ctypes.byref(kp_p), ctypes.byref(d_p))
    assert n >= 0
    kps = np.zeros(n, KEYPOINT_DTYPE)
    desc = np.zeros((n, 128), np.float32)
    if n:
        ctypes.memmove(kps.ctypes.data, kp_p.value, n * 28)
        ctypes.memmove(desc.ctypes.data, d_p.value, n * 128 * 4)
    lib().rs_free(kp_p)
    lib().rs_free(d_p)
    return kps, desc


def solve3(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Matx33f::solve(b, DECOMP_LU) of the stand-in header (zeros when singular)."""
    a = np.ascontiguousarray(a, np.float32).reshape(9)
    b = np.ascontiguousarray(b, np.float32).reshape(3)
    x = np.zeros(3, np.float32)
    lib().rs_solve3(_fp(a), _fp(b), _fp(x))
    return x


def saturate_u8(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a, np.float32)
    out = np.empty_like(a)
    lib().rs_saturate_u8(_fp(a), _fp(out), a.size)
    return out


def helper(op: int, a: np.ndarray, b: np.ndarray | None = None) -> np.ndarray:
    """The op codes of oracle.helper, evaluated by the stand-in header's
    primitives (0 exp32f, 1 fastAtan2, 2 magnitude32f, 6 cvRound, 7 cvFloor) and
    by libm as src/sift.cpp calls it (3 cosf, 4 sinf, 5 powf(2.f, a))."""
    a = np.ascontiguousarray(a, np.float32)
    bb = np.ascontiguousarray(b if b is not None else a, np.float32)
    out = np.empty_like(a)
    lib().rs_helper(int(op), _fp(a), _fp(bb), _fp(out), a.size)
    return out
