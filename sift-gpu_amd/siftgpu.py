"""Python host binding for libsift_hip.so (MI355X SIFT detect + compute).

Mirrors the reference API (canhld94/SIFT-GPU include/sift.hpp:36-67) with the
same function names and argument meaning, on numpy arrays, by calling the C ABI
declared in include/sift_hip.h through ctypes.  There is no CPU fallback: if
the HIP library cannot be loaded or no GPU is present, every call raises.

    kps, desc = SIFT_NCL(img)                     # src/sift.cpp:59-91
    dst = Gaussian_Blur(src, sigma)               # src/sift.cpp:123-153
    dst = Gaussian_Blur_1D(src, sigma)            # src/sift.cpp:170-217
    gpyr = buildGaussianPyramid(img, nOctaves)    # src/sift.cpp:229-263
    dog = buildDoGPyramid(gpyr, nOctaves)         # src/sift.cpp:265-283
    kps = findScaleSpaceExtrema(gpyr, dog, nOctaves)        # :547-577
    desc = calDescriptor(gpyr, kps, firstOctave)             # :733-753

Pyramids are lists of 2-D float32 planes indexed o*5+s (Gaussian) / o*4+s
(DoG).  Keypoints are numpy structured arrays laid out like cv::KeyPoint.

`Context` exposes the device-resident batch path used by bench.py; buffers are
torch tensors (PyTorch is used only for device memory and streams).
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libsift_hip.so")

SIFT_OK, SIFT_E_INVALID, SIFT_E_HIP, SIFT_E_CAPACITY, SIFT_E_SIZE, SIFT_E_NOMEM = 0, -1, -2, -3, -4, -5
SIFT_MULTI_SELF_P2P = 0x100  # sift_multi_create: device 0's own records over RCCL too (tests)
SIFT_E_WORKSPACE = -6  # internal candidate workspace overflow: an error, never the sizing case
SIFT_FLAG_FAST, SIFT_FLAG_PROFILE, SIFT_FLAG_VERBOSE, SIFT_FLAG_NO_GRAPH = 0x1, 0x2, 0x4, 0x8
N_SCALES, N_DOG, DESC_LEN = 5, 4, 128
HOMOGRAPHY_ROUND = 64  # hypotheses per round of the segmented homography (scratch.hpp kHomogRound)
AFFINE_ROUND = 128  # hypotheses per round of the segmented affine / similarity estimate (scratch.hpp kAffineRound)
FUND_ROUND = 256  # hypotheses per round of the segmented fundamental-matrix estimate (scratch.hpp kFundRound)
# sift_estimate_affine[_segmented[_device]]: the motion model
SIFT_MODEL_AFFINE, SIFT_MODEL_SIMILARITY = 0, 1
# sift_cross_match_segmented_device's metric: the distance and the type of the descriptor rows
SIFT_METRIC_L1_F32, SIFT_METRIC_L1_U8, SIFT_METRIC_L2SQR_U8 = 0, 1, 2
SIFT_METRIC_L2SQR_F32 = 3  # a name only: the one-call cross-match and the windowed matcher reject it
# sift_warp_perspective[_segmented_device]: the pixel type and the flag
SIFT_PIXEL_F32, SIFT_PIXEL_U8 = 0, 1
SIFT_WARP_INVERSE_MAP = 0x1

KEYPOINT_DTYPE = np.dtype(
    [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KEYPOINT_DTYPE.itemsize == 28
# sift_match: one kept match of ratioMatches (query / train local to their segments)
MATCH_DTYPE = np.dtype([("query", "<i4"), ("train", "<i4"), ("distance", "<f4"), ("segment", "<i4")])
assert MATCH_DTYPE.itemsize == 16
JOIN_QUERY, JOIN_TRAIN = 0, 1  # SIFT_JOIN_*: the index of a record that names the shared view's keypoint


class SiftError(RuntimeError):
    def __init__(self, fn, code, msg):
        super().__init__(f"{fn} failed ({code}): {msg}")
        self.code = code


class StageStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 32), ("launches", ctypes.c_int), ("ms", ctypes.c_double),
                ("flops", ctypes.c_double), ("bytes", ctypes.c_double)]


_lib = None
_lib_lock = threading.Lock()


def build() -> str:
    """Compile libsift_hip.so (hipcc, gfx950) in-tree."""
    subprocess.run(["make", "-s", "-C", HERE, "-j8"], check=True)
    return LIB_PATH


def lib():
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built (run make -C {HERE}); no CPU fallback exists")
        L = ctypes.CDLL(LIB_PATH)
        vp, ip, fp, sz = ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_size_t
        pint, pdbl = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
        sigs = {
            "sift_ctx_create": (ip, [ip, ip, ip, ip, ctypes.c_uint, ctypes.POINTER(vp)]),
            "sift_ctx_destroy": (ip, [vp]),
            "sift_last_error": (ctypes.c_char_p, [vp]),
            "sift_set_stream": (ip, [vp, vp]),
            "sift_get_stream": (vp, [vp]),
            "sift_set_flags": (ip, [vp, ctypes.c_uint]),
            "sift_set_octaves": (ip, [vp, ip]),
            "sift_sync": (ip, [vp]),
            "sift_set_candidate_capacity": (ip, [vp, ip]),
            "sift_set_max_features": (ip, [vp, ip]),
            "sift_set_upsample": (ip, [vp, ip]),
            "sift_upsample2x": (ip, [vp, fp, ip, ip, sz, fp]),
            "sift_upsample2x_device": (ip, [vp, vp, ip, ip, ip, sz, sz, vp, sz, sz]),
            "sift_warp_perspective_segmented_device": (ip, [vp, ip, ip, vp, ip, ip, sz, sz, vp, vp, ip, ctypes.c_uint,
                                                            vp, ip, ip, sz, sz]),
            "sift_warp_perspective": (ip, [vp, ip, ip, vp, ip, ip, sz, ctypes.POINTER(ctypes.c_double),
                                           ctypes.c_uint, vp, ip, ip]),
            "sift_version": (ctypes.c_char_p, []),
            "sift_graph_stats": (ip, [vp, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong),
                                      ctypes.POINTER(ctypes.c_longlong)]),
            "sift_octave_shapes": (ip, [ip, ip, ip, pint, pint]),
            "sift_packed_size": (sz, [ip, ip, ip, ip]),
            "sift_detect_compute": (ip, [vp, fp, ip, ip, sz, vp, fp, ip, pint]),
            "sift_detect_compute_batch": (ip, [vp, vp, ip, ip, ip, sz, sz, vp, vp, ip, vp]),
            "sift_detect_compute_masked": (ip, [vp, fp, ip, ip, sz, vp, sz, vp, fp, ip, pint]),
            "sift_detect_compute_batch_masked": (ip, [vp, vp, ip, ip, ip, sz, sz, vp, sz, sz, vp, vp, ip, vp]),
            "sift_compute_batch": (ip, [vp, vp, ip, ip, ip, sz, sz, vp, vp, ip, ip, vp]),
            "sift_compute": (ip, [vp, fp, ip, ip, sz, vp, ip, ip, fp]),
            "sift_copy_results": (ip, [vp, vp, fp, ip, pint]),
            "sift_synth_images": (ip, [vp, vp, ip, ip, ip, sz, sz, ip]),
            "sift_gaussian_blur": (ip, [vp, fp, ip, ip, ctypes.c_double, fp]),
            "sift_gaussian_blur_1d": (ip, [vp, fp, ip, ip, ctypes.c_double, fp]),
            "sift_build_gaussian_pyramid": (ip, [vp, fp, ip, ip, ip, fp]),
            "sift_build_dog_pyramid": (ip, [vp, fp, ip, ip, ip, fp]),
            "sift_find_scale_space_extrema": (ip, [vp, fp, fp, ip, ip, ip, vp, ip, pint]),
            "sift_calc_descriptors": (ip, [vp, fp, ip, ip, ip, vp, ip, fp, ip]),
            "sift_get_stage_stats": (ip, [vp, ctypes.POINTER(StageStat), ip, pint, ip]),
            "sift_selftest_math": (ip, [vp, ip, fp, fp, fp, ip]),
            "sift_selftest_g4_points": (ip, [vp, fp, ip, ip, pint, ip, fp]),
            "sift_g4_fill_stats": (ip, [vp, pint, pint, pint]),
            "sift_knn_match_l1": (ip, [vp, fp, ip, fp, ip, ip, pint, fp]),
            "sift_bgr8_to_gray": (ip, [vp, vp, ip, ip, sz, ip, ip, fp]),
            "sift_find_homography": (ip, [fp, fp, ip, ctypes.c_double, ip, ctypes.c_double,
                                          ctypes.POINTER(ctypes.c_double), vp]),
            "sift_perspective_transform": (ip, [ctypes.POINTER(ctypes.c_double), fp, ip, fp]),
            "sift_bgr8_to_gray_device": (ip, [vp, vp, ip, ip, ip, sz, sz, ip, ip, vp, sz, sz]),
            "sift_knn_match_l1_device": (ip, [vp, vp, ip, vp, ip, ip, vp, vp]),
            "sift_knn_match_l1_segmented_device": (ip, [vp, vp, vp, ip, ip, vp, vp, ip, ip, vp, vp]),
            "sift_knn_match_l1_segmented": (ip, [vp, fp, pint, ip, ip, fp, pint, ip, ip, pint, fp]),
            "sift_descriptors_to_u8_device": (ip, [vp, vp, vp, ip, vp]),
            "sift_descriptors_to_u8": (ip, [vp, fp, ip, vp]),
            "sift_knn_match_l1_u8_segmented_device": (ip, [vp, vp, vp, ip, ip, vp, vp, ip, ip, vp, vp]),
            "sift_knn_match_l1_u8_segmented": (ip, [vp, vp, pint, ip, ip, vp, pint, ip, ip, pint, fp]),
            "sift_knn_match_l1_u8": (ip, [vp, vp, ip, vp, ip, ip, pint, fp]),
            "sift_knn_match_l2sqr_u8_segmented_device": (ip, [vp, vp, vp, ip, ip, vp, vp, ip, ip, vp, vp]),
            "sift_knn_match_l2sqr_u8_segmented": (ip, [vp, vp, pint, ip, ip, vp, pint, ip, ip, pint, fp]),
            "sift_knn_match_l2sqr_u8": (ip, [vp, vp, ip, vp, ip, ip, pint, fp]),
            "sift_knn_match_l2sqr_f32_segmented_device": (ip, [vp, vp, vp, ip, ip, vp, vp, ip, ip, vp, vp]),
            "sift_knn_match_l2sqr_f32_segmented": (ip, [vp, fp, pint, ip, ip, fp, pint, ip, ip, pint, fp]),
            "sift_knn_match_l2sqr_f32": (ip, [vp, fp, ip, fp, ip, ip, pint, fp]),
            "sift_ratio_matches_device": (ip, [vp, vp, vp, vp, ip, ip, ctypes.c_double, vp, vp, vp, vp, vp, vp, ip,
                                               vp]),
            "sift_ratio_matches": (ip, [vp, pint, fp, pint, ip, ip, ctypes.c_double, vp, vp, ip, pint, vp, fp, fp,
                                        ip, pint]),
            "sift_cross_check_matches_device": (ip, [vp, vp, vp, ip, vp, ip, ip, vp, ip, vp, ip, ctypes.c_double, vp,
                                                     vp, vp, vp, vp, ip, vp]),
            "sift_cross_check_matches": (ip, [vp, pint, fp, ip, pint, ip, ip, pint, ip, pint, ip, ctypes.c_double, vp,
                                              vp, vp, fp, fp, ip, pint]),
            "sift_cross_match_segmented_device": (ip, [vp, ip, vp, vp, ip, ip, vp, vp, ip, ctypes.c_double, vp, vp,
                                                       vp, vp, vp, ip, vp]),
            "sift_knn_match_window_segmented_device": (ip, [vp, ip, vp, vp, vp, ip, ip, vp, vp, vp, ip, vp, vp,
                                                            ctypes.c_float, ip, ip, ip, vp, vp]),
            "sift_knn_match_window_segmented": (ip, [vp, ip, vp, vp, pint, ip, ip, vp, vp, pint, ip, vp, pint,
                                                     ctypes.c_float, ip, ip, ip, pint, fp]),
            "sift_knn_match_epipolar_segmented_device": (ip, [vp, ip, vp, vp, vp, ip, ip, vp, vp, vp, ip, vp, vp,
                                                              ctypes.c_double, ctypes.c_float, ip, ip, ip, vp, vp]),
            "sift_knn_match_epipolar_segmented": (ip, [vp, ip, vp, vp, pint, ip, ip, vp, vp, pint, ip, vp, pint,
                                                       ctypes.c_double, ctypes.c_float, ip, ip, ip, pint, fp]),
            "sift_find_homography_segmented_device": (ip, [vp, vp, vp, vp, ip, ip, ctypes.c_double, ip,
                                                           ctypes.c_double, vp, vp, vp]),
            "sift_find_homography_segmented": (ip, [vp, fp, fp, pint, ip, ip, ctypes.c_double, ip, ctypes.c_double,
                                                    ctypes.POINTER(ctypes.c_double), pint, vp]),
            "sift_perspective_transform_segmented_device": (ip, [vp, vp, vp, ip, vp, ip, vp]),
            "sift_estimate_affine": (ip, [fp, fp, ip, ip, ctypes.c_double, ip, ctypes.c_double,
                                          ctypes.POINTER(ctypes.c_double), vp]),
            "sift_estimate_affine_segmented_device": (ip, [vp, vp, vp, vp, ip, ip, ip, ctypes.c_double, ip,
                                                           ctypes.c_double, vp, vp, vp]),
            "sift_estimate_affine_segmented": (ip, [vp, fp, fp, pint, ip, ip, ip, ctypes.c_double, ip,
                                                    ctypes.c_double, ctypes.POINTER(ctypes.c_double), pint, vp]),
            "sift_find_fundamental": (ip, [fp, fp, ip, ctypes.c_double, ip, ctypes.c_double,
                                           ctypes.POINTER(ctypes.c_double), vp]),
            "sift_find_fundamental_segmented_device": (ip, [vp, vp, vp, vp, ip, ip, ctypes.c_double, ip,
                                                            ctypes.c_double, vp, vp, vp]),
            "sift_find_fundamental_segmented": (ip, [vp, fp, fp, pint, ip, ip, ctypes.c_double, ip, ctypes.c_double,
                                                     ctypes.POINTER(ctypes.c_double), pint, vp]),
            "sift_recover_pose": (ip, [pdbl, pdbl, pdbl, fp, fp, ip, vp, ctypes.c_double, pdbl, pdbl, vp, vp, pint]),
            "sift_recover_pose_segmented_device": (ip, [vp, vp, vp, vp, ip, ip, vp, vp, vp, vp, ip, vp,
                                                        ctypes.c_double, vp, vp, vp, vp, vp, vp]),
            "sift_recover_pose_segmented": (ip, [vp, fp, fp, pint, ip, ip, pdbl, pint, pdbl, pdbl, ip, vp,
                                                 ctypes.c_double, pdbl, pdbl, pint, pint, vp, vp]),
            "sift_triangulate_points": (ip, [pdbl, pdbl, fp, fp, ip, pdbl]),
            "sift_triangulate_points_segmented_device": (ip, [vp, vp, vp, vp, ip, ip, vp, vp, vp]),
            "sift_solve_p3p": (ip, [pdbl, fp, pdbl, pdbl, pint]),
            "sift_solve_pnp": (ip, [pdbl, fp, ip, vp, pdbl, ctypes.c_double, ip, ctypes.c_double, pdbl, vp, pint]),
            "sift_solve_pnp_segmented_device": (ip, [vp, vp, vp, vp, ip, ip, vp, vp, ip, ctypes.c_double, ip,
                                                     ctypes.c_double, vp, vp, vp, vp]),
            "sift_solve_pnp_segmented": (ip, [vp, pdbl, fp, pint, ip, ip, vp, pdbl, ip, ctypes.c_double, ip,
                                              ctypes.c_double, pdbl, pint, pint, vp]),
            "sift_join_matches": (ip, [vp, ip, ip, vp, vp, vp, ip, ip, vp, vp, ip, vp, vp, vp, vp, vp]),
            "sift_join_matches_segmented_device": (ip, [vp, vp, vp, ip, ip, vp, vp, vp, vp, ip, ip, vp, vp, vp, ip,
                                                        ip, vp, vp, vp, vp, vp, ip, vp]),
            "sift_join_matches_segmented": (ip, [vp, vp, vp, ip, ip, vp, vp, vp, vp, ip, ip, vp, vp, vp, ip, ip, vp,
                                                 vp, vp, vp, vp, ip, vp]),
            "sift_undistort_batch_device": (ip, [vp, ip, ip, vp, ip, ip, sz, sz, vp, vp, vp, ip, ip, vp, ip, ip, sz, sz]),
            "sift_undistort": (ip, [vp, ip, ip, vp, ip, ip, sz, pdbl, pdbl, pdbl, vp, ip, ip]),
            "sift_undistort_points": (ip, [pdbl, pdbl, pdbl, ip, vp, vp, sz, ip]),
            "sift_undistort_points_segmented_device": (ip, [vp, vp, vp, sz, vp, ip, ip, vp, vp, vp, ip, ip, vp]),
            "sift_undistort_points_segmented": (ip, [vp, vp, vp, sz, pint, ip, ip, pdbl, pdbl, pdbl, ip, ip, pint]),
            "sift_multi_shard": (ip, [ip, ip, ip, pint, pint]),
            "sift_multi_merge_offsets": (ip, [ctypes.POINTER(pint), pint, ip, pint]),
            "sift_multi_create": (ip, [pint, ip, ip, ip, ip, ctypes.c_uint, ip, ip, ip, ctypes.POINTER(vp)]),
            "sift_multi_set_octaves": (ip, [vp, ip]),
            "sift_multi_set_flags": (ip, [vp, ctypes.c_uint]),
            "sift_multi_set_max_features": (ip, [vp, ip]),
            "sift_multi_destroy": (ip, [vp]),
            "sift_multi_last_error": (ctypes.c_char_p, [vp]),
            "sift_multi_context": (vp, [vp, ip]),
            "sift_multi_step": (ip, [vp, ctypes.POINTER(vp), pint, ip, ip, sz, sz]),
            "sift_multi_step_masked": (ip, [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), pint, ip, ip, sz, sz, sz,
                                            sz]),
            "sift_multi_flush": (ip, [vp]),
            "sift_multi_gathered": (ip, [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), pint, ip, pint,
                                         ctypes.POINTER(ctypes.c_longlong)]),
            "sift_multi_stats": (ip, [vp, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong),
                                      ctypes.POINTER(ctypes.c_longlong)]),
            "sift_multi_rccl_version": (ip, []),
            "sift_multi_copy_gathered": (ip, [vp, vp, fp, ip, pint]),
        }
        optional = {"sift_graph_stats", "sift_g4_fill_stats", "sift_set_max_features",
                    "sift_multi_set_max_features", "sift_detect_compute_masked", "sift_detect_compute_batch_masked",
                    "sift_multi_step_masked", "sift_compute_batch", "sift_compute",
                    "sift_knn_match_window_segmented_device", "sift_knn_match_window_segmented",
                    "sift_set_upsample", "sift_upsample2x", "sift_upsample2x_device",
                    "sift_warp_perspective_segmented_device", "sift_warp_perspective", "sift_estimate_affine",
                    "sift_estimate_affine_segmented_device", "sift_estimate_affine_segmented",
                    "sift_find_fundamental", "sift_find_fundamental_segmented_device",
                    "sift_find_fundamental_segmented", "sift_knn_match_epipolar_segmented_device",
                    "sift_knn_match_epipolar_segmented", "sift_recover_pose",
                    "sift_recover_pose_segmented_device", "sift_recover_pose_segmented", "sift_triangulate_points",
                    "sift_triangulate_points_segmented_device", "sift_undistort_batch_device", "sift_undistort",
                    "sift_undistort_points", "sift_undistort_points_segmented_device",
                    "sift_undistort_points_segmented", "sift_solve_p3p", "sift_solve_pnp",
                    "sift_solve_pnp_segmented_device", "sift_solve_pnp_segmented", "sift_join_matches",
                    "sift_join_matches_segmented_device", "sift_join_matches_segmented"}  # absent from older builds (A/B runs against a saved library)
        for name, (res, args) in sigs.items():
            if name in optional and not hasattr(L, name):
                continue
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
        return L


def _fp(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def _pixel_args(img: np.ndarray):
    """(SIFT_PIXEL_*, channels) of a float32 H x W or uint8 H x W / H x W x 3 image."""
    if img.dtype == np.float32 and img.ndim == 2:
        return SIFT_PIXEL_F32, 1
    if img.dtype == np.uint8 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)):
        return SIFT_PIXEL_U8, 1 if img.ndim == 2 else 3
    raise ValueError("expected a float32 H x W or a uint8 H x W / H x W x 3 image")


def _camera(K, dist, M):
    """(K [9], dist [8] zero-padded, M [9] or None) as contiguous float64."""
    Kd = np.ascontiguousarray(K, np.float64).reshape(9)
    d = np.asarray(dist, np.float64).reshape(-1)
    if len(d) > 8:
        raise ValueError("at most eight distortion coefficients (k1 k2 p1 p2 k3 k4 k5 k6)")
    dd = np.zeros(8, np.float64)
    dd[:len(d)] = d
    return Kd, dd, None if M is None else np.ascontiguousarray(M, np.float64).reshape(9)


def _detection_mask(mask, shape):
    """The detection mask of SIFT_NCL as packed uint8 (None stays None): a uint8 or
    bool array of the image's shape, zero / False = no keypoint here.  Anything
    else raises ValueError -- before any library call."""
    if mask is None:
        return None
    m = np.asarray(mask)
    if m.dtype != np.uint8 and m.dtype != np.bool_:
        raise ValueError(f"mask must be uint8 or bool, not {m.dtype}")
    if m.shape != tuple(shape):
        raise ValueError(f"mask has shape {m.shape}, the image has {tuple(shape)}")
    return np.ascontiguousarray(m).view(np.uint8)


def octave_shapes(rows: int, cols: int, n_octaves: int = 5):
    out, r, c = [], rows, cols
    for _ in range(n_octaves):
        out.append((r, c))
        r //= 2
        c //= 2
    return out


def pack_planes(planes, rows, cols, n_octaves, per) -> np.ndarray:
    shapes = octave_shapes(rows, cols, n_octaves)
    if len(planes) < n_octaves * per:
        raise ValueError("too few planes")
    parts = []
    for o, (r, c) in enumerate(shapes):
        for s in range(per):
            p = np.ascontiguousarray(planes[o * per + s], np.float32)
            if p.shape != (r, c):
                raise ValueError(f"plane {o * per + s} has shape {p.shape}, octave shape is {(r, c)}")
            parts.append(p.reshape(-1))
    return np.ascontiguousarray(np.concatenate(parts))


def split_planes(packed: np.ndarray, rows, cols, n_octaves, per):
    planes, off = [], 0
    for (r, c) in octave_shapes(rows, cols, n_octaves):
        for _ in range(per):
            planes.append(packed[off:off + r * c].reshape(r, c))
            off += r * c
    return planes


class Context:
    """A device context (one HIP stream, workspace for max_rows x max_cols x max_batch)."""

    def __init__(self, max_rows: int, max_cols: int, max_batch: int = 1, device: int = 0,
                 flags: int = 0):
        self._L = lib()
        h = ctypes.c_void_p()
        rc = self._L.sift_ctx_create(device, max_rows, max_cols, max_batch, flags, ctypes.byref(h))
        if rc != SIFT_OK:
            raise SiftError("sift_ctx_create", rc, "could not create a device context (no GPU?)")
        self.h = h
        self.max_rows, self.max_cols, self.max_batch, self.device = max_rows, max_cols, max_batch, device

    def close(self):
        if getattr(self, "h", None):
            self._L.sift_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, fn, rc):
        if rc != SIFT_OK:
            raise SiftError(fn, rc, self._L.sift_last_error(self.h).decode())

    # ---- configuration --------------------------------------------------
    def set_flags(self, flags):
        self._check("sift_set_flags", self._L.sift_set_flags(self.h, flags))

    def set_octaves(self, n):
        self._check("sift_set_octaves", self._L.sift_set_octaves(self.h, n))

    def set_stream(self, stream_handle: int):
        self._check("sift_set_stream", self._L.sift_set_stream(self.h, ctypes.c_void_p(stream_handle)))

    def sync(self):
        self._check("sift_sync", self._L.sift_sync(self.h))

    def graph_stats(self):
        """(captures, in-place updates, instantiations) of the context's hipGraph cache."""
        v = [ctypes.c_longlong(0) for _ in range(3)]
        self._check("sift_graph_stats", self._L.sift_graph_stats(self.h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def g4_fill_stats(self):
        """(first-fill slots, waiting slots after the first step, most fills of one slot) of the last
        batch call's point evaluation of plane 4; zeros when it ran the dense flow."""
        v = [ctypes.c_int(0) for _ in range(3)]
        self._check("sift_g4_fill_stats", self._L.sift_g4_fill_stats(self.h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def set_candidate_capacity(self, per_image: int):
        self._check("sift_set_candidate_capacity", self._L.sift_set_candidate_capacity(self.h, per_image))

    def set_max_features(self, n: int):
        """Per-image keypoint budget of SIFT_NCL and the batch calls (SIFT::create(nfeatures)); 0 = all.
        Each image keeps its n best keypoints by response plus every tie at the cut, in the unlimited
        order (cv::KeyPointsFilter::retainBest; include/sift_hip.h)."""
        self._check("sift_set_max_features", self._L.sift_set_max_features(self.h, n))

    def set_upsample(self, on: bool):
        """The upsampled first octave (SIFT::create()'s firstOctave = -1; sift_set_upsample in
        include/sift_hip.h): SIFT_NCL, detect_compute_batch, compute and compute_batch double each
        image on the device and run on that; keypoints come out in the original image's frame with
        octave bytes from 255 (octave -1) up.  The context must hold the doubled shape."""
        self._check("sift_set_upsample", self._L.sift_set_upsample(self.h, int(bool(on))))
        self._upsample = bool(on)

    class _UpsampleCall:
        """upsample=True of one call: the setting on for its span, then as it was."""

        def __init__(self, ctx, on):
            self.ctx, self.flip = ctx, bool(on) and not getattr(ctx, "_upsample", False)

        def __enter__(self):
            if self.flip:
                self.ctx.set_upsample(True)

        def __exit__(self, *a):
            if self.flip:
                self.ctx.set_upsample(False)

    # ---- host-memory API (reference names) ------------------------------
    def SIFT_NCL_upsampled(self, img: np.ndarray, row_stride_bytes: int | None = None, mask=None, keypoints=None):
        """SIFT_NCL with set_upsample(True) for the span of this call (then the setting as it was)."""
        with self._UpsampleCall(self, True):
            return self.SIFT_NCL(img, row_stride_bytes, mask, keypoints)

    def SIFT_NCL(self, img: np.ndarray, row_stride_bytes: int | None = None, mask=None, keypoints=None):
        """Runs under the context's set_upsample setting (SIFT_NCL_upsampled: on for one call).
        keypoints given (detectAndCompute's useProvidedKeypoints): they are described
        unchanged -- (keypoints, self.compute(img, keypoints)) -- and the mask is
        ignored, as OpenCV ignores it.  Otherwise:
        row_stride_bytes None: img is copied to a contiguous float32 array.
        A number: img's own memory is passed with that row stride (img must be
        2-D float32 with unit column stride and rows that many bytes apart;
        0 is the ABI's default, cols * 4).
        mask: detectAndCompute's mask, a uint8 or bool array of the image's shape;
        a keypoint at (x, y) is dropped iff mask[int(y + 0.5), int(x + 0.5)] == 0
        (on the device, before the descriptors; include/sift_hip.h)."""
        if keypoints is not None:
            kps = np.ascontiguousarray(keypoints, KEYPOINT_DTYPE)
            return kps, self.compute(img, kps)
        mask = _detection_mask(mask, np.shape(img))
        if row_stride_bytes is None:
            img = np.ascontiguousarray(img, np.float32)
            row_stride_bytes = img.shape[1] * 4
        elif (img.dtype != np.float32 or img.ndim != 2 or img.strides[1] != 4
              or img.strides[0] != (row_stride_bytes or img.shape[1] * 4)):
            raise ValueError("img must be a 2-D float32 view whose rows are row_stride_bytes apart")
        r, c = img.shape
        n = ctypes.c_int(0)
        if mask is None:
            rc = self._L.sift_detect_compute(self.h, img.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), r, c,
                                             row_stride_bytes, None, None, 0, ctypes.byref(n))
        else:
            rc = self._L.sift_detect_compute_masked(self.h, img.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), r, c,
                                                    row_stride_bytes, mask.ctypes.data, c, None, None, 0,
                                                    ctypes.byref(n))
        if rc not in (SIFT_OK, SIFT_E_CAPACITY):
            self._check("sift_detect_compute", rc)
        kps = np.zeros(n.value, KEYPOINT_DTYPE)
        desc = np.zeros((n.value, DESC_LEN), np.float32)
        if n.value:
            rc = self._L.sift_copy_results(self.h, kps.ctypes.data, _fp(desc), n.value, ctypes.byref(n))
            self._check("sift_copy_results", rc)
        return kps, desc

    def Gaussian_Blur(self, src: np.ndarray, sigma: float) -> np.ndarray:
        src = np.ascontiguousarray(src, np.float32)
        dst = np.empty_like(src)
        self._check("sift_gaussian_blur",
                    self._L.sift_gaussian_blur(self.h, _fp(src), src.shape[0], src.shape[1], float(sigma), _fp(dst)))
        return dst

    def Gaussian_Blur_1D(self, src: np.ndarray, sigma: float) -> np.ndarray:
        src = np.ascontiguousarray(src, np.float32)
        dst = np.empty_like(src)
        self._check("sift_gaussian_blur_1d",
                    self._L.sift_gaussian_blur_1d(self.h, _fp(src), src.shape[0], src.shape[1], float(sigma), _fp(dst)))
        return dst

    def buildGaussianPyramid(self, image: np.ndarray, nOctaves: int = 5):
        image = np.ascontiguousarray(image, np.float32)
        r, c = image.shape
        out = np.empty(self._L.sift_packed_size(r, c, nOctaves, N_SCALES), np.float32)
        self._check("sift_build_gaussian_pyramid",
                    self._L.sift_build_gaussian_pyramid(self.h, _fp(image), r, c, nOctaves, _fp(out)))
        return split_planes(out, r, c, nOctaves, N_SCALES)

    def buildDoGPyramid(self, gpyr, nOctaves: int = 5):
        r, c = gpyr[0].shape
        g = pack_planes(gpyr, r, c, nOctaves, N_SCALES)
        out = np.empty(self._L.sift_packed_size(r, c, nOctaves, N_DOG), np.float32)
        self._check("sift_build_dog_pyramid",
                    self._L.sift_build_dog_pyramid(self.h, _fp(g), r, c, nOctaves, _fp(out)))
        return split_planes(out, r, c, nOctaves, N_DOG)

    def findScaleSpaceExtrema(self, gpyr, dogpyr, nOctaves: int = 5) -> np.ndarray:
        r, c = gpyr[0].shape
        g = pack_planes(gpyr, r, c, nOctaves, N_SCALES)
        d = pack_planes(dogpyr, r, c, nOctaves, N_DOG)
        n = ctypes.c_int(0)
        rc = self._L.sift_find_scale_space_extrema(self.h, _fp(g), _fp(d), r, c, nOctaves, None, 0, ctypes.byref(n))
        if rc not in (SIFT_OK, SIFT_E_CAPACITY):
            self._check("sift_find_scale_space_extrema", rc)
        kps = np.zeros(n.value, KEYPOINT_DTYPE)
        if n.value:
            rc = self._L.sift_copy_results(self.h, kps.ctypes.data, None, n.value, ctypes.byref(n))
            self._check("sift_copy_results", rc)
        return kps

    def compute(self, img: np.ndarray, keypoints: np.ndarray, max_layer: int = 4,
                upsample: bool = False) -> np.ndarray:
        """Feature2D::compute: the descriptors [n, 128] of img at the given keypoints
        (KEYPOINT_DTYPE rows, unchanged), in the pyramid SIFT_NCL builds for img.
        max_layer: no keypoint names a scale above it (3 for detected keypoints
        spares the widest blur).  A row outside the pyramid raises SiftError.
        upsample True: set_upsample(True) for this call -- the doubled image's
        pyramid, keypoints in img's own frame, octave -1 (byte 255) valid."""
        img = np.ascontiguousarray(img, np.float32)
        kps = np.ascontiguousarray(keypoints, KEYPOINT_DTYPE).reshape(-1)
        r, c = img.shape
        desc = np.zeros((len(kps), DESC_LEN), np.float32)
        with self._UpsampleCall(self, upsample):
            rc = self._L.sift_compute(self.h, _fp(img), r, c, c * 4, kps.ctypes.data, len(kps), max_layer, _fp(desc))
        self._check("sift_compute", rc)
        return desc

    def upsample2x(self, img: np.ndarray) -> np.ndarray:
        """img doubled along both axes: cv::resize(img, (2 * cols, 2 * rows), INTER_LINEAR) on
        float32 by the rule in include/sift_hip.h (sift_upsample2x); [2 * rows, 2 * cols] float32."""
        img = np.ascontiguousarray(img, np.float32)
        if img.ndim != 2:
            raise ValueError("expected a 2-D image")
        r, c = img.shape
        out = np.empty((2 * r, 2 * c), np.float32)
        self._check("sift_upsample2x", self._L.sift_upsample2x(self.h, _fp(img), r, c, c * 4, _fp(out)))
        return out

    def upsample2x_device(self, src_ptr: int, batch: int, rows: int, cols: int, row_stride: int, img_stride: int,
                          dst_ptr: int, out_row_stride: int, out_img_stride: int):
        """Device-pointer form (no sync) for a batch; strides in elements (floats)."""
        self._check("sift_upsample2x_device",
                    self._L.sift_upsample2x_device(self.h, ctypes.c_void_p(src_ptr), batch, rows, cols, row_stride,
                                                   img_stride, ctypes.c_void_p(dst_ptr), out_row_stride,
                                                   out_img_stride))

    def warpPerspective(self, img: np.ndarray, H, dsize, inverse: bool = False) -> np.ndarray:
        """cv::warpPerspective(img, H, dsize, INTER_LINEAR [| WARP_INVERSE_MAP], BORDER_CONSTANT, 0)
        by the rule in include/sift_hip.h (sift_warp_perspective).  img: float32 H x W, or uint8
        H x W / H x W x 3; dsize = (width, height) as in OpenCV; the result has img's dtype and
        channels.  An H that warps to nothing (singular, non-finite) raises SiftError with
        SIFT_E_INVALID."""
        img = np.asarray(img)
        if img.dtype == np.float32 and img.ndim == 2:
            pixel, ch = SIFT_PIXEL_F32, 1
        elif img.dtype == np.uint8 and (img.ndim == 2 or (img.ndim == 3 and img.shape[2] == 3)):
            pixel, ch = SIFT_PIXEL_U8, 1 if img.ndim == 2 else 3
        else:
            raise ValueError("expected a float32 H x W or a uint8 H x W / H x W x 3 image")
        img = np.ascontiguousarray(img)
        Hd = np.ascontiguousarray(H, np.float64).reshape(9)
        oc, orows = int(dsize[0]), int(dsize[1])
        if oc < 1 or orows < 1:
            raise ValueError("dsize must be (width, height), both at least 1")
        out = np.empty((orows, oc) if img.ndim == 2 else (orows, oc, 3), img.dtype)
        r, c = img.shape[:2]
        self._check("sift_warp_perspective",
                    self._L.sift_warp_perspective(self.h, pixel, ch, img.ctypes.data, r, c, 0,
                                                  Hd.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                  SIFT_WARP_INVERSE_MAP if inverse else 0, out.ctypes.data, orows, oc))
        return out

    def warp_perspective_segmented_device(self, pixel: int, channels: int, src_ptr: int, rows: int, cols: int,
                                          row_stride: int, img_stride: int, H_ptr: int, found_ptr: int,
                                          n_segments: int, flags: int, dst_ptr: int, out_rows: int, out_cols: int,
                                          out_row_stride: int = 0, out_img_stride: int = 0):
        """Device-pointer form (no sync): image b warped by H[b] ([n_segments][9] doubles, found_ptr
        [n_segments] ints or 0), exactly what find_homography_segmented_device leaves.  Strides in
        bytes, 0 = packed; img_stride 0 = one source image for every H."""
        vp = ctypes.c_void_p
        self._check("sift_warp_perspective_segmented_device",
                    self._L.sift_warp_perspective_segmented_device(
                        self.h, pixel, channels, vp(src_ptr), rows, cols, row_stride, img_stride, vp(H_ptr),
                        vp(found_ptr or None), n_segments, flags, vp(dst_ptr), out_rows, out_cols, out_row_stride,
                        out_img_stride))

    # ---- lens undistortion (undistort.hip; include/sift_hip.h has the rule) ----
    def undistort(self, img: np.ndarray, K, dist, newK=None, dsize=None) -> np.ndarray:
        """cv::undistort(img, K, dist, newK) with INTER_LINEAR and a zero border.  img: float32
        H x W, or uint8 H x W / H x W x 3; dist: up to eight coefficients (k1 k2 p1 p2 k3 k4 k5 k6);
        dsize = (width, height) of the result, the source size by default.  A camera with no rule
        (singular, non-finite) raises SiftError with SIFT_E_INVALID."""
        img = np.asarray(img)
        pixel, ch = _pixel_args(img)
        img = np.ascontiguousarray(img)
        Kd, dd, Nd = _camera(K, dist, newK)
        r, c = img.shape[:2]
        oc, orows = (c, r) if dsize is None else (int(dsize[0]), int(dsize[1]))
        if oc < 1 or orows < 1:
            raise ValueError("dsize must be (width, height), both at least 1")
        out = np.empty((orows, oc) if img.ndim == 2 else (orows, oc, 3), img.dtype)
        pdbl = ctypes.POINTER(ctypes.c_double)
        self._check("sift_undistort",
                    self._L.sift_undistort(self.h, pixel, ch, img.ctypes.data, r, c, 0, Kd.ctypes.data_as(pdbl),
                                           dd.ctypes.data_as(pdbl), None if Nd is None else Nd.ctypes.data_as(pdbl),
                                           out.ctypes.data, orows, oc))
        return out

    def undistort_batch_device(self, pixel: int, channels: int, src_ptr: int, rows: int, cols: int, row_stride: int,
                               img_stride: int, K_ptr: int, dist_ptr: int, newK_ptr: int, k_per_segment: int, n: int,
                               dst_ptr: int, out_rows: int, out_cols: int, out_row_stride: int = 0,
                               out_img_stride: int = 0):
        """Device-pointer form (no sync): n images through one camera (k_per_segment 0: K_ptr 9,
        dist_ptr 8, newK_ptr 9 float64, newK_ptr 0 = K) or one per image (k_per_segment 1).
        Strides in bytes, 0 = packed; img_stride 0 = one source image for every camera."""
        vp = ctypes.c_void_p
        self._check("sift_undistort_batch_device",
                    self._L.sift_undistort_batch_device(
                        self.h, pixel, channels, vp(src_ptr), rows, cols, row_stride, img_stride, vp(K_ptr),
                        vp(dist_ptr), vp(newK_ptr or None), int(k_per_segment), n, vp(dst_ptr), out_rows, out_cols,
                        out_row_stride, out_img_stride))

    def undistort_points_segmented_device(self, src_ptr: int, dst_ptr: int, xy_stride_bytes: int, m_offsets_ptr: int,
                                          n_segments: int, m_cap: int, K_ptr: int, dist_ptr: int, P_ptr: int,
                                          k_per_segment: int, iters: int, ok_ptr: int):
        """Device-pointer form (no sync) of undistortPoints for every segment of (x, y) float rows
        xy_stride_bytes apart (8: a point array; 28: a keypoint array); dst_ptr may be src_ptr;
        P_ptr 0 = normalised coordinates; ok_ptr [n_segments] int32."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_undistort_points_segmented_device",
                    self._L.sift_undistort_points_segmented_device(
                        self.h, vp(src_ptr), vp(dst_ptr), xy_stride_bytes, vp(m_offsets_ptr), n_segments, m_cap,
                        vp(K_ptr), vp(dist_ptr), vp(P_ptr), int(k_per_segment), int(iters), vp(ok_ptr)))

    def undistortPointsSegmented(self, xy, m_offsets, K, dist, P=None, iters: int = 5):
        """undistortPoints for every segment at once (host arrays): xy float32 [n, 2] or a
        KEYPOINT_DTYPE array (only x and y change), K / dist / P one camera or one per segment
        ([n_segments, 3, 3], [n_segments, <= 8], [n_segments, 3, 3]) -> (a new array like xy, ok
        int32 [n_segments]); rows outside the segments come back as they went in."""
        a = np.asarray(xy)
        if a.dtype == KEYPOINT_DTYPE:
            out, stride = np.ascontiguousarray(a).copy(), KEYPOINT_DTYPE.itemsize
        else:
            out, stride = np.ascontiguousarray(a, np.float32).reshape(-1, 2).copy(), 8
        mo = np.ascontiguousarray(m_offsets, np.int32)
        if mo.ndim != 1 or len(mo) < 1:
            raise ValueError("m_offsets must have n_segments + 1 entries")
        nseg = len(mo) - 1
        Ka = np.ascontiguousarray(K, np.float64).reshape(-1, 9)
        per = 0 if len(Ka) == 1 else 1
        da = np.asarray(dist, np.float64)
        da = da.reshape(len(Ka), -1) if per else da.reshape(1, -1)
        if da.shape[1] > 8:
            raise ValueError("at most eight distortion coefficients (k1 k2 p1 p2 k3 k4 k5 k6)")
        dd = np.zeros((len(Ka), 8), np.float64)
        dd[:, :da.shape[1]] = da
        Pa = None if P is None else np.ascontiguousarray(P, np.float64).reshape(-1, 9)
        if (per and len(Ka) != nseg) or (Pa is not None and len(Pa) != len(Ka)):
            raise ValueError("K, dist and P must all be one camera or all one per segment")
        ok = np.zeros(nseg, np.int32)
        pint, pdbl = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
        self._check("sift_undistort_points_segmented",
                    self._L.sift_undistort_points_segmented(
                        self.h, out.ctypes.data, out.ctypes.data, stride, mo.ctypes.data_as(pint), nseg, len(out),
                        Ka.ctypes.data_as(pdbl), dd.ctypes.data_as(pdbl),
                        None if Pa is None else Pa.ctypes.data_as(pdbl), per, int(iters), ok.ctypes.data_as(pint)))
        return out, ok

    def calDescriptor(self, gpyr, keypoints: np.ndarray, firstOctave: int = 0) -> np.ndarray:
        r, c = gpyr[0].shape
        n_oct = len(gpyr) // N_SCALES
        g = pack_planes(gpyr, r, c, n_oct, N_SCALES)
        kps = np.ascontiguousarray(keypoints, KEYPOINT_DTYPE)
        desc = np.zeros((len(kps), DESC_LEN), np.float32)
        self._check("sift_calc_descriptors",
                    self._L.sift_calc_descriptors(self.h, _fp(g), r, c, n_oct, kps.ctypes.data, len(kps),
                                                  _fp(desc), firstOctave))
        return desc

    def bgr8_to_gray(self, bgr: np.ndarray, out_rows: int | None = None, out_cols: int | None = None,
                     row_stride: int | None = None):
        """readImage's conversion (src/main.cpp:83-85) of decoded BGR bytes:
        optional INTER_LINEAR resize, COLOR_RGB2GRAY on BGR, CV_32F.
        row_stride None: bgr is copied to a packed array.  A number: bgr's own
        memory is passed with that row stride in bytes (an H x W x 3 uint8 view,
        such as an ROI, with packed pixels and rows that far apart); only the
        (H - 1) * row_stride + 3 * W bytes the view owns are read."""
        if row_stride is None:
            bgr = np.ascontiguousarray(bgr, np.uint8)
        if bgr.ndim != 3 or bgr.shape[2] != 3:
            raise ValueError("expected an H x W x 3 uint8 BGR image")
        r, c = bgr.shape[:2]
        if row_stride is None:
            row_stride = c * 3
        elif (bgr.dtype != np.uint8 or bgr.strides[1:] != (3, 1) or row_stride < c * 3
              or (r > 1 and bgr.strides[0] != row_stride)):
            raise ValueError("bgr must be an H x W x 3 uint8 view with packed pixels and rows row_stride bytes apart")
        orows, ocols = out_rows or r, out_cols or c
        gray = np.empty((orows, ocols), np.float32)
        self._check("sift_bgr8_to_gray",
                    self._L.sift_bgr8_to_gray(self.h, bgr.ctypes.data, r, c, row_stride, orows, ocols, _fp(gray)))
        return gray

    def bgr8_to_gray_device(self, src_ptr: int, batch: int, rows: int, cols: int, row_stride: int,
                            img_stride: int, out_rows: int, out_cols: int, dst_ptr: int, out_row_stride: int,
                            out_img_stride: int):
        self._check("sift_bgr8_to_gray_device",
                    self._L.sift_bgr8_to_gray_device(self.h, ctypes.c_void_p(src_ptr), batch, rows, cols,
                                                     row_stride, img_stride, out_rows, out_cols,
                                                     ctypes.c_void_p(dst_ptr), out_row_stride, out_img_stride))

    def knnMatch(self, query: np.ndarray, train: np.ndarray, k: int = 2):
        """BFMatcher(NORM_L1).knnMatch as arrays (src/main.cpp:25-27): idx, dist
        [n_query, k]; idx -1 / dist +inf where fewer than k train rows are at a
        finite distance (a row at +inf is never a neighbour)."""
        q = np.ascontiguousarray(query, np.float32).reshape(-1, DESC_LEN)
        t = np.ascontiguousarray(train, np.float32).reshape(-1, DESC_LEN)
        idx = np.empty((len(q), k), np.int32)
        dist = np.empty((len(q), k), np.float32)
        self._check("sift_knn_match_l1",
                    self._L.sift_knn_match_l1(self.h, _fp(q), len(q), _fp(t), len(t), k,
                                              idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _fp(dist)))
        return idx, dist

    def knn_match_device(self, query_ptr: int, n_query: int, train_ptr: int, n_train: int, k: int,
                         idx_ptr: int, dist_ptr: int):
        """Device-pointer form, enqueued on the context stream (no sync)."""
        self._check("sift_knn_match_l1_device",
                    self._L.sift_knn_match_l1_device(self.h, ctypes.c_void_p(query_ptr), n_query,
                                                     ctypes.c_void_p(train_ptr), n_train, k,
                                                     ctypes.c_void_p(idx_ptr), ctypes.c_void_p(dist_ptr)))

    # ---- a whole batch: segmented matcher + ratio test + point pairs -------
    # The three metrics' segmented entry points take the same arguments: one
    # helper per form, keyed by the C function's name.
    def _seg_device(self, fn, query_ptr, q_offsets_ptr, n_segments, q_cap, train_ptr, t_offsets_ptr, t_cap, k, idx_ptr,
                    dist_ptr):
        vp = ctypes.c_void_p
        self._check(fn, getattr(self._L, fn)(self.h, vp(query_ptr), vp(q_offsets_ptr), n_segments, q_cap, vp(train_ptr),
                                             vp(t_offsets_ptr or None), t_cap, k, vp(idx_ptr), vp(dist_ptr)))

    @staticmethod
    def _rows_arg(a):  # float rows go as float*, byte rows as void*
        return _fp(a) if a.dtype == np.float32 else a.ctypes.data

    def _seg_host(self, fn, q, q_offsets, t, t_offsets, k):
        qo = np.ascontiguousarray(q_offsets, np.int32)
        to = None if t_offsets is None else np.ascontiguousarray(t_offsets, np.int32)
        if qo.ndim != 1 or len(qo) < 1 or (to is not None and to.shape != qo.shape):
            raise ValueError("offsets must be 1-D, n_segments + 1 entries each")
        pint = ctypes.POINTER(ctypes.c_int)
        idx = np.full((len(q), k), -1, np.int32)
        dist = np.full((len(q), k), np.inf, np.float32)
        self._check(fn, getattr(self._L, fn)(
            self.h, self._rows_arg(q), qo.ctypes.data_as(pint), len(qo) - 1, len(q), self._rows_arg(t),
            None if to is None else to.ctypes.data_as(pint), len(t), k, idx.ctypes.data_as(pint), _fp(dist)))
        return idx, dist

    def _one_seg_u8(self, fn, query, train, k):
        q, t = self._u8_rows(query), self._u8_rows(train)
        idx = np.empty((len(q), k), np.int32)
        dist = np.empty((len(q), k), np.float32)
        self._check(fn, getattr(self._L, fn)(self.h, q.ctypes.data, len(q), t.ctypes.data, len(t), k,
                                             idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _fp(dist)))
        return idx, dist

    def knn_match_segmented_device(self, query_ptr: int, q_offsets_ptr: int, n_segments: int, q_cap: int,
                                   train_ptr: int, t_offsets_ptr: int | None, t_cap: int, k: int, idx_ptr: int,
                                   dist_ptr: int):
        """Device-pointer form (no sync): segment b = query rows
        [q_offsets[b], q_offsets[b+1]), offsets read on the device and clamped to
        q_cap / t_cap; t_offsets_ptr None = one shared train set.  Consecutive
        frames of a batch: train_ptr = query_ptr, t_offsets_ptr = q_offsets_ptr + 4,
        n_segments = batch - 1."""
        self._seg_device("sift_knn_match_l1_segmented_device", query_ptr, q_offsets_ptr, n_segments, q_cap, train_ptr,
                         t_offsets_ptr, t_cap, k, idx_ptr, dist_ptr)

    def ratio_matches_device(self, idx_ptr: int, dist_ptr: int, q_offsets_ptr: int, n_segments: int, q_cap: int,
                             ratio: float, q_kpts_ptr: int | None, t_kpts_ptr: int | None,
                             t_offsets_ptr: int | None, matches_ptr: int, src_xy_ptr: int | None,
                             dst_xy_ptr: int | None, m_cap: int, m_offsets_ptr: int):
        """Device-pointer form (no sync) of the ratio test, ordered compaction and
        point gather (src/main.cpp:28-52); q_kpts_ptr None = no point pairs."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_ratio_matches_device",
                    self._L.sift_ratio_matches_device(self.h, vp(idx_ptr), vp(dist_ptr), vp(q_offsets_ptr),
                                                      n_segments, q_cap, float(ratio), vp(q_kpts_ptr),
                                                      vp(t_kpts_ptr), vp(t_offsets_ptr), vp(matches_ptr),
                                                      vp(src_xy_ptr), vp(dst_xy_ptr), m_cap, vp(m_offsets_ptr)))

    def knnMatchSegmented(self, query: np.ndarray, q_offsets, train: np.ndarray, t_offsets=None, k: int = 2):
        """knnMatch for every segment at once (host arrays): idx, dist [len(query), k]
        with train indices local to the segment's train rows -- all of `train`
        (t_offsets None) or rows [t_offsets[b], t_offsets[b+1]).  Rows outside
        [q_offsets[0], q_offsets[-1]) keep idx -1 / dist +inf."""
        q = np.ascontiguousarray(query, np.float32).reshape(-1, DESC_LEN)
        t = np.ascontiguousarray(train, np.float32).reshape(-1, DESC_LEN)
        return self._seg_host("sift_knn_match_l1_segmented", q, q_offsets, t, t_offsets, k)

    def ratioMatches(self, idx: np.ndarray, dist: np.ndarray, q_offsets, ratio: float = 0.86, q_kpts=None,
                     t_kpts=None, t_offsets=None):
        """Ratio test + ordered compaction (+ point pairs with q_kpts / t_kpts) on
        knnMatchSegmented's k = 2 output: (matches [MATCH_DTYPE], m_offsets
        [n_segments + 1], src_xy, dst_xy [n, 2] float32 or None)."""
        ix = np.ascontiguousarray(idx, np.int32).reshape(-1, 2)
        ds = np.ascontiguousarray(dist, np.float32).reshape(-1, 2)
        qo = np.ascontiguousarray(q_offsets, np.int32)
        to = None if t_offsets is None else np.ascontiguousarray(t_offsets, np.int32)
        if len(ix) != len(ds) or qo.ndim != 1 or len(qo) < 1 or (to is not None and to.shape != qo.shape):
            raise ValueError("idx / dist must be [n, 2] and the offsets n_segments + 1 entries each")
        if (q_kpts is None) != (t_kpts is None):
            raise ValueError("point pairs need both q_kpts and t_kpts")
        pint = ctypes.POINTER(ctypes.c_int)
        n = len(ix)
        matches = np.zeros(n, MATCH_DTYPE)
        moff = np.zeros(len(qo), np.int32)
        qk = tk = src = dst = None
        if q_kpts is not None:
            qk = np.ascontiguousarray(q_kpts, KEYPOINT_DTYPE)
            tk = np.ascontiguousarray(t_kpts, KEYPOINT_DTYPE)
            if len(qk) != n:
                raise ValueError("q_kpts must have one row per query row")
            src, dst = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        self._check("sift_ratio_matches",
                    self._L.sift_ratio_matches(
                        self.h, ix.ctypes.data_as(pint), _fp(ds), qo.ctypes.data_as(pint), len(qo) - 1, n,
                        float(ratio), None if qk is None else qk.ctypes.data, None if tk is None else tk.ctypes.data,
                        0 if tk is None else len(tk), None if to is None else to.ctypes.data_as(pint),
                        matches.ctypes.data, None if src is None else _fp(src), None if dst is None else _fp(dst),
                        n, moff.ctypes.data_as(pint)))
        m = int(moff[-1])
        return matches[:m], moff, (None if src is None else src[:m]), (None if dst is None else dst[:m])

    # ---- 8-bit descriptors: the quantiser and the byte matcher (opt-in) --------
    def descriptors_to_u8_device(self, desc_ptr: int, n_rows_ptr: int | None, row_cap: int, out_ptr: int):
        """Device-pointer form (no sync): out[i][e] = saturate_cast<uchar>(desc[i][e] * 512)
        for rows [0, min(*n_rows_ptr, row_cap)), all row_cap rows with n_rows_ptr None.
        After detect_compute_batch: n_rows_ptr = offs_ptr + 4 * batch."""
        self._check("sift_descriptors_to_u8_device",
                    self._L.sift_descriptors_to_u8_device(self.h, ctypes.c_void_p(desc_ptr),
                                                          ctypes.c_void_p(n_rows_ptr or None), row_cap,
                                                          ctypes.c_void_p(out_ptr)))

    def descriptorsToU8(self, desc: np.ndarray) -> np.ndarray:
        """Float descriptors [n, 128] -> uint8 [n, 128] by the rule above (host arrays)."""
        d = np.ascontiguousarray(desc, np.float32).reshape(-1, DESC_LEN)
        out = np.empty((len(d), DESC_LEN), np.uint8)
        self._check("sift_descriptors_to_u8",
                    self._L.sift_descriptors_to_u8(self.h, _fp(d), len(d), out.ctypes.data))
        return out

    def knn_match_u8_segmented_device(self, query_ptr: int, q_offsets_ptr: int, n_segments: int, q_cap: int,
                                      train_ptr: int, t_offsets_ptr: int | None, t_cap: int, k: int, idx_ptr: int,
                                      dist_ptr: int):
        """knn_match_segmented_device on uint8 rows (no sync): same arguments and
        contract; dist stays float32 and holds the exact integer distance, so
        ratio_matches_device takes the output unchanged."""
        self._seg_device("sift_knn_match_l1_u8_segmented_device", query_ptr, q_offsets_ptr, n_segments, q_cap, train_ptr,
                         t_offsets_ptr, t_cap, k, idx_ptr, dist_ptr)

    @staticmethod
    def _u8_rows(a):
        a = np.asarray(a)
        if a.dtype != np.uint8:
            raise ValueError("expected uint8 descriptors")
        return np.ascontiguousarray(a).reshape(-1, DESC_LEN)

    def knnMatchU8Segmented(self, query: np.ndarray, q_offsets, train: np.ndarray, t_offsets=None, k: int = 2):
        """knnMatchSegmented on uint8 descriptors (host arrays): idx int32, dist
        float32 (integer-valued) [len(query), k]."""
        return self._seg_host("sift_knn_match_l1_u8_segmented", self._u8_rows(query), q_offsets, self._u8_rows(train), t_offsets, k)

    def knnMatchU8(self, query: np.ndarray, train: np.ndarray, k: int = 2):
        """knnMatch on uint8 descriptors: idx int32, dist float32 (integer-valued)
        [n_query, k]; idx -1 / dist +inf where there are fewer than k train rows."""
        return self._one_seg_u8("sift_knn_match_l1_u8", query, train, k)

    # ---- squared L2 on 8-bit descriptors (integer MFMA; opt-in) ----------------
    def knn_match_l2sqr_u8_segmented_device(self, query_ptr: int, q_offsets_ptr: int, n_segments: int, q_cap: int,
                                            train_ptr: int, t_offsets_ptr: int | None, t_cap: int, k: int,
                                            idx_ptr: int, dist_ptr: int):
        """knn_match_u8_segmented_device with the squared L2 distance (no sync):
        same arguments and contract; dist is float32 and holds the exact integer
        sum of (q - t)^2, at most 8,323,200.  No square root is taken: pass
        ratio * ratio to ratio_matches_device (0.86 ** 2 for the usual 0.86)."""
        self._seg_device("sift_knn_match_l2sqr_u8_segmented_device", query_ptr, q_offsets_ptr, n_segments, q_cap, train_ptr,
                         t_offsets_ptr, t_cap, k, idx_ptr, dist_ptr)

    def knnMatchL2SqrU8Segmented(self, query: np.ndarray, q_offsets, train: np.ndarray, t_offsets=None, k: int = 2):
        """knnMatchU8Segmented with the squared L2 distance (host arrays): idx
        int32, dist float32 (integer-valued, squared) [len(query), k]."""
        return self._seg_host("sift_knn_match_l2sqr_u8_segmented", self._u8_rows(query), q_offsets, self._u8_rows(train), t_offsets, k)

    def knnMatchL2SqrU8(self, query: np.ndarray, train: np.ndarray, k: int = 2):
        """knnMatchU8 with the squared L2 distance: idx int32, dist float32
        (integer-valued, squared) [n_query, k]; idx -1 / dist +inf where there
        are fewer than k train rows."""
        return self._one_seg_u8("sift_knn_match_l2sqr_u8", query, train, k)

    # ---- squared L2 on float descriptors (f32 MFMA; opt-in) --------------------
    def knn_match_l2sqr_f32_segmented_device(self, query_ptr: int, q_offsets_ptr: int, n_segments: int, q_cap: int,
                                             train_ptr: int, t_offsets_ptr: int | None, t_cap: int, k: int,
                                             idx_ptr: int, dist_ptr: int):
        """knn_match_segmented_device with the squared L2 distance on the float
        rows (no sync): same arguments and contract; dist is the squared distance
        by the rule of sift_hip.h (a fixed-order fmaf chain, d = nq + nt - 2 dot
        clamped at 0).  No square root is taken: pass ratio * ratio to
        ratio_matches_device (0.86 ** 2 for the usual 0.86).  Cross-check: a second
        call with the sides exchanged and k = 1, then cross_check_matches_device."""
        self._seg_device("sift_knn_match_l2sqr_f32_segmented_device", query_ptr, q_offsets_ptr, n_segments, q_cap,
                         train_ptr, t_offsets_ptr, t_cap, k, idx_ptr, dist_ptr)

    @staticmethod
    def _f32_rows(a):
        return np.ascontiguousarray(a, np.float32).reshape(-1, DESC_LEN)

    def knnMatchL2SqrF32Segmented(self, query: np.ndarray, q_offsets, train: np.ndarray, t_offsets=None, k: int = 2):
        """knnMatchSegmented with the squared L2 distance (host arrays): idx int32,
        dist float32 (squared) [len(query), k]."""
        return self._seg_host("sift_knn_match_l2sqr_f32_segmented", self._f32_rows(query), q_offsets,
                              self._f32_rows(train), t_offsets, k)

    def knnMatchL2SqrF32(self, query: np.ndarray, train: np.ndarray, k: int = 2):
        """knnMatch with the squared L2 distance on float descriptors: idx int32,
        dist float32 (squared) [n_query, k]; idx -1 / dist +inf where there are
        fewer than k train rows."""
        q, t = self._f32_rows(query), self._f32_rows(train)
        idx = np.empty((len(q), k), np.int32)
        dist = np.empty((len(q), k), np.float32)
        self._check("sift_knn_match_l2sqr_f32",
                    self._L.sift_knn_match_l2sqr_f32(self.h, _fp(q), len(q), _fp(t), len(t), k,
                                                     idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _fp(dist)))
        return idx, dist

    # ---- matching within a search window (spatially gated kNN) for a whole batch ----
    def knn_match_window_segmented_device(self, metric: int, query_ptr: int, q_kpts_ptr: int, q_offsets_ptr: int,
                                          n_segments: int, q_cap: int, train_ptr: int, t_kpts_ptr: int,
                                          t_offsets_ptr: int | None, t_cap: int, H_ptr: int | None,
                                          found_ptr: int | None, radius: float, rows: int, cols: int, k: int,
                                          idx_ptr: int, dist_ptr: int):
        """Device-pointer form (no sync) of the windowed matcher: the segmented
        matcher of the metric (SIFT_METRIC_L1_F32 / _L1_U8 / _L2SQR_U8), where a
        train row is a candidate only if its keypoint lies within `radius` (a closed
        square, float compare) of the query keypoint's predicted position: the
        position itself (H_ptr None, or found[b] == 0), else H[b] applied to it
        (H [n_segments][9] float64 and found [n_segments] int32 as
        find_homography_segmented_device writes them).  rows, cols: the train
        images' extent, a hint for the search grid only.  Same outputs and contract
        as knn_match_segmented_device otherwise."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_knn_match_window_segmented_device",
                    self._L.sift_knn_match_window_segmented_device(
                        self.h, int(metric), vp(query_ptr), vp(q_kpts_ptr), vp(q_offsets_ptr), n_segments, q_cap,
                        vp(train_ptr), vp(t_kpts_ptr), vp(t_offsets_ptr), t_cap, vp(H_ptr), vp(found_ptr),
                        float(radius), rows, cols, k, vp(idx_ptr), vp(dist_ptr)))

    def knnMatchWindowSegmented(self, metric: int, query: np.ndarray, q_kpts: np.ndarray, q_offsets,
                                train: np.ndarray, t_kpts: np.ndarray, t_offsets=None, radius: float = 32.0,
                                H=None, found=None, image_size=(1080, 1920), k: int = 2):
        """knn_match_window_segmented_device on host arrays (synchronous): idx int32,
        dist float32 [len(query), k].  query / train are float32 rows for
        SIFT_METRIC_L1_F32 and uint8 rows otherwise; q_kpts / t_kpts are
        KEYPOINT_DTYPE arrays, one per row; H is [n_segments, 9] (or [n_segments, 3,
        3]) float64, found [n_segments] int32; image_size = (rows, cols)."""
        if metric == SIFT_METRIC_L1_F32:
            q = np.ascontiguousarray(query, np.float32).reshape(-1, DESC_LEN)
            t = np.ascontiguousarray(train, np.float32).reshape(-1, DESC_LEN)
        else:
            q, t = self._u8_rows(query), self._u8_rows(train)
        qk, tk = np.ascontiguousarray(q_kpts, KEYPOINT_DTYPE), np.ascontiguousarray(t_kpts, KEYPOINT_DTYPE)
        if len(qk) != len(q) or len(tk) != len(t):
            raise ValueError("one keypoint per descriptor row")
        qo = np.ascontiguousarray(q_offsets, np.int32)
        to = None if t_offsets is None else np.ascontiguousarray(t_offsets, np.int32)
        if qo.ndim != 1 or len(qo) < 1 or (to is not None and to.shape != qo.shape):
            raise ValueError("offsets must be 1-D, n_segments + 1 entries each")
        n = len(qo) - 1
        Hh = None if H is None else np.ascontiguousarray(H, np.float64).reshape(-1, 9)
        fh = None if found is None else np.ascontiguousarray(found, np.int32)
        if (Hh is not None and len(Hh) != n) or (fh is not None and fh.shape != (n,)):
            raise ValueError("H is [n_segments, 9], found [n_segments]")
        pint = ctypes.POINTER(ctypes.c_int)
        idx = np.full((len(q), k), -1, np.int32)
        dist = np.full((len(q), k), np.inf, np.float32)
        self._check("sift_knn_match_window_segmented",
                    self._L.sift_knn_match_window_segmented(
                        self.h, int(metric), q.ctypes.data, qk.ctypes.data, qo.ctypes.data_as(pint), n, len(q),
                        t.ctypes.data, tk.ctypes.data, None if to is None else to.ctypes.data_as(pint), len(t),
                        None if Hh is None else Hh.ctypes.data, None if fh is None else fh.ctypes.data_as(pint),
                        float(radius), int(image_size[0]), int(image_size[1]), k, idx.ctypes.data_as(pint),
                        _fp(dist)))
        return idx, dist

    # ---- matching along epipolar lines (kNN gated by the batch's fundamental matrices) ----
    def knn_match_epipolar_segmented_device(self, metric: int, query_ptr: int, q_kpts_ptr: int, q_offsets_ptr: int,
                                            n_segments: int, q_cap: int, train_ptr: int, t_kpts_ptr: int,
                                            t_offsets_ptr: int | None, t_cap: int, F_ptr: int | None,
                                            found_ptr: int | None, band: float, radius: float, rows: int, cols: int,
                                            k: int, idx_ptr: int, dist_ptr: int):
        """Device-pointer form (no sync) of the epipolar matcher: the windowed
        matcher around the query keypoint's own position (`radius`, a closed square,
        float compare; +inf: no window), where a train row is a candidate only if
        the pair is also an inlier of the segment's fundamental matrix at `band`
        pixels -- find_fundamental's own float test, both point-to-epipolar-line
        distances <= band (src = query, dst = train).  F [n_segments][9] float64
        and found [n_segments] int32 as find_fundamental_segmented_device writes
        them; F_ptr None, or found[b] == 0: the window alone.  rows, cols: the train
        images' extent, a hint for the search grid only.  Same outputs and contract
        as knn_match_window_segmented_device otherwise."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_knn_match_epipolar_segmented_device",
                    self._L.sift_knn_match_epipolar_segmented_device(
                        self.h, int(metric), vp(query_ptr), vp(q_kpts_ptr), vp(q_offsets_ptr), n_segments, q_cap,
                        vp(train_ptr), vp(t_kpts_ptr), vp(t_offsets_ptr), t_cap, vp(F_ptr), vp(found_ptr),
                        float(band), float(radius), rows, cols, k, vp(idx_ptr), vp(dist_ptr)))

    def knnMatchEpipolarSegmented(self, metric: int, query: np.ndarray, q_kpts: np.ndarray, q_offsets,
                                  train: np.ndarray, t_kpts: np.ndarray, t_offsets=None, F=None, found=None,
                                  band: float = 3.0, radius: float = float("inf"), image_size=(1080, 1920),
                                  k: int = 2):
        """knn_match_epipolar_segmented_device on host arrays (synchronous): idx
        int32, dist float32 [len(query), k].  query / train are float32 rows for
        SIFT_METRIC_L1_F32 and uint8 rows otherwise; q_kpts / t_kpts are
        KEYPOINT_DTYPE arrays, one per row; F is [n_segments, 9] (or [n_segments, 3,
        3]) float64, found [n_segments] int32; image_size = (rows, cols)."""
        if metric == SIFT_METRIC_L1_F32:
            q = np.ascontiguousarray(query, np.float32).reshape(-1, DESC_LEN)
            t = np.ascontiguousarray(train, np.float32).reshape(-1, DESC_LEN)
        else:
            q, t = self._u8_rows(query), self._u8_rows(train)
        qk, tk = np.ascontiguousarray(q_kpts, KEYPOINT_DTYPE), np.ascontiguousarray(t_kpts, KEYPOINT_DTYPE)
        if len(qk) != len(q) or len(tk) != len(t):
            raise ValueError("one keypoint per descriptor row")
        qo = np.ascontiguousarray(q_offsets, np.int32)
        to = None if t_offsets is None else np.ascontiguousarray(t_offsets, np.int32)
        if qo.ndim != 1 or len(qo) < 1 or (to is not None and to.shape != qo.shape):
            raise ValueError("offsets must be 1-D, n_segments + 1 entries each")
        n = len(qo) - 1
        Fh = None if F is None else np.ascontiguousarray(F, np.float64).reshape(-1, 9)
        fh = None if found is None else np.ascontiguousarray(found, np.int32)
        if (Fh is not None and len(Fh) != n) or (fh is not None and fh.shape != (n,)):
            raise ValueError("F is [n_segments, 9], found [n_segments]")
        pint = ctypes.POINTER(ctypes.c_int)
        idx = np.full((len(q), k), -1, np.int32)
        dist = np.full((len(q), k), np.inf, np.float32)
        self._check("sift_knn_match_epipolar_segmented",
                    self._L.sift_knn_match_epipolar_segmented(
                        self.h, int(metric), q.ctypes.data, qk.ctypes.data, qo.ctypes.data_as(pint), n, len(q),
                        t.ctypes.data, tk.ctypes.data, None if to is None else to.ctypes.data_as(pint), len(t),
                        None if Fh is None else Fh.ctypes.data, None if fh is None else fh.ctypes.data_as(pint),
                        float(band), float(radius), int(image_size[0]), int(image_size[1]), k,
                        idx.ctypes.data_as(pint), _fp(dist)))
        return idx, dist

    # ---- cross-check (mutual nearest neighbours) for a whole batch ------------
    def cross_check_matches_device(self, idx_ptr: int, dist_ptr: int, fwd_k: int, q_offsets_ptr: int, n_segments: int,
                                   q_cap: int, ridx_ptr: int, rev_k: int, t_offsets_ptr: int, t_cap: int,
                                   ratio: float, q_kpts_ptr: int | None, t_kpts_ptr: int | None, matches_ptr: int,
                                   src_xy_ptr: int | None, dst_xy_ptr: int | None, m_cap: int, m_offsets_ptr: int):
        """Device-pointer form (no sync) of the cross-check stage: joins a forward
        result idx / dist [q_cap][fwd_k] with the reverse result ridx [t_cap][rev_k]
        (the same matcher with query and train exchanged; column 0 is read) into
        ratio_matches_device's outputs.  Row i of segment b is kept iff train row
        j = idx[i][0] of the segment's train range has ridx[j][0] == i (local), and,
        with ratio > 0 (needs fwd_k == 2), it passes the ratio test as well;
        ratio 0 = cross-check only.  t_offsets_ptr is required."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_cross_check_matches_device",
                    self._L.sift_cross_check_matches_device(
                        self.h, vp(idx_ptr), vp(dist_ptr), fwd_k, vp(q_offsets_ptr), n_segments, q_cap, vp(ridx_ptr),
                        rev_k, vp(t_offsets_ptr), t_cap, float(ratio), vp(q_kpts_ptr), vp(t_kpts_ptr),
                        vp(matches_ptr), vp(src_xy_ptr), vp(dst_xy_ptr), m_cap, vp(m_offsets_ptr)))

    def cross_match_segmented_device(self, metric: int, query_ptr: int, q_offsets_ptr: int, n_segments: int,
                                     q_cap: int, train_ptr: int, t_offsets_ptr: int, t_cap: int, ratio: float,
                                     q_kpts_ptr: int | None, t_kpts_ptr: int | None, matches_ptr: int,
                                     src_xy_ptr: int | None, dst_xy_ptr: int | None, m_cap: int, m_offsets_ptr: int):
        """Device-pointer form (no sync) of the whole job: the forward pass of the
        metric's segmented matcher (SIFT_METRIC_L1_F32 / _L1_U8 / _L2SQR_U8; k = 2
        when ratio > 0), the reverse pass and the cross-check stage, the tables in
        context scratch.  Consecutive frames of a batch: train_ptr = query_ptr,
        t_offsets_ptr = q_offsets_ptr + 4, t_cap = q_cap, n_segments = batch - 1.
        With SIFT_METRIC_L2SQR_U8 pass ratio * ratio."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_cross_match_segmented_device",
                    self._L.sift_cross_match_segmented_device(
                        self.h, int(metric), vp(query_ptr), vp(q_offsets_ptr), n_segments, q_cap, vp(train_ptr),
                        vp(t_offsets_ptr), t_cap, float(ratio), vp(q_kpts_ptr), vp(t_kpts_ptr), vp(matches_ptr),
                        vp(src_xy_ptr), vp(dst_xy_ptr), m_cap, vp(m_offsets_ptr)))

    def crossCheckMatches(self, idx: np.ndarray, ridx: np.ndarray, q_offsets, t_offsets, dist=None,
                          ratio: float = 0.0, q_kpts=None, t_kpts=None):
        """The cross-check stage on host arrays: idx [n_query, k] (and dist, the same
        shape; zeros when None, which needs ratio 0) from a segmented matcher, ridx
        [n_train, k'] from the same matcher with the sides exchanged, k and k' 1 or
        2 (1-D arrays count as k = 1).  Returns ratioMatches' tuple: (matches
        [MATCH_DTYPE], m_offsets [n_segments + 1], src_xy, dst_xy [n, 2] float32 or
        None)."""
        def rows(a, dtype):  # [n] -> [n, 1]; an empty array has no column count of its own
            a = np.ascontiguousarray(a, dtype)
            return a.reshape(len(a), -1) if a.size else a.reshape(0, 1)
        ix, rx = rows(idx, np.int32), rows(ridx, np.int32)
        if dist is None:
            if ratio != 0:
                raise ValueError("the ratio test needs dist")
            ds = np.zeros(ix.shape, np.float32)
        else:
            ds = rows(dist, np.float32)
        qo = np.ascontiguousarray(q_offsets, np.int32)
        to = np.ascontiguousarray(t_offsets, np.int32)
        if ix.shape[1] not in (1, 2) or rx.shape[1] not in (1, 2) or ds.shape != ix.shape:
            raise ValueError("idx / dist must be [n, 1] or [n, 2] (the same shape) and ridx [m, 1] or [m, 2]")
        if qo.ndim != 1 or len(qo) < 1 or to.shape != qo.shape:
            raise ValueError("the offsets must be 1-D, n_segments + 1 entries each")
        if (q_kpts is None) != (t_kpts is None):
            raise ValueError("point pairs need both q_kpts and t_kpts")
        pint = ctypes.POINTER(ctypes.c_int)
        n = len(ix)
        matches = np.zeros(n, MATCH_DTYPE)
        moff = np.zeros(len(qo), np.int32)
        qk = tk = src = dst = None
        if q_kpts is not None:
            qk = np.ascontiguousarray(q_kpts, KEYPOINT_DTYPE)
            tk = np.ascontiguousarray(t_kpts, KEYPOINT_DTYPE)
            if len(qk) != n or len(tk) != len(rx):
                raise ValueError("q_kpts / t_kpts must have one row per query / train row")
            src, dst = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        self._check("sift_cross_check_matches",
                    self._L.sift_cross_check_matches(
                        self.h, ix.ctypes.data_as(pint), _fp(ds), ix.shape[1], qo.ctypes.data_as(pint), len(qo) - 1, n,
                        rx.ctypes.data_as(pint), rx.shape[1], to.ctypes.data_as(pint), len(rx), float(ratio),
                        None if qk is None else qk.ctypes.data, None if tk is None else tk.ctypes.data,
                        matches.ctypes.data, None if src is None else _fp(src), None if dst is None else _fp(dst),
                        n, moff.ctypes.data_as(pint)))
        m = int(moff[-1])
        return matches[:m], moff, (None if src is None else src[:m]), (None if dst is None else dst[:m])

    # ---- a whole batch: homography per segment of the ratio stage's pairs ---
    def find_homography_segmented_device(self, src_xy_ptr: int, dst_xy_ptr: int, m_offsets_ptr: int,
                                         n_segments: int, m_cap: int, H_ptr: int, found_ptr: int,
                                         mask_ptr: int | None = None, ransacReprojThreshold: float = 3.0,
                                         maxIters: int = 2000, confidence: float = 0.995):
        """Device-pointer form (no sync) of findHomography(RANSAC) for every
        segment [m_offsets[b], m_offsets[b+1]) of ratio_matches_device's point
        pairs: H_ptr [n_segments][9] float64, found_ptr [n_segments] int32,
        mask_ptr [m_cap] uint8 or None."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_find_homography_segmented_device",
                    self._L.sift_find_homography_segmented_device(
                        self.h, vp(src_xy_ptr), vp(dst_xy_ptr), vp(m_offsets_ptr), n_segments, m_cap,
                        float(ransacReprojThreshold), int(maxIters), float(confidence), vp(H_ptr), vp(found_ptr),
                        vp(mask_ptr)))

    def perspective_transform_segmented_device(self, H_ptr: int, found_ptr: int, n_segments: int, xy_ptr: int,
                                               n_pts: int, out_xy_ptr: int):
        """Device-pointer form (no sync): out[b][i] = perspectiveTransform(xy[i], H[b]),
        zeros where found[b] == 0; out_xy_ptr is [n_segments][n_pts][2] float32."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_perspective_transform_segmented_device",
                    self._L.sift_perspective_transform_segmented_device(self.h, vp(H_ptr), vp(found_ptr), n_segments,
                                                                        vp(xy_ptr), n_pts, vp(out_xy_ptr)))

    def findHomographyBatch(self, src, dst, m_offsets, ransacReprojThreshold: float = 3.0, maxIters: int = 2000,
                            confidence: float = 0.995):
        """findHomography(RANSAC) for every segment at once (host arrays): a list
        of (H 3x3 float64 or None, inlier mask uint8[segment's pairs]) per
        segment, offsets clamped to the number of pairs."""
        s = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
        d = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
        mo = np.ascontiguousarray(m_offsets, np.int32)
        if len(s) != len(d) or mo.ndim != 1 or len(mo) < 1:
            raise ValueError("src / dst must be [n, 2] and m_offsets n_segments + 1 entries")
        nseg, n = len(mo) - 1, len(s)
        H = np.zeros((nseg, 9), np.float64)
        found = np.zeros(nseg, np.int32)
        mask = np.zeros(n, np.uint8)
        pint = ctypes.POINTER(ctypes.c_int)
        self._check("sift_find_homography_segmented",
                    self._L.sift_find_homography_segmented(
                        self.h, _fp(s), _fp(d), mo.ctypes.data_as(pint), nseg, n, float(ransacReprojThreshold),
                        int(maxIters), float(confidence), H.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                        found.ctypes.data_as(pint), mask.ctypes.data))
        o = np.clip(mo.astype(np.int64), 0, n)
        return [(H[b].reshape(3, 3).copy() if found[b] else None, mask[o[b]:max(o[b], o[b + 1])].copy())
                for b in range(nseg)]

    # ---- a whole batch: affine / similarity transform per segment of the same pairs ---
    def estimate_affine_segmented_device(self, src_xy_ptr: int, dst_xy_ptr: int, m_offsets_ptr: int,
                                         n_segments: int, m_cap: int, model: int, H_ptr: int, found_ptr: int,
                                         mask_ptr: int | None = None, ransacReprojThreshold: float = 3.0,
                                         maxIters: int = 2000, confidence: float = 0.99):
        """Device-pointer form (no sync) of estimateAffine2D (model SIFT_MODEL_AFFINE)
        or estimateAffinePartial2D (SIFT_MODEL_SIMILARITY) for every segment
        [m_offsets[b], m_offsets[b+1]) of ratio_matches_device's point pairs:
        H_ptr [n_segments][9] float64 with the last row 0 0 1 (what the warp, the
        corner transform and the windowed matcher take), found_ptr [n_segments]
        int32, mask_ptr [m_cap] uint8 or None."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_estimate_affine_segmented_device",
                    self._L.sift_estimate_affine_segmented_device(
                        self.h, vp(src_xy_ptr), vp(dst_xy_ptr), vp(m_offsets_ptr), n_segments, m_cap, int(model),
                        float(ransacReprojThreshold), int(maxIters), float(confidence), vp(H_ptr), vp(found_ptr),
                        vp(mask_ptr)))

    def estimateAffineBatch(self, src, dst, m_offsets, model: int, ransacReprojThreshold: float = 3.0,
                            maxIters: int = 2000, confidence: float = 0.99):
        """estimateAffine2D / estimateAffinePartial2D for every segment at once
        (host arrays): a list of (A 2x3 float64 or None, inlier mask
        uint8[segment's pairs]) per segment, offsets clamped to the number of pairs."""
        s = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
        d = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
        mo = np.ascontiguousarray(m_offsets, np.int32)
        if len(s) != len(d) or mo.ndim != 1 or len(mo) < 1:
            raise ValueError("src / dst must be [n, 2] and m_offsets n_segments + 1 entries")
        nseg, n = len(mo) - 1, len(s)
        H = np.zeros((nseg, 9), np.float64)
        found = np.zeros(nseg, np.int32)
        mask = np.zeros(n, np.uint8)
        pint = ctypes.POINTER(ctypes.c_int)
        self._check("sift_estimate_affine_segmented",
                    self._L.sift_estimate_affine_segmented(
                        self.h, _fp(s), _fp(d), mo.ctypes.data_as(pint), nseg, n, int(model),
                        float(ransacReprojThreshold), int(maxIters), float(confidence),
                        H.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), found.ctypes.data_as(pint),
                        mask.ctypes.data))
        o = np.clip(mo.astype(np.int64), 0, n)
        return [(H[b, :6].reshape(2, 3).copy() if found[b] else None, mask[o[b]:max(o[b], o[b + 1])].copy())
                for b in range(nseg)]

    # ---- a whole batch: fundamental matrix per segment of the same pairs ---
    def find_fundamental_segmented_device(self, src_xy_ptr: int, dst_xy_ptr: int, m_offsets_ptr: int,
                                          n_segments: int, m_cap: int, F_ptr: int, found_ptr: int,
                                          mask_ptr: int | None = None, ransacReprojThreshold: float = 3.0,
                                          maxIters: int = 1000, confidence: float = 0.99):
        """Device-pointer form (no sync) of findFundamentalMat(FM_RANSAC) for every
        segment [m_offsets[b], m_offsets[b+1]) of ratio_matches_device's point
        pairs: F_ptr [n_segments][9] float64 ([dst;1]^T F [src;1] = 0), found_ptr
        [n_segments] int32, mask_ptr [m_cap] uint8 or None."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_find_fundamental_segmented_device",
                    self._L.sift_find_fundamental_segmented_device(
                        self.h, vp(src_xy_ptr), vp(dst_xy_ptr), vp(m_offsets_ptr), n_segments, m_cap,
                        float(ransacReprojThreshold), int(maxIters), float(confidence), vp(F_ptr), vp(found_ptr),
                        vp(mask_ptr)))

    def findFundamentalBatch(self, src, dst, m_offsets, ransacReprojThreshold: float = 3.0, maxIters: int = 1000,
                             confidence: float = 0.99):
        """findFundamentalMat(FM_RANSAC) for every segment at once (host arrays): a
        list of (F 3x3 float64 or None, inlier mask uint8[segment's pairs]) per
        segment, offsets clamped to the number of pairs."""
        s = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
        d = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
        mo = np.ascontiguousarray(m_offsets, np.int32)
        if len(s) != len(d) or mo.ndim != 1 or len(mo) < 1:
            raise ValueError("src / dst must be [n, 2] and m_offsets n_segments + 1 entries")
        nseg, n = len(mo) - 1, len(s)
        F = np.zeros((nseg, 9), np.float64)
        found = np.zeros(nseg, np.int32)
        mask = np.zeros(n, np.uint8)
        pint = ctypes.POINTER(ctypes.c_int)
        self._check("sift_find_fundamental_segmented",
                    self._L.sift_find_fundamental_segmented(
                        self.h, _fp(s), _fp(d), mo.ctypes.data_as(pint), nseg, n, float(ransacReprojThreshold),
                        int(maxIters), float(confidence), F.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                        found.ctypes.data_as(pint), mask.ctypes.data))
        o = np.clip(mo.astype(np.int64), 0, n)
        return [(F[b].reshape(3, 3).copy() if found[b] else None, mask[o[b]:max(o[b], o[b + 1])].copy())
                for b in range(nseg)]

    # ---- a whole batch: relative pose per segment from its fundamental matrix, and triangulation ---
    def recover_pose_segmented_device(self, src_xy_ptr: int, dst_xy_ptr: int, m_offsets_ptr: int, n_segments: int,
                                      m_cap: int, F_ptr: int, found_ptr: int, K_src_ptr: int, K_dst_ptr: int,
                                      pose_ptr: int, pose_found_ptr: int, n_good_ptr: int, k_per_segment: int = 0,
                                      mask_in_ptr: int | None = None, distanceThresh: float = 50.0,
                                      E_ptr: int | None = None, mask_out_ptr: int | None = None,
                                      xyz_ptr: int | None = None):
        """Device-pointer form (no sync) of recoverPose for every segment
        [m_offsets[b], m_offsets[b+1]) of the point pairs: F_ptr / found_ptr /
        mask_in_ptr exactly as find_fundamental_segmented_device leaves them,
        K_*_ptr one 3x3 float64 each (k_per_segment 0) or [n_segments][9] (1);
        pose_ptr [n_segments][12] float64 ([R | t] by rows), pose_found_ptr and
        n_good_ptr [n_segments] int32, E_ptr [n_segments][9], mask_out_ptr [m_cap]
        uint8 and xyz_ptr [m_cap][3] float64 or None."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_recover_pose_segmented_device",
                    self._L.sift_recover_pose_segmented_device(
                        self.h, vp(src_xy_ptr), vp(dst_xy_ptr), vp(m_offsets_ptr), n_segments, m_cap, vp(F_ptr),
                        vp(found_ptr), vp(K_src_ptr), vp(K_dst_ptr), int(k_per_segment), vp(mask_in_ptr),
                        float(distanceThresh), vp(pose_ptr), vp(E_ptr), vp(pose_found_ptr), vp(n_good_ptr),
                        vp(mask_out_ptr), vp(xyz_ptr)))

    def recoverPoseBatch(self, F, found, K_src, K_dst, src, dst, m_offsets, mask=None, distanceThresh: float = 50.0):
        """recoverPose for every segment at once (host arrays): F [n_segments, 3, 3]
        or [n_segments, 9] and found [n_segments] as findFundamentalBatch gives
        them (None / 0 = no model), K_src / K_dst one 3x3 or [n_segments, 3, 3],
        mask [n] or None -> a list of (R 3x3, t 3, E 3x3, mask uint8[segment's
        pairs], xyz float64[segment's pairs, 3], n_good) per segment, R = t = E =
        None where the segment has no pose; offsets clamped to the number of pairs."""
        s = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
        d = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
        mo = np.ascontiguousarray(m_offsets, np.int32)
        if len(s) != len(d) or mo.ndim != 1 or len(mo) < 1:
            raise ValueError("src / dst must be [n, 2] and m_offsets n_segments + 1 entries")
        nseg, n = len(mo) - 1, len(s)
        Fa = np.ascontiguousarray(np.asarray(F, np.float64).reshape(nseg, 9))
        fa = np.ascontiguousarray(found, np.int32).reshape(nseg)
        Ks = np.ascontiguousarray(K_src, np.float64).reshape(-1, 9)
        Kd = np.ascontiguousarray(K_dst, np.float64).reshape(-1, 9)
        per = 0 if len(Ks) == 1 and len(Kd) == 1 else 1
        if per and (len(Ks) != nseg or len(Kd) != nseg):
            raise ValueError("K_src / K_dst must both be one 3x3 or both [n_segments, 3, 3]")
        mi = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
        if mi is not None and len(mi) != n:
            raise ValueError("mask must have one byte per pair")
        pose, E = np.zeros((nseg, 12), np.float64), np.zeros((nseg, 9), np.float64)
        pf, ng = np.zeros(nseg, np.int32), np.zeros(nseg, np.int32)
        mout, xyz = np.zeros(n, np.uint8), np.zeros((n, 3), np.float64)
        pint, pdbl = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
        self._check("sift_recover_pose_segmented",
                    self._L.sift_recover_pose_segmented(
                        self.h, _fp(s), _fp(d), mo.ctypes.data_as(pint), nseg, n, Fa.ctypes.data_as(pdbl),
                        fa.ctypes.data_as(pint), Ks.ctypes.data_as(pdbl), Kd.ctypes.data_as(pdbl), per,
                        None if mi is None else mi.ctypes.data, float(distanceThresh), pose.ctypes.data_as(pdbl),
                        E.ctypes.data_as(pdbl), pf.ctypes.data_as(pint), ng.ctypes.data_as(pint), mout.ctypes.data,
                        xyz.ctypes.data))
        o = np.clip(mo.astype(np.int64), 0, n)
        out = []
        for b in range(nseg):
            rows = slice(o[b], max(o[b], o[b + 1]))
            P = pose[b].reshape(3, 4)
            out.append((P[:, :3].copy() if pf[b] else None, P[:, 3].copy() if pf[b] else None,
                        E[b].reshape(3, 3).copy() if pf[b] else None, mout[rows].copy(), xyz[rows].copy(), int(ng[b])))
        return out

    def triangulate_points_segmented_device(self, src_xy_ptr: int, dst_xy_ptr: int, m_offsets_ptr: int,
                                            n_segments: int, m_cap: int, P_src_ptr: int, P_dst_ptr: int,
                                            xyzw_ptr: int):
        """Device-pointer form (no sync) of triangulatePoints for every segment of
        the point pairs under its own cameras: P_*_ptr [n_segments][12] float64
        (recover_pose_segmented_device's pose_ptr is a P_dst), xyzw_ptr [m_cap][4]
        float64, homogeneous and not divided."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_triangulate_points_segmented_device",
                    self._L.sift_triangulate_points_segmented_device(
                        self.h, vp(src_xy_ptr), vp(dst_xy_ptr), vp(m_offsets_ptr), n_segments, m_cap, vp(P_src_ptr),
                        vp(P_dst_ptr), vp(xyzw_ptr)))

    # ---- a whole batch: absolute pose per segment from 3-D / 2-D rows (PnP RANSAC over P3P) ---
    def solve_pnp_segmented_device(self, xyz_ptr: int, xy_ptr: int, m_offsets_ptr: int, n_segments: int, m_cap: int,
                                   K_ptr: int, pose_ptr: int, found_ptr: int, n_inliers_ptr: int,
                                   k_per_segment: int = 0, row_mask_ptr: int | None = None,
                                   reprojectionError: float = 8.0, iterationsCount: int = 100,
                                   confidence: float = 0.99, inlier_mask_ptr: int | None = None):
        """Device-pointer form (no sync) of solvePnPRansac for every segment
        [m_offsets[b], m_offsets[b+1]) of the rows: xyz_ptr [m_cap][3] float64 and
        row_mask_ptr [m_cap] uint8 (or None) exactly as
        recover_pose_segmented_device leaves xyz_ptr / mask_out_ptr, xy_ptr
        [m_cap][2] float32 pixels of the view to register, K_ptr one 3x3 float64
        (k_per_segment 0) or [n_segments][9] (1); pose_ptr [n_segments][12]
        float64 ([R | t] by rows, X_cam = R X + t), found_ptr and n_inliers_ptr
        [n_segments] int32, inlier_mask_ptr [m_cap] uint8 or None."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_solve_pnp_segmented_device",
                    self._L.sift_solve_pnp_segmented_device(
                        self.h, vp(xyz_ptr), vp(xy_ptr), vp(m_offsets_ptr), n_segments, m_cap, vp(row_mask_ptr),
                        vp(K_ptr), int(k_per_segment), float(reprojectionError), int(iterationsCount),
                        float(confidence), vp(pose_ptr), vp(found_ptr), vp(n_inliers_ptr), vp(inlier_mask_ptr)))

    def solvePnPBatch(self, objectPoints, imagePoints, m_offsets, K, reprojectionError: float = 8.0,
                      iterationsCount: int = 100, confidence: float = 0.99, row_mask=None):
        """solvePnPRansac for every segment at once (host arrays): objectPoints
        [n, 3], imagePoints [n, 2], K one 3x3 or [n_segments, 3, 3], row_mask [n]
        or None -> a list of (R 3x3, t 3, mask uint8[segment's rows], n_inliers)
        per segment, R = t = None where the segment has no model; offsets clamped
        to the number of rows."""
        X = np.ascontiguousarray(objectPoints, np.float64).reshape(-1, 3)
        p = np.ascontiguousarray(imagePoints, np.float32).reshape(-1, 2)
        mo = np.ascontiguousarray(m_offsets, np.int32)
        if len(X) != len(p) or mo.ndim != 1 or len(mo) < 1:
            raise ValueError("objectPoints [n, 3] / imagePoints [n, 2] and m_offsets n_segments + 1 entries")
        nseg, n = len(mo) - 1, len(X)
        Ka = np.ascontiguousarray(K, np.float64).reshape(-1, 9)
        per = 0 if len(Ka) == 1 else 1
        if per and len(Ka) != nseg:
            raise ValueError("K must be one 3x3 or [n_segments, 3, 3]")
        mi = None if row_mask is None else np.ascontiguousarray(row_mask, np.uint8).reshape(-1)
        if mi is not None and len(mi) != n:
            raise ValueError("row_mask must have one byte per row")
        pose = np.zeros((nseg, 12), np.float64)
        fo, ni = np.zeros(nseg, np.int32), np.zeros(nseg, np.int32)
        mout = np.zeros(n, np.uint8)
        pint, pdbl = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
        self._check("sift_solve_pnp_segmented",
                    self._L.sift_solve_pnp_segmented(
                        self.h, X.ctypes.data_as(pdbl), _fp(p), mo.ctypes.data_as(pint), nseg, n,
                        None if mi is None else mi.ctypes.data, Ka.ctypes.data_as(pdbl), per,
                        float(reprojectionError), int(iterationsCount), float(confidence), pose.ctypes.data_as(pdbl),
                        fo.ctypes.data_as(pint), ni.ctypes.data_as(pint), mout.ctypes.data))
        o = np.clip(mo.astype(np.int64), 0, n)
        out = []
        for b in range(nseg):
            rows = slice(o[b], max(o[b], o[b + 1]))
            P = pose[b].reshape(3, 4)
            out.append((P[:, :3].copy() if fo[b] else None, P[:, 3].copy() if fo[b] else None, mout[rows].copy(),
                        int(ni[b])))
        return out

    # ---- a whole batch: the join of two match tables on a shared keypoint (2-D / 3-D rows) ---
    def join_matches_segmented_device(self, a_ptr: int, a_offsets_ptr: int, a_cap: int, a_key_side: int,
                                      a_xyz_ptr: int | None, b_ptr: int, b_offsets_ptr: int, b_cap: int,
                                      b_key_side: int, b_xy_ptr: int | None, key_offsets_ptr: int, key_cap: int,
                                      n_segments: int, j_cap: int, j_offsets_ptr: int,
                                      xyz_out_ptr: int | None = None, xy_out_ptr: int | None = None,
                                      a_row_ptr: int | None = None, b_row_ptr: int | None = None,
                                      b_joined_ptr: int | None = None, a_mask_ptr: int | None = None,
                                      b_mask_ptr: int | None = None):
        """Device-pointer form (no sync) of joinMatches for every segment: segment s
        joins A rows [a_offsets[s], a_offsets[s+1]) with B rows [b_offsets[s],
        b_offsets[s+1]) on a key below key_offsets[s+1] - key_offsets[s] (offsets read
        on the device and clamped to a_cap / b_cap / key_cap).  a_xyz_ptr [a_cap][3]
        float64 and a_mask_ptr [a_cap] uint8 exactly as recover_pose_segmented_device
        leaves xyz_ptr / mask_out_ptr; b_xy_ptr [b_cap][2] float32.  Outputs:
        xyz_out_ptr [j_cap][3] float64, xy_out_ptr [j_cap][2] float32, a_row_ptr /
        b_row_ptr [j_cap] int32 (absolute rows), b_joined_ptr [b_cap] uint8,
        j_offsets_ptr [n_segments + 1] int32 (the last entry is the true total).
        Consecutive frames of a batch, on ratio_matches_device's one table: b_ptr =
        a_ptr, b_offsets_ptr = a_offsets_ptr + 4, a_key_side = JOIN_TRAIN, b_key_side =
        JOIN_QUERY, b_xy_ptr = dst_xy_ptr, key_offsets_ptr = the keypoint offsets + 4,
        n_segments = batch - 2; xyz_out_ptr, xy_out_ptr and j_offsets_ptr then feed
        solve_pnp_segmented_device."""
        vp = lambda p: ctypes.c_void_p(p or None)  # noqa: E731
        self._check("sift_join_matches_segmented_device",
                    self._L.sift_join_matches_segmented_device(
                        self.h, vp(a_ptr), vp(a_offsets_ptr), a_cap, int(a_key_side), vp(a_mask_ptr), vp(a_xyz_ptr),
                        vp(b_ptr), vp(b_offsets_ptr), b_cap, int(b_key_side), vp(b_mask_ptr), vp(b_xy_ptr),
                        vp(key_offsets_ptr), key_cap, n_segments, vp(xyz_out_ptr), vp(xy_out_ptr), vp(a_row_ptr),
                        vp(b_row_ptr), vp(b_joined_ptr), j_cap, vp(j_offsets_ptr)))

    def joinMatchesSegmented(self, a, a_offsets, a_xyz, b, b_offsets, b_xy, key_offsets, a_key_side: int,
                             b_key_side: int, a_mask=None, b_mask=None, j_cap: int | None = None,
                             key_cap: int | None = None):
        """joinMatches for every segment at once (host arrays): a / b MATCH_DTYPE
        tables, a_xyz [len(a), 3], b_xy [len(b), 2], the three offset arrays
        n_segments + 1 entries each, key_offsets the shared views' keypoint offsets
        -> (xyz [n, 3], xy [n, 2], a_row [n], b_row [n], b_joined uint8[len(b)],
        j_offsets [n_segments + 1]); rows are absolute, n = min(j_offsets[-1],
        j_cap), j_cap defaults to len(b), key_cap (the keypoint count the key
        offsets are clamped to) to the largest key offset."""
        A, B, X, P, am, bm = _join_tables(a, a_xyz, b, b_xy, a_mask, b_mask)
        ao, bo, ko = (np.ascontiguousarray(o, np.int32) for o in (a_offsets, b_offsets, key_offsets))
        if ao.ndim != 1 or len(ao) < 1 or bo.shape != ao.shape or ko.shape != ao.shape:
            raise ValueError("a_offsets, b_offsets and key_offsets must have n_segments + 1 entries each")
        cap = len(B) if j_cap is None else int(j_cap)
        key_cap = int(max(0, ko.max())) if key_cap is None else int(key_cap)
        n = max(cap, 1)
        xyz, xy = np.zeros((n, 3), np.float64), np.zeros((n, 2), np.float32)
        ar, br = np.zeros(n, np.int32), np.zeros(n, np.int32)
        bj, jo = np.zeros(max(len(B), 1), np.uint8), np.zeros(len(ao), np.int32)
        d = lambda v: None if v is None else v.ctypes.data  # noqa: E731
        self._check("sift_join_matches_segmented",
                    self._L.sift_join_matches_segmented(
                        self.h, d(A), d(ao), len(A), int(a_key_side), d(am), d(X), d(B), d(bo), len(B),
                        int(b_key_side), d(bm), d(P), d(ko), key_cap, len(ao) - 1, d(xyz), d(xy), d(ar), d(br), d(bj),
                        cap, d(jo)))
        m = min(int(jo[-1]), cap)
        return xyz[:m], xy[:m], ar[:m], br[:m], bj[:len(B)], jo

    # ---- device batch API ------------------------------------------------
    def synth_images(self, out_ptr: int, batch: int, rows: int, cols: int, row_stride: int,
                     img_stride: int, seed_base: int = 0):
        self._check("sift_synth_images",
                    self._L.sift_synth_images(self.h, ctypes.c_void_p(out_ptr), batch, rows, cols,
                                              row_stride, img_stride, seed_base))

    def detect_compute_batch(self, imgs_ptr: int, batch: int, rows: int, cols: int, row_stride: int,
                             img_stride: int, kpts_ptr: int, desc_ptr: int, kp_cap: int, offs_ptr: int,
                             masks_ptr: int = 0, mask_row_stride: int = 0, mask_img_stride: int = 0):
        """masks_ptr: device uint8 detection masks, image b's at masks_ptr + b * mask_img_stride with rows
        mask_row_stride bytes apart (mask_img_stride 0: one mask for the whole batch); 0 = no mask."""
        if not masks_ptr:
            self._check("sift_detect_compute_batch",
                        self._L.sift_detect_compute_batch(self.h, ctypes.c_void_p(imgs_ptr), batch, rows, cols,
                                                          row_stride, img_stride, ctypes.c_void_p(kpts_ptr),
                                                          ctypes.c_void_p(desc_ptr), kp_cap,
                                                          ctypes.c_void_p(offs_ptr)))
            return
        self._check("sift_detect_compute_batch_masked",
                    self._L.sift_detect_compute_batch_masked(self.h, ctypes.c_void_p(imgs_ptr), batch, rows, cols,
                                                             row_stride, img_stride, ctypes.c_void_p(masks_ptr),
                                                             mask_row_stride, mask_img_stride,
                                                             ctypes.c_void_p(kpts_ptr), ctypes.c_void_p(desc_ptr),
                                                             kp_cap, ctypes.c_void_p(offs_ptr)))

    def compute_batch(self, imgs_ptr: int, batch: int, rows: int, cols: int, row_stride: int, img_stride: int,
                      kpts_ptr: int, kp_offsets_ptr: int, kp_cap: int, desc_ptr: int, max_layer: int = 4):
        """Device-pointer form (no sync) of Feature2D::compute for a batch: describes rows
        [kp_offsets[b], kp_offsets[b+1]) of kpts_ptr in image b -- the offsets are device
        ints as detect_compute_batch leaves them, clamped to kp_cap -- into the same rows of
        desc_ptr.  max_layer: no row names a scale above it (include/sift_hip.h)."""
        self._check("sift_compute_batch",
                    self._L.sift_compute_batch(self.h, ctypes.c_void_p(imgs_ptr), batch, rows, cols, row_stride,
                                               img_stride, ctypes.c_void_p(kpts_ptr),
                                               ctypes.c_void_p(kp_offsets_ptr), kp_cap, max_layer,
                                               ctypes.c_void_p(desc_ptr)))

    def selftest_math(self, op: int, a: np.ndarray, b: np.ndarray | None = None) -> np.ndarray:
        """One device helper element-wise (sift_hip.h lists ops 0..7); ops 8 / 9 are the
        homography's update_num_iters(0.995 / 0.5, (b - a) / b, 4, 2000) for a = good
        inliers of b = n pairs, integers as float32, the result as float32."""
        a = np.ascontiguousarray(a, np.float32)
        bb = np.ascontiguousarray(b if b is not None else a, np.float32)
        out = np.empty_like(a)
        self._check("sift_selftest_math",
                    self._L.sift_selftest_math(self.h, op, _fp(a), _fp(bb), _fp(out), a.size))
        return out

    def selftest_g4_points(self, plane: np.ndarray, rc: np.ndarray) -> np.ndarray:
        """Gaussian_Blur(plane, sig[4]) on the 3x3 around each point (r, c) of rc [n, 2], by the
        point evaluation of batch SIFT_NCL's sparse flow: [n, 3, 3] float32."""
        plane = np.ascontiguousarray(plane, np.float32)
        rc = np.ascontiguousarray(rc, np.int32).reshape(-1, 2)
        out = np.empty((len(rc), 3, 3), np.float32)
        self._check("sift_selftest_g4_points",
                    self._L.sift_selftest_g4_points(self.h, _fp(plane), plane.shape[0], plane.shape[1],
                                                    rc.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), len(rc), _fp(out)))
        return out

    def stage_stats(self, reset: bool = True):
        buf = (StageStat * 32)()
        n = ctypes.c_int(0)
        self._check("sift_get_stage_stats",
                    self._L.sift_get_stage_stats(self.h, buf, 32, ctypes.byref(n), int(reset)))
        return {buf[i].name.decode(): dict(launches=buf[i].launches, ms=buf[i].ms, flops=buf[i].flops,
                                           bytes=buf[i].bytes) for i in range(n.value)}


def multi_shard(batch: int, n_devices: int, index: int) -> tuple[int, int]:
    """(first, count) of device `index`'s contiguous shard (sift_multi_shard)."""
    f, c = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib().sift_multi_shard(batch, n_devices, index, ctypes.byref(f), ctypes.byref(c))
    if rc != SIFT_OK:
        raise SiftError("sift_multi_shard", rc, "bad arguments")
    return f.value, c.value


def multi_merge_offsets(shard_offsets) -> np.ndarray:
    """Global per-image offsets from each shard's own (sift_multi_merge_offsets)."""
    arrs = [np.ascontiguousarray(o, np.int32) for o in shard_offsets]
    pint = ctypes.POINTER(ctypes.c_int)
    ptrs = (pint * len(arrs))(*[a.ctypes.data_as(pint) for a in arrs])
    counts = np.array([len(a) - 1 for a in arrs], np.int32)
    out = np.zeros(int(counts.sum()) + 1, np.int32)
    rc = lib().sift_multi_merge_offsets(ptrs, counts.ctypes.data_as(pint), len(arrs), out.ctypes.data_as(pint))
    if rc != SIFT_OK:
        raise SiftError("sift_multi_merge_offsets", rc, "bad arguments")
    return out


class MultiContext:
    """Multi-GPU batch mode (sift_multi_*): one context + stream per device,
    contiguous image shards, the keypoint records (and optionally the
    descriptors) gathered to devices[0] over RCCL one step behind."""

    def __init__(self, devices, max_rows: int, max_cols: int, max_batch_per_device: int, kp_cap_per_device: int,
                 flags: int = 0, gather_desc: bool = False, streams_per_device: int = 0):
        self._L = lib()
        self.devices = list(devices)
        dv = (ctypes.c_int * len(self.devices))(*self.devices)
        h = ctypes.c_void_p()
        rc = self._L.sift_multi_create(dv, len(self.devices), max_rows, max_cols, max_batch_per_device, flags,
                                       streams_per_device, kp_cap_per_device, int(gather_desc), ctypes.byref(h))
        if rc != SIFT_OK:
            raise SiftError("sift_multi_create", rc, "could not create the multi-GPU context (see stderr)")
        self.h = h
        self.gather_desc = gather_desc

    def close(self):
        if getattr(self, "h", None):
            self._L.sift_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, fn, rc):
        if rc != SIFT_OK:
            raise SiftError(fn, rc, self._L.sift_multi_last_error(self.h).decode())

    def context_handle(self, index: int):
        return self._L.sift_multi_context(self.h, index)

    def set_octaves(self, n: int):
        self._check("sift_multi_set_octaves", self._L.sift_multi_set_octaves(self.h, n))

    def set_flags(self, flags: int):
        self._check("sift_multi_set_flags", self._L.sift_multi_set_flags(self.h, flags))

    def set_max_features(self, n: int):
        """Context.set_max_features on every context."""
        self._check("sift_multi_set_max_features", self._L.sift_multi_set_max_features(self.h, n))

    def synth_images(self, index: int, out_ptr: int, batch: int, rows: int, cols: int, row_stride: int,
                     img_stride: int, seed_base: int = 0):
        rc = self._L.sift_synth_images(ctypes.c_void_p(self.context_handle(index)), ctypes.c_void_p(out_ptr), batch,
                                       rows, cols, row_stride, img_stride, seed_base)
        self._check("sift_synth_images", rc)

    def step(self, img_ptrs, counts, rows: int, cols: int, row_stride: int, img_stride: int, mask_ptrs=None,
             mask_row_stride: int = 0, mask_img_stride: int = 0):
        """mask_ptrs: per device, a pointer to its uint8 detection masks (strides in bytes as in
        Context.detect_compute_batch) or 0 / None for no mask on that device; None = no masks."""
        n = len(self.devices)
        ptrs = (ctypes.c_void_p * n)(*[ctypes.c_void_p(p) for p in img_ptrs])
        cnt = (ctypes.c_int * n)(*counts)
        if mask_ptrs is None:
            self._check("sift_multi_step",
                        self._L.sift_multi_step(self.h, ptrs, cnt, rows, cols, row_stride, img_stride))
            return
        if len(mask_ptrs) != n:
            raise ValueError("mask_ptrs needs one entry per device")
        mptrs = (ctypes.c_void_p * n)(*[ctypes.c_void_p(p or None) for p in mask_ptrs])
        self._check("sift_multi_step_masked",
                    self._L.sift_multi_step_masked(self.h, ptrs, mptrs, cnt, rows, cols, row_stride, img_stride,
                                                   mask_row_stride, mask_img_stride))

    def flush(self):
        self._check("sift_multi_flush", self._L.sift_multi_flush(self.h))

    def gathered(self, offsets_cap: int):
        """(device pointer to the records, to the descriptors or None, global
        offsets as numpy, step index) of the last gathered step."""
        k, d = ctypes.c_void_p(), ctypes.c_void_p()
        offs = np.zeros(offsets_cap, np.int32)
        bt, st = ctypes.c_int(0), ctypes.c_longlong(0)
        self._check("sift_multi_gathered",
                    self._L.sift_multi_gathered(self.h, ctypes.byref(k), ctypes.byref(d),
                                                offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), offsets_cap,
                                                ctypes.byref(bt), ctypes.byref(st)))
        return k.value, d.value, offs[:bt.value + 1].copy(), st.value

    def copy_gathered(self):
        """Host copies (keypoints, descriptors or None) of the last gathered step."""
        n = ctypes.c_int(0)
        rc = self._L.sift_multi_copy_gathered(self.h, None, None, 0, ctypes.byref(n))
        if rc not in (SIFT_OK, SIFT_E_CAPACITY):
            self._check("sift_multi_copy_gathered", rc)
        kps = np.zeros(n.value, KEYPOINT_DTYPE)
        desc = np.zeros((n.value, DESC_LEN), np.float32) if self.gather_desc else None
        if n.value:
            self._check("sift_multi_copy_gathered",
                        self._L.sift_multi_copy_gathered(self.h, kps.ctypes.data,
                                                         _fp(desc) if desc is not None else None, n.value,
                                                         ctypes.byref(n)))
        return kps, desc

    def stats(self):
        v = [ctypes.c_longlong(0) for _ in range(3)]
        self._check("sift_multi_stats", self._L.sift_multi_stats(self.h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("steps", "records", "transfers"), (x.value for x in v)))


def rccl_version() -> int:
    return lib().sift_multi_rccl_version()


# ---- module-level API with the reference's names (one shared context) -------
_default = None


def _ctx(rows, cols):
    global _default
    if _default is None or rows > _default.max_rows or cols > _default.max_cols:
        mr = max(rows, _default.max_rows if _default else 0)
        mc = max(cols, _default.max_cols if _default else 0)
        if _default is not None:
            _default.close()
        _default = Context(mr, mc, 1, int(os.environ.get("SIFT_HIP_DEVICE", "0")))
    return _default


def _ctx_for(image, upsample):
    r, c = np.shape(image)
    return _ctx(2 * r, 2 * c) if upsample else _ctx(r, c)  # the doubled image must fit the context


def SIFT_NCL(image, mask=None, keypoints=None):
    """mask: detectAndCompute's mask (uint8 or bool, the image's shape; zero = no keypoint here).
    keypoints: useProvidedKeypoints -- describe these and detect nothing; the mask is ignored."""
    if keypoints is not None:
        return _ctx(*image.shape).SIFT_NCL(image, keypoints=keypoints)
    mask = _detection_mask(mask, np.shape(image))
    return _ctx(*image.shape).SIFT_NCL(image, mask=mask)


def SIFT_NCL_upsampled(image, mask=None, keypoints=None):
    """SIFT_NCL with SIFT::create()'s firstOctave = -1: the image is doubled on the device first
    and the keypoints come back in its own frame, octave bytes from 255 (octave -1) up."""
    if keypoints is None:
        mask = _detection_mask(mask, np.shape(image))
    return _ctx_for(image, True).SIFT_NCL_upsampled(image, mask=mask, keypoints=keypoints)


def compute(image, keypoints, upsample=False):
    """Feature2D::compute(image, keypoints): the [n, 128] descriptors at the given keypoints
    (upsample: in the doubled image's pyramid, octave -1 valid)."""
    return _ctx_for(image, upsample).compute(image, keypoints, upsample=upsample)


def Gaussian_Blur(src, sigma):
    return _ctx(*src.shape).Gaussian_Blur(src, sigma)


def Gaussian_Blur_1D(src, sigma):
    return _ctx(*src.shape).Gaussian_Blur_1D(src, sigma)


def buildGaussianPyramid(image, nOctaves=5):
    return _ctx(*image.shape).buildGaussianPyramid(image, nOctaves)


def buildDoGPyramid(gpyr, nOctaves=5):
    return _ctx(*gpyr[0].shape).buildDoGPyramid(gpyr, nOctaves)


def findScaleSpaceExtrema(gpyr, dogpyr, nOctaves=5):
    return _ctx(*gpyr[0].shape).findScaleSpaceExtrema(gpyr, dogpyr, nOctaves)


def calDescriptor(gpyr, keypoints, firstOctave=0):
    return _ctx(*gpyr[0].shape).calDescriptor(gpyr, keypoints, firstOctave)


# ---- image front end -------------------------------------
def imread(filename) -> np.ndarray:
    """cv::imread(filename) layout: H x W x 3 uint8 BGR (decoded with PIL)."""
    from PIL import Image
    rgb = np.asarray(Image.open(filename).convert("RGB"), np.uint8)
    return np.ascontiguousarray(rgb[..., ::-1])


def readImage(filename_or_bgr, resized: bool):
    """src/main.cpp:79-87 -> (img, gray): gray is the CV_32F plane SIFT_NCL
    takes (960 x 960 when resized), produced on the GPU (frontend.hip); img is
    the decoded BGR image (the reference keeps the resized copy, which only its
    drawMatches uses -- not produced here)."""
    bgr = imread(filename_or_bgr) if isinstance(filename_or_bgr, (str, os.PathLike)) else \
        np.ascontiguousarray(filename_or_bgr, np.uint8)
    rows, cols = (960, 960) if resized else bgr.shape[:2]
    gray = _ctx(rows, cols).bgr8_to_gray(bgr, rows, cols)
    return bgr, gray


# ---- matcher: the reference application's consumer ------
class DMatch:
    """cv::DMatch fields (queryIdx, trainIdx, imgIdx, distance)."""
    __slots__ = ("queryIdx", "trainIdx", "imgIdx", "distance")

    def __init__(self, queryIdx, trainIdx, imgIdx, distance):
        self.queryIdx, self.trainIdx, self.imgIdx, self.distance = queryIdx, trainIdx, imgIdx, distance

    def __repr__(self):
        return f"DMatch({self.queryIdx}, {self.trainIdx}, {self.imgIdx}, {self.distance!r})"


NORM_L1 = 2  # cv::NORM_L1
NORM_L2SQR = 5  # cv::NORM_L2SQR


class BFMatcher:
    """`cv::BFMatcher(NORM_L1)` as the reference uses it (src/main.cpp:25-27):
    knnMatch(queryDescriptors, trainDescriptors, k) -> per query a list of up to
    k DMatch, nearest first.  k in (1, 2), no mask argument / crossCheck (the
    reference uses none); the mask that matters in practice, a search window
    around each keypoint's predicted position, is the module function
    window_match(query_desc, query_kpts, train_desc, train_kpts, radius, H).
    NORM_L1: float descriptors take the float matcher; two uint8
    arrays take the byte matcher (integer distances).  NORM_L2SQR: two uint8
    arrays only, DMatch.distance is the squared distance (for a ratio test use
    ratio_test(matches, ratio ** 2)).  NORM_L2 (the square root) is not
    implemented here: Euclidean matching of float descriptors is the module
    function l2_match(query, train, k, squared).  crossCheck=True raises: the mutual-nearest-neighbour filter is
    the module function cross_check_match(query, train, normType)."""

    def __init__(self, normType: int = NORM_L1, crossCheck: bool = False, ctx: Context | None = None):
        if normType not in (NORM_L1, NORM_L2SQR) or crossCheck:
            raise ValueError("only BFMatcher(NORM_L1) and BFMatcher(NORM_L2SQR) without crossCheck are implemented")
        self._norm = normType
        self._ctx = ctx

    def knnMatch(self, queryDescriptors, trainDescriptors, k: int = 2):
        both_u8 = np.asarray(queryDescriptors).dtype == np.uint8 and np.asarray(trainDescriptors).dtype == np.uint8
        if self._norm == NORM_L2SQR and not both_u8:
            raise ValueError("BFMatcher(NORM_L2SQR) takes two uint8 descriptor arrays")
        ctx = self._ctx or _ctx(1, 1)
        if self._norm == NORM_L2SQR:
            idx, dist = ctx.knnMatchL2SqrU8(queryDescriptors, trainDescriptors, k)
        elif both_u8:
            idx, dist = ctx.knnMatchU8(queryDescriptors, trainDescriptors, k)
        else:
            idx, dist = ctx.knnMatch(queryDescriptors, trainDescriptors, k)
        return [[DMatch(i, int(idx[i, j]), 0, float(dist[i, j])) for j in range(k) if idx[i, j] >= 0]
                for i in range(len(idx))]


def cross_check_match(query, train, normType: int = NORM_L1, ctx: Context | None = None):
    """`cv::BFMatcher(normType, crossCheck=True).match(query, train)` for one pair
    of descriptor sets: the list of DMatch (q, t) where t is q's nearest train row
    and q is t's nearest query row, in query order; the lower index wins at equal
    distance in both directions.  The matcher is picked from the dtypes as
    BFMatcher.knnMatch picks it (NORM_L2SQR: two uint8 arrays, squared distances;
    for float descriptors under L2 see l2_match and Context.knnMatchL2SqrF32Segmented).
    Two matcher passes and the cross-check stage (Context.crossCheckMatches)."""
    both_u8 = np.asarray(query).dtype == np.uint8 and np.asarray(train).dtype == np.uint8
    if normType not in (NORM_L1, NORM_L2SQR):
        raise ValueError("only NORM_L1 and NORM_L2SQR are implemented")
    if normType == NORM_L2SQR and not both_u8:
        raise ValueError("NORM_L2SQR takes two uint8 descriptor arrays")
    ctx = ctx or _ctx(1, 1)
    knn = ctx.knnMatchL2SqrU8Segmented if normType == NORM_L2SQR else \
        ctx.knnMatchU8Segmented if both_u8 else ctx.knnMatchSegmented
    q, t = np.asarray(query).reshape(-1, DESC_LEN), np.asarray(train).reshape(-1, DESC_LEN)
    qo, to = [0, len(q)], [0, len(t)]
    idx, dist = knn(q, qo, t, to, 1)
    ridx, _ = knn(t, to, q, qo, 1)
    m, _, _, _ = ctx.crossCheckMatches(idx, ridx, qo, to, dist)
    return [DMatch(int(r["query"]), int(r["train"]), 0, float(r["distance"])) for r in m]


def window_match(query_desc, query_kpts, train_desc, train_kpts, radius, H=None, normType: int = NORM_L1,
                 k: int = 2, image_size=None, ctx: Context | None = None):
    """`BFMatcher(normType).knnMatch(query, train, k, mask)` for one pair of
    descriptor sets, with the mask of guided matching: train row t is a candidate
    for query row q only if |tx - px| <= radius and |ty - py| <= radius (float32),
    (px, py) being q's keypoint position, or H (3 x 3, query -> train) applied to
    it.  Per query a list of up to k DMatch, nearest first.  The matcher is picked
    from the dtypes as BFMatcher.knnMatch picks it.  image_size = (rows, cols) of
    the train image only shapes the search grid (default: the extent of the train
    keypoints); no result depends on it.  Float descriptors under L2 have no
    windowed form; l2_match is their dense matcher."""
    both_u8 = np.asarray(query_desc).dtype == np.uint8 and np.asarray(train_desc).dtype == np.uint8
    if normType not in (NORM_L1, NORM_L2SQR):
        raise ValueError("only NORM_L1 and NORM_L2SQR are implemented")
    if normType == NORM_L2SQR and not both_u8:
        raise ValueError("NORM_L2SQR takes two uint8 descriptor arrays")
    metric = SIFT_METRIC_L2SQR_U8 if normType == NORM_L2SQR else SIFT_METRIC_L1_U8 if both_u8 else SIFT_METRIC_L1_F32
    q = np.asarray(query_desc).reshape(-1, DESC_LEN)
    t = np.asarray(train_desc).reshape(-1, DESC_LEN)
    tk = np.ascontiguousarray(train_kpts, KEYPOINT_DTYPE)
    if image_size is None:
        ext = [tk[f][np.isfinite(tk[f])] for f in ("y", "x")]
        image_size = tuple(int(min(max(float(e.max()) + 1, 1), 1 << 30)) if len(e) else 1 for e in ext)
    ctx = ctx or _ctx(1, 1)
    idx, dist = ctx.knnMatchWindowSegmented(metric, q, query_kpts, [0, len(q)], t, tk, None, radius,
                                            None if H is None else np.asarray(H, np.float64).reshape(1, 9), None,
                                            image_size, k)
    return [[DMatch(i, int(idx[i, j]), 0, float(dist[i, j])) for j in range(k) if idx[i, j] >= 0]
            for i in range(len(idx))]


def epipolar_match(query_desc, query_kpts, train_desc, train_kpts, F, band: float = 3.0,
                   radius: float = float("inf"), normType: int = NORM_L1, k: int = 2, image_size=None,
                   ctx: Context | None = None):
    """Guided matching along epipolar lines for one pair of descriptor sets:
    `BFMatcher(normType).knnMatch(query, train, k, mask)` with the mask of F (3 x 3,
    [train; 1]^T F [query; 1] = 0, as findFundamentalMat returns it).  Train row t
    is a candidate for query row q only if both points lie within `band` pixels of
    the other's epipolar line (find_fundamental's float32 inlier test at that
    threshold) and, with a finite `radius`, |tx - qx| <= radius and |ty - qy| <=
    radius (the disparity bound).  Per query a list of up to k DMatch, nearest
    first.  The matcher is picked from the dtypes as BFMatcher.knnMatch picks it;
    image_size = (rows, cols) of the train image only shapes the search grid.
    F None: the window alone (window_match without a prior)."""
    both_u8 = np.asarray(query_desc).dtype == np.uint8 and np.asarray(train_desc).dtype == np.uint8
    if normType not in (NORM_L1, NORM_L2SQR):
        raise ValueError("only NORM_L1 and NORM_L2SQR are implemented")
    if normType == NORM_L2SQR and not both_u8:
        raise ValueError("NORM_L2SQR takes two uint8 descriptor arrays")
    metric = SIFT_METRIC_L2SQR_U8 if normType == NORM_L2SQR else SIFT_METRIC_L1_U8 if both_u8 else SIFT_METRIC_L1_F32
    q = np.asarray(query_desc).reshape(-1, DESC_LEN)
    t = np.asarray(train_desc).reshape(-1, DESC_LEN)
    tk = np.ascontiguousarray(train_kpts, KEYPOINT_DTYPE)
    if image_size is None:
        ext = [tk[f][np.isfinite(tk[f])] for f in ("y", "x")]
        image_size = tuple(int(min(max(float(e.max()) + 1, 1), 1 << 30)) if len(e) else 1 for e in ext)
    ctx = ctx or _ctx(1, 1)
    idx, dist = ctx.knnMatchEpipolarSegmented(metric, q, query_kpts, [0, len(q)], t, tk, None,
                                              None if F is None else np.asarray(F, np.float64).reshape(1, 9), None,
                                              band, radius, image_size, k)
    return [[DMatch(i, int(idx[i, j]), 0, float(dist[i, j])) for j in range(k) if idx[i, j] >= 0]
            for i in range(len(idx))]


def l2_match(query, train, k: int = 2, squared: bool = False, ctx: Context | None = None):
    """`cv::BFMatcher(NORM_L2).knnMatch(query, train, k)` on float descriptors
    (squared=True: NORM_L2SQR): per query a list of up to k DMatch, nearest first,
    the lower train index first at equal distance.  The device forms the squared
    distance by the fixed rule of sift_hip.h (Context.knnMatchL2SqrF32);
    squared=False takes np.sqrt of those float32 values on the host, which is
    correctly rounded.  A ratio test on squared distances is
    ratio_test(matches, ratio ** 2)."""
    ctx = ctx or _ctx(1, 1)
    idx, dist = ctx.knnMatchL2SqrF32(query, train, k)
    if not squared:
        dist = np.sqrt(dist)
    return [[DMatch(i, int(idx[i, j]), 0, float(dist[i, j])) for j in range(k) if idx[i, j] >= 0]
            for i in range(len(idx))]


def ratio_test(matches, ratio: float = 0.86):
    """src/main.cpp:28-40: keep m1 where m1.distance <= ratio * m2.distance
    (a query with fewer than two matches is skipped)."""
    return [m[0] for m in matches if len(m) >= 2 and m[0].distance <= ratio * m[1].distance]


# ---- homography: src/main.cpp:44-62 ------------------------
RANSAC = 8  # cv::RANSAC


def findHomography(srcPoints, dstPoints, method: int = RANSAC, ransacReprojThreshold: float = 3.0,
                   mask=None, maxIters: int = 2000, confidence: float = 0.995):
    """cv::findHomography(obj, scene, RANSAC) -> (H 3x3 float64 or None, inlier mask).
    Host code in the library (homography.hip); None where OpenCV returns an empty Mat."""
    if method != RANSAC:
        raise ValueError("only RANSAC is implemented (the reference uses RANSAC)")
    src = np.ascontiguousarray(srcPoints, np.float32).reshape(-1, 2)
    dst = np.ascontiguousarray(dstPoints, np.float32).reshape(-1, 2)
    if len(src) != len(dst):
        raise ValueError("point counts differ")
    H = np.zeros(9, np.float64)
    m = np.zeros(max(len(src), 1), np.uint8)
    rc = lib().sift_find_homography(_fp(src), _fp(dst), len(src), float(ransacReprojThreshold), int(maxIters),
                                    float(confidence), H.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                    m.ctypes.data)
    if rc != SIFT_OK:
        return None, np.zeros(len(src), np.uint8)
    return H.reshape(3, 3), m[:len(src)]


def perspectiveTransform(points, H):
    """cv::perspectiveTransform for Point2f with a 3x3 double H."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
    Hd = np.ascontiguousarray(H, np.float64).reshape(9)
    out = np.empty_like(pts)
    rc = lib().sift_perspective_transform(Hd.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _fp(pts), len(pts),
                                          _fp(out))
    if rc != SIFT_OK:
        raise SiftError("sift_perspective_transform", rc, "bad argument")
    return out


def _estimate_affine(model, from_, to, ransacReprojThreshold, maxIters, confidence):
    src = np.ascontiguousarray(from_, np.float32).reshape(-1, 2)
    dst = np.ascontiguousarray(to, np.float32).reshape(-1, 2)
    if len(src) != len(dst):
        raise ValueError("point counts differ")
    A = np.zeros(6, np.float64)
    m = np.zeros(max(len(src), 1), np.uint8)
    rc = lib().sift_estimate_affine(_fp(src), _fp(dst), len(src), model, float(ransacReprojThreshold), int(maxIters),
                                    float(confidence), A.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                    m.ctypes.data)
    if rc != SIFT_OK:
        return None, np.zeros(len(src), np.uint8)
    return A.reshape(2, 3), m[:len(src)]


def estimateAffine2D(from_, to, ransacReprojThreshold: float = 3.0, maxIters: int = 2000, confidence: float = 0.99):
    """cv::estimateAffine2D(from, to, RANSAC) -> (A 2x3 float64 or None, inlier mask).  Host code in
    the library (affine.hip); the final model is the least-squares fit to the inliers, the minimum
    OpenCV's refineIters look for (include/sift_hip.h), so there is no refineIters argument."""
    return _estimate_affine(SIFT_MODEL_AFFINE, from_, to, ransacReprojThreshold, maxIters, confidence)


def estimateAffinePartial2D(from_, to, ransacReprojThreshold: float = 3.0, maxIters: int = 2000,
                            confidence: float = 0.99):
    """cv::estimateAffinePartial2D(from, to, RANSAC): rotation, uniform scale and translation,
    A = (a -b tx; b a ty) -> (A 2x3 float64 or None, inlier mask)."""
    return _estimate_affine(SIFT_MODEL_SIMILARITY, from_, to, ransacReprojThreshold, maxIters, confidence)


def findFundamentalMat(src, dst, thr: float = 3.0, max_iters: int = 1000, confidence: float = 0.99):
    """cv::findFundamentalMat(points1, points2, FM_RANSAC, thr, confidence, max_iters) -> (F 3x3 float64
    or None, inlier mask), [dst;1]^T F [src;1] = 0.  Host code in the library (fundamental.hip): the
    normalised 8-point solve inside RANSAC and again over the inliers (include/sift_hip.h has the rule)."""
    s = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
    d = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
    if len(s) != len(d):
        raise ValueError("point counts differ")
    F = np.zeros(9, np.float64)
    m = np.zeros(max(len(s), 1), np.uint8)
    rc = lib().sift_find_fundamental(_fp(s), _fp(d), len(s), float(thr), int(max_iters), float(confidence),
                                     F.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), m.ctypes.data)
    if rc != SIFT_OK:
        return None, np.zeros(len(s), np.uint8)
    return F.reshape(3, 3), m[:len(s)]


def recoverPose(F, K_src, K_dst, src, dst, mask=None, distanceThresh: float = 50.0):
    """cv::recoverPose(E, points1, points2, K, R, t, distanceThresh, mask, triangulatedPoints) for
    E = K_dst^T F K_src -> (R 3x3, t 3, E 3x3, mask uint8[n], xyz float64[n, 3], n_good), with
    X_dst = R X_src + t and xyz in the src camera's frame; R = t = E = None when there is no pose.
    Host code in the library (pose.hip; include/sift_hip.h has the rule)."""
    s = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
    d = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
    if len(s) != len(d):
        raise ValueError("point counts differ")
    n = len(s)
    Fa = np.ascontiguousarray(F, np.float64).reshape(9)
    Ks, Kd = np.ascontiguousarray(K_src, np.float64).reshape(9), np.ascontiguousarray(K_dst, np.float64).reshape(9)
    mi = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(-1)
    if mi is not None and len(mi) != n:
        raise ValueError("mask must have one byte per pair")
    pose, E = np.zeros(12, np.float64), np.zeros(9, np.float64)
    mout, xyz = np.zeros(max(n, 1), np.uint8), np.zeros((max(n, 1), 3), np.float64)
    ng = ctypes.c_int(0)
    pdbl = ctypes.POINTER(ctypes.c_double)
    rc = lib().sift_recover_pose(Fa.ctypes.data_as(pdbl), Ks.ctypes.data_as(pdbl), Kd.ctypes.data_as(pdbl), _fp(s),
                                 _fp(d), n, None if mi is None else mi.ctypes.data, float(distanceThresh),
                                 pose.ctypes.data_as(pdbl), E.ctypes.data_as(pdbl), mout.ctypes.data, xyz.ctypes.data,
                                 ctypes.byref(ng))
    if rc != SIFT_OK:
        return None, None, None, np.zeros(n, np.uint8), np.zeros((n, 3), np.float64), 0
    P = pose.reshape(3, 4)
    return P[:, :3].copy(), P[:, 3].copy(), E.reshape(3, 3), mout[:n], xyz[:n], ng.value


def triangulatePoints(P_src, P_dst, src, dst):
    """cv::triangulatePoints(projMatr1, projMatr2, projPoints1, projPoints2) -> float64 [n, 4],
    homogeneous and not divided (OpenCV returns the transpose, 4 x n).  Host code in the library."""
    s = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
    d = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
    if len(s) != len(d):
        raise ValueError("point counts differ")
    Ps, Pd = np.ascontiguousarray(P_src, np.float64).reshape(12), np.ascontiguousarray(P_dst, np.float64).reshape(12)
    out = np.zeros((max(len(s), 1), 4), np.float64)
    pdbl = ctypes.POINTER(ctypes.c_double)
    rc = lib().sift_triangulate_points(Ps.ctypes.data_as(pdbl), Pd.ctypes.data_as(pdbl), _fp(s), _fp(d), len(s),
                                       out.ctypes.data_as(pdbl))
    if rc != SIFT_OK:
        raise SiftError("sift_triangulate_points", rc, "bad argument")
    return out[:len(s)]


def solveP3P(objectPoints, imagePoints, K):
    """cv::solveP3P for three 3-D points and their pixels -> a list of up to four (R 3x3, t 3),
    X_cam = R X + t, in the library's fixed order.  Host code in the library (pnp.hip;
    include/sift_hip.h has the rule)."""
    X = np.ascontiguousarray(objectPoints, np.float64).reshape(-1, 3)
    p = np.ascontiguousarray(imagePoints, np.float32).reshape(-1, 2)
    if len(X) != 3 or len(p) != 3:
        raise ValueError("solveP3P takes exactly three rows")
    Ka = np.ascontiguousarray(K, np.float64).reshape(9)
    poses = np.zeros((4, 12), np.float64)
    ns = ctypes.c_int(0)
    pdbl = ctypes.POINTER(ctypes.c_double)
    rc = lib().sift_solve_p3p(X.ctypes.data_as(pdbl), _fp(p), Ka.ctypes.data_as(pdbl), poses.ctypes.data_as(pdbl),
                              ctypes.byref(ns))
    if rc != SIFT_OK:
        raise SiftError("sift_solve_p3p", rc, "bad argument")
    return [(poses[k].reshape(3, 4)[:, :3].copy(), poses[k].reshape(3, 4)[:, 3].copy()) for k in range(ns.value)]


def solvePnPRansac(objectPoints, imagePoints, K, reprojectionError: float = 8.0, iterationsCount: int = 100,
                   confidence: float = 0.99, row_mask=None):
    """cv::solvePnPRansac(objectPoints, imagePoints, K, noArray(), ..., SOLVEPNP_P3P) on undistorted
    pixels -> (R 3x3, t 3, mask uint8[n], n_inliers), X_cam = R X + t; R = t = None when there is no
    model.  row_mask [n] (or None) takes rows out, as recoverPose's mask does.  Host code in the library."""
    X = np.ascontiguousarray(objectPoints, np.float64).reshape(-1, 3)
    p = np.ascontiguousarray(imagePoints, np.float32).reshape(-1, 2)
    if len(X) != len(p):
        raise ValueError("point counts differ")
    n = len(X)
    Ka = np.ascontiguousarray(K, np.float64).reshape(9)
    mi = None if row_mask is None else np.ascontiguousarray(row_mask, np.uint8).reshape(-1)
    if mi is not None and len(mi) != n:
        raise ValueError("row_mask must have one byte per row")
    pose = np.zeros(12, np.float64)
    mout = np.zeros(max(n, 1), np.uint8)
    Xs = X if n else np.zeros((1, 3), np.float64)
    ps = p if n else np.zeros((1, 2), np.float32)
    ni = ctypes.c_int(0)
    pdbl = ctypes.POINTER(ctypes.c_double)
    rc = lib().sift_solve_pnp(Xs.ctypes.data_as(pdbl), _fp(ps), n, None if mi is None else mi.ctypes.data,
                              Ka.ctypes.data_as(pdbl), float(reprojectionError), int(iterationsCount),
                              float(confidence), pose.ctypes.data_as(pdbl), mout.ctypes.data, ctypes.byref(ni))
    if rc != SIFT_OK:
        return None, None, np.zeros(n, np.uint8), 0
    P = pose.reshape(3, 4)
    return P[:, :3].copy(), P[:, 3].copy(), mout[:n], ni.value


def _join_tables(a, a_xyz, b, b_xy, a_mask, b_mask):
    """The two tables of a join as contiguous arrays, their row counts checked."""
    A, B = np.ascontiguousarray(a, MATCH_DTYPE).reshape(-1), np.ascontiguousarray(b, MATCH_DTYPE).reshape(-1)
    X = np.ascontiguousarray(a_xyz, np.float64).reshape(-1, 3)
    P = np.ascontiguousarray(b_xy, np.float32).reshape(-1, 2)
    am = None if a_mask is None else np.ascontiguousarray(a_mask, np.uint8).reshape(-1)
    bm = None if b_mask is None else np.ascontiguousarray(b_mask, np.uint8).reshape(-1)
    if len(X) != len(A) or len(P) != len(B):
        raise ValueError("a_xyz needs one row per record of a, b_xy one per record of b")
    if (am is not None and len(am) != len(A)) or (bm is not None and len(bm) != len(B)):
        raise ValueError("a mask must have one byte per record")
    return A, B, X, P, am, bm


def joinMatches(a, a_xyz, b, b_xy, n_keys: int, a_key_side: int, b_key_side: int, a_mask=None, b_mask=None):
    """The 2-D / 3-D rows of a new view from two match tables that share a view: table a (MATCH_DTYPE)
    carries a_xyz [len(a), 3] by record (recoverPose's points, a_mask its mask), table b the new view's
    pixel b_xy [len(b), 2] by record; a_key_side / b_key_side (JOIN_QUERY, JOIN_TRAIN) say which index of
    a record names the shared view's keypoint, n_keys is that view's keypoint count.  Per key the unmasked
    record of a with the smallest distance (then the lowest row) wins; every unmasked record of b whose
    key has a winner joins, in b's order -> (xyz [n, 3], xy [n, 2], a_row [n], b_row [n], b_joined
    uint8[len(b)]).  Host code in the library (include/sift_hip.h has the rule)."""
    A, B, X, P, am, bm = _join_tables(a, a_xyz, b, b_xy, a_mask, b_mask)
    n = max(len(B), 1)
    xyz, xy = np.zeros((n, 3), np.float64), np.zeros((n, 2), np.float32)
    ar, br, bj = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8)
    d = lambda v: None if v is None else v.ctypes.data  # noqa: E731
    m = lib().sift_join_matches(d(A), len(A), int(a_key_side), d(am), d(X), d(B), len(B), int(b_key_side), d(bm), d(P),
                                int(n_keys), d(xyz), d(xy), d(ar), d(br), d(bj))
    if m < 0:
        raise SiftError("sift_join_matches", m, "bad argument")
    return xyz[:m], xy[:m], ar[:m], br[:m], bj[:len(B)]


WARP_INVERSE_MAP = 16  # cv::WARP_INVERSE_MAP


def warpPerspective(src, M, dsize, flags: int = 0):
    """cv::warpPerspective(src, M, dsize, flags) with INTER_LINEAR (flags 0 or 1), BORDER_CONSTANT
    and a zero border value; flags may add WARP_INVERSE_MAP.  src: float32 H x W, or uint8 H x W /
    H x W x 3; dsize = (width, height).  On the GPU (warp.hip) by the rule in include/sift_hip.h."""
    if flags & ~(WARP_INVERSE_MAP | 1):
        raise ValueError("only INTER_LINEAR, optionally with WARP_INVERSE_MAP, is implemented")
    return _ctx(1, 1).warpPerspective(src, M, dsize, inverse=bool(flags & WARP_INVERSE_MAP))


def undistort(image, K, dist, newK=None):
    """cv::undistort(image, K, dist, newK) with INTER_LINEAR and a zero border, for the rational
    model's (k1 k2 p1 p2 k3 k4 k5 k6).  image: float32 H x W, or uint8 H x W / H x W x 3.  On the
    GPU (undistort.hip) by the rule in include/sift_hip.h."""
    return _ctx(1, 1).undistort(image, K, dist, newK)


def undistortPoints(xy, K, dist, P=None, iters: int = 5):
    """cv::undistortPoints(xy, K, dist, noArray(), P) with a fixed iteration count -> float32 [n, 2]:
    normalised coordinates with P None, ideal pixels with P = K.  xy may be a KEYPOINT_DTYPE array:
    a copy comes back with only x and y changed.  Host code in the library (undistort.hip;
    include/sift_hip.h has the rule).  A camera with no rule raises SiftError."""
    a = np.asarray(xy)
    if a.dtype == KEYPOINT_DTYPE:
        out, stride = np.ascontiguousarray(a).copy(), KEYPOINT_DTYPE.itemsize
    else:
        out, stride = np.ascontiguousarray(a, np.float32).reshape(-1, 2).copy(), 8
    if not 0 <= int(iters) <= 100:
        raise ValueError("iters must be 0 .. 100")
    Kd, dd, Pd = _camera(K, dist, P)
    pdbl = ctypes.POINTER(ctypes.c_double)
    rc = lib().sift_undistort_points(Kd.ctypes.data_as(pdbl), dd.ctypes.data_as(pdbl),
                                     None if Pd is None else Pd.ctypes.data_as(pdbl), int(iters),
                                     out.ctypes.data if len(out) else None, out.ctypes.data if len(out) else None,
                                     stride, len(out))
    if rc != SIFT_OK:
        raise SiftError("sift_undistort_points", rc, "the camera has no rule (singular or non-finite)")
    return out
