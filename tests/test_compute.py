"""CPU tests of the provided-keypoint boundary (sift_compute_batch, sift_compute):
declared, exported, wrapped, and the argument checks that need no device.  The
numpy restatement the GPU tests classify rows with is checked against the
oracle's own rounding."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import compute_inputs as CI
from conftest import PKG, ROOT

HEADER = os.path.join(ROOT, "include", "sift_hip.h")


def test_entry_points_are_declared_exported_and_wrapped(siftgpu):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    L = siftgpu.lib()
    for name, nargs in (("sift_compute_batch", 12), ("sift_compute", 9)):
        m = re.search(r"\bint " + name + r"\s*\(([^;]*)\);", text)
        assert m, f"{name} is not declared in sift_hip.h"
        assert len(m.group(1).split(",")) == nargs
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and len(f.argtypes) == nargs
    for meth in ("compute_batch", "compute"):
        assert callable(getattr(siftgpu.Context, meth))
    assert callable(siftgpu.compute)
    sig = inspect.signature(siftgpu.Context.compute_batch)
    assert list(sig.parameters)[1:] == ["imgs_ptr", "batch", "rows", "cols", "row_stride", "img_stride", "kpts_ptr",
                                        "kp_offsets_ptr", "kp_cap", "desc_ptr", "max_layer"]
    assert sig.parameters["max_layer"].default == 4
    assert inspect.signature(siftgpu.Context.compute).parameters["max_layer"].default == 4


def test_null_context_is_rejected_first(siftgpu):
    """Before 'nothing to do' (batch 0, kp_cap 0, n 0) and before the max_layer range."""
    L = siftgpu.lib()
    for batch, cap, max_layer in ((0, 0, 4), (1, 0, 4), (0, 16, 4), (1, 16, -1), (1, 16, 5), (1, 16, 3)):
        assert L.sift_compute_batch(None, None, batch, 64, 64, 64, 4096, None, None, cap, max_layer,
                                    None) == siftgpu.SIFT_E_INVALID
    for n, max_layer in ((0, 4), (3, 4), (3, -1), (3, 5)):
        assert L.sift_compute(None, None, 64, 64, 0, None, n, max_layer, None) == siftgpu.SIFT_E_INVALID


def test_existing_signatures_accept_their_old_calls(siftgpu):
    for fn in (siftgpu.SIFT_NCL, siftgpu.Context.SIFT_NCL):
        p = inspect.signature(fn).parameters
        assert p["keypoints"].default is None and p["mask"].default is None
    # positional order of the arguments that existed before is unchanged
    assert list(inspect.signature(siftgpu.SIFT_NCL).parameters) == ["image", "mask", "keypoints"]
    assert list(inspect.signature(siftgpu.Context.SIFT_NCL).parameters) == ["self", "img", "row_stride_bytes", "mask",
                                                                           "keypoints"]
    assert list(inspect.signature(siftgpu.Context.detect_compute_batch).parameters)[1:11] == [
        "imgs_ptr", "batch", "rows", "cols", "row_stride", "img_stride", "kpts_ptr", "desc_ptr", "kp_cap", "offs_ptr"]
    # the mask is still validated when no keypoints are given, before any library call
    with pytest.raises(ValueError):
        siftgpu.SIFT_NCL(np.zeros((8, 8), np.float32), mask=np.zeros((4, 4), np.uint8))


def test_shim_exports_the_five_argument_overload(siftgpu):
    syms = subprocess.run(["nm", "-DC", os.path.join(PKG, "lib", "libsift_shim.so")], capture_output=True, text=True,
                          check=True).stdout
    over = [ln for ln in syms.splitlines() if " T SIFT_NCL(" in ln]
    assert len(over) == 3 and any(ln.rstrip().endswith(", bool)") for ln in over), over


def test_cli_compiles(tmp_path, siftgpu):
    exe = tmp_path / "compute_cli"
    lib = os.path.join(PKG, "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "compute_cli.cpp"), "-o", str(exe), "-L", lib, "-lsift_shim",
                    "-lsift_hip", f"-Wl,-rpath,{lib}"], check=True)
    assert exe.exists()


def test_stage_names(siftgpu):
    """The stages sift_compute_batch reports under SIFT_FLAG_PROFILE are in the library's table."""
    data = open(siftgpu.LIB_PATH, "rb").read()
    assert b"compute_prep\0" in data and b"gradient\0" in data


def test_input_helpers(oracle):
    """compute_inputs.window restates the kernel's float32 setup: its rounding is the
    oracle's cvRound, and the crafted rows land where their comments say."""
    for v in (0.5, 1.5, 2.5, 39.5, 40.5, 40.49999, -0.5):
        assert int(np.rint(np.float32(v))) == oracle.cv_round(float(np.float32(v)))
    for shape in CI.SHAPES:
        r = CI.crafted(shape)
        rad, px, py, rows, cols, clamped = CI.window(r, shape)
        assert list(rad[5:9]) == [40, 41, 40, 41]
        det = CI.takes_det(r, shape)
        assert list(det[5:9]) == [True, False, True, False]
        assert clamped[9] and clamped[11] and not det[9]
        assert det[17] and det[18] and not det[14] and not det[15] and not det[16]
        assert CI.valid(r).all() and not CI.valid(r, 3).all()
    for _, octave, layer, max_layer in CI.INVALID:
        assert not CI.valid(CI.invalid_row(octave, layer), max_layer).any()
    g = CI.dense_grid(CI.SHAPES[0], 4)
    det = CI.takes_det(g, CI.SHAPES[0])
    assert len(g) == 51 * 39 and det.sum() == 50 * 39 and not det[g["y"] == 202].any()   # the last row is the border
