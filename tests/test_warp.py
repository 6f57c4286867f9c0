"""CPU tests of the perspective warp (sift_warp_perspective[_segmented_device]):
the numpy restatement of tests/warp_inputs.py on hand-written cases, the rule's
header csrc/warp_math.hpp compiled on the host (tests/cpp/warp_rule.cpp)
against the restatement over the whole case table, bit for bit, and the
argument errors of the two entry points that need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import warp_inputs as W
from conftest import ROOT, assert_bits_equal
from test_abi import HEADER, declared_symbols

f32, f64 = np.float32, np.float64


# ---- the restatement on hand-written cases ------------------------------------------------
@pytest.mark.parametrize("kind", W.PIXELS)
def test_identity_is_a_copy(kind):
    src = W.pixels(kind, (9, 13), 1)
    assert_bits_equal(W.warp_ref(src, np.eye(3), (9, 13)), src, "identity")
    assert_bits_equal(W.warp_ref(src, np.eye(3), (9, 13), inverse=True), src, "identity, inverse map")
    # a larger destination: the source, then zeros
    big = W.warp_ref(src, np.eye(3), (11, 16))
    assert_bits_equal(big[:9, :13], src, "identity into a larger destination")
    assert not big[9:].any() and not big[:, 13:].any()


@pytest.mark.parametrize("kind", W.PIXELS)
@pytest.mark.parametrize("tx,ty", [(3, 2), (-4, 1), (2, -5), (-1, -1)])
def test_integer_translation_is_a_shifted_copy_with_zero_fill(kind, tx, ty):
    src = W.pixels(kind, (8, 10), 2)
    want = np.zeros_like(src)
    ys, xs = slice(max(ty, 0), min(8, 8 + ty)), slice(max(tx, 0), min(10, 10 + tx))
    want[ys, xs] = src[max(-ty, 0):max(-ty, 0) + ys.stop - ys.start, max(-tx, 0):max(-tx, 0) + xs.stop - xs.start]
    H = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], f64)
    assert_bits_equal(W.warp_ref(src, H, (8, 10)), want, f"shift ({tx}, {ty})")


@pytest.mark.parametrize("kind", W.PIXELS)
@pytest.mark.parametrize("name", ["rotation_30", "projective", "scale_2", "shift_x+1"])
def test_inverse_flag_with_the_rules_own_inverse_equals_the_default_call(kind, name):
    src = W.pixels(kind, (17, 31), 3)
    H = W.homographies(17, 31, 31, 17)[name][0]
    a = W.warp_ref(src, H, (31, 17))
    assert a.any()
    assert_bits_equal(W.warp_ref(src, W.inverse_rule(H), (31, 17), inverse=True), a, name)


def test_half_pixel_shift_of_a_ramp_gives_the_exact_midpoints():
    ramp = np.tile(np.arange(0, 24, 2, dtype=f32), (3, 1))   # 0, 2, .. 22
    out = W.warp_ref(ramp, np.array([[1, 0, 0.5], [0, 1, 0], [0, 0, 1]], f64), (3, 12), inverse=True)
    assert_bits_equal(out[:, :11], np.tile(np.arange(1, 23, 2, dtype=f32), (3, 1)), "midpoints")
    assert_bits_equal(out[:, 11], np.full(3, 11.0, f32), "the last column mixes with the zero border")
    ramp8 = ramp.astype(np.uint8)
    out8 = W.warp_ref(ramp8, np.array([[1, 0, 0.5], [0, 1, 0], [0, 0, 1]], f64), (3, 12), inverse=True)
    assert out8[0].tolist() == list(range(1, 23, 2)) + [11]


def test_u8_identity_is_exact_for_all_256_values():
    src = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert_bits_equal(W.warp_ref(src, np.eye(3), (16, 16)), src, "u8 identity")
    rgb = np.stack([src, src[::-1], src.T], axis=-1)
    assert_bits_equal(W.warp_ref(rgb, np.eye(3), (16, 16)), rgb, "u8 x 3 identity")


def test_ties_go_to_even_and_weights_are_exact():
    sx, ax, sy, ay, valid = W.source_coords(np.array([1, 0, 1 / 64, 0, 1, 3 / 64, 0, 0, 1], f64), 4, 4)
    assert valid.all() and (ax == 0).all() and (ay == 2).all()           # 32 x + 0.5 -> 32 x; 32 y + 1.5 -> 32 y + 2
    assert sx[0].tolist() == [0, 1, 2, 3] and sy[:, 0].tolist() == [0, 1, 2, 3]
    sx, ax, _, _, _ = W.source_coords(np.array([1, 0, -1 / 64, 0, 1, 0, 0, 0, 1], f64), 1, 3)
    assert (sx[0].tolist(), ax[0].tolist()) == ([0, 1, 2], [0, 0, 0])     # -0.5 -> -0, 31.5 -> 32
    sx, ax, _, _, _ = W.source_coords(np.array([1, 0, -3 / 64, 0, 1, 0, 0, 0, 1], f64), 1, 2)
    assert (sx[0].tolist(), ax[0].tolist()) == ([-1, 0], [30, 30])        # -1.5 -> -2: an arithmetic shift


def test_degenerate_homographies_of_the_table():
    hs = W.homographies(17, 31, 31, 17)
    for name in ("singular", "nan_entry", "nan_entry_inverse", "inf_entry", "overflowing_inverse"):
        H, inverse, _ = hs[name]
        M, ok = W.warp_matrix(H, inverse)
        assert not ok and not M.any(), name
    assert np.isfinite(hs["overflowing_inverse"][0]).all()
    # the horizon: one column with Wd == 0 takes S[0][0], and Wd changes sign across it
    src = W.pixels("f32", (17, 31), 4)
    M = hs["horizon"][0].reshape(9)
    out = W.warp_ref(src, M.reshape(3, 3), (31, 17), inverse=True)
    assert_bits_equal(out[:, 8], np.full(31, src[0, 0], f32), "the W = 0 column")
    x = np.arange(17.0)
    wd = M[6] * x + M[8]
    assert (wd < 0).any() and (wd > 0).any() and (wd == 0).sum() == 1
    # the clamp and the NaN coordinate
    sx, _, sy, _, valid = W.source_coords(hs["clamp_1e12"][0].reshape(9), 3, 3)
    assert sx[0].tolist() == [-(1 << 26), 0, (1 << 26) - 1] and valid.all()
    _, _, _, _, valid = W.source_coords(hs["zero_times_inf"][0].reshape(9), 3, 3)
    assert not valid[0].any() and not valid[:, 0].any() and valid[1:, 1:].all()


def test_the_case_table_covers_what_it_should():
    names = [c["name"] for c in W.CASES]
    assert len(names) == len(set(names))
    for kind in W.PIXELS:
        for h in W.homographies(17, 31, 31, 17):
            assert f"{kind}-17x31to31x17-{h}" in names
    for (s, o) in W.SHAPES:
        assert any(f"{s[0]}x{s[1]}to{o[0]}x{o[1]}" in n for n in names)
    f = np.concatenate([c["src"].reshape(-1) for c in W.CASES if c["kind"] == "f32"])
    with np.errstate(invalid="ignore"):
        assert (f < 0).any() and ((np.abs(f) < f32(2.0 ** -126)) & (f != 0)).any() and np.isnan(f).any()
    u = np.concatenate([c["src"].reshape(-1) for c in W.CASES if c["kind"] != "f32"])
    assert ((u[:-1] == 0) & (u[1:] == 255)).any() or ((u[:-1] == 255) & (u[1:] == 0)).any()
    # most cases draw something
    drawn = sum(bool(np.any(W.expected(c).view(np.uint8))) for c in W.CASES)
    assert drawn > len(W.CASES) * 0.6


# ---- the header on the host against the restatement ------------------------------------
def _build_rule(tmp_path, sanitize):
    src = os.path.join(ROOT, "tests", "cpp", "warp_rule.cpp")
    exe = tmp_path / ("warp_rule_san" if sanitize else "warp_rule")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", src, "-o", str(exe)]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    return exe if r.returncode == 0 else None, r.stderr


def _run_rule(exe, tmp_path):
    cases, results = tmp_path / "cases.bin", tmp_path / "results.bin"
    W.write_cases(cases, W.CASES)
    r = subprocess.run([str(exe), str(cases), str(results)], capture_output=True, text=True)
    assert r.returncode == 0 and f"warp rule ok: {len(W.CASES)} cases" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    return W.read_results(results, W.CASES)


def _compare(results):
    for c, (M, ok, img) in zip(W.CASES, results):
        wantM, want_ok = W.warp_matrix(c["H"], c["inverse"])
        assert ok == int(want_ok), c["name"]
        assert_bits_equal(M, wantM, f"{c['name']}: M")
        assert_bits_equal(W.canonical(img), W.canonical(W.expected(c)), c["name"])


def test_header_on_the_host_equals_the_restatement(tmp_path):
    """Fails to build before csrc/warp_math.hpp exists.  Built with the address and
    undefined-behaviour sanitizers (their runtimes linked statically into the program; nothing
    sanitised is loaded into Python) where the host compiler has them, without otherwise."""
    exe, _ = _build_rule(tmp_path, True)
    if exe is None:
        exe, err = _build_rule(tmp_path, False)
        assert exe is not None, err[-3000:]
    _compare(_run_rule(exe, tmp_path))


# ---- the entry points -----------------------------------------------------------------------
NEW = ["sift_warp_perspective_segmented_device", "sift_warp_perspective"]


def test_header_declares_the_entry_points_and_states_the_rule():
    assert set(NEW) <= set(declared_symbols())
    text = open(HEADER).read()
    for macro, value in (("SIFT_WARP_INVERSE_MAP", "0x1u"), ("SIFT_PIXEL_F32", "0"), ("SIFT_PIXEL_U8", "1")):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", text), macro
    assert re.search(r"int\s+sift_warp_perspective\(sift_ctx\*\s*\w*,\s*int\s+pixel,\s*int\s+channels,\s*const\s+void\*\s*src,"
                     r"\s*int\s+rows,\s*int\s+cols,\s*size_t\s+row_stride,\s*const\s+double\*\s*H,\s*unsigned\s+flags,"
                     r"\s*void\*\s*dst,\s*int\s+out_rows,\s*int\s+out_cols\);", text)
    for phrase in ("32.0 / Wd", "ties to even", "+ 512) >> 10", "by construction"):
        assert phrase in text, phrase


def _bind(L):
    vp, ip, sz, u = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_uint
    L.sift_warp_perspective_segmented_device.restype = ip
    L.sift_warp_perspective_segmented_device.argtypes = [vp, ip, ip, vp, ip, ip, sz, sz, vp, vp, ip, u, vp, ip, ip, sz, sz]
    L.sift_warp_perspective.restype = ip
    L.sift_warp_perspective.argtypes = [vp, ip, ip, vp, ip, ip, sz, vp, u, vp, ip, ip]
    return L


def test_library_exports_the_entry_points_and_rejects_a_null_context(siftgpu):
    L = _bind(ctypes.CDLL(siftgpu.LIB_PATH))
    assert all(hasattr(L, s) for s in NEW)
    src, dst, H = np.zeros((2, 2), f32), np.full((2, 2), 5.0, f32), np.eye(3)
    # a NULL context is SIFT_E_INVALID whatever else is passed (no device needed), and nothing is written
    assert L.sift_warp_perspective(None, 0, 1, src.ctypes.data, 2, 2, 0, H.ctypes.data, 0, dst.ctypes.data, 2, 2) \
        == siftgpu.SIFT_E_INVALID
    assert L.sift_warp_perspective(None, 7, 9, None, 0, 0, 0, None, 0, None, 0, 0) == siftgpu.SIFT_E_INVALID
    assert L.sift_warp_perspective_segmented_device(None, 0, 1, None, 2, 2, 0, 0, None, None, 1, 0, None, 2, 2, 0, 0) \
        == siftgpu.SIFT_E_INVALID
    assert L.sift_warp_perspective_segmented_device(None, 0, 1, None, 2, 2, 0, 0, None, None, 0, 0, None, 2, 2, 0, 0) \
        == siftgpu.SIFT_E_INVALID
    assert (dst == 5.0).all()


def test_python_interface(siftgpu):
    for name in ("warpPerspective", "warp_perspective_segmented_device"):
        assert callable(getattr(siftgpu.Context, name, None)), name
    assert callable(siftgpu.warpPerspective) and siftgpu.WARP_INVERSE_MAP == 16
    assert (siftgpu.SIFT_PIXEL_F32, siftgpu.SIFT_PIXEL_U8, siftgpu.SIFT_WARP_INVERSE_MAP) == (0, 1, 1)
    # argument errors raised before any library call (no device needed)
    with pytest.raises(ValueError):
        siftgpu.warpPerspective(np.zeros((2, 2), f32), np.eye(3), (2, 2), flags=2)   # INTER_CUBIC
