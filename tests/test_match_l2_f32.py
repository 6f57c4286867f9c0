"""The squared-L2 kNN matcher on float descriptors: what holds without a GPU.

The exports, the null-context checks, the Python names, the layout program, and
the oracle of match_l2_f32_inputs on its own: its float32 fma against libm's
fmaf, the dyadic identity against the integer reference, a census of rows whose
bits depend on the summation order, a census of the planted ties, and the
rule's error bound on real descriptors against float64."""
import ctypes
import ctypes.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal

import match_l2_f32_inputs as F
import match_l2_inputs as L2
import match_u8_inputs as U

NEW = ["sift_knn_match_l2sqr_f32_segmented_device", "sift_knn_match_l2sqr_f32_segmented", "sift_knn_match_l2sqr_f32"]
f32 = np.float32


def test_l2_f32_entry_points_declared_exported_and_wrapped(siftgpu):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sift_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert getattr(siftgpu.lib(), name).argtypes is not None, name
    assert re.search(r"#define\s+SIFT_METRIC_L2SQR_F32\s+3\b", text)
    assert b"match_l2sqr_f32_segmented\0" in open(siftgpu.LIB_PATH, "rb").read()     # the stage's name


def test_l2_f32_entry_points_reject_null_context(siftgpu):
    L = siftgpu.lib()
    f = np.zeros(128, np.float32)
    off = np.array([0, 1], np.int32)
    ix = np.zeros(2, np.int32)
    pf = f.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    pi = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))  # noqa: E731
    E = siftgpu.SIFT_E_INVALID
    assert L.sift_knn_match_l2sqr_f32_segmented_device(None, f.ctypes.data, off.ctypes.data, 1, 1, f.ctypes.data, None,
                                                       1, 2, ix.ctypes.data, f.ctypes.data) == E
    assert L.sift_knn_match_l2sqr_f32_segmented(None, pf, pi(off), 1, 1, pf, None, 1, 2, pi(ix), pf) == E
    assert L.sift_knn_match_l2sqr_f32(None, pf, 1, pf, 1, 2, pi(ix), pf) == E
    # and with nothing to do: the null context is still rejected first
    assert L.sift_knn_match_l2sqr_f32_segmented_device(None, None, None, 0, 0, None, None, 0, 2, None, None) == E
    assert L.sift_knn_match_l2sqr_f32_segmented(None, None, None, 0, 0, None, None, 0, 2, None, None) == E
    assert L.sift_knn_match_l2sqr_f32(None, None, 0, None, 0, 2, None, None) == E


def test_l2_f32_python_names_and_pinned_rejections(siftgpu):
    for meth in ["knn_match_l2sqr_f32_segmented_device", "knnMatchL2SqrF32Segmented", "knnMatchL2SqrF32"]:
        assert callable(getattr(siftgpu.Context, meth)), meth
    assert siftgpu.SIFT_METRIC_L2SQR_F32 == 3
    sig = inspect.signature(siftgpu.l2_match)
    assert list(sig.parameters) == ["query", "train", "k", "squared", "ctx"]
    assert [sig.parameters[p].default for p in ("k", "squared", "ctx")] == [2, False, None]
    f = np.zeros((2, 128), np.float32)
    with pytest.raises(ValueError):
        siftgpu.BFMatcher(4)                                       # plain NORM_L2 stays out of BFMatcher
    with pytest.raises(ValueError):
        siftgpu.BFMatcher(siftgpu.NORM_L2SQR).knnMatch(f, f, 2)    # raised before any context is made
    with pytest.raises(ValueError):
        siftgpu.cross_check_match(f, f, siftgpu.NORM_L2SQR)
    with pytest.raises(ValueError):
        siftgpu.window_match(f, None, f, None, 1.0, normType=siftgpu.NORM_L2SQR)
    for doc in (siftgpu.BFMatcher.__doc__, siftgpu.cross_check_match.__doc__, siftgpu.window_match.__doc__):
        assert "l2_match" in doc


def test_match_l2_f32_layouts(tmp_path):
    """tests/cpp/match_l2_f32_layout.cpp, built like test_match_l2_u8.py::test_match_l2_u8_layouts:
    with the address and undefined-behaviour sanitizers (runtimes linked
    statically into the program) where the host compiler has them."""
    src = os.path.join(ROOT, "tests", "cpp", "match_l2_f32_layout.cpp")
    exe = tmp_path / "match_l2_f32_layout"
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "match l2 f32 layouts ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- the oracle's fma --------------------------------------------------------------------
def _libm_fmaf(a, b, c):
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    m.fmaf.restype = ctypes.c_float
    m.fmaf.argtypes = [ctypes.c_float] * 3
    return np.array([m.fmaf(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], f32)


def test_fma32_equals_libm_fmaf():
    rng = np.random.default_rng(150)
    n = 20000
    a, b = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    c = (rng.standard_normal(n) * rng.choice([1e-6, 1e-3, 1.0, 1e3], n)).astype(f32)
    a[:5000], b[:5000] = F.rows(rng, 40).ravel()[:5000], F.rows(rng, 40).ravel()[:5000]   # descriptor-like
    c[:5000] = np.abs(c[:5000])
    assert_bits_equal(F.fma32(a, b, c), _libm_fmaf(a, b, c), "random triples")
    # crafted midpoints: the product of two odd 12.x-bit integers in [2^24, 2^25) is an odd 25-bit
    # integer, exactly half way between two float32; an addend far below float64's last bit of the
    # sum decides the side, but the float64 sum drops it and the cast then goes to even
    m = 4000
    x = (2 * rng.integers(2048, 2896, m) + 1).astype(f32)
    y = (2 * rng.integers(2048, 2896, m) + 1).astype(f32)
    prod = x.astype(np.int64) * y.astype(np.int64)
    assert ((prod >= 1 << 24) & (prod < 1 << 25) & (prod % 2 == 1)).all()
    scale = (2.0 ** rng.integers(-30, 10, m)).astype(f32)
    z = (rng.choice([-1.0, 1.0], m) * 2.0 ** rng.integers(-60, -40, m)).astype(f32)
    z[:m // 8] = 0                                                                      # true ties: to even
    x, z = x * scale, z * scale
    ref = _libm_fmaf(x, y, z)
    assert_bits_equal(F.fma32(x, y, z), ref, "midpoint products with an addend below float64's rounding")
    naive = (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(f32)
    assert (naive.view(np.int32) != ref.view(np.int32)).sum() > m // 8, "the crafted cases do trap a double rounding"
    # and in the subnormal range of float32
    x, y, z = x[:500] * f32(2.0 ** -100), y[:500] * f32(2.0 ** -60), z[:500] * f32(2.0 ** -100)
    assert_bits_equal(F.fma32(x, y, z), _libm_fmaf(x, y, z), "subnormal results")


# ---- the dyadic identity -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["weights", "extremes", "dense65x64", "bits300x65"])
def test_oracle_dyadic_identity(name):
    """On rows u / 512 the oracle's d is the int64 squared distance times 2^-18 exactly,
    indices included: every product, sum and norm is an integer below 2^24 in units of
    2^-18, so no summation order matters."""
    u = {"weights": L2.weights_case, "extremes": L2.extremes_case,
         "dense65x64": lambda: L2.tie_case(U.TIE_IDS.index("dense65x64")),
         "bits300x65": lambda: L2.tie_case(U.TIE_IDS.index("bits300x65"))}[name]()
    idx, dist = F.seg_ref(F.dyadic(u.q), u.qoff, F.dyadic(u.t), u.toff, 2, u.q_cap, u.t_cap)
    assert_bits_equal(idx, u.idx, name + " idx")
    assert_bits_equal(dist * F.SCALE, u.dist, name + " dist * 2^18")
    rev = F.seg_ref(F.dyadic(u.q), u.qoff, F.dyadic(u.t), u.toff, 2, u.q_cap, u.t_cap, order=F.PI[::-1])
    assert_bits_equal(rev[1], dist, name + " in the reversed order")


# ---- the censuses ------------------------------------------------------------------------
def test_oracle_order_census():
    """On the random float inputs the oracle under PI and under the reversed order differ in
    the bits of the nearest distance on at least a tenth of the rows (a sum of 128 products
    rounded 128 times lands on another float for most orders), so the GPU's bit comparison
    pins the order and is not vacuous."""
    c = F.edges_case(False)
    q = c.q[c.qoff[11]:c.qoff[12]]
    a = F.knn_ref(q, c.t, 1)[1]
    b = F.knn_ref(q, c.t, 1, order=F.PI[::-1])[1]
    ident = F.knn_ref(q, c.t, 1, order=np.arange(128))[1]
    differ = int((a.view(np.int32) != b.view(np.int32)).sum())
    differ_id = int((a.view(np.int32) != ident.view(np.int32)).sum())
    print(f"rows whose d1 differs: reversed {differ}, identity {differ_id} of {len(q)}")
    assert differ >= len(q) // 10 and differ_id >= len(q) // 10


@pytest.mark.parametrize("which", ["shared", "segmented", "splits"])
def test_oracle_tie_census(which):
    """Every tie input still has rows tied for first place, and rows tied for second place
    behind a unique nearer row: the planted ones, by the oracle's distances."""
    c = {"shared": lambda: F.edges_case(False), "segmented": lambda: F.edges_case(True), "splits": F.splits_case}[which]()
    first, second = F.census(c)
    print(f"{c.name}: {first} rows tied for first place, {second} for second")
    assert first >= 4 and second >= 4


# ---- sanity of the rule itself -----------------------------------------------------------
def real_pairs():
    """(name, query, train) from the descriptors of the golden images."""
    g = lambda n: np.load(os.path.join(ROOT, "tests", "golden", n), allow_pickle=False)  # noqa: E731
    book, synth, m = g("book.npz")["desc"], g("ref_synth_240x320.npz")["desc"], g("match.npz")
    # (match.npz's "dup" rows are copies planted for ties: no gap to rank by, so they are not used here)
    return [("book-synth", book, synth), ("synth-book", synth, book), ("noisy-book", m["noisy"], book)]


GAMMA130 = 130 * 2.0 ** -24 / (1 - 130 * 2.0 ** -24)


def check_against_float64(name, q, t, idx, dist):
    """Asserts |d - d64| <= B = 2 gamma_130 (nq + nt) on the returned neighbours and that the
    indices are the float64 ranking's on every row whose 1st-2nd and 2nd-3rd gaps exceed 2 B.
    Returns the number of rows exempt from the index check."""
    q64, t64 = np.asarray(q, np.float64), np.asarray(t, np.float64)
    d64 = ((q64[:, None, :] - t64[None, :, :]) ** 2).sum(-1)
    bound = 2 * GAMMA130 * ((q64 ** 2).sum(-1)[:, None] + (t64 ** 2).sum(-1)[None, :])
    rows = np.arange(len(q))
    for j in range(2):
        err = np.abs(dist[:, j].astype(np.float64) - d64[rows, idx[:, j]])
        lim = bound[rows, idx[:, j]]
        print(f"{name}: column {j} max |d - d64| = {err.max():.3e}, min slack = {(lim - err).min():.3e}")
        assert (err <= lim).all(), name
    order = np.argsort(d64, axis=1, kind="stable")
    s = np.take_along_axis(d64, order[:, :3], axis=1)
    b = bound.max(axis=1)
    clear = ((s[:, 1] - s[:, 0]) > 2 * b) & ((s[:, 2] - s[:, 1]) > 2 * b)
    assert (idx[clear] == order[clear, :2]).all(), name
    print(f"{name}: {int((~clear).sum())} of {len(q)} rows exempt")
    return int((~clear).sum())


def test_oracle_rule_against_float64_on_real_descriptors():
    """The oracle alone stays within the bound and within 1 % exempt rows on the chosen images."""
    for name, q, t in real_pairs():
        idx, dist = F.knn_ref(q, t, 2)
        exempt = check_against_float64(name, q, t, idx, dist)
        assert exempt <= 0.01 * len(q), (name, exempt, len(q))
