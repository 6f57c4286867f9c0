"""GPU tests of the provided-keypoint calls (sift_compute_batch, sift_compute, the
keypoints argument of SIFT_NCL, the five-argument SIFT_NCL of sift.hpp).  Every
comparison is bit for bit.  Descriptor buffers are filled with a sentinel and
hold extra rows on both sides of the rows a call owns."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import compute_inputs as CI
from conftest import GOLDEN, PKG, ROOT, assert_bits_equal, kp_bytes

pytestmark = pytest.mark.gpu

SHAPE = CI.SHAPES[0]
SENT = -7.0
EXTRA = 4          # descriptor rows past kp_cap: never written
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _img(oracle, seed, shape=SHAPE):
    return _once(("img", seed, shape), lambda: oracle.synth_image(seed, *shape))


def _gpyr(oracle, seed, shape=SHAPE):
    return _once(("gpyr", seed, shape), lambda: oracle.build_gaussian_pyramid(_img(oracle, seed, shape), CI.N_OCT))


def _want(oracle, seed, kps, shape=SHAPE, max_layer=4):
    """The oracle's descriptors of the valid rows, zeros in the invalid ones."""
    ok = CI.valid(kps, max_layer)
    out = np.zeros((len(kps), 128), np.float32)
    out[ok] = oracle.calc_descriptors(_gpyr(oracle, seed, shape), shape[0], shape[1], kps[ok], CI.N_OCT, 0)
    return out


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _imgs_t(oracle, seeds, shape=SHAPE, pad_cols=0, pad_rows=0):
    a = np.full((len(seeds), shape[0] + pad_rows, shape[1] + pad_cols), np.nan, np.float32)
    for i, s in enumerate(seeds):
        a[i, :shape[0], :shape[1]] = _img(oracle, s, shape)
    return _dev(a)


def _filler(n):
    """Rows that belong to no image: invalid ones, so describing one would set the error bit."""
    k = np.zeros(n, CI.KEYPOINT_DTYPE)
    k["octave"] = 0x0509
    return k


def _compute(ctx, imgs_t, shape, kps, offs, cap, max_layer=4, sync=True):
    """Runs compute_batch on kps (placed in a buffer of cap rows); returns the host result,
    cap + EXTRA rows of 128."""
    import torch
    B = imgs_t.shape[0]
    kbuf = _filler(cap)
    kbuf[:min(len(kps), cap)] = kps[:cap]
    k_t = _dev(kbuf.view(np.int32).reshape(cap, 7))
    o_t = _dev(np.asarray(offs, np.int32))
    d_t = torch.full((cap + EXTRA, 128), SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.compute_batch(imgs_t.data_ptr(), B, shape[0], shape[1], imgs_t.shape[2], imgs_t.shape[1] * imgs_t.shape[2],
                      k_t.data_ptr(), o_t.data_ptr(), cap, d_t.data_ptr(), max_layer)
    if not sync:
        return d_t, (k_t, o_t)
    ctx.sync()
    assert k_t.cpu().numpy().tobytes() == kbuf.tobytes(), "the keypoints are only read"
    return d_t.cpu().numpy()


def _detect(ctx, imgs_t, shape, cap, masks_t=None):
    import torch
    B = imgs_t.shape[0]
    k = torch.full((cap, 7), -1, dtype=torch.int32, device="cuda")
    d = torch.full((cap, 128), SENT, dtype=torch.float32, device="cuda")
    o = torch.full((B + 1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    kw = {} if masks_t is None else dict(masks_ptr=masks_t.data_ptr(), mask_row_stride=shape[1], mask_img_stride=0)
    ctx.detect_compute_batch(imgs_t.data_ptr(), B, shape[0], shape[1], imgs_t.shape[2],
                             imgs_t.shape[1] * imgs_t.shape[2], k.data_ptr(), d.data_ptr(), cap, o.data_ptr(), **kw)
    ctx.sync()
    return k.cpu().numpy().view(CI.KEYPOINT_DTYPE).reshape(cap), d.cpu().numpy(), o.cpu().numpy()


# ---- 1. round trip ---------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ["exact", "fast", "exact_nograph", "fast_nograph", "exact_scatter"])
def test_round_trip(siftgpu, oracle, flags, monkeypatch):
    if flags == "exact_scatter":
        # the scatter blur at this size (read at context creation): with max_layer 3
        # every octave leaves plane 4 out, and detection after it must not see that
        monkeypatch.setenv("SIFT_HIP_SYM_MIN", "0")
    fl = (siftgpu.SIFT_FLAG_FAST if "fast" in flags else 0) | (siftgpu.SIFT_FLAG_NO_GRAPH if "nograph" in flags else 0)
    imgs = _imgs_t(oracle, [0, 1, 2])
    cap = 6000
    with siftgpu.Context(*SHAPE, 3, device=0, flags=fl) as ctx:
        k, d, o = _detect(ctx, imgs, SHAPE, cap)
        n = int(o[3])
        assert 0 < n < cap - 8 and o[0] == 0
        if "fast" not in flags:
            assert_bits_equal(d[:o[1]], oracle.sift(_img(oracle, 0))[1], "the detect call itself")
        # shifted by 5 rows, so rows on both sides of the offsets must stay untouched
        kk = np.concatenate([_filler(5), k[:n]])
        for max_layer in (3, 4):
            got = _compute(ctx, imgs, SHAPE, kk, o + 5, cap, max_layer)
            assert_bits_equal(got[5:5 + n], d[:n], f"{flags} max_layer {max_layer}: compute of the detected keypoints")
            assert np.all(got[:5] == SENT) and np.all(got[5 + n:] == SENT), "rows outside the offsets were written"
        k2, d2, o2 = _detect(ctx, imgs, SHAPE, cap)
        assert_bits_equal(d2, d, "detect after compute")
        assert_bits_equal(o2, o, "offsets after compute")


# ---- 2. crafted rows against the oracle and the sub-modules -------------------------------------
@pytest.mark.parametrize("shape", CI.SHAPES)
def test_crafted_rows(siftgpu, oracle, shape):
    seeds = [3, 4]
    rows = [CI.crafted(shape, v) for v in range(len(seeds))]
    for r in rows:
        det = CI.takes_det(r, shape)
        rad, px, py, orows, ocols, clamped = CI.window(r, shape)
        assert det.any() and (~det).any(), "both row lists must be non-empty"
        assert (rad[det] == 40).any() and (rad == 41).any() and clamped.any()
        assert ((px < 0) | (px >= ocols)).any() and ((px == 0) & ~det).any()
        lay = CI.unpack(r)[1]
        assert (lay == 0).any() and (lay == 4).any() and (CI.unpack(r)[0] == 4).any()
    kps = np.concatenate(rows)
    offs = CI.offsets([len(r) for r in rows])
    cap = len(kps) + 9
    imgs = _imgs_t(oracle, seeds, shape)
    with siftgpu.Context(*shape, 2, device=0) as ctx:
        got = _compute(ctx, imgs, shape, kps, offs, cap)
        for b, s in enumerate(seeds):
            sl = slice(offs[b], offs[b + 1])
            assert_bits_equal(got[sl], _want(oracle, s, kps[sl], shape), f"image {b} against the oracle")
            planes = ctx.buildGaussianPyramid(_img(oracle, s, shape), CI.N_OCT)
            assert_bits_equal(got[sl], ctx.calDescriptor(planes, kps[sl], 0), f"image {b} against calDescriptor")
        assert np.all(got[len(kps):] == SENT)


# ---- 3. invalid rows -----------------------------------------------------------------------------
@pytest.mark.parametrize("what,octave,layer,max_layer", CI.INVALID)
def test_invalid_rows(siftgpu, oracle, what, octave, layer, max_layer):
    good = CI.crafted(SHAPE)
    good = good[CI.valid(good, max_layer)]
    bad = CI.invalid_row(octave, layer)
    kps = np.concatenate([good[:4], bad, good[4:], bad])
    assert not CI.valid(bad, max_layer).any()
    want = _want(oracle, 5, kps, max_layer=max_layer)
    assert not want[4].any() and not want[-1].any() and want[3].any()
    imgs = _imgs_t(oracle, [5])
    with siftgpu.Context(*SHAPE, 1, device=0) as ctx:
        d_t, keep = _compute(ctx, imgs, SHAPE, kps, [0, len(kps)], len(kps) + 3, max_layer, sync=False)
        assert ctx._L.sift_sync(ctx.h) == siftgpu.SIFT_E_INVALID, what
        assert ctx._L.sift_sync(ctx.h) == siftgpu.SIFT_OK, "reported once"
        got = d_t.cpu().numpy()
        assert_bits_equal(got[:len(kps)], want, what)
        assert np.all(got[len(kps):] == SENT)
        # the host form: SIFT_E_INVALID, the rows written all the same
        out = np.full((len(kps), 128), SENT, np.float32)
        img = np.ascontiguousarray(_img(oracle, 5))
        rc = ctx._L.sift_compute(ctx.h, img.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), SHAPE[0], SHAPE[1], 0,
                                 kps.ctypes.data, len(kps), max_layer,
                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        assert rc == siftgpu.SIFT_E_INVALID
        assert_bits_equal(out, want, what + ", host form")
        assert ctx._L.sift_sync(ctx.h) == siftgpu.SIFT_OK
        # valid rows alone: no error
        assert_bits_equal(ctx.compute(img, good, max_layer), _want(oracle, 5, good, max_layer=max_layer), "valid rows")


# ---- 4. offsets ----------------------------------------------------------------------------------
def test_offsets(siftgpu, oracle):
    seeds = [6, 7, 8, 9]
    rows = CI.crafted(SHAPE)
    n = len(rows)
    imgs = _imgs_t(oracle, seeds)
    padded = _imgs_t(oracle, seeds, pad_cols=11, pad_rows=3)
    want = {s: _want(oracle, s, rows) for s in seeds}
    with siftgpu.Context(*SHAPE, 4, device=0) as ctx:
        def run(counts, first=0, cap=None, src=imgs, offs=None):
            kps = np.concatenate([_filler(first)] + [rows[:c] for c in counts])
            o = first + CI.offsets(counts) if offs is None else np.asarray(offs, np.int32)
            cap = len(kps) + 6 if cap is None else cap
            got = _compute(ctx, src[:len(counts)], SHAPE, kps, o, cap)
            at = first
            assert np.all(got[:first] == SENT)
            for b, c in enumerate(counts):
                keep = max(0, min(c, cap - at))
                assert_bits_equal(got[at:at + keep], want[seeds[b]][:keep], f"counts {counts} first {first} image {b}")
                at += c
            assert np.all(got[min(at, cap):] == SENT)
            return got

        run([0, n, 7, n])            # an empty first image
        run([n, 0, 0, 5])            # empty middle images
        run([3, n, 9, 0])            # an empty last image
        run([n, 4, n, 2], first=7)   # off[0] > 0
        run([n], first=2)            # batch 1
        run([n, n, n, n], cap=3 * n + 5)   # off[batch] > kp_cap: clamped, no error (run() syncs through _check)
        run([5, n], offs=[-4, 5, 5 + n])   # a negative offset is clamped to 0: image 0 owns rows [0, 5)
        run([n, 3, n, 6], src=padded)      # padded row and image strides
        run([n, n, n, n], cap=40000)       # kp_cap above every earlier call: the scratch grows
        run([2, n, 1, n])                  # and a smaller call after it


# ---- 5. dense grid -------------------------------------------------------------------------------
def test_dense_grid(siftgpu, oracle):
    seeds = [10, 11, 12]
    grid = CI.dense_grid(SHAPE, 4, 4.0)
    n = len(grid)
    det = CI.takes_det(grid, SHAPE)
    assert det.sum() > 4 * 256 and 0 < (~det).sum() < 256    # several ranking chunks per image; the border row apart
    imgs = _imgs_t(oracle, seeds)
    with siftgpu.Context(*SHAPE, 3, device=0) as ctx:
        ctx.set_candidate_capacity(64)   # detection here could emit 18 x 64 keypoints per image: far fewer than n
        assert n > 18 * 64
        got = _compute(ctx, imgs, SHAPE, np.concatenate([grid] * 3), CI.offsets([n] * 3), 3 * n + 4, max_layer=1)
        sample = np.random.default_rng(7).choice(n, 256, replace=False)
        for b, s in enumerate(seeds):
            mine = got[b * n:(b + 1) * n]
            assert_bits_equal(mine[sample], _want(oracle, s, grid[sample]), f"image {b}: the sample against the oracle")
            planes = ctx.buildGaussianPyramid(_img(oracle, s), CI.N_OCT)
            assert_bits_equal(mine, ctx.calDescriptor(planes, grid, 0), f"image {b}: every row against calDescriptor")
        assert np.all(got[3 * n:] == SENT)


# ---- 6. graph cache ------------------------------------------------------------------------------
def test_graph_cache(siftgpu, oracle):
    import torch
    rows = CI.crafted(SHAPE)
    rows = rows[CI.valid(rows, 3)]      # valid under both values of max_layer used below
    imgs = _imgs_t(oracle, [3, 4])
    kps = np.concatenate([rows, rows])
    offs, cap = CI.offsets([len(rows)] * 2), 2 * len(rows) + 2
    with siftgpu.Context(*SHAPE, 2, device=0) as ctx:
        k_t = [_dev(np.concatenate([kps, kps[:2]]).view(np.int32).reshape(cap, 7)) for _ in range(2)]
        o_t = _dev(offs)
        d_t = torch.full((cap, 128), SENT, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def call(k, max_layer):
            ctx.compute_batch(imgs.data_ptr(), 2, SHAPE[0], SHAPE[1], SHAPE[1], SHAPE[0] * SHAPE[1], k.data_ptr(),
                              o_t.data_ptr(), cap, d_t.data_ptr(), max_layer)
            ctx.sync()
            return ctx.graph_stats()

        c0 = ctx.graph_stats()
        c1 = call(k_t[0], 4)
        first = d_t.cpu().numpy().copy()
        assert (c1[0], c1[2]) == (c0[0] + 1, c0[2] + 1), "the first call captures and instantiates"
        assert call(k_t[0], 4) == c1, "a repeat call captures nothing"
        c2 = call(k_t[0], 3)
        assert (c2[0], c2[1], c2[2]) == (c1[0] + 1, c1[1], c1[2] + 1), "another max_layer is a new entry"
        c3 = call(k_t[1], 4)
        assert (c3[0], c3[1], c3[2]) == (c2[0] + 1, c2[1] + 1, c2[2]), "another keypoint buffer is an update"
        assert_bits_equal(d_t.cpu().numpy(), first, "the updated sequence")


# ---- 7. isolation --------------------------------------------------------------------------------
@pytest.mark.parametrize("budget", [False, True])
def test_isolation(siftgpu, oracle, budget):
    imgs = _imgs_t(oracle, [0, 1, 2])
    rows = CI.crafted(SHAPE)
    kps, offs = np.concatenate([rows] * 3), CI.offsets([len(rows)] * 3)
    cap = 6000
    mask = None
    with siftgpu.Context(*SHAPE, 3, device=0) as ctx:
        alone = _compute(ctx, imgs, SHAPE, kps, offs, len(kps) + 2)
        if budget:
            ctx.set_max_features(50)
            m = np.ones(SHAPE, np.uint8)
            m[:, SHAPE[1] // 2:] = 0
            mask = _dev(m)
        a = _detect(ctx, imgs, SHAPE, cap, mask)
        mid = _compute(ctx, imgs, SHAPE, kps, offs, len(kps) + 2)
        b = _detect(ctx, imgs, SHAPE, cap, mask)
        last = _compute(ctx, imgs, SHAPE, kps, offs, len(kps) + 2)
        for x, y, what in zip(a, b, ("keypoints", "descriptors", "offsets")):
            assert_bits_equal(x, y, f"detect after compute: {what}")
        assert_bits_equal(mid, alone, "compute after detect (neither the budget nor a mask applies)")
        assert_bits_equal(last, alone, "compute -> detect -> compute")
        if budget:
            assert 0 < a[2][3] < _detect_total(oracle)


def _detect_total(oracle):
    return sum(len(oracle.sift(_img(oracle, s))[0]) for s in (0, 1, 2))


# ---- 8. front ends -------------------------------------------------------------------------------
def test_front_ends(siftgpu, oracle, tmp_path):
    img = _img(oracle, 3)
    rows = CI.crafted(SHAPE)
    want = _want(oracle, 3, rows)
    with siftgpu.Context(*SHAPE, 1, device=0) as ctx:
        assert_bits_equal(ctx.compute(img, rows), want, "Context.compute")
        assert_bits_equal(ctx.compute(img, rows[CI.valid(rows, 3)], max_layer=3), want[CI.valid(rows, 3)], "max_layer 3")
        k, d = ctx.SIFT_NCL(img, keypoints=rows, mask=np.zeros(SHAPE, np.uint8))
        assert_bits_equal(kp_bytes(k), kp_bytes(rows), "SIFT_NCL(keypoints=) returns them unchanged")
        assert_bits_equal(d, want, "SIFT_NCL(keypoints=): the mask is ignored")
        e = ctx.compute(img, rows[:0])
        assert e.shape == (0, 128) and e.dtype == np.float32
        det = ctx.SIFT_NCL(img)
        assert_bits_equal(ctx.compute(img, det[0], max_layer=3), det[1], "compute of SIFT_NCL's own keypoints")
        for bad in (-1, 5):
            with pytest.raises(siftgpu.SiftError) as ei:
                ctx.compute(img, rows, max_layer=bad)
            assert ei.value.code == siftgpu.SIFT_E_INVALID
        with pytest.raises(siftgpu.SiftError) as ei:
            ctx.compute(np.zeros((SHAPE[0] + 1, SHAPE[1]), np.float32), rows)
        assert ei.value.code == siftgpu.SIFT_E_SIZE
    assert_bits_equal(siftgpu.compute(img, rows), want, "module-level compute")
    k, d = siftgpu.SIFT_NCL(img, keypoints=rows)
    assert_bits_equal(d, want, "module-level SIFT_NCL(keypoints=)")


def test_cpp_overload(siftgpu, tmp_path):
    """tests/cpp/compute_cli.cpp: detect, then describe the same keypoints with
    useProvidedKeypoints true (equal descriptors) and run false (the detect call)."""
    exe = tmp_path / "compute_cli"
    lib = os.path.join(PKG, "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "compute_cli.cpp"), "-o", str(exe), "-L", lib,
                    "-lsift_shim", "-lsift_hip", f"-Wl,-rpath,{lib}"], check=True)
    r = subprocess.run([str(exe), os.path.join(GOLDEN, "book_gray.pgm")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    n, detect, provided, again, subset = int(words[0]), words[1], words[2], words[3], words[4]
    assert n > 100
    assert provided == detect, "useProvidedKeypoints = true differs from the detect call's descriptors"
    assert again == detect, "useProvidedKeypoints = false is not the masked detect call"
    assert subset != detect
