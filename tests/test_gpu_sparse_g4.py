"""GPU tests of batch SIFT_NCL's sparse flow: octaves on the scatter blur do not
blur their widest scale (plane 4); the extrema pass keeps layer-2 pixels that
pass their other 17 neighbours, and plane 4 is evaluated point by point on
the 3x3 around each candidate that sits on layer 2 (g4_fill_kernel), in rounds
with the Newton steps.  Everything is compared bit for bit with the CPU
oracle; the scatter path is forced at small sizes through SIFT_HIP_SYM_MIN.
"""
import numpy as np
import pytest

import adversarial_inputs as A
from conftest import assert_bits_equal, kp_bytes

pytestmark = pytest.mark.gpu

_refs = {}


def _ref(oracle, key, make):
    """(image, oracle keypoints, oracle descriptors, extrema_stats), once per run."""
    if key not in _refs:
        img = make()
        kps, desc = oracle.sift(img)
        _refs[key] = (img, kps, desc, oracle.extrema_stats())
    return _refs[key]


def _force_scatter(monkeypatch, sym_min=0):
    monkeypatch.setenv("SIFT_HIP_SYM_MIN", str(sym_min))
    monkeypatch.setenv("SIFT_HIP_SYM_ROWS_MIN", "0")


def _run_batch(ctx, imgs, cap=30000):
    import torch
    B = len(imgs)
    R, C = imgs[0].shape
    buf = torch.from_numpy(np.ascontiguousarray(np.stack(imgs), np.float32)).cuda()
    kpts = torch.full((cap, 7), -1, dtype=torch.int32, device="cuda")
    desc = torch.full((cap, 128), -1.0, dtype=torch.float32, device="cuda")
    offs = torch.full((B + 1,), -1, dtype=torch.int32, device="cuda")
    ctx.detect_compute_batch(buf.data_ptr(), B, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                             offs.data_ptr())
    ctx.sync()
    return offs.cpu().numpy(), kpts.cpu().numpy().view(np.uint8).reshape(cap, 28), desc.cpu().numpy()


def _check_batch(out, refs, what):
    o, k, d = out
    assert o[0] == 0
    for b, (kr, dr) in enumerate(refs):
        assert o[b + 1] - o[b] == len(kr), f"{what} image {b}: {o[b + 1] - o[b]} keypoints, expected {len(kr)}"
        assert_bits_equal(k[o[b]:o[b + 1]], kp_bytes(kr), f"{what} image {b} keypoints")
        assert_bits_equal(d[o[b]:o[b + 1]], dr, f"{what} image {b} descriptors")
    assert np.all(k[o[len(refs)]:].view(np.int32) == -1), f"{what}: keypoint writes past the total"


# 97 x 131, 160 x 200: columns no multiple of 64, odd rows in some octave.
# sym_min 6 at 160 x 200 x 3: octaves 0 and 1 (4 and 2 strips x 3 images) on the
# scatter blur, octaves 2.. (1 strip x 3) on the 2-D tiles with a dense plane 4
# -- both kinds of octave in one candidate list.
@pytest.mark.parametrize("shape,batch,sym_min", [((97, 131), 2, 0), ((97, 131), 3, 0), ((160, 200), 2, 0),
                                                 ((160, 200), 3, 0), ((160, 200), 3, 6)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_sparse_batch_matches_oracle(siftgpu, oracle, monkeypatch, shape, batch, sym_min):
    _force_scatter(monkeypatch, sym_min)
    refs = [_ref(oracle, ("synth", 70 + b, shape), lambda b=b: oracle.synth_image(70 + b, *shape))
            for b in range(batch)]
    assert all(len(kr) > 0 for _, kr, _, _ in refs)
    with siftgpu.Context(*shape, batch, device=0) as ctx:
        for rep in range(2):  # the second call replays the captured sequence
            _check_batch(_run_batch(ctx, [im for im, _, _, _ in refs]), [(kr, dr) for _, kr, dr, _ in refs],
                         f"{shape} x {batch} sym_min {sym_min} call {rep}")


def test_point_evaluation_equals_dense_plane(siftgpu, oracle):
    """Every pixel of a 70 x 90 plane: the 37 x 37 window leaves the image on
    all four sides, and the last row and column are the zero quirk's
    (src/sift.cpp:116).  The centre of each patch and its eight neighbours
    against the dense blur of the same plane, GPU and CPU."""
    R, C = 70, 90
    img = oracle.synth_image(3, R, C)
    with siftgpu.Context(R, C, 1, device=0) as ctx:
        planes = ctx.buildGaussianPyramid(img, 1)
        rc = np.stack(np.mgrid[0:R, 0:C], -1).reshape(-1, 2)
        got = ctx.selftest_g4_points(planes[0], rc).reshape(R, C, 3, 3)
        outside = ctx.selftest_g4_points(planes[0], np.array([[-1, -1], [R, C], [-30, 40], [35, C + 25]]))
    cpu = oracle.split_planes(oracle.build_gaussian_pyramid(img, 1), R, C, 1, 5)
    assert_bits_equal(planes[4], cpu[4], "dense plane 4, GPU against CPU")
    dense = planes[4]
    assert_bits_equal(got[:, :, 1, 1], dense, "patch centres")
    for dy in range(3):
        for dx in range(3):
            # patch entry (dy, dx) of pixel (r, c) is the plane at (r + dy - 1, c + dx - 1)
            rs = slice(max(0, 1 - dy), R - max(0, dy - 1))
            cs = slice(max(0, 1 - dx), C - max(0, dx - 1))
            want = dense[rs.start + dy - 1:rs.stop + dy - 1, cs.start + dx - 1:cs.stop + dx - 1]
            assert_bits_equal(got[rs, cs, dy, dx], want, f"patch entry ({dy}, {dx})")
    # points off the plane: their in-plane neighbours still match, nothing faults
    assert outside[0, 2, 2] == dense[0, 0] and outside[1, 0, 0] == dense[R - 1, C - 1]
    assert np.isfinite(outside).all()


def _plateau_image(rows, cols, seed=21):
    """2 x 2 blocks of few integer levels, mirrored left-right: plateaus.  (The
    blur's raster-order chain and zero last column break the mirror bit-wise;
    exact ties are test_sparse_batch_exact_ties' business.)"""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 4, ((rows + 1) // 2, (cols + 3) // 4)) * 85.0
    half = np.kron(b, np.ones((2, 2)))[:rows, :(cols + 1) // 2]
    return np.ascontiguousarray(np.concatenate([half, half[:, ::-1]], 1)[:, :cols], np.float32)


@pytest.mark.parametrize("shape", A.IMAGE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sparse_batch_crafted_images(siftgpu, oracle, monkeypatch, shape):
    """Plateaus (stars, mirrored integer blocks), a flat image between
    them, noise, and two synthetic images whose refinement moves in (r, c),
    changes layer and runs out of steps (the oracle's counters, checked
    here), with keypoints next to the 5-pixel border on every side."""
    _force_scatter(monkeypatch)
    fams = ["stars", "constant", "noise_u8"]
    refs = [_ref(oracle, (f, shape), lambda f=f: A.IMAGE_FAMILIES[f](*shape)) for f in fams]
    refs.append(_ref(oracle, ("plateau", shape), lambda: _plateau_image(*shape)))
    lively = [_ref(oracle, ("synth", s, shape), lambda s=s: oracle.synth_image(s, *shape)) for s in (0, 2)]
    refs += lively
    assert len(refs[1][1]) == 0, "the flat image has no keypoints"
    for _, _, _, st in lively:
        assert st["moved_layer"] > 0 and st["moved_rc"] > 0 and st["rej_max_interp"] > 0, st
    # octave-0 keypoints whose refined pixel is on the first / last row and column the border leaves
    k = np.concatenate([r[1] for r in lively])
    o0 = k[(k["octave"] & 255) == 0]
    ys, xs = np.rint(o0["y"]).astype(int), np.rint(o0["x"]).astype(int)
    assert (ys == 5).any() and (xs == 5).any() and (ys == shape[0] - 6).any() and (xs == shape[1] - 6).any()
    with siftgpu.Context(*shape, len(refs), device=0) as ctx:
        _check_batch(_run_batch(ctx, [r[0] for r in refs]), [(r[1], r[2]) for r in refs], f"crafted {shape}")


def _tie_counts(oracle, img):
    """From the oracle's Gaussian planes, over every octave: layer-2 pixels inside the border that pass
    the threshold and their 17 neighbours in DoG 1 and DoG 2 (`partial`), those that also pass the nine
    in DoG 3 (`kept`), kept ones whose value EQUALS the largest (smallest) DoG 3 neighbour (`tie3_kept`)
    and kept ones whose value equals the largest (smallest) of the 17 (`tie12_kept`)."""
    R, C = img.shape
    g = oracle.split_planes(oracle.build_gaussian_pyramid(img, 5), R, C, 5, 5)

    def nb(a, skip_centre):
        sh = [a[1 + dy:a.shape[0] - 1 + dy, 1 + dx:a.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)
              if not (skip_centre and dy == 0 and dx == 0)]
        return np.maximum.reduce(sh), np.minimum.reduce(sh)
    out = dict(partial=0, kept=0, tie3_kept=0, tie12_kept=0)
    for o in range(5):
        G = g[5 * o:5 * o + 5]
        r, c = G[0].shape
        if r < 13 or c < 13:
            continue
        d = [G[s + 1] - G[s] for s in range(4)]     # float32: the reference's own subtraction
        v = d[2][1:-1, 1:-1]
        (m1x, m1n), (m2x, m2n), (m3x, m3n) = nb(d[1], False), nb(d[2], True), nb(d[3], False)
        inside = np.zeros_like(v, bool)
        inside[4:r - 6, 4:c - 6] = True               # rows 5 .. r - 6 of the plane
        px, pn = np.maximum(m1x, m2x), np.minimum(m1n, m2n)
        part = inside & (np.abs(v) > 8) & (((v > 0) & (v >= px)) | ((v < 0) & (v <= pn)))
        kept = part & (((v > 0) & (v >= m3x)) | ((v < 0) & (v <= m3n)))
        out["partial"] += int(part.sum())
        out["kept"] += int(kept.sum())
        out["tie3_kept"] += int((kept & (((v > 0) & (v == m3x)) | ((v < 0) & (v == m3n)))).sum())
        out["tie12_kept"] += int((kept & (((v > 0) & (v == px)) | ((v < 0) & (v == pn)))).sum())
    return out


def _tie3_image(oracle):
    """Synthetic seed 70 at 97 x 131 minus a smooth bump (1 - d^2 / 18^2)^2 around (22, 35), whose
    amplitude was bisected on the CPU oracle until the layer-2 candidate at (22, 35) of octave 0
    has DoG 2 == its largest DoG 3 neighbour to the bit: with >= the candidate stays and becomes
    a keypoint, with > both would go.  Only IEEE adds, multiplies and divides build it, so it is
    the same on every host."""
    R, C = 97, 131
    yy, xx = np.mgrid[0:R, 0:C].astype(np.float64)
    q = 1.0 - ((yy - 22.0) ** 2 + (xx - 35.0) ** 2) / 324.0
    bump = (np.maximum(q, 0.0) ** 2).astype(np.float32)
    return (oracle.synth_image(70, R, C) + np.float32(-float.fromhex("0x1.3ed77cp+3")) * bump).astype(np.float32)


def _tie12_image(oracle):
    """Synthetic seed 0 at 160 x 200, four times the contrast on an offset of 2^20: the planes are
    multiples of 1/8, so candidates that equal a DoG 1 / DoG 2 neighbour exactly are common."""
    return (oracle.synth_image(0, 160, 200) * 4 + 2.0 ** 20).astype(np.float32)


@pytest.mark.parametrize("which", ["dog3", "dog12"])
def test_sparse_batch_exact_ties(siftgpu, oracle, monkeypatch, which):
    """Ties pass: a kept layer-2 candidate whose value equals a DoG 3 neighbour (the nine
    comparisons after the first fill) and kept ones that equal a DoG 1 / DoG 2 neighbour (the
    walk's 17-neighbour test).  The ties are asserted here on the oracle's planes; a > or < in
    either place would drop those candidates and their keypoints."""
    _force_scatter(monkeypatch)
    img = _tie3_image(oracle) if which == "dog3" else _tie12_image(oracle)
    ties = _tie_counts(oracle, img)
    assert ties["partial"] > ties["kept"] > 0, ties
    assert ties["tie3_kept" if which == "dog3" else "tie12_kept"] >= 1, ties
    refs = [_ref(oracle, ("tie", which), lambda: img),
            _ref(oracle, ("synth", 71, img.shape), lambda: oracle.synth_image(71, *img.shape))]
    assert len(refs[0][1]) > 0
    if which == "dog3":  # the tied candidate is not refined away: its keypoint is in the reference
        k = refs[0][1]
        at = (k["octave"] & 0xffff) == (2 << 8)
        assert (at & (np.abs(k["x"] - 35) < 1) & (np.abs(k["y"] - 22) < 1)).any()
    with siftgpu.Context(*img.shape, 2, device=0) as ctx:
        _check_batch(_run_batch(ctx, [r[0] for r in refs]), [(r[1], r[2]) for r in refs], f"ties {which}")


def test_sparse_capacity_and_dense_entry_points(siftgpu, oracle, monkeypatch):
    """A candidate capacity below the partial candidates trips the workspace
    status (no overflow); after that, and after a sparse batch call, the
    pyramid entry point of the same context returns the dense plane 4, and the
    batch call is right again."""
    _force_scatter(monkeypatch)
    shape, B = (160, 200), 2
    refs = [_ref(oracle, ("synth", 70 + b, shape), lambda b=b: oracle.synth_image(70 + b, *shape)) for b in range(B)]
    imgs = [r[0] for r in refs]
    want = [(r[1], r[2]) for r in refs]
    with siftgpu.Context(*shape, B, device=0) as ctx:
        _check_batch(_run_batch(ctx, imgs), want, "before")
        ctx.set_candidate_capacity(8)
        with pytest.raises(siftgpu.SiftError) as e:
            _run_batch(ctx, imgs)
        assert e.value.code == siftgpu.SIFT_E_WORKSPACE
        ctx.set_candidate_capacity(A.default_candidate_capacity(*shape))
        _check_batch(_run_batch(ctx, imgs), want, "after the overflow")
        gp = ctx.buildGaussianPyramid(imgs[1], 5)
        for i, (p, q) in enumerate(zip(gp, oracle.split_planes(oracle.build_gaussian_pyramid(imgs[1]), *shape, 5, 5))):
            assert_bits_equal(p, q, f"pyramid plane {i} after a sparse batch call")
        _check_batch(_run_batch(ctx, imgs), want, "after the pyramid call")
