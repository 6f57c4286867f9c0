"""GPU tests of the first fill's list and of the group order in which the
plane-4 kernels of the sparse flow serve it: 21-slot groups handed out to a
resident grid, each XCD (blocks b, b + 8, ...) taking a contiguous eighth.
SIFT_HIP_G4_GRID bounds the grid at 8 or 16 blocks, so small inputs reach
fewer groups than XCDs, empty XCD ranges and striding with a short last group.
Everything is compared bit for bit with the dense blur or the CPU oracle, the
scatter path forced at small sizes as in test_gpu_g4_fill_tail.py.
"""
import numpy as np
import pytest

import adversarial_inputs as A
from conftest import assert_bits_equal, kp_bytes

pytestmark = pytest.mark.gpu

GROUP = 21   # slots per wave pass
GRIDS = [None, 8, 16]   # SIFT_HIP_G4_GRID: the resident grid, one block per XCD, two

_refs = {}


def _ref(oracle, key, make):
    """(image, oracle keypoints, oracle descriptors), once per run."""
    if key not in _refs:
        img = make()
        kps, desc = oracle.sift(img)
        _refs[key] = (img, kps, desc)
    return _refs[key]


def _synth(oracle, seed, shape):
    return _ref(oracle, ("synth", seed, shape), lambda: oracle.synth_image(seed, *shape))


def _flat(oracle, shape):
    return _ref(oracle, ("constant", shape), lambda: A.IMAGE_FAMILIES["constant"](*shape))


def _partials(oracle, ref):
    """Partial candidates of the image, from the oracle's Gaussian planes over
    every octave: layer-2 pixels of rows 5 .. r - 6 and columns 5 .. c - 6
    (SIFT_IMG_BORDER) that pass the threshold and their 17 neighbours in DoG 1
    and DoG 2, with the reference's >= / <= rule.  With every octave sparse
    these are the first fill's slots."""
    key = ("partial", id(ref[0]))
    if key in _refs:
        return _refs[key]
    R, C = ref[0].shape
    g = oracle.split_planes(oracle.build_gaussian_pyramid(ref[0], 5), R, C, 5, 5)

    def nb(a, skip_centre):
        sh = [a[1 + dy:a.shape[0] - 1 + dy, 1 + dx:a.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)
              if not (skip_centre and dy == 0 and dx == 0)]
        return np.maximum.reduce(sh), np.minimum.reduce(sh)
    n = 0
    for o in range(5):
        G = g[5 * o:5 * o + 5]
        r, c = G[0].shape
        if r < 11 or c < 11:
            continue  # no pixel inside the border
        d1, d2 = G[2] - G[1], G[3] - G[2]   # float32: the reference's own subtraction
        v = d2[1:-1, 1:-1]
        (m1x, m1n), (m2x, m2n) = nb(d1, False), nb(d2, True)
        inside = np.zeros_like(v, bool)
        inside[4:r - 6, 4:c - 6] = True
        px, pn = np.maximum(m1x, m2x), np.minimum(m1n, m2n)
        n += int((inside & (np.abs(v) > 8) & (((v > 0) & (v >= px)) | ((v < 0) & (v <= pn)))).sum())
    _refs[key] = n
    return n


def _setup(monkeypatch, grid, sym_min=0):
    monkeypatch.setenv("SIFT_HIP_SYM_MIN", str(sym_min))
    monkeypatch.setenv("SIFT_HIP_SYM_ROWS_MIN", "0")
    if grid is None:
        monkeypatch.delenv("SIFT_HIP_G4_GRID", raising=False)
    else:
        monkeypatch.setenv("SIFT_HIP_G4_GRID", str(grid))


def _enqueue(ctx, imgs, cap=30000):
    import torch
    B = len(imgs)
    R, C = imgs[0].shape
    buf = torch.from_numpy(np.ascontiguousarray(np.stack(imgs), np.float32)).cuda()
    kpts = torch.full((cap, 7), -1, dtype=torch.int32, device="cuda")
    desc = torch.full((cap, 128), -1.0, dtype=torch.float32, device="cuda")
    offs = torch.full((B + 1,), -1, dtype=torch.int32, device="cuda")
    ctx.detect_compute_batch(buf.data_ptr(), B, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                             offs.data_ptr())
    return buf, offs, kpts, desc


def _run_batch(ctx, imgs, cap=30000):
    _, offs, kpts, desc = _enqueue(ctx, imgs, cap)
    ctx.sync()
    return offs.cpu().numpy(), kpts.cpu().numpy().view(np.uint8).reshape(cap, 28), desc.cpu().numpy()


def _check_batch(out, refs, what):
    o, k, d = out
    assert o[0] == 0
    for b, r in enumerate(refs):
        kr, dr = r[1], r[2]
        assert o[b + 1] - o[b] == len(kr), f"{what} image {b}: {o[b + 1] - o[b]} keypoints, expected {len(kr)}"
        assert_bits_equal(k[o[b]:o[b + 1]], kp_bytes(kr), f"{what} image {b} keypoints")
        assert_bits_equal(d[o[b]:o[b + 1]], dr, f"{what} image {b} descriptors")
    assert np.all(k[o[len(refs)]:].view(np.int32) == -1), f"{what}: keypoint writes past the total"


# ---- 1. the group assignment through the test entry ----------------------------
_R, _C = 70, 90
_COUNTS = [0, 1, GROUP - 1, GROUP, GROUP + 1, 8 * GROUP - 1, 8 * GROUP, 8 * GROUP + 1, _R * _C]


def _dense4(oracle):
    if "dense4" not in _refs:
        img = oracle.synth_image(3, _R, _C)
        _refs["dense4"] = (img, oracle.split_planes(oracle.build_gaussian_pyramid(img, 1), _R, _C, 1, 5)[4])
    return _refs["dense4"]


def _expected_patches(dense, rc):
    """[n, 3, 3]: the dense plane around each in-plane point (every test point has its 3x3 in the plane or is
    checked entry by entry)."""
    pad = np.full((_R + 2, _C + 2), np.nan, np.float32)
    pad[1:-1, 1:-1] = dense
    return np.stack([pad[r:r + 3, c:c + 3] for r, c in rc]) if len(rc) else np.zeros((0, 3, 3), np.float32)


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid{g}")
def test_points_group_counts(siftgpu, oracle, monkeypatch, grid):
    """0 .. 8 * 21 + 1 points and every pixel of the plane (300 groups: striding at 8 and 16 blocks, the last
    XCD's range short): every in-plane patch entry is the dense plane's float, whatever block served it."""
    _setup(monkeypatch, grid)
    img, dense = _dense4(oracle)
    every = np.array([(r, c) for r in range(_R) for c in range(_C)], np.int32)
    rng = np.random.default_rng(5)
    with siftgpu.Context(_R, _C, 1, device=0) as ctx:
        plane0 = ctx.buildGaussianPyramid(img, 1)[0]
        for n in _COUNTS:
            rc = every if n == len(every) else every[rng.permutation(len(every))[:n]]
            got = ctx.selftest_g4_points(plane0, rc).reshape(len(rc), 3, 3)
            want = _expected_patches(dense, rc)
            inside = ~np.isnan(want)
            assert np.isfinite(got).all()
            bad = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & inside)
            assert len(bad) == 0, (grid, n, bad[:5], len(bad))


# ---- 2. the batch call ------------------------------------------------------------
_BATCHES = {
    "two": ((97, 131), [("synth", 0), ("synth", 2)], 0),
    "three": ((97, 131), [("synth", 16), ("synth", 36), ("synth", 12)], 0),
    "flat_between": ((97, 131), [("synth", 0), ("flat", 0), ("synth", 2)], 0),
    "mixed_octaves": ((160, 200), [("synth", 70), ("synth", 71), ("synth", 72)], 6),  # octaves 0, 1 sparse
}


def _batch_refs(oracle, shape, spec):
    return [_synth(oracle, s, shape) if kind == "synth" else _flat(oracle, shape) for kind, s in spec]


@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"grid{g}")
@pytest.mark.parametrize("name", list(_BATCHES))
def test_batch_through_the_list(siftgpu, oracle, monkeypatch, name, grid):
    shape, spec, sym_min = _BATCHES[name]
    _setup(monkeypatch, grid, sym_min)
    refs = _batch_refs(oracle, shape, spec)
    with siftgpu.Context(*shape, len(refs), device=0) as ctx:
        for rep in range(2):  # the second call replays the captured sequence
            _check_batch(_run_batch(ctx, [r[0] for r in refs]), refs, f"{name} grid {grid} call {rep}")
            first = ctx.g4_fill_stats()[0]
            if sym_min == 0:  # every octave sparse: the list holds every partial candidate
                assert first == sum(_partials(oracle, r) for r in refs), (name, grid, rep)
            else:
                assert 0 < first < sum(_partials(oracle, r) for r in refs)


def test_list_counter_resets(siftgpu, oracle, monkeypatch):
    """A textured batch, then a constant one on the same context: the list's
    length and the other counters start the second call at 0, so nothing of the
    first call's list is served again; then the textured batch once more."""
    _setup(monkeypatch, 16)
    shape = (97, 131)
    tex = [_synth(oracle, 0, shape), _synth(oracle, 2, shape)]
    flat = [_flat(oracle, shape)] * 2
    with siftgpu.Context(*shape, 2, device=0) as ctx:
        _check_batch(_run_batch(ctx, [r[0] for r in tex]), tex, "textured")
        s_tex = ctx.g4_fill_stats()
        assert s_tex[0] == sum(_partials(oracle, r) for r in tex) > 0
        _check_batch(_run_batch(ctx, [r[0] for r in flat]), flat, "constant")
        assert ctx.g4_fill_stats() == (0, 0, 0)
        _check_batch(_run_batch(ctx, [r[0] for r in tex]), tex, "textured again")
        assert ctx.g4_fill_stats() == s_tex


@pytest.mark.parametrize("per_image", [8, 150])
def test_capacity_below_the_candidates(siftgpu, oracle, monkeypatch, per_image):
    """Fewer candidate slots than candidates (16: no layer-2 slot below the
    capacity, an empty list; 300: the cut falls among them): the workspace status, a list that
    holds only slots below the capacity (no slot past it is filled or read),
    and the oracle's output again once the capacity is back."""
    _setup(monkeypatch, None)
    shape, B = (160, 200), 2
    refs = [_synth(oracle, 70 + b, shape) for b in range(B)]
    imgs = [r[0] for r in refs]
    with siftgpu.Context(*shape, B, device=0) as ctx:
        ctx.set_candidate_capacity(per_image)
        keep = _enqueue(ctx, imgs)
        with pytest.raises(siftgpu.SiftError) as e:
            ctx.sync()
        assert e.value.code == siftgpu.SIFT_E_WORKSPACE
        first, waiting, most = ctx.g4_fill_stats()
        print(f"capacity {per_image} x {B}: first {first} waiting {waiting} most fills {most}")
        # (a slot of another layer can wait too, so the waiting count is not bounded by the first fill's)
        assert 0 <= first <= per_image * B and 0 <= waiting <= per_image * B
        del keep
        ctx.set_candidate_capacity(A.default_candidate_capacity(*shape))
        _check_batch(_run_batch(ctx, imgs), refs, f"after the overflow at {per_image}")
        assert ctx.g4_fill_stats()[0] == sum(_partials(oracle, r) for r in refs)
