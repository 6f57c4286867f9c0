"""GPU tests of the sparse flow's two kernels after the first step: the first
fill (g4_fill_kernel, through selftest_g4_points) at the seams of its chunk and
group sizes, and the waiting list with its one tail launch (g4_tail_kernel)
at every depth a slot can reach.  Everything is compared bit for bit with the
CPU oracle through the batch call, the scatter path forced at small sizes as in
test_gpu_sparse_g4.py; Context.g4_fill_stats() tells what the kernels did.
"""
import numpy as np
import pytest

import adversarial_inputs as A
from conftest import assert_bits_equal, kp_bytes

pytestmark = pytest.mark.gpu

K_MAX_INTERP = 5     # SIFT_MAX_INTERP_STEPS: the most fills one slot can take
GROUP, CHUNK = 21, 256   # slots per wave pass (first fill and tail), slots a first-fill wave scans

_refs = {}


def _ref(oracle, key, make):
    """(image, oracle keypoints, oracle descriptors, extrema_stats), once per run."""
    if key not in _refs:
        img = make()
        kps, desc = oracle.sift(img)
        _refs[key] = (img, kps, desc, oracle.extrema_stats())
    return _refs[key]


def _synth(oracle, seed, shape):
    return _ref(oracle, ("synth", seed, shape), lambda: oracle.synth_image(seed, *shape))


def _flat(oracle, shape):
    return _ref(oracle, ("constant", shape), lambda: A.IMAGE_FAMILIES["constant"](*shape))


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
    for b, r in enumerate(refs):
        kr, dr = r[1], r[2]
        assert o[b + 1] - o[b] == len(kr), f"{what} image {b}: {o[b + 1] - o[b]} keypoints, expected {len(kr)}"
        assert_bits_equal(k[o[b]:o[b + 1]], kp_bytes(kr), f"{what} image {b} keypoints")
        assert_bits_equal(d[o[b]:o[b + 1]], dr, f"{what} image {b} descriptors")
    assert np.all(k[o[len(refs)]:].view(np.int32) == -1), f"{what}: keypoint writes past the total"


# ---- 1. list seams of the first fill ------------------------------------------
_R, _C = 70, 90
# window off the plane on each side, the zero last row and column, the corners, the interior
_SEAM_POINTS = [(0, 0), (0, 45), (35, 0), (_R - 1, _C - 1), (_R - 1, 40), (30, _C - 1), (_R - 2, _C - 2), (35, 45),
                (18, 18), (19, 19), (_R - 20, _C - 20), (1, _C - 2), (_R - 2, 1), (17, 60), (52, 71), (40, 3)]
_OFF_PLANE = [(-1, -1), (_R, _C), (-30, 40), (35, _C + 25)]


def _dense4(oracle):
    if "dense4" not in _refs:
        img = oracle.synth_image(3, _R, _C)
        _refs["dense4"] = (img, oracle.split_planes(oracle.build_gaussian_pyramid(img, 1), _R, _C, 1, 5)[4])
    return _refs["dense4"]


@pytest.mark.parametrize("n", [1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP, 2 * GROUP + 1, 63, 64, 65, CHUNK - 1, CHUNK,
                               CHUNK + 1, CHUNK + GROUP, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1])
def test_first_fill_list_seams(siftgpu, oracle, n):
    """n points -- the seams of the 21-slot pass, the 64 lanes and the 256-slot
    chunk -- then the same points again (repeats) and four points off the plane:
    every in-plane patch entry is the dense plane's float."""
    img, dense = _dense4(oracle)
    rng = np.random.default_rng(n)
    pts = [_SEAM_POINTS[i % len(_SEAM_POINTS)] if i < 2 * len(_SEAM_POINTS) else
           (int(rng.integers(0, _R)), int(rng.integers(0, _C))) for i in range(n)]
    rc = np.array(pts + pts[:min(n, 5)] + _OFF_PLANE, np.int32)
    with siftgpu.Context(_R, _C, 1, device=0) as ctx:
        plane0 = ctx.buildGaussianPyramid(img, 1)[0]
        got = ctx.selftest_g4_points(plane0, rc).reshape(len(rc), 3, 3)
    assert np.isfinite(got).all()
    for i, (r, c) in enumerate(rc[:n + min(n, 5)]):
        for dy in range(3):
            for dx in range(3):
                y, x = r + dy - 1, c + dx - 1
                if 0 <= y < _R and 0 <= x < _C:
                    assert got[i, dy, dx].tobytes() == dense[y, x].tobytes(), (n, i, (r, c), dy, dx)
    off = got[n + min(n, 5):]
    assert off[0, 2, 2] == dense[0, 0] and off[1, 0, 0] == dense[_R - 1, _C - 1]


# ---- 2. tail depth ---------------------------------------------------------------
# (shape, seeds of the batch, fills): the largest fill count of one slot that
# g4_fill_stats reports for the batch (read off the GPU when the test was
# written): 3 on the first; all five on the others -- a slot that moves on
# layer 2 at every iteration and is rejected, the oracle's rej_max_interp
_TAIL_CASES = [((97, 131), (16, 36), 3), ((97, 131), (0, 2), K_MAX_INTERP), ((160, 200), (0, 2, 70), K_MAX_INTERP)]


@pytest.mark.parametrize("shape,seeds,fills", _TAIL_CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tail_depth(siftgpu, oracle, monkeypatch, shape, seeds, fills):
    _force_scatter(monkeypatch)
    refs = [_synth(oracle, s, shape) for s in seeds]
    assert sum(r[3]["moved_rc"] for r in refs) > 0
    if fills == K_MAX_INTERP:
        assert sum(r[3]["rej_max_interp"] for r in refs) > 0
    with siftgpu.Context(*shape, len(refs), device=0) as ctx:
        for rep in range(2):  # the second call replays the captured sequence
            _check_batch(_run_batch(ctx, [r[0] for r in refs]), refs, f"{shape} seeds {seeds} call {rep}")
            first, waiting, most = ctx.g4_fill_stats()
            print(f"tail depth {shape} {seeds} call {rep}: first {first} waiting {waiting} most fills {most}")
            assert first > 0 and waiting > 0 and most == fills


@pytest.mark.parametrize("family", ["stars", "noise_u8", "fractional"])
def test_tail_crafted_families(siftgpu, oracle, monkeypatch, family):
    _force_scatter(monkeypatch)
    shape = (97, 131)
    refs = [_ref(oracle, (family, shape), lambda: A.IMAGE_FAMILIES[family](*shape)), _synth(oracle, 2, shape)]
    with siftgpu.Context(*shape, 2, device=0) as ctx:
        for rep in range(2):
            _check_batch(_run_batch(ctx, [r[0] for r in refs]), refs, f"{family} call {rep}")
        assert ctx.g4_fill_stats()[1] > 0


# ---- 3. empty and single tail --------------------------------------------------------
def test_empty_tail(siftgpu, oracle, monkeypatch):
    """Flat images alone: no candidate, the first fill serves nothing and the tail sees count 0."""
    _force_scatter(monkeypatch)
    shape = (97, 131)
    refs = [_flat(oracle, shape)] * 2
    assert len(refs[0][1]) == 0
    with siftgpu.Context(*shape, 2, device=0) as ctx:
        for rep in range(2):
            _check_batch(_run_batch(ctx, [r[0] for r in refs]), refs, f"flat call {rep}")
            assert ctx.g4_fill_stats() == (0, 0, 0)


_SINGLE = ((97, 131), 12, 1)   # (shape, seed, waiting-list length): one entry (seeds 0..49 read off the GPU)


def test_short_tail(siftgpu, oracle, monkeypatch):
    _force_scatter(monkeypatch)
    shape, seed, want = _SINGLE
    refs = [_synth(oracle, seed, shape), _flat(oracle, shape)]
    with siftgpu.Context(*shape, 2, device=0) as ctx:
        for rep in range(2):
            _check_batch(_run_batch(ctx, [r[0] for r in refs]), refs, f"short tail call {rep}")
            first, waiting, most = ctx.g4_fill_stats()
            print(f"short tail: first {first} waiting {waiting} most fills {most}")
            assert waiting == want and most == 2


# ---- 4. mixed octaves ------------------------------------------------------------------
def test_tail_mixed_octaves(siftgpu, oracle, monkeypatch):
    """sym_min 6 at 160 x 200 x 3: octaves 0 and 1 sparse, the others with a dense
    plane 4, in one candidate list.  Slots of the dense octaves never wait (they
    refine from the dense plane), so the sparse octaves alone make the list:
    shorter than with every octave sparse, and the output is the oracle's."""
    shape = (160, 200)
    refs = [_synth(oracle, 70 + b, shape) for b in range(3)]
    stats = {}
    for sym_min in (6, 0):
        _force_scatter(monkeypatch, sym_min)
        with siftgpu.Context(*shape, 3, device=0) as ctx:
            for rep in range(2):
                _check_batch(_run_batch(ctx, [r[0] for r in refs]), refs, f"sym_min {sym_min} call {rep}")
            stats[sym_min] = ctx.g4_fill_stats()
    print("mixed octaves:", stats)
    assert 0 < stats[6][0] < stats[0][0] and 0 < stats[6][1] <= stats[0][1]


# ---- 5. counter reset --------------------------------------------------------------------
def test_counters_reset_between_calls(siftgpu, oracle, monkeypatch):
    """Two different batches back to back on one context, the second with fewer
    candidates, then the first again: a waiting count left from the earlier
    call would make the tail walk stale entries."""
    _force_scatter(monkeypatch)
    shape = (160, 200)
    big = [_synth(oracle, 70, shape), _synth(oracle, 71, shape)]
    small = [_synth(oracle, 72, shape), _flat(oracle, shape)]
    with siftgpu.Context(*shape, 2, device=0) as ctx:
        _check_batch(_run_batch(ctx, [r[0] for r in big]), big, "first batch")
        s_big = ctx.g4_fill_stats()
        _check_batch(_run_batch(ctx, [r[0] for r in small]), small, "second batch")
        s_small = ctx.g4_fill_stats()
        _check_batch(_run_batch(ctx, [r[0] for r in big]), big, "first batch again")
        assert ctx.g4_fill_stats() == s_big
    assert 0 < s_small[0] < s_big[0] and s_small[1] < s_big[1]
