"""GPU tests of the detection mask (sift_detect_compute_masked,
sift_detect_compute_batch_masked, sift_multi_step_masked, the four-argument
SIFT_NCL of sift.hpp).  Every output is compared bit for bit -- keypoint bytes,
descriptor bits, offsets, and that nothing past the total is written -- with the
numpy rule of tests/detect_mask_inputs.py applied to the unmasked output: the
CPU oracle's in exact mode, the context's own under SIFT_FLAG_FAST, which is not
bit-exact.

The one-image case names two inputs, synth 2 and the stars at 203 x 157.  Neither
alone has what the checkerboard needs to tell the rounding rule from its near
misses (synth 2: 137 distinct positions, fewer than a workgroup's 256 threads;
the stars: no keypoint above octave 0), so a third input of the same shape,
detect_mask_inputs.stars_blobs_image, carries all of the asserted properties and
the two named ones assert the part they have."""
import os
import subprocess

import numpy as np
import pytest

import adversarial_inputs as A
import detect_mask_inputs as M
import retain_best_inputs as R
from conftest import GOLDEN, PKG, ROOT, assert_bits_equal, book_image, kp_bytes, load_golden

pytestmark = pytest.mark.gpu

CAP = 4000
FORMS = {"block": str(1 << 40), "grid": "0"}   # SIFT_HIP_SELECT_BLOCK_MAX: 0 = many workgroups per image
_refs = {}


def _ref(oracle, key, make):
    """(image, oracle keypoints, oracle descriptors), once per run and never changed."""
    if key not in _refs:
        img = make()
        kps, desc = oracle.sift(img)
        _refs[key] = (img, kps, desc)
    return _refs[key]


ONE_IMAGE = {"stars_blobs": lambda o: M.stars_blobs_image(),
             "synth2_203x157": lambda o: o.synth_image(2, *M.SHAPE),
             "ref_stars_203x157": lambda o: A.img_stars(*M.SHAPE)}


def _one(oracle, name):
    return _ref(oracle, name, lambda: ONE_IMAGE[name](oracle))


def _batch_refs(oracle, n=5):
    return [_ref(oracle, ("synth", s, M.BATCH_SHAPE), lambda s=s: oracle.synth_image(s, *M.BATCH_SHAPE))
            for s in range(n)]


def _batch_masks(refs):
    """ones, checkerboard, zeros, half-plane, window: the empty image in the middle."""
    z, o, cb, hp, w = M.batch_masks(M.BATCH_SHAPE, refs[4][1])
    return [o, cb, z, hp, w]


def _masked(refs, masks):
    return [(r[0],) + M.filter_keypoints(r[1], r[2], m) for r, m in zip(refs, masks)]


class Bufs:
    def __init__(self, batch, cap=CAP):
        import torch
        self.cap, self.batch = cap, batch
        self.k = torch.empty((cap, 7), dtype=torch.int32, device="cuda")
        self.d = torch.empty((cap, 128), dtype=torch.float32, device="cuda")
        self.o = torch.empty((batch + 1,), dtype=torch.int32, device="cuda")

    def clear(self):
        import torch
        self.k.fill_(-1)
        self.d.fill_(-1.0)
        self.o.fill_(-1)
        torch.cuda.synchronize()  # the fills ran on torch's stream, the call runs on the context's

    def host(self):
        return (self.o.cpu().numpy(), self.k.cpu().numpy().view(np.uint8).reshape(self.cap, 28), self.d.cpu().numpy())


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def _enqueue(ctx, imgs_t, bufs, masks_t=None, mask_row_stride=None, mask_img_stride=None):
    B, R_, C_ = imgs_t.shape
    bufs.clear()
    if masks_t is None:
        ctx.detect_compute_batch(imgs_t.data_ptr(), B, R_, C_, C_, R_ * C_, bufs.k.data_ptr(), bufs.d.data_ptr(),
                                 bufs.cap, bufs.o.data_ptr())
        return
    rs = masks_t.shape[-1] if mask_row_stride is None else mask_row_stride
    ims = (R_ * masks_t.shape[-1] if masks_t.dim() == 3 else 0) if mask_img_stride is None else mask_img_stride
    ctx.detect_compute_batch(imgs_t.data_ptr(), B, R_, C_, C_, R_ * C_, bufs.k.data_ptr(), bufs.d.data_ptr(),
                             bufs.cap, bufs.o.data_ptr(), masks_ptr=masks_t.data_ptr(), mask_row_stride=rs,
                             mask_img_stride=ims)


def _run(ctx, imgs_t, bufs, masks_t=None, **kw):
    _enqueue(ctx, imgs_t, bufs, masks_t, **kw)
    ctx.sync()
    return bufs.host()


def _check(out, want, what):
    o, k, d = out
    assert o[0] == 0
    for b, r in enumerate(want):
        kr, dr = r[1], r[2]
        assert o[b + 1] - o[b] == len(kr), f"{what} image {b}: {o[b + 1] - o[b]} keypoints, expected {len(kr)}"
        assert_bits_equal(k[o[b]:o[b + 1]], kp_bytes(kr), f"{what} image {b} keypoints")
        assert_bits_equal(d[o[b]:o[b + 1]], dr, f"{what} image {b} descriptors")
    assert np.all(k[o[len(want)]:].view(np.int32) == -1), f"{what}: keypoint writes past the total"
    assert np.all(d[o[len(want)]:] == -1.0), f"{what}: descriptor writes past the total"


def _same(got, want, what):
    gk, gd = got
    assert len(gk) == len(want[0]), f"{what}: {len(gk)} keypoints, expected {len(want[0])}"
    assert_bits_equal(kp_bytes(gk), kp_bytes(want[0]), f"{what} keypoints")
    assert_bits_equal(gd, want[1], f"{what} descriptors")


# ---- 1. one image, the host call ---------------------------------------------------------
@pytest.mark.parametrize("name", list(ONE_IMAGE))
def test_one_image(siftgpu, oracle, name):
    img, kps, desc = _one(oracle, name)
    with siftgpu.Context(*M.SHAPE, 1, device=0) as ctx:   # 5 octaves, the default
        un = ctx.SIFT_NCL(img)
        _same(un, (kps, desc), f"{name} unmasked against the CPU oracle")
        uk = un[0]
        # what lets the checkerboard tell the rule from truncation, from exchanged
        # coordinates and from a single pass of the workgroup: asserted on the unmasked run
        for v in (uk["x"], uk["y"]):
            lo, hi = M.fractions(v)
            assert lo > 0 and hi > 0
        if name != "ref_stars_203x157":
            assert ((uk["octave"] & 255) >= 1).any()
        if name != "synth2_203x157":
            assert M.distinct_positions(uk) > M.MARK_THREADS   # the stride loop runs
        for value in (1, 255, 77):
            _same(ctx.SIFT_NCL(img, mask=M.full(M.SHAPE, value)), un, f"{name} mask of {value}s")
        _same(ctx.SIFT_NCL(img, mask=np.ones(M.SHAPE, bool)), un, f"{name} bool mask of True")
        zk, zd = ctx.SIFT_NCL(img, mask=M.zeros(M.SHAPE))
        assert len(zk) == 0 and zd.shape == (0, 128)
        for mname, mask in (("checkerboard", M.checkerboard(M.SHAPE)), ("half plane", M.half_plane(M.SHAPE)),
                            ("window", M.window_on_keypoints(M.SHAPE, kps))):
            want = M.filter_keypoints(kps, desc, mask)
            assert 0 < len(want[0]) < len(kps), mname
            for rep in range(2):   # the second call replays the captured sequence
                _same(ctx.SIFT_NCL(img, mask=mask), want, f"{name} {mname} call {rep}")
        _same(ctx.SIFT_NCL(img), un, f"{name} unmasked again")
        # sift_find_scale_space_extrema mirrors the reference function: no mask, same count
        g = ctx.buildGaussianPyramid(img)
        assert len(ctx.findScaleSpaceExtrema(g, ctx.buildDoGPyramid(g))) == len(kps)


def test_module_level_call(siftgpu, oracle):
    img, kps, desc = _one(oracle, "synth2_203x157")
    mask = M.checkerboard(M.SHAPE)
    _same(siftgpu.SIFT_NCL(img, mask=mask), M.filter_keypoints(kps, desc, mask), "module SIFT_NCL(image, mask)")
    _same(siftgpu.SIFT_NCL(img, mask != 0), M.filter_keypoints(kps, desc, mask), "module SIFT_NCL, bool mask")
    _same(siftgpu.SIFT_NCL(img), (kps, desc), "module SIFT_NCL(image)")


# ---- 2. padded mask rows -----------------------------------------------------------------
def test_padded_mask_rows(siftgpu, oracle):
    import ctypes
    img, kps, desc = _one(oracle, "synth2_203x157")
    R_, C_ = M.SHAPE
    imgs_t = _dev(img[None])
    bufs = Bufs(1)
    with siftgpu.Context(R_, C_, 1, device=0) as ctx:
        for mname, mask in (("checkerboard", M.checkerboard(M.SHAPE)), ("half plane", M.half_plane(M.SHAPE))):
            want = [(img,) + M.filter_keypoints(kps, desc, mask)]
            pm = M.padded(mask, 37)
            assert pm.shape == (R_, C_ + 37)
            _check(_run(ctx, imgs_t, bufs, _dev(mask)), want, f"packed {mname}")
            _check(_run(ctx, imgs_t, bufs, _dev(pm)), want, f"padded {mname}")
            # the host call with the same padded rows
            n = ctypes.c_int(0)
            hk = np.zeros(len(kps), siftgpu.KEYPOINT_DTYPE)
            hd = np.zeros((len(kps), 128), np.float32)
            rc = ctx._L.sift_detect_compute_masked(ctx.h, img.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), R_, C_, 0,
                                                   pm.ctypes.data, C_ + 37, hk.ctypes.data,
                                                   hd.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(kps),
                                                   ctypes.byref(n))
            assert rc == siftgpu.SIFT_OK
            _same((hk[:n.value], hd[:n.value]), want[0][1:], f"host call, padded {mname}")
        # a row stride below cols: refused, nothing enqueued
        mt = _dev(M.full(M.SHAPE))
        bufs.clear()
        with pytest.raises(siftgpu.SiftError) as e:
            ctx.detect_compute_batch(imgs_t.data_ptr(), 1, R_, C_, C_, R_ * C_, bufs.k.data_ptr(), bufs.d.data_ptr(),
                                     bufs.cap, bufs.o.data_ptr(), masks_ptr=mt.data_ptr(), mask_row_stride=C_ - 1,
                                     mask_img_stride=0)
        assert e.value.code == siftgpu.SIFT_E_INVALID
        ctx.sync()
        assert bufs.o.cpu().numpy().tolist() == [-1, -1]
        n = ctypes.c_int(0)
        m = M.full(M.SHAPE)
        rc = ctx._L.sift_detect_compute_masked(ctx.h, img.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), R_, C_, 0,
                                               m.ctypes.data, C_ - 1, None, None, 0, ctypes.byref(n))
        assert rc == siftgpu.SIFT_E_INVALID
        # without a mask the strides mean nothing
        _check(_run(ctx, imgs_t, bufs), [(img, kps, desc)], "unmasked after the refusals")


# ---- 3. a batch with five different masks --------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_batch_of_five(siftgpu, oracle, monkeypatch, form):
    monkeypatch.setenv("SIFT_HIP_SELECT_BLOCK_MAX", FORMS[form])
    refs = _batch_refs(oracle)
    masks = _batch_masks(refs)
    want = _masked(refs, masks)
    assert len(want[2][1]) == 0 and len(want[0][1]) == len(refs[0][1])
    assert all(0 < len(want[b][1]) < len(refs[b][1]) for b in (1, 3, 4))
    imgs_t = _dev(np.stack([r[0] for r in refs]))
    bufs = Bufs(5)
    with siftgpu.Context(*M.BATCH_SHAPE, 5, device=0) as ctx:
        for rep in range(2):
            _check(_run(ctx, imgs_t, bufs, _dev(np.stack(masks))), want, f"{form}: five masks, call {rep}")
        for shared in (masks[1], masks[3]):   # one mask for all five: mask_img_stride = 0
            _check(_run(ctx, imgs_t, bufs, _dev(shared)), _masked(refs, [shared] * 5), f"{form}: a shared mask")
        _check(_run(ctx, imgs_t, bufs), refs, f"{form}: unmasked")


# ---- 4. capacity -------------------------------------------------------------------------
def test_capacity_refers_to_the_kept_keypoints(siftgpu, oracle):
    import ctypes
    refs = _batch_refs(oracle)
    masks = _batch_masks(refs)
    want = _masked(refs, masks)
    kept, total = sum(len(w[1]) for w in want), sum(len(r[1]) for r in refs)
    assert 20 < kept < total - 20
    imgs_t, masks_t = _dev(np.stack([r[0] for r in refs])), _dev(np.stack(masks))
    allk = np.concatenate([kp_bytes(w[1]) for w in want])
    alld = np.concatenate([w[2] for w in want])
    offs = np.concatenate([[0], np.cumsum([len(w[1]) for w in want])]).tolist()
    with siftgpu.Context(*M.BATCH_SHAPE, 5, device=0) as ctx:
        for cap in (kept, (kept + total) // 2):  # below the unmasked total: success, a clean sync
            _check(_run(ctx, imgs_t, Bufs(5, cap), masks_t), want, f"kp_cap {cap}")
        cap = kept - 7                           # below the kept total
        bufs = Bufs(5, cap)
        _enqueue(ctx, imgs_t, bufs, masks_t)
        with pytest.raises(siftgpu.SiftError) as e:
            ctx.sync()
        assert e.value.code == siftgpu.SIFT_E_CAPACITY
        o, k, d = bufs.host()
        assert o.tolist() == offs                # the true kept total in the last offset
        assert_bits_equal(k, allk[:cap], "first kp_cap keypoints")
        assert_bits_equal(d, alld[:cap], "first kp_cap descriptors")
        _check(_run(ctx, imgs_t, Bufs(5), masks_t), want, "after the overflow")
    # the host call: two-call sizing and sift_copy_results report the kept count
    img, kps, desc = refs[3]
    wk, wd = want[3][1], want[3][2]
    with siftgpu.Context(*M.BATCH_SHAPE, 1, device=0) as ctx:
        n = ctypes.c_int(0)
        fp = ctypes.POINTER(ctypes.c_float)
        rc = ctx._L.sift_detect_compute_masked(ctx.h, img.ctypes.data_as(fp), *M.BATCH_SHAPE, 0, masks[3].ctypes.data,
                                               0, None, None, 0, ctypes.byref(n))
        assert rc == siftgpu.SIFT_E_CAPACITY and n.value == len(wk) < len(kps)
        hk = np.zeros(len(wk), siftgpu.KEYPOINT_DTYPE)
        hd = np.zeros((len(wk), 128), np.float32)
        m = ctypes.c_int(0)
        assert ctx._L.sift_copy_results(ctx.h, hk.ctypes.data, hd.ctypes.data_as(fp), len(wk) - 1,
                                        ctypes.byref(m)) == siftgpu.SIFT_E_CAPACITY and m.value == len(wk)
        assert ctx._L.sift_copy_results(ctx.h, hk.ctypes.data, hd.ctypes.data_as(fp), len(wk),
                                        ctypes.byref(m)) == siftgpu.SIFT_OK and m.value == len(wk)
        _same((hk, hd), (wk, wd), "sift_copy_results after the sizing call")
        # a capacity between the kept and the unmasked count: one call
        hk2 = np.zeros(len(kps) - 1, siftgpu.KEYPOINT_DTYPE)
        hd2 = np.zeros((len(kps) - 1, 128), np.float32)
        rc = ctx._L.sift_detect_compute_masked(ctx.h, img.ctypes.data_as(fp), *M.BATCH_SHAPE, 0, masks[3].ctypes.data,
                                               M.BATCH_SHAPE[1], hk2.ctypes.data, hd2.ctypes.data_as(fp), len(hk2),
                                               ctypes.byref(n))
        assert rc == siftgpu.SIFT_OK and n.value == len(wk)
        _same((hk2[:n.value], hd2[:n.value]), (wk, wd), "host call, capacity below the unmasked count")


# ---- 5. order with the budget -------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_budget_runs_before_the_mask(siftgpu, oracle, monkeypatch, form):
    monkeypatch.setenv("SIFT_HIP_SELECT_BLOCK_MAX", FORMS[form])
    refs = _batch_refs(oracle, 2)
    n = 40
    hp = M.half_plane(M.BATCH_SHAPE)
    want, other = [], []
    for img, kps, desc in refs:
        assert len(kps) > n
        a = M.filter_keypoints(*R.filter_keypoints(kps, desc, n), hp)   # the budget, then the mask
        b = R.filter_keypoints(*M.filter_keypoints(kps, desc, hp), n)   # the other order
        assert kp_bytes(a[0]).tobytes() != kp_bytes(b[0]).tobytes()     # else the order would be untested
        assert len(a[0]) < n                                            # fewer than n although unmasked ones were cut
        want.append((img,) + a)
        other.append((img,) + b)
    imgs_t, bufs = _dev(np.stack([r[0] for r in refs])), Bufs(2)
    with siftgpu.Context(*M.BATCH_SHAPE, 2, device=0) as ctx:
        ctx.set_max_features(n)
        _check(_run(ctx, imgs_t, bufs, _dev(hp)), want, f"{form}: budget {n} and a half plane")
        _same(ctx.SIFT_NCL(refs[0][0], mask=hp), want[0][1:], f"{form}: host call")
        _check(_run(ctx, imgs_t, bufs), [(r[0],) + R.filter_keypoints(r[1], r[2], n) for r in refs],
               f"{form}: budget alone")
        ctx.set_max_features(0)
        _check(_run(ctx, imgs_t, bufs, _dev(hp)), _masked(refs, [hp, hp]), f"{form}: mask alone")


# ---- 6. the graph cache ---------------------------------------------------------------------
def test_graph_cache(siftgpu, oracle):
    """One context, one shape: unmasked, mask A, mask B from another buffer, mask A
    again, unmasked again.  A masked and an unmasked call are two cached
    executables; going from buffer A to buffer B patches the masked one in place
    (sift_graph_stats: one more update, no new executable).  Each result equals
    its SIFT_FLAG_NO_GRAPH twin."""
    refs = _batch_refs(oracle, 3)
    mA = [M.checkerboard(M.BATCH_SHAPE), M.half_plane(M.BATCH_SHAPE), M.full(M.BATCH_SHAPE)]
    mB = [M.half_plane(M.BATCH_SHAPE), M.zeros(M.BATCH_SHAPE), M.checkerboard(M.BATCH_SHAPE, 1)]
    tA, tB = _dev(np.stack(mA)), _dev(np.stack(mB))
    assert tA.data_ptr() != tB.data_ptr()
    imgs_t, bufs = _dev(np.stack([r[0] for r in refs])), Bufs(3)
    steps = [("unmasked", None, refs), ("A", tA, _masked(refs, mA)), ("B", tB, _masked(refs, mB)),
             ("A again", tA, _masked(refs, mA)), ("unmasked again", None, refs)]
    outs, stats = [], []
    with siftgpu.Context(*M.BATCH_SHAPE, 3, device=0) as ctx:
        stats.append(ctx.graph_stats())
        for what, t, want in steps:
            out = _run(ctx, imgs_t, bufs, t)
            _check(out, want, what)
            outs.append(out)
            stats.append(ctx.graph_stats())
        ctx.set_flags(siftgpu.SIFT_FLAG_NO_GRAPH)
        for (what, t, want), g in zip(steps, outs):
            out = _run(ctx, imgs_t, bufs, t)
            for a, b in zip(out, g):
                assert a.tobytes() == b.tobytes(), f"{what}: SIFT_FLAG_NO_GRAPH differs"
        assert ctx.graph_stats() == stats[-1]
    d = [tuple(b - a for a, b in zip(stats[i], stats[i + 1])) for i in range(5)]   # (captures, updates, instantiations)
    assert d[0] == (1, 0, 1), d       # unmasked: a new executable
    assert d[1] == (1, 0, 1), d       # masked: a second entry, not an update of the first
    assert d[2] == (1, 1, 0), d       # buffer A -> buffer B: patched in place, no new executable
    assert d[3] == (1, 1, 0), d       # and back
    assert d[4] == (0, 0, 0), d       # the unmasked entry is still there: replayed as it is


# ---- 7. SIFT_FLAG_FAST, _PROFILE, _VERBOSE ------------------------------------------------------
def test_fast_flag(siftgpu, oracle):
    refs = _batch_refs(oracle, 3)
    masks = [M.checkerboard(M.BATCH_SHAPE), M.half_plane(M.BATCH_SHAPE), M.window_on_keypoints(M.BATCH_SHAPE, refs[2][1], 32)]
    imgs_t, bufs = _dev(np.stack([r[0] for r in refs])), Bufs(3)
    with siftgpu.Context(*M.BATCH_SHAPE, 3, device=0, flags=siftgpu.SIFT_FLAG_FAST) as ctx:
        o, k, d = _run(ctx, imgs_t, bufs)
        assert o[3] > 50
        own = []
        for b in range(3):
            kk = np.ascontiguousarray(k[o[b]:o[b + 1]]).view(siftgpu.KEYPOINT_DTYPE).reshape(-1)
            own.append((refs[b][0], kk, d[o[b]:o[b + 1]].copy()))
        want = _masked(own, masks)
        assert 0 < sum(len(w[1]) for w in want) < o[3]
        _check(_run(ctx, imgs_t, bufs, _dev(np.stack(masks))), want, "FAST")


@pytest.mark.parametrize("flag", ["SIFT_FLAG_PROFILE", "SIFT_FLAG_VERBOSE"])
def test_direct_launch_flags(siftgpu, oracle, flag, capfd):
    refs = _batch_refs(oracle, 3)
    masks = [M.checkerboard(M.BATCH_SHAPE), M.zeros(M.BATCH_SHAPE), M.half_plane(M.BATCH_SHAPE)]
    imgs_t, bufs = _dev(np.stack([r[0] for r in refs])), Bufs(3)
    with siftgpu.Context(*M.BATCH_SHAPE, 3, device=0, flags=getattr(siftgpu, flag)) as ctx:
        _check(_run(ctx, imgs_t, bufs), refs, f"{flag}, unmasked")
        if flag == "SIFT_FLAG_PROFILE":
            assert "detect_mask" not in ctx.stage_stats()
        _check(_run(ctx, imgs_t, bufs, _dev(np.stack(masks))), _masked(refs, masks), f"{flag}, masked")
        if flag == "SIFT_FLAG_PROFILE":
            st = ctx.stage_stats()
            assert st["detect_mask"]["launches"] == 1 and "descriptor" in st and "select_best" not in st
    capfd.readouterr()


# ---- 8. the multi-GPU path -----------------------------------------------------------------
def test_multi_context_two_streams(siftgpu, oracle):
    import torch
    refs = _batch_refs(oracle, 5) + [_ref(oracle, ("synth", 7, M.BATCH_SHAPE),
                                          lambda: oracle.synth_image(7, *M.BATCH_SHAPE))]
    masks = _batch_masks(refs) + [M.checkerboard(M.BATCH_SHAPE, 3)]
    want = _masked(refs, masks)
    R_, C_ = M.BATCH_SHAPE
    imgs_t, masks_t = _dev(np.stack([r[0] for r in refs])), _dev(np.stack(masks))
    with siftgpu.Context(R_, C_, 6, device=0) as ctx:
        bo, bk, bd = _run(ctx, imgs_t, Bufs(6), masks_t)
    _check((bo, bk, bd), want, "the masked batch call")
    torch.cuda.synchronize()
    with siftgpu.MultiContext([0], R_, C_, 6, CAP, gather_desc=True, streams_per_device=2) as m:
        with pytest.raises(siftgpu.SiftError) as e:
            m.step([imgs_t.data_ptr()], [6], R_, C_, C_, R_ * C_, mask_ptrs=[masks_t.data_ptr()],
                   mask_row_stride=C_ - 1, mask_img_stride=R_ * C_)
        assert e.value.code == siftgpu.SIFT_E_INVALID   # refused before anything ran: still usable
        m.step([imgs_t.data_ptr()], [6], R_, C_, C_, R_ * C_, mask_ptrs=[masks_t.data_ptr()], mask_row_stride=C_,
               mask_img_stride=R_ * C_)
        m.flush()
        kps, desc = m.copy_gathered()
        _, _, offs, _ = m.gathered(7)
        assert offs.tolist() == bo.tolist()
        total = int(bo[6])
        assert kp_bytes(kps).tobytes() == bk[:total].tobytes() and desc.tobytes() == bd[:total].tobytes()
        # a NULL entry is no mask on that device; then one mask shared by both sub-batches
        m.step([imgs_t.data_ptr()], [6], R_, C_, C_, R_ * C_, mask_ptrs=[0])
        m.flush()
        _, _, offs, _ = m.gathered(7)
        assert np.diff(offs).tolist() == [len(r[1]) for r in refs]
        shared = _dev(masks[3])
        m.step([imgs_t.data_ptr()], [6], R_, C_, C_, R_ * C_, mask_ptrs=[shared.data_ptr()], mask_row_stride=C_,
               mask_img_stride=0)
        m.flush()
        kps, _ = m.copy_gathered()
        ws = _masked(refs, [masks[3]] * 6)
        assert kp_bytes(kps).tobytes() == np.concatenate([kp_bytes(w[1]) for w in ws]).tobytes()


# ---- 9. the C++ drop-in ------------------------------------------------------------------------
def test_cpp_shim_four_arguments(tmp_path, siftgpu):
    exe = tmp_path / "detect_mask_cli"
    lib = os.path.join(PKG, "lib")
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "detect_mask_cli.cpp"), "-o", str(exe), "-L", lib,
                    "-lsift_shim", "-lsift_hip", f"-Wl,-rpath,{lib}"], check=True)
    out = tmp_path / "out.bin"
    subprocess.run([str(exe), os.path.join(GOLDEN, "book_gray.pgm"), str(out)], check=True, timeout=300)
    raw = out.read_bytes()
    got, at = [], 0
    for _ in range(3):
        n = int(np.frombuffer(raw[at:at + 4], np.int32)[0])
        k = np.frombuffer(raw[at + 4:at + 4 + 28 * n], siftgpu.KEYPOINT_DTYPE)
        d = np.frombuffer(raw[at + 4 + 28 * n:at + 4 + 540 * n], np.float32).reshape(n, 128)
        got.append((k, d))
        at += 4 + 540 * n
    assert at == len(raw)
    g = load_golden("book")
    assert_bits_equal(kp_bytes(got[0][0]), g["kps"], "three-argument keypoints")
    assert_bits_equal(got[0][1], g["desc"], "three-argument descriptors")
    want = M.filter_keypoints(got[0][0], got[0][1], M.half_plane(book_image().shape))
    assert 0 < len(want[0]) < len(got[0][0])
    _same(got[1], want, "four-argument call with the half plane")
    _same(got[2], got[0], "four-argument call with an empty mask")
