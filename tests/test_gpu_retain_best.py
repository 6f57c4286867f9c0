"""GPU tests of the per-image keypoint budget (sift_set_max_features): every
output is compared bit for bit -- keypoint bytes, descriptor bits, offsets, and
that nothing past the total is written -- with the numpy rule of
tests/retain_best_inputs.py applied to the CPU oracle's unlimited output (to
the context's own unlimited output under SIFT_FLAG_FAST, which is not
bit-exact).  test_retain_best.py asserts that these inputs cut where the cases
say they do."""
import numpy as np
import pytest

import adversarial_inputs as A
import retain_best_inputs as R
from conftest import assert_bits_equal, kp_bytes

pytestmark = pytest.mark.gpu

CAP = 4000
FORMS = {"block": str(1 << 40), "grid": "0"}   # SIFT_HIP_SELECT_BLOCK_MAX: candidate slots per image up to which
#                                                one workgroup per image selects; 0 = always the multi-workgroup form
_refs = {}


def _ref(oracle, key, make):
    """(image, oracle keypoints, oracle descriptors), once per run and never changed."""
    if key not in _refs:
        img = make()
        kps, desc = oracle.sift(img)
        _refs[key] = (img, kps, desc)
    return _refs[key]


def _synth(oracle, seed, shape=R.SHAPE):
    return _ref(oracle, ("synth", seed, shape), lambda: oracle.synth_image(seed, *shape))


def _batch3(oracle):
    """{synth 0, constant, synth 2}: the image without keypoints in the middle."""
    return [_synth(oracle, 0), _ref(oracle, "constant", R.constant_image), _synth(oracle, 2)]


def _tiled(oracle):
    return _ref(oracle, "tiled", lambda: R.tiled_image(oracle))


def _limited(refs, n):
    return [(r[0],) + R.filter_keypoints(r[1], r[2], n) for r in refs]


def _enqueue(ctx, imgs, cap=CAP, bufs=None):
    import torch
    B = len(imgs)
    R_, C_ = imgs[0].shape
    buf = torch.from_numpy(np.ascontiguousarray(np.stack(imgs), np.float32)).cuda()
    if bufs is None:
        bufs = (torch.empty((cap, 7), dtype=torch.int32, device="cuda"),
                torch.empty((cap, 128), dtype=torch.float32, device="cuda"),
                torch.empty((B + 1,), dtype=torch.int32, device="cuda"))
    kpts, desc, offs = bufs
    kpts.fill_(-1)
    desc.fill_(-1.0)
    offs.fill_(-1)
    torch.cuda.synchronize()  # the fills ran on torch's stream, the call runs on the context's
    ctx.detect_compute_batch(buf.data_ptr(), B, R_, C_, C_, R_ * C_, kpts.data_ptr(), desc.data_ptr(), cap,
                             offs.data_ptr())
    return buf, bufs


def _run(ctx, imgs, cap=CAP, bufs=None):
    _, (kpts, desc, offs) = _enqueue(ctx, imgs, cap, bufs)
    ctx.sync()
    return offs.cpu().numpy(), kpts.cpu().numpy().view(np.uint8).reshape(cap, 28), desc.cpu().numpy()


def _check(out, refs, what):
    """test_gpu_g4_groups.py::_check_batch, and the descriptor rows past the total too."""
    o, k, d = out
    assert o[0] == 0
    for b, r in enumerate(refs):
        kr, dr = r[1], r[2]
        assert o[b + 1] - o[b] == len(kr), f"{what} image {b}: {o[b + 1] - o[b]} keypoints, expected {len(kr)}"
        assert_bits_equal(k[o[b]:o[b + 1]], kp_bytes(kr), f"{what} image {b} keypoints")
        assert_bits_equal(d[o[b]:o[b + 1]], dr, f"{what} image {b} descriptors")
    assert np.all(k[o[len(refs)]:].view(np.int32) == -1), f"{what}: keypoint writes past the total"
    assert np.all(d[o[len(refs)]:] == -1.0), f"{what}: descriptor writes past the total"


# ---- 1. the batch ---------------------------------------------------------------------
@pytest.mark.parametrize("n", R.BATCH_N)
def test_batch(siftgpu, oracle, n):
    refs = _batch3(oracle)
    with siftgpu.Context(*R.SHAPE, 3, device=0) as ctx:
        ctx.set_max_features(n)
        for rep in range(2):  # the second call replays the captured sequence
            _check(_run(ctx, [r[0] for r in refs]), _limited(refs, n), f"n {n} call {rep}")


# ---- 2. ties at the cut across distinct candidates -----------------------------------
@pytest.mark.parametrize("where", ["alone", "middle"])
def test_ties(siftgpu, oracle, where):
    t = _tiled(oracle)
    ties = R.tie_budgets(t[1])
    assert len(ties) >= 1
    side = _ref(oracle, ("synth", 9, R.TILED_SHAPE), lambda: oracle.synth_image(9, *R.TILED_SHAPE))
    refs = [t] if where == "alone" else [side, t, side]
    imgs = [r[0] for r in refs]
    import torch
    bufs = (torch.empty((CAP, 7), dtype=torch.int32, device="cuda"),
            torch.empty((CAP, 128), dtype=torch.float32, device="cuda"),
            torch.empty((len(refs) + 1,), dtype=torch.int32, device="cuda"))
    with siftgpu.Context(*R.TILED_SHAPE, len(refs), device=0) as ctx:
        for n in ties:
            ctx.set_max_features(n)
            want = _limited(refs, n)
            assert len(want[len(refs) // 2][1]) > n
            _check(_run(ctx, imgs, bufs=bufs), want, f"tiled {where} n {n}")


# ---- 3. the host path ------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 40])
def test_host_path(siftgpu, oracle, n):
    img, kps, desc = _synth(oracle, 0)
    wk, wd = R.filter_keypoints(kps, desc, n)
    assert len(wk) < len(kps)
    with siftgpu.Context(*R.SHAPE, 1, device=0) as ctx:
        ctx.set_max_features(n)
        for rep in range(2):
            gk, gd = ctx.SIFT_NCL(img)   # the one-image kernels; sizing call, then sift_copy_results
            assert_bits_equal(kp_bytes(gk), kp_bytes(wk), f"SIFT_NCL n {n} call {rep} keypoints")
            assert_bits_equal(gd, wd, f"SIFT_NCL n {n} call {rep} descriptors")
        _check(_run(ctx, [img]), [(img, wk, wd)], f"batch of one, n {n}")
        # findScaleSpaceExtrema mirrors the reference function: no budget
        g = ctx.buildGaussianPyramid(img)
        assert len(ctx.findScaleSpaceExtrema(g, ctx.buildDoGPyramid(g))) == len(kps)


# ---- 4. toggling the setting --------------------------------------------------------
def test_toggling(siftgpu, oracle):
    import torch
    refs = _batch3(oracle)
    imgs = [r[0] for r in refs]
    bufs = (torch.empty((CAP, 7), dtype=torch.int32, device="cuda"),
            torch.empty((CAP, 128), dtype=torch.float32, device="cuda"),
            torch.empty((4,), dtype=torch.int32, device="cuda"))
    with siftgpu.Context(*R.SHAPE, 3, device=0) as ctx:
        unlimited = _run(ctx, imgs, bufs=bufs)
        _check(unlimited, refs, "before any budget")
        for n in (10, 0, 20, 10):
            ctx.set_max_features(n)
            out = _run(ctx, imgs, bufs=bufs)
            _check(out, _limited(refs, n), f"toggled to {n}")
            if n == 0:
                for a, b in zip(out, unlimited):
                    assert a.tobytes() == b.tobytes()


def test_stage_is_listed_only_with_a_budget(siftgpu, oracle):
    refs = _batch3(oracle)
    imgs = [r[0] for r in refs]
    with siftgpu.Context(*R.SHAPE, 3, device=0, flags=siftgpu.SIFT_FLAG_PROFILE) as ctx:
        _check(_run(ctx, imgs), refs, "profiled, no budget")
        assert "select_best" not in ctx.stage_stats()
        ctx.set_max_features(10)
        _check(_run(ctx, imgs), _limited(refs, 10), "profiled, n 10")
        st = ctx.stage_stats()
        assert st["select_best"]["launches"] == 1 and "descriptor" in st
        ctx.set_max_features(0)
        _check(_run(ctx, imgs), refs, "profiled, budget off again")
        assert "select_best" not in ctx.stage_stats()


# ---- 5. capacity ----------------------------------------------------------------------
def test_capacity_refers_to_the_kept_keypoints(siftgpu, oracle):
    refs = _batch3(oracle)
    imgs = [r[0] for r in refs]
    n = 10
    want = _limited(refs, n)
    kept, total = sum(len(w[1]) for w in want), sum(len(r[1]) for r in refs)
    assert kept == 20 and total == 120
    with siftgpu.Context(*R.SHAPE, 3, device=0) as ctx:
        ctx.set_max_features(n)
        for cap in (kept, 64):  # below the unlimited total: success
            _check(_run(ctx, imgs, cap=cap), want, f"kp_cap {cap}")
        cap = 13                # below the kept total
        _, (kpts, desc, offs) = _enqueue(ctx, imgs, cap=cap)
        with pytest.raises(siftgpu.SiftError) as e:
            ctx.sync()
        assert e.value.code == siftgpu.SIFT_E_CAPACITY
        o = offs.cpu().numpy()
        assert o.tolist() == [0, 10, 10, 20]   # the true kept total in the last offset
        allk = np.concatenate([kp_bytes(w[1]) for w in want])
        alld = np.concatenate([w[2] for w in want])
        assert_bits_equal(kpts.cpu().numpy().view(np.uint8).reshape(cap, 28), allk[:cap], "first kp_cap keypoints")
        assert_bits_equal(desc.cpu().numpy(), alld[:cap], "first kp_cap descriptors")
        _check(_run(ctx, imgs), want, "after the overflow")


# ---- 6. workspace -----------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_workspace_overflow_stays_the_only_error(siftgpu, oracle, monkeypatch, form):
    """Fewer candidate slots than candidates: the offsets past the capacity are
    clamped by the select as by every other kernel."""
    monkeypatch.setenv("SIFT_HIP_SELECT_BLOCK_MAX", FORMS[form])
    refs = _batch3(oracle)
    imgs = [r[0] for r in refs]
    with siftgpu.Context(*R.SHAPE, 3, device=0) as ctx:
        ctx.set_max_features(10)
        ctx.set_candidate_capacity(8)
        keep = _enqueue(ctx, imgs)
        with pytest.raises(siftgpu.SiftError) as e:
            ctx.sync()
        assert e.value.code == siftgpu.SIFT_E_WORKSPACE
        ctx.sync()   # nothing else is pending
        del keep
        ctx.set_candidate_capacity(A.default_candidate_capacity(*R.SHAPE))
        _check(_run(ctx, imgs), _limited(refs, 10), "after the workspace overflow")


# ---- 7. the select forms ------------------------------------------------------------
@pytest.mark.parametrize("n", R.BATCH_N)
@pytest.mark.parametrize("form", list(FORMS))
def test_select_forms(siftgpu, oracle, monkeypatch, form, n):
    monkeypatch.setenv("SIFT_HIP_SELECT_BLOCK_MAX", FORMS[form])
    refs = _batch3(oracle)
    with siftgpu.Context(*R.SHAPE, 3, device=0) as ctx:
        ctx.set_max_features(n)
        _check(_run(ctx, [r[0] for r in refs]), _limited(refs, n), f"{form} form, n {n}")


@pytest.mark.parametrize("form", list(FORMS))
def test_select_forms_more_than_one_stride(siftgpu, oracle, monkeypatch, form):
    """240 x 320: 470 keypoints from 373 candidates out of more slots than a
    workgroup's 256 threads, so the multi-workgroup form adds the histograms of
    several workgroups per image, and a segment starts inside a workgroup's stride."""
    monkeypatch.setenv("SIFT_HIP_SELECT_BLOCK_MAX", FORMS[form])
    shape = (240, 320)
    refs = [_synth(oracle, 1, shape), _synth(oracle, 0, shape)]
    assert len(refs[0][1]) == 470 and int(R.candidate_ids(refs[0][1]).max()) + 1 == 373
    with siftgpu.Context(*shape, 2, device=0) as ctx:
        for n in (1, 100, 300, 469):
            ctx.set_max_features(n)
            _check(_run(ctx, [r[0] for r in refs], cap=2000), _limited(refs, n), f"{form} form 240 x 320, n {n}")
        ctx.set_max_features(100)
        gk, gd = ctx.SIFT_NCL(refs[0][0])
        wk, wd = R.filter_keypoints(refs[0][1], refs[0][2], 100)
        assert_bits_equal(kp_bytes(gk), kp_bytes(wk), f"{form} form SIFT_NCL keypoints")
        assert_bits_equal(gd, wd, f"{form} form SIFT_NCL descriptors")


# ---- 8. SIFT_FLAG_FAST ----------------------------------------------------------------
def test_fast_flag(siftgpu, oracle):
    refs = _batch3(oracle)
    imgs = [r[0] for r in refs]
    with siftgpu.Context(*R.SHAPE, 3, device=0, flags=siftgpu.SIFT_FLAG_FAST) as ctx:
        o, k, d = _run(ctx, imgs)
        assert o[3] > 50
        own = []
        for b in range(3):
            kk = np.ascontiguousarray(k[o[b]:o[b + 1]]).view(siftgpu.KEYPOINT_DTYPE).reshape(-1)
            own.append((imgs[b], kk, d[o[b]:o[b + 1]].copy()))
        for n in (1, 10, 44):
            ctx.set_max_features(n)
            want = _limited(own, n)
            assert sum(len(w[1]) for w in want) < o[3]
            _check(_run(ctx, imgs), want, f"FAST n {n}")


# ---- 9. bad arguments ------------------------------------------------------------------
def test_bad_arguments(siftgpu, oracle):
    refs = _batch3(oracle)
    with siftgpu.Context(*R.SHAPE, 3, device=0) as ctx:
        with pytest.raises(siftgpu.SiftError) as e:
            ctx.set_max_features(-1)
        assert e.value.code == siftgpu.SIFT_E_INVALID
        _check(_run(ctx, [r[0] for r in refs]), refs, "after set_max_features(-1)")
        ctx.set_max_features(10)
        with pytest.raises(siftgpu.SiftError):
            ctx.set_max_features(-5)
        _check(_run(ctx, [r[0] for r in refs]), _limited(refs, 10), "after a refused change")


# ---- 10. the multi-GPU path ------------------------------------------------------------
def test_multi_context(siftgpu, oracle):
    import torch
    refs = _batch3(oracle)
    imgs = torch.from_numpy(np.ascontiguousarray(np.stack([r[0] for r in refs]), np.float32)).cuda()
    R_, C_ = R.SHAPE
    with siftgpu.Context(*R.SHAPE, 3, device=0) as ctx:
        ctx.set_max_features(10)
        bo, bk, bd = _run(ctx, [r[0] for r in refs])
    _check((bo, bk, bd), _limited(refs, 10), "the batch call")
    torch.cuda.synchronize()
    with siftgpu.MultiContext([0], R_, C_, 3, CAP, gather_desc=True) as m:
        with pytest.raises(siftgpu.SiftError) as e:
            m.set_max_features(-1)
        assert e.value.code == siftgpu.SIFT_E_INVALID
        m.set_max_features(10)
        m.step([imgs.data_ptr()], [3], R_, C_, C_, R_ * C_)
        m.flush()
        kps, desc = m.copy_gathered()
        _, _, offs, _ = m.gathered(4)
    assert offs.tolist() == bo.tolist()
    total = int(bo[3])
    assert kp_bytes(kps).tobytes() == bk[:total].tobytes() and desc.tobytes() == bd[:total].tobytes()
