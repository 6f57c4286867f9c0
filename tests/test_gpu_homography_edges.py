"""The segmented homography on the GPU (-m gpu) over the crafted inputs of
homography_edge_inputs.py: seam-sized segments, inliers placed against the
refit's chunks, 8K and negative coordinates, duplicates, degenerate quadruples,
thr 0 / -3 / 1e30, max_iters around a round boundary, the refit and lm_solve
failures and non-finite rows.  Every H double, found flag and mask byte equals
oracle/homography.py and the host path; the harness (sentinel-filled outputs)
is test_gpu_homography_batch.py's."""
import numpy as np
import pytest

from conftest import assert_bits_equal

import homography as HO
import homography_edge_inputs as E
from test_gpu_homography_batch import (H_SENT, M_SENT, _check, _homog_device, _host_per_segment,  # noqa: F401
                                       _transform_device)

pytestmark = pytest.mark.gpu
FINITE_CALLS = [c.name for c in E.calls() if c.name != "NONFINITE"]


@pytest.mark.parametrize("name", FINITE_CALLS)
def test_gpu_edges_bitexact_per_call(ctx, siftgpu, name):
    c = E.call(name)
    eH, ef, em, _ = E.expected()[name]
    out = _homog_device(ctx, c.src, c.dst, c.moff, None, c.thr, c.max_iters, c.confidence)
    for b, label in enumerate(c.labels):
        print(f"{name} {label}: n={c.sizes[b]} found={out[1][b]} (oracle {ef[b]})")
    _check(out, (eH, ef, em), c.moff, len(c.src), name)
    _check(out, _host_per_segment(siftgpu, c.src, c.dst, c.moff, len(c.src), c.thr, c.max_iters, c.confidence),
           c.moff, len(c.src), name + " against the host path")
    H2, f2, m2 = _homog_device(ctx, c.src, c.dst, c.moff, None, c.thr, c.max_iters, c.confidence, with_mask=False)
    assert H2.tobytes() == out[0].tobytes() and f2.tobytes() == out[1].tobytes() and (m2 == M_SENT).all()


def test_gpu_nonfinite_segments_are_isolated(ctx, siftgpu):
    """Every loop a NaN reaches is bounded (get_subset by its 10000 attempts, the
    rounds by max_iters, the Jacobi by its 60 sweeps, LM by its 10 steps); the
    host path, the same homography_math.hpp, runs these inputs in
    test_homography_edges.py.  The neighbours equal their stand-alone oracle
    results; the non-finite segments equal the host path in found and mask, and
    in H where it holds no NaN."""
    c = E.call("NONFINITE")
    eH, ef, em, _ = E.expected()["NONFINITE"]
    H, found, mask = _homog_device(ctx, c.src, c.dst, c.moff, None, c.thr, c.max_iters, c.confidence)
    hH, hf, hm = _host_per_segment(siftgpu, c.src, c.dst, c.moff, len(c.src), c.thr, c.max_iters, c.confidence)
    for b, label in enumerate(c.labels):
        lo, hi = int(c.moff[b]), int(c.moff[b + 1])
        print(f"{label}: n={hi - lo} found={found[b]} host {hf[b]} inliers {int(mask[lo:hi].sum())}")
        if E.finite_segment(c, b):
            assert found[b] == ef[b] == 1 and H[b].tobytes() == eH[b].tobytes(), f"{label}: {H[b]} != {eH[b]}"
            assert_bits_equal(mask[lo:hi], em[lo:hi], label + " mask")
        else:
            assert found[b] == hf[b], label
            assert_bits_equal(mask[lo:hi], hm[lo:hi], label + " mask against the host path")
            bad = ~(np.isfinite(c.src[lo:hi]).all(axis=1) & np.isfinite(c.dst[lo:hi]).all(axis=1))
            assert not mask[lo:hi][bad].any(), label + ": a non-finite row is an inlier"
            if not found[b]:
                assert (H[b] == 0).all(), label
            elif np.isfinite(hH[b]).all():
                assert H[b].tobytes() == hH[b].tobytes(), f"{label}: {H[b]} != host {hH[b]}"
    assert (H[len(c.labels):] == H_SENT).all() and (mask[len(c.src):] == M_SENT).all()
    assert found[c.index("all_nan")] == 0 and found[c.index("nan_row")] == 1


def test_gpu_seams_under_an_offset(ctx):
    """The seam sizes once more: three rows before m_offsets[0], a zero-length
    segment before and after each seam segment, and m_cap cutting the last
    segment (257 rows) to 256."""
    c = E.call("SEAMS")
    assert c.sizes[-1] == 257
    pad = np.full((3, 2), 1e6, np.float32)
    src, dst = np.concatenate([pad, c.src]), np.concatenate([pad, c.dst])
    moff = np.concatenate([[3], np.repeat(c.moff[1:] + 3, 2)]).astype(np.int32)
    moff = np.concatenate([[3], moff]).astype(np.int32)       # empty, seam, empty, seam, ..., seam, empty
    sizes = np.diff(moff)
    assert (sizes[0::2] == 0).all() and sizes[1::2].tolist() == c.sizes and len(sizes) == 2 * len(c.sizes) + 1
    m_cap = len(src) - 1
    exp = E.expect_segments(src, dst, moff, m_cap, c.thr, c.max_iters, c.confidence)
    assert exp[1][1::2].all() and not exp[1][0::2].any()
    out = _homog_device(ctx, src, dst, moff, m_cap=m_cap)
    _check(out, exp, moff, m_cap, "seams under an offset")
    assert (out[2][m_cap:] == M_SENT).all() and (out[2][:3] == M_SENT).all()


def test_gpu_transform_at_the_limit(ctx):
    """Points on an H's line at infinity and one float either side of |w| =
    FLT_EPSILON; the 1e15 model of the collinear quadruple; found == 0 between."""
    H, pts = E.transform_limit_case()
    c = E.call("FOUR")
    wild = E.expected()["FOUR"][0][c.index("collinear")]
    assert np.abs(wild).max() > 1e12
    out = _transform_device(ctx, np.stack([H, np.zeros(9), wild]), [1, 0, 1], pts)
    assert_bits_equal(out[0], HO.perspective_transform(list(H), pts), "the limit case")
    assert (out[0][:4] == 0).all() and (out[0][4:] != 0).any(axis=1).all(), out[0]
    assert (out[1] == 0).all()
    assert_bits_equal(out[2], HO.perspective_transform(list(wild), pts), "the collinear quadruple's model")
    assert (out[3] == -5.0).all()


@pytest.mark.parametrize("n_pts", [1, 255, 256, 257])
def test_gpu_transform_across_blocks(ctx, n_pts):
    """3 segments x n_pts: the flat index crosses the 256-thread block boundary inside and between segments."""
    eH, ef, _, _ = E.expected()["SCALE"]
    Hs, found = np.stack([eH[0], eH[1], eH[2]]), [1, 0, 1]
    pts = np.random.default_rng(n_pts).uniform(-100, 8000, (n_pts, 2)).astype(np.float32)
    out = _transform_device(ctx, Hs, found, pts)
    for b in range(3):
        ref = HO.perspective_transform(list(Hs[b]), pts) if found[b] else np.zeros_like(pts)
        assert_bits_equal(out[b], ref, f"segment {b}")
    assert (out[3] == -5.0).all()


@pytest.mark.parametrize("op,conf", [(8, 0.995), (9, 0.5)])
def test_gpu_update_num_iters_over_its_domain(ctx, op, conf):
    """The device's update_num_iters (its own pow and log) equals the oracle's
    on every input of the sweep -- no tolerance."""
    good, n = E.sweep()
    got = ctx.selftest_math(op, good.astype(np.float32), n.astype(np.float32))
    want = np.array([HO.update_num_iters(conf, (int(k) - int(g)) / int(k), 4, 2000) for g, k in zip(good, n)],
                    np.float32)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(int(good[i]), int(n[i]), float(got[i]), float(want[i])) for i in bad[:10]]
