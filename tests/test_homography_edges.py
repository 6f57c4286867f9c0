"""The homography on crafted inputs, without a GPU (homography_edge_inputs.py):
the host path sift_find_homography against oracle/homography.py on every
segment, bit for bit; the census that shows on the oracle alone that the inputs
reach what they were built for; and update_num_iters -- the one libm-dependent
site -- against a 50-digit evaluation over its whole domain."""
import decimal
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bits_equal

import homography as HO
import homography_edge_inputs as E

CALLS = [c.name for c in E.calls()]


def _segments(c):
    for b, label in enumerate(c.labels):
        lo, hi = int(c.moff[b]), int(c.moff[b + 1])
        yield b, label, c.src[lo:hi], c.dst[lo:hi], lo, hi


def _rows():
    """[(call, label, n, found, mask, census)] over every segment with oracle values."""
    e = E.expected()
    return [(c, label, hi - lo, int(e[c.name][1][b]), e[c.name][2][lo:hi], e[c.name][3][b])
            for c in E.calls() for b, label, _, _, lo, hi in _segments(c) if E.finite_segment(c, b)]


def _row(call, label):
    return next(r for r in _rows() if r[0].name == call and r[1] == label)


@pytest.mark.parametrize("name", CALLS)
def test_host_path_matches_oracle(siftgpu, name):
    c = E.call(name)
    eH, ef, em, _ = E.expected()[name]
    for b, label, s, d, lo, hi in _segments(c):
        h, m = siftgpu.findHomography(s, d, siftgpu.RANSAC, c.thr, None, c.max_iters, c.confidence)
        if not E.finite_segment(c, b):
            # the call returned; a row with a non-finite coordinate is not an inlier
            bad = ~(np.isfinite(s).all(axis=1) & np.isfinite(d).all(axis=1))
            assert bad.any() and not m[bad].any(), (name, label)
            continue
        assert (h is not None) == bool(ef[b]), f"{name} {label}: host found {h is not None}, oracle {ef[b]}"
        if h is not None:
            assert h.reshape(9).tobytes() == eH[b].tobytes(), f"{name} {label}: {h.reshape(9)} != {eH[b]}"
        assert_bits_equal(m, em[lo:hi], f"{name} {label} mask")


def test_oracle_results_are_none_or_finite():
    """x86 and gfx950 generate different NaN bit patterns, and every comparison is bitwise."""
    for c in E.calls():
        H, found, _, _ = E.expected()[c.name]
        assert np.isfinite(H).all(), c.name
        assert (H[found == 0] == 0).all(), c.name


def test_four_pair_fits():
    """n == 4 bypasses check_subset: the outcome of each degenerate quadruple on the oracle."""
    c = E.call("FOUR")
    H, found, mask, _ = E.expected()["FOUR"]
    got = dict(zip(c.labels, found.tolist()))
    assert got == {"identical": 0, "common_dst": 0, "common_x": 0, "collinear": 1, "two_identical": 1, "swapped": 1,
                   "similarity": 1}, got
    assert np.abs(H[c.index("collinear")]).max() > 1e12, "the collinear quadruple's model is no longer meaningless"
    np.testing.assert_allclose(H[c.index("similarity")], E.SIMILARITY_H, rtol=0, atol=1e-9)
    for b in range(len(c.labels)):
        assert (mask[c.moff[b]:c.moff[b + 1]] == found[b]).all()


def test_inputs_census(siftgpu):
    """Each line is a condition on the seeds, shown on the oracle alone."""
    R = siftgpu.HOMOGRAPHY_ROUND
    rows = _rows()
    print("call      segment            n found inliers iters  src  dst flip lm+ lm- refit lm_solve")
    for c, label, n, found, mask, cen in rows:
        rej = cen["rejects"]
        print(f"{c.name:9s} {label:16s} {n:4d} {found:5d} {int(mask.sum()):7d} {cen['iterations']:5d} "
              f"{len(rej['src']):4d} {len(rej['dst']):4d} {len(rej['flip']):4d} {cen['lm_accepted']:3d} "
              f"{cen['lm_rejected']:3d} {'fails' if cen['refit_failed'] else 'ok':>5s} "
              f"{'fails' if cen['lm_solve_failed'] else 'ok':>8s}")
    # every segment ends within a few hundred iterations: the oracle stays quick
    assert max(cen["iterations"] for *_, cen in rows) <= 300
    # inliers against the refit's 64-pair chunks
    m = _row("PLACED", "first64_out")[4]
    assert not m[:64].any() and m[64:].sum() > 64, "first64_out: an inlier among the first 64 rows"
    m = _row("PLACED", "tail_only")[4]
    assert len(m) % 64 and not m[:64 * (len(m) // 64)].any() and m[64 * (len(m) // 64):].any(), \
        "tail_only: inliers outside the last, partial chunk"
    m = _row("PLACED", "last_row_in")[4]
    assert len(m) % 64 == 1 and m[-1] == 1, "last_row_in: the last row is not an inlier"
    assert _row("PLACED", "in64")[4].sum() == 64, "in64: not exactly 64 inliers"
    assert _row("PLACED", "in65")[4].sum() == 65, "in65: not exactly 65 inliers"
    for n in E.SEAM_SIZES:      # a mask write that skips row 0 or row n - 1 shows
        m = _row("SEAMS", f"n{n}")[4]
        assert m[0] == 1 and m[-1] == 1 and not m.all(), f"n{n}: the first and the last row must be inliers"
    # get_subset's retry path in the middle of a run, for each reason
    for why in ("src", "dst", "flip"):
        assert any(found and any(it > 0 for it in cen["rejects"][why]) for _, _, _, found, _, cen in rows), \
            f"no subset rejected in mid-run for {why}"
    assert any(cen["lm_accepted"] for *_, cen in rows) and any(cen["lm_rejected"] for *_, cen in rows)
    cen = _row("DUPS", "three_positions")
    assert cen[3] == 0 and cen[5]["iterations"] == 0 and len(cen[5]["rejects"]["src"]) == 10000
    for cap in (1, 63, 64, 65):
        assert _row(f"CAP{cap}", "long")[5]["iterations"] == cap, f"max_iters = {cap} is not reached"
    assert {1, 63, 64, 65} & {R - 1, R, R + 1} == {63, 64, 65}
    # thr: 0 admits no pair, -3 is 3, 1e30 squared is +inf in float and admits every pair after one hypothesis
    assert all(_row("THR0", k)[3] == 0 for k in ("clean", "out30"))
    cn = E.call("THRNEG")
    for b, label, s, d, lo, hi in _segments(cn):
        h, m, _ = E.oracle(s, d, 3.0, cn.max_iters, cn.confidence)
        assert h == list(E.expected()["THRNEG"][0][b]) and (m == E.expected()["THRNEG"][2][lo:hi]).all()
    for k in ("clean", "out30"):
        _, _, n, found, mask, cen = _row("THRBIG", k)
        assert found and mask.all() and cen["iterations"] == 1 and cen["updates"][0][1] == 0.0, k
    # the branches no ordinary input reaches
    assert _row("DEGEN", "refit_fails")[5]["refit_failed"] and not _row("DEGEN", "refit_fails")[5]["lm_solve_failed"]
    assert _row("DEGEN", "lm_fails")[5]["refit_failed"] and _row("DEGEN", "lm_fails")[5]["lm_solve_failed"]
    assert all(_row("DEGEN", k)[3] == 1 and _row("DEGEN", k)[4].sum() == 4 for k in ("refit_fails", "lm_fails"))
    # run_kernel never fails on a subset that check_subset accepted (DESIGN.md 6b says why)
    assert not any(cen["kernel_failures"] for *_, cen in rows)


def test_perspective_transform_at_the_limit(siftgpu):
    """(0, 0) when |w| <= FLT_EPSILON: on the limit, one float below and one above."""
    H, pts = E.transform_limit_case()
    out = siftgpu.perspectiveTransform(pts, H)
    assert_bits_equal(out, HO.perspective_transform(list(H), pts), "host transform")
    assert (out[:4] == 0).all() and (out[4:] != 0).any(axis=1).all(), out


# ---- update_num_iters over its domain ---------------------------------------------
D = decimal.Decimal
HALF_MARGIN, COMPARE_MARGIN = D("1e-6"), D("1e-7")


def _exact_update(conf, ep, max_iters):
    """update_num_iters evaluated in the current decimal context from the same doubles -> (result, |q - nearest half-integer| or
    None, relative gap of the max_iters comparison or None)."""
    num = max(1 - D(conf), D(HO.DBL_MIN))
    denom = 1 - (1 - D(ep)) ** 4
    if denom < D(HO.DBL_MIN):
        return 0, None, None
    a, b = -num.ln(), max_iters * -denom.ln()
    gap = abs(a - b) / max(a, b)
    if a >= b:
        return max_iters, None, gap
    q = a * max_iters / b
    return int(q.to_integral_value(decimal.ROUND_HALF_EVEN)), abs(q - int(q) - D("0.5")), gap


def test_update_num_iters_over_its_domain():
    """The oracle's update_num_iters equals the correctly rounded result for every
    (n - good) / n with n = 5..512, and no input is near a decision point: the
    quotient stays 1e-6 from every half-integer and the two sides of the
    max_iters comparison 1e-7 apart (relative).  A libm that is an ulp off in
    pow or log moves the quotient by about 1e-13, so device, host and oracle
    agree on all of it; test_gpu_homography_edges.py evaluates the device."""
    good, n = E.sweep()
    eps = sorted({(int(k) - int(g)) / int(k) for g, k in zip(good, n)})
    assert eps[0] == 0.0 and eps[-1] < 1.0 and len(eps) > 50000
    for conf, max_iters in E.SWEEP_PARAMS:
        closest_half, closest_cmp = (D(1), None), (D(1), None)
        for ep in eps:
            with decimal.localcontext(decimal.Context(prec=50)):
                r, half, gap = _exact_update(conf, ep, max_iters)
            assert HO.update_num_iters(conf, ep, 4, max_iters) == r, (conf, max_iters, ep, r)
            if half is not None and half < closest_half[0]:
                closest_half = (half, ep)
            if gap is not None and gap < closest_cmp[0]:
                closest_cmp = (gap, ep)
        print(f"confidence {conf} max_iters {max_iters}: closest half-integer approach {float(closest_half[0]):.3g} "
              f"at ep = {closest_half[1]!r}; closest max_iters comparison {float(closest_cmp[0]):.3g} (relative) "
              f"at ep = {closest_cmp[1]!r}")
        assert closest_half[0] >= HALF_MARGIN, closest_half
        assert closest_cmp[0] >= COMPARE_MARGIN, closest_cmp


def test_host_update_num_iters_over_its_domain(tmp_path):
    """homography_math.hpp's update_num_iters, compiled for the host
    (tests/cpp/update_num_iters_sweep.cpp), equals the oracle on the same sweep."""
    exe = tmp_path / "update_num_iters_sweep"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                    "-I", os.path.join(ROOT, "sift-gpu_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "update_num_iters_sweep.cpp"), "-o", str(exe)], check=True)
    good, n = E.sweep()
    for conf, max_iters in E.SWEEP_PARAMS:
        r = subprocess.run([str(exe), repr(conf), str(max_iters)], capture_output=True, check=True)
        got = np.frombuffer(r.stdout, np.int32)
        want = np.array([HO.update_num_iters(conf, (int(k) - int(g)) / int(k), 4, max_iters) for g, k in zip(good, n)],
                        np.int32)
        assert_bits_equal(got, want, f"host update_num_iters, confidence {conf}, max_iters {max_iters}")
