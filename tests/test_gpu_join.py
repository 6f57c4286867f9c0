"""The join of two match tables on a shared keypoint on the GPU (-m gpu), under the
default flags and SIFT_FLAG_NO_GRAPH: the census call of join_inputs.py against
join_oracle.py and the host sift_join_matches per segment, byte for byte, with
sentinels around every output; one table aliased as both sides; records straight
from the ratio stage; and the chain fundamental -> pose recovery -> join -> PnP for
a third view whose rows are not in pair-row order, against the host forms chained
the same way."""
import numpy as np
import pytest

from conftest import assert_bits_equal

import fundamental_inputs as FI
import join_inputs as I
import join_oracle as JO
import pnp_inputs as PI

pytestmark = pytest.mark.gpu
D_SENT, F_SENT, I_SENT, M_SENT = -7.0, -3.0, -77, 0xEE
PAD = 3                                 # spare rows behind every row output
ROWS = ("xyz", "xy", "a_row", "b_row")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _recs(a):
    """A MATCH_DTYPE table as int32 [n, 4] (torch has no structured dtype)."""
    return np.ascontiguousarray(a).view(np.int32).reshape(-1, 4)


def _outputs(j_cap, b_cap, nseg):
    import torch
    return {"xyz": torch.full((j_cap + PAD, 3), D_SENT, dtype=torch.float64, device="cuda"),
            "xy": torch.full((j_cap + PAD, 2), F_SENT, dtype=torch.float32, device="cuda"),
            "a_row": torch.full((j_cap + PAD,), I_SENT, dtype=torch.int32, device="cuda"),
            "b_row": torch.full((j_cap + PAD,), I_SENT, dtype=torch.int32, device="cuda"),
            "b_joined": torch.full((b_cap + 64,), M_SENT, dtype=torch.uint8, device="cuda"),
            "j_offsets": torch.full((nseg + 1 + PAD,), I_SENT, dtype=torch.int32, device="cuda")}


def _join_device(ctx, c, a_side, b_side, optional=True):
    """The census call into sentinel-filled outputs -> dict of numpy arrays; optional False: every
    optional buffer NULL (masks, gathered rows, every output but the offsets)."""
    import torch
    ins = [_dev(_recs(c.a)), _dev(c.a_off), _dev(c.a_mask), _dev(c.a_xyz), _dev(_recs(c.b)), _dev(c.b_off),
           _dev(c.b_mask), _dev(c.b_xy), _dev(c.k_off)]
    keep = [t.clone() for t in ins]
    o = _outputs(c.j_cap, c.b_cap, c.n_segments)
    p = lambda t: t.data_ptr() if optional else None  # noqa: E731
    torch.cuda.synchronize()                  # the context's stream does not wait for torch's
    ctx.join_matches_segmented_device(
        ins[0].data_ptr(), ins[1].data_ptr(), c.a_cap, a_side, p(ins[3]), ins[4].data_ptr(), ins[5].data_ptr(), c.b_cap,
        b_side, p(ins[7]), ins[8].data_ptr(), c.key_cap, c.n_segments, c.j_cap, o["j_offsets"].data_ptr(),
        p(o["xyz"]), p(o["xy"]), p(o["a_row"]), p(o["b_row"]), p(o["b_joined"]), p(ins[2]), p(ins[6]))
    ctx.sync()
    for t, k in zip(ins, keep):               # the inputs are only read
        assert torch.equal(t.view(torch.uint8), k.view(torch.uint8))
    return {k: v.cpu().numpy() for k, v in o.items()}


def _check(out, exp, c, what, rows=True):
    """The offsets are the true counts; the first min(total, j_cap) rows equal the expected ones;
    everything behind them, bytes of b_joined no segment owns and the spare entries keep their
    sentinels."""
    nseg = c.n_segments
    assert_bits_equal(out["j_offsets"][:nseg + 1], exp["j_offsets"], what + " j_offsets")
    assert (out["j_offsets"][nseg + 1:] == I_SENT).all(), what + ": offsets past n_segments + 1 written"
    n = min(int(exp["j_offsets"][-1]), c.j_cap)
    sent = {"xyz": D_SENT, "xy": F_SENT, "a_row": I_SENT, "b_row": I_SENT}
    if not rows:
        for k in ROWS:
            assert (out[k] == sent[k]).all(), f"{what}: {k} written though NULL was passed"
        assert (out["b_joined"] == M_SENT).all(), what + ": b_joined written though NULL was passed"
        return
    for k in ROWS:
        assert_bits_equal(out[k][:n], exp[k][:n], f"{what} {k}")
        assert (out[k][n:] == sent[k]).all(), f"{what}: {k} rows past the joined rows written"
    w = exp["b_written"]
    assert_bits_equal(out["b_joined"][:c.b_cap][w], exp["b_joined"][w], what + " b_joined")
    assert (out["b_joined"][:c.b_cap][~w] == M_SENT).all() and (out["b_joined"][c.b_cap:] == M_SENT).all(), \
        what + ": b_joined bytes outside the segments written"


def _host_expected(siftgpu, c, a_side, b_side):
    """sift_join_matches per segment, put together as join_oracle.join_segmented does."""
    parts, joff = [], [0]
    joined, written = np.zeros(c.b_cap, np.uint8), np.zeros(c.b_cap, bool)
    for s in range(c.n_segments):
        alo, ahi, blo, bhi, nk = I.bounds(c, s)
        xyz, xy, ar, br, bj = siftgpu.joinMatches(c.a[alo:ahi], c.a_xyz[alo:ahi], c.b[blo:bhi], c.b_xy[blo:bhi], nk,
                                                  a_side, b_side, c.a_mask[alo:ahi], c.b_mask[blo:bhi])
        parts.append({"xyz": xyz, "xy": xy, "a_row": ar + np.int32(alo), "b_row": br + np.int32(blo)})
        joined[blo:bhi], written[blo:bhi] = bj, True
        joff.append(joff[-1] + len(br))
    e = {k: np.concatenate([p[k] for p in parts])[:c.j_cap] for k in ROWS}
    e.update(j_offsets=np.array(joff, np.int32), b_joined=joined, b_written=written)
    return e


@pytest.fixture(params=["default", "no_graph"])
def any_ctx(request, ctx, siftgpu):
    """The session context (default flags), and one created with SIFT_FLAG_NO_GRAPH."""
    if request.param == "default":
        yield ctx
        return
    c = siftgpu.Context(64, 64, 1, device=0, flags=siftgpu.SIFT_FLAG_NO_GRAPH)
    yield c
    c.close()


def test_gpu_census_against_oracle_and_host(any_ctx, siftgpu):
    """The 14-segment call under the four settings of the key sides against the oracle and the host
    path; again with every optional buffer NULL; then the host-buffer form."""
    ctx, c = any_ctx, I.call()
    for a_side, b_side in I.SIDES:
        exp = I.expected(a_side, b_side)
        out = _join_device(ctx, c, a_side, b_side)
        print(f"sides {a_side}{b_side}: j_offsets {out['j_offsets'][:c.n_segments + 1].tolist()} (j_cap {c.j_cap})")
        _check(out, exp, c, f"join, sides {a_side}{b_side}")
        _check(out, _host_expected(siftgpu, c, a_side, b_side), c, f"join against the host path, sides {a_side}{b_side}")
    # every optional buffer NULL: no mask takes a row out, and only the offsets are written
    bare = _join_device(ctx, c, 1, 0, optional=False)
    _check(bare, I.expected(1, 0, False), c, "join, optional buffers NULL", rows=False)
    assert bare["j_offsets"][c.n_segments] > I.expected(1, 0)["j_offsets"][-1]
    # the host-buffer form gives the same bytes
    exp = I.expected(1, 0)
    xyz, xy, ar, br, bj, jo = ctx.joinMatchesSegmented(c.a, c.a_off, c.a_xyz, c.b, c.b_off, c.b_xy, c.k_off, 1, 0,
                                                       c.a_mask, c.b_mask, j_cap=c.j_cap, key_cap=c.key_cap)
    assert_bits_equal(jo, exp["j_offsets"], "host form j_offsets")
    for got, k in zip((xyz, xy, ar, br), ROWS):
        assert_bits_equal(got, exp[k], "host form " + k)
    assert_bits_equal(bj, exp["b_joined"], "host form b_joined")     # every B row of the census has an owner
    full = ctx.joinMatchesSegmented(c.a, c.a_off, c.a_xyz, c.b, c.b_off, c.b_xy, c.k_off, 1, 0, c.a_mask, c.b_mask,
                                    key_cap=c.key_cap)
    whole = I.expected(1, 0, True, c.b_cap)
    assert len(full[3]) == whole["j_offsets"][-1] and full[3].tobytes() == whole["b_row"].tobytes()
    assert full[0].tobytes() == whole["xyz"].tobytes()


def test_gpu_entry_point_rules(ctx, siftgpu):
    """With a live context: nothing to do returns SIFT_OK whatever the buffers; a null required
    buffer, a negative count, a bad side and an unaligned table are SIFT_E_INVALID with a message,
    and nothing is enqueued; b_cap == 0 writes offsets of zeros."""
    import torch
    L, h, E = siftgpu.lib(), ctx.h, siftgpu.SIFT_E_INVALID
    buf = torch.full((512,), D_SENT, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    # r: a, a_off, b, b_off, key_off, j_off
    join = lambda r, nseg=1, a_cap=4, b_cap=4, sa=0, sb=1, key_cap=4, j_cap=4, ax=p, bp=p, xo=p, po=p: \
        L.sift_join_matches_segmented_device(h, r[0], r[1], a_cap, sa, None, ax, r[2], r[3], b_cap, sb, None, bp, r[4],
                                             key_cap, nseg, xo, po, None, None, None, j_cap, r[5])  # noqa: E731
    assert join([None] * 6, 0) == 0
    assert L.sift_join_matches_segmented(h, None, None, 0, 0, None, None, None, None, 0, 1, None, None, None, 0, 0, None,
                                         None, None, None, None, 0, None) == 0
    for k in range(6):
        r = [p] * 6
        r[k] = None
        assert join(r) == E and b"null" in L.sift_last_error(h), k
    assert join([p] * 6, ax=None) == E and join([p] * 6, bp=None) == E
    assert join([p] * 6, -1) == E and join([p] * 6, a_cap=-1) == E and join([p] * 6, b_cap=-1) == E
    assert join([p] * 6, key_cap=-1) == E and join([p] * 6, j_cap=-1) == E
    for bad in (-1, 2):
        assert join([p] * 6, sa=bad) == E and join([p] * 6, sb=bad) == E
    assert join([p + 8, p, p, p, p, p]) == E and b"aligned" in L.sift_last_error(h)
    assert L.sift_join_matches_segmented_device(None, p, p, 4, 0, None, p, p, p, 4, 1, None, p, p, 4, 1, p, p, None,
                                                None, None, 4, p) == E
    ctx.sync()
    assert (buf == D_SENT).all()              # nothing was enqueued
    # no B rows: the offsets are zeros, nothing else is written; NULL tables are fine at capacity 0
    joff = torch.full((8,), I_SENT, dtype=torch.int32, device="cuda")
    assert join([None, p, None, p, p, joff.data_ptr()], 3, 0, 0) == 0
    ctx.sync()
    assert joff.cpu().tolist() == [0, 0, 0, 0] + [I_SENT] * 4 and (buf == D_SENT).all()


def _views_table(seed, n_views, per):
    """One table over the pairs of n_views views with about `per` records each: keys below 90."""
    rng = np.random.default_rng(seed)
    sizes = [per + int(d) for d in rng.integers(-9, 9, n_views - 1)]
    t = np.zeros(sum(sizes), I.MATCH)
    t["query"], t["train"] = rng.integers(0, 90, len(t)), rng.integers(0, 90, len(t))
    t["distance"] = rng.integers(0, 9, len(t)).astype(np.float32) / 2
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    keys = np.arange(n_views + 1, dtype=np.int32) * 90
    return t, off, keys, rng.standard_normal((len(t), 3)), rng.random((len(t), 2)).astype(np.float32), \
        (rng.random(len(t)) < 0.8).astype(np.uint8)


def test_gpu_one_table_aliased(any_ctx, siftgpu):
    """Consecutive frames on one table: d_b = d_a, d_b_offsets = d_a_offsets + 1, key offsets + 1, A's key
    its train and B's its query.  Four views of about 120 records per pair; the result equals the same
    join on two separate copies of the table, byte for byte, and the oracle."""
    import torch
    ctx = any_ctx
    t, off, keys, xyz, xy, mask = _views_table(77, 4, 120)
    nseg, cap = len(off) - 2, len(t)
    d = {"t": _dev(_recs(t)), "off": _dev(off), "keys": _dev(keys), "xyz": _dev(xyz), "xy": _dev(xy), "mask": _dev(mask)}
    copy = {"t": d["t"].clone(), "off": _dev(off[1:])}

    def run(b_table, b_off_ptr):
        o = _outputs(cap, cap, nseg)
        torch.cuda.synchronize()
        ctx.join_matches_segmented_device(
            d["t"].data_ptr(), d["off"].data_ptr(), cap, siftgpu.JOIN_TRAIN, d["xyz"].data_ptr(), b_table.data_ptr(),
            b_off_ptr, cap, siftgpu.JOIN_QUERY, d["xy"].data_ptr(), d["keys"].data_ptr() + 4, int(keys[-1]), nseg, cap,
            o["j_offsets"].data_ptr(), o["xyz"].data_ptr(), o["xy"].data_ptr(), o["a_row"].data_ptr(),
            o["b_row"].data_ptr(), o["b_joined"].data_ptr(), d["mask"].data_ptr(), None)
        ctx.sync()
        return {k: v.cpu().numpy() for k, v in o.items()}

    aliased, apart = run(d["t"], d["off"].data_ptr() + 4), run(copy["t"], copy["off"].data_ptr())
    for k in aliased:
        assert aliased[k].tobytes() == apart[k].tobytes(), k
    exp = JO.join_segmented(t, off[:-1], cap, 1, mask, xyz, t, off[1:], cap, 0, None, xy, keys[1:], int(keys[-1]), cap)
    total = int(exp["j_offsets"][-1])
    assert total > 100 and aliased["j_offsets"][:nseg + 1].tolist() == exp["j_offsets"].tolist()
    for k in ROWS:
        assert_bits_equal(aliased[k][:total], exp[k], "aliased " + k)
    # B's rows are the pairs after the first: the first pair's bytes of b_joined keep their sentinel
    assert (aliased["b_joined"][:off[1]] == M_SENT).all()
    assert_bits_equal(aliased["b_joined"][off[1]:cap], exp["b_joined"][off[1]:cap], "aliased b_joined")


def test_gpu_records_from_the_ratio_stage(any_ctx, siftgpu):
    """Three frames of about 200 descriptor rows -> segmented kNN (consecutive frames) -> ratio test
    with keypoints -> the join on its d_matches / d_dst_xy / d_m_offsets, all on the context stream
    with no host value between the calls.  The result is the oracle's on the records read back
    afterwards."""
    import torch
    ctx = any_ctx
    rng = np.random.default_rng(5)
    sizes = [200, 190, 205]
    base = rng.random((230, 128)).astype(np.float32)
    desc, kp = [], []
    for n in sizes:                    # every frame sees a shuffled subset of the base rows, with noise
        rows = rng.permutation(len(base))[:n]
        desc.append(base[rows] + rng.random((n, 128)).astype(np.float32) * 0.05)
        k = np.zeros(n, siftgpu.KEYPOINT_DTYPE)
        k["x"], k["y"] = rng.random(n) * 640, rng.random(n) * 480
        kp.append(k)
    desc, kp = np.concatenate(desc), np.concatenate(kp)
    qoff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    cap, npairs = len(desc), len(sizes) - 1
    d_desc, d_kp, d_qoff = _dev(desc), _dev(kp.view(np.uint8)), _dev(qoff)
    d_idx = torch.full((cap, 2), -1, dtype=torch.int32, device="cuda")
    d_dist = torch.full((cap, 2), float("inf"), dtype=torch.float32, device="cuda")
    d_m = torch.zeros((cap, 4), dtype=torch.int32, device="cuda")
    d_src, d_dst = (torch.zeros((cap, 2), dtype=torch.float32, device="cuda") for _ in range(2))
    d_moff = torch.zeros(npairs + 1, dtype=torch.int32, device="cuda")
    xyz = rng.standard_normal((cap, 3))
    mask = (rng.random(cap) < 0.8).astype(np.uint8)
    d_xyz, d_mask = _dev(xyz), _dev(mask)
    o = _outputs(cap, cap, 1)
    torch.cuda.synchronize()
    ctx.knn_match_segmented_device(d_desc.data_ptr(), d_qoff.data_ptr(), npairs, cap, d_desc.data_ptr(),
                                   d_qoff.data_ptr() + 4, cap, 2, d_idx.data_ptr(), d_dist.data_ptr())
    ctx.ratio_matches_device(d_idx.data_ptr(), d_dist.data_ptr(), d_qoff.data_ptr(), npairs, cap, 0.9, d_kp.data_ptr(),
                             d_kp.data_ptr(), d_qoff.data_ptr() + 4, d_m.data_ptr(), d_src.data_ptr(), d_dst.data_ptr(),
                             cap, d_moff.data_ptr())
    ctx.join_matches_segmented_device(
        d_m.data_ptr(), d_moff.data_ptr(), cap, siftgpu.JOIN_TRAIN, d_xyz.data_ptr(), d_m.data_ptr(),
        d_moff.data_ptr() + 4, cap, siftgpu.JOIN_QUERY, d_dst.data_ptr(), d_qoff.data_ptr() + 4, cap, npairs - 1, cap,
        o["j_offsets"].data_ptr(), o["xyz"].data_ptr(), o["xy"].data_ptr(), o["a_row"].data_ptr(), o["b_row"].data_ptr(),
        o["b_joined"].data_ptr(), d_mask.data_ptr(), None)
    ctx.sync()
    moff = d_moff.cpu().numpy()
    rec = d_m.cpu().numpy().view(I.MATCH).reshape(-1)
    dst = d_dst.cpu().numpy()
    out = {k: v.cpu().numpy() for k, v in o.items()}
    print(f"ratio stage kept {np.diff(moff).tolist()} of {sizes[:-1]} rows; joined {out['j_offsets'][:2].tolist()}")
    assert moff[1] > 100 and moff[2] - moff[1] > 100
    exp = JO.join_segmented(rec, moff[:-1], cap, 1, mask, xyz, rec, moff[1:], cap, 0, None, dst, qoff[1:], cap, cap)
    total = int(exp["j_offsets"][-1])
    assert total > 50 and out["j_offsets"][:2].tolist() == exp["j_offsets"].tolist() and out["j_offsets"][2] == I_SENT
    for k in ROWS:
        assert_bits_equal(out[k][:total], exp[k], "ratio records " + k)
        assert (out[k][total:] == {"xyz": D_SENT, "xy": F_SENT}.get(k, I_SENT)).all(), k
    w = exp["b_written"]
    assert_bits_equal(out["b_joined"][:cap][w], exp["b_joined"][w], "ratio records b_joined")
    assert (out["b_joined"][:cap][~w] == M_SENT).all() and (out["b_joined"][cap:] == M_SENT).all()
    # the joined pixel is the new frame's keypoint the B record names, the 3-D row the A record's
    br, ar = out["b_row"][:total], out["a_row"][:total]
    assert (rec["train"][ar] == rec["query"][br]).all()
    k2 = kp[qoff[2]:][rec["train"][br]]
    assert_bits_equal(out["xy"][:total], np.c_[k2["x"], k2["y"]].astype(np.float32), "the new view's pixels")


# ---- the real chain: three views whose keypoints are shuffled per view -----------------------
_A3 = 0.12
R3 = np.array([[np.cos(_A3), 0, -np.sin(_A3)], [0, 1, 0], [np.sin(_A3), 0, np.cos(_A3)]]) @ \
    np.array([[1, 0, 0], [0, np.cos(0.05), -np.sin(0.05)], [0, np.sin(0.05), np.cos(0.05)]])
T3 = np.array([0.9, -0.2, 0.4])


def _pair_table(rng, order_q, order_t, kp_q, kp_t, n_pts):
    """Records between two views of the same points, in query-keypoint order as the ratio stage
    leaves them: 12 % of the points have no record, 30 % of the records name a wrong train keypoint.
    order_v[p] = the keypoint index of point p in view v."""
    pts = np.sort(rng.permutation(n_pts)[:int(n_pts * 0.88)])
    q, t = order_q[pts], order_t[pts].copy()
    wrong = rng.permutation(len(pts))[:int(len(pts) * 0.3)]
    t[wrong] = (t[wrong] + rng.integers(1, len(kp_t) - 1, len(wrong))) % len(kp_t)
    by_q = np.argsort(q, kind="stable")
    rec = np.zeros(len(pts), I.MATCH)
    rec["query"], rec["train"] = q[by_q], t[by_q]
    rec["distance"] = rng.integers(1, 40, len(pts)).astype(np.float32)
    return rec, kp_q[rec["query"]], kp_t[rec["train"]]


def _scene(seed, n_pts):
    """Three views of n_pts points (fundamental_inputs' two cameras and a planted third), 0.25 px of
    noise, each view's keypoints in its own shuffled order with 15 more that see nothing ->
    (table 0-1, table 1-2, keypoints of view 1)."""
    rng = np.random.default_rng(seed)
    P = np.c_[rng.uniform(-2, 2, n_pts), rng.uniform(-1.5, 1.5, n_pts), rng.uniform(4, 10, n_pts)]
    cams = [(np.eye(3), np.zeros(3)), (FI.R_TRUE, FI.T_TRUE), (R3, T3)]
    order, kps = [], []
    for R, t in cams:
        px = PI.project(FI.K, P @ R.T + t) + rng.uniform(-0.25, 0.25, (n_pts, 2))
        px = np.r_[px, rng.uniform(0, 480, (15, 2))]
        where = rng.permutation(n_pts + 15)            # where[i] = the keypoint index of row i of px
        kp = np.zeros((n_pts + 15, 2), np.float32)
        kp[where] = px
        order.append(where[:n_pts]), kps.append(kp)
    t01 = _pair_table(rng, order[0], order[1], kps[0], kps[1], n_pts)
    t12 = _pair_table(rng, order[1], order[2], kps[1], kps[2], n_pts)
    return t01, t12, len(kps[1])


def test_gpu_chain_fundamental_pose_join_pnp(any_ctx, siftgpu):
    """find_fundamental_segmented_device -> recover_pose_segmented_device on the table between views
    0 and 1 -> join_matches_segmented_device with the table between views 1 and 2 ->
    solve_pnp_segmented_device, on the context stream with no synchronisation and no host value
    between the calls; two scenes are the two segments.  Every byte equals the host forms chained
    the same way; the first two calls leave the bytes they leave without the later ones; the third
    pose is the planted one up to the scale |t| = 1 fixes, within the 2e-2 (R) / 5e-2 (t) that
    test_gpu_pnp.py allows its RANSAC chain."""
    import torch
    ctx = any_ctx
    scenes = [_scene(900 + s, 260) for s in range(2)]
    nseg = len(scenes)
    A = [s[0] for s in scenes]
    B = [s[1] for s in scenes]
    cat = lambda parts, k: np.concatenate([p[k] for p in parts])  # noqa: E731
    a_rec, a_src, a_dst, b_rec, b_dst = cat(A, 0), cat(A, 1), cat(A, 2), cat(B, 0), cat(B, 2)
    a_off = np.concatenate([[0], np.cumsum([len(p[0]) for p in A])]).astype(np.int32)
    b_off = np.concatenate([[0], np.cumsum([len(p[0]) for p in B])]).astype(np.int32)
    k_off = np.concatenate([[0], np.cumsum([s[2] for s in scenes])]).astype(np.int32)
    a_cap, b_cap, key_cap = len(a_rec), len(b_rec), int(k_off[-1])
    K = FI.K.reshape(9)
    dv = {"a": _dev(_recs(a_rec)), "src": _dev(a_src), "dst": _dev(a_dst), "aoff": _dev(a_off), "b": _dev(_recs(b_rec)),
          "bxy": _dev(b_dst), "boff": _dev(b_off), "koff": _dev(k_off), "K": _dev(K)}
    f64 = lambda *shape: torch.full(shape, D_SENT, dtype=torch.float64, device="cuda")  # noqa: E731
    i32 = lambda *shape: torch.full(shape, I_SENT, dtype=torch.int32, device="cuda")  # noqa: E731
    u8 = lambda *shape: torch.full(shape, M_SENT, dtype=torch.uint8, device="cuda")  # noqa: E731
    first = ("F", "found", "fmask", "pose", "pf", "ng", "mo", "xyz")

    def run(whole):
        o = {"F": f64(nseg + 1, 9), "found": i32(nseg + 1), "fmask": u8(a_cap + 64), "pose": f64(nseg + 1, 12),
             "pf": i32(nseg + 1), "ng": i32(nseg + 1), "mo": u8(a_cap + 64), "xyz": f64(a_cap + 2, 3),
             "pose3": f64(nseg + 1, 12), "f3": i32(nseg + 1), "ni": i32(nseg + 1), "m3": u8(b_cap + 64)}
        o.update({"j_" + k: v for k, v in _outputs(b_cap, b_cap, nseg).items()})
        p = {k: v.data_ptr() for k, v in o.items()}
        torch.cuda.synchronize()
        ctx.find_fundamental_segmented_device(dv["src"].data_ptr(), dv["dst"].data_ptr(), dv["aoff"].data_ptr(), nseg,
                                              a_cap, p["F"], p["found"], p["fmask"])
        ctx.recover_pose_segmented_device(dv["src"].data_ptr(), dv["dst"].data_ptr(), dv["aoff"].data_ptr(), nseg, a_cap,
                                          p["F"], p["found"], dv["K"].data_ptr(), dv["K"].data_ptr(), p["pose"], p["pf"],
                                          p["ng"], 0, p["fmask"], 50.0, None, p["mo"], p["xyz"])
        if whole:
            ctx.join_matches_segmented_device(
                dv["a"].data_ptr(), dv["aoff"].data_ptr(), a_cap, siftgpu.JOIN_TRAIN, p["xyz"], dv["b"].data_ptr(),
                dv["boff"].data_ptr(), b_cap, siftgpu.JOIN_QUERY, dv["bxy"].data_ptr(), dv["koff"].data_ptr(), key_cap,
                nseg, b_cap, p["j_j_offsets"], p["j_xyz"], p["j_xy"], p["j_a_row"], p["j_b_row"], p["j_b_joined"],
                p["mo"], None)
            ctx.solve_pnp_segmented_device(p["j_xyz"], p["j_xy"], p["j_j_offsets"], nseg, b_cap, dv["K"].data_ptr(),
                                           p["pose3"], p["f3"], p["ni"], 0, None, 8.0, 100, 0.99, p["m3"])
        ctx.sync()
        return {k: v.cpu().numpy() for k, v in o.items()}

    got, bare = run(True), run(False)
    for k in first:                                 # unchanged around the new calls
        assert got[k].tobytes() == bare[k].tobytes(), k
    assert (bare["pose3"] == D_SENT).all() and (bare["j_j_offsets"] == I_SENT).all() and (bare["j_xyz"] == D_SENT).all()
    assert (got["pose3"][nseg:] == D_SENT).all() and (got["j_j_offsets"][nseg + 1:] == I_SENT).all()
    scale = np.linalg.norm(FI.T_TRUE)
    joff = got["j_j_offsets"]
    assert joff[0] == 0
    for s in range(nseg):
        alo, ahi, blo, bhi = int(a_off[s]), int(a_off[s + 1]), int(b_off[s]), int(b_off[s + 1])
        hF, hm = siftgpu.findFundamentalMat(a_src[alo:ahi], a_dst[alo:ahi])
        R, t, E, m, p3, g = siftgpu.recoverPose(hF, K, K, a_src[alo:ahi], a_dst[alo:ahi], hm)
        assert R is not None and p3.tobytes() == got["xyz"][alo:ahi].tobytes() and m.tobytes() == got["mo"][alo:ahi].tobytes()
        xyz, xy, ar, br, bj = siftgpu.joinMatches(a_rec[alo:ahi], p3, b_rec[blo:bhi], b_dst[blo:bhi],
                                                  int(k_off[s + 1] - k_off[s]), siftgpu.JOIN_TRAIN, siftgpu.JOIN_QUERY, m)
        jlo, jhi = int(joff[s]), int(joff[s + 1])
        assert jhi - jlo == len(br) > 80, (s, jhi - jlo, len(br))
        assert xyz.tobytes() == got["j_xyz"][jlo:jhi].tobytes() and xy.tobytes() == got["j_xy"][jlo:jhi].tobytes()
        assert (ar + alo).tobytes() == got["j_a_row"][jlo:jhi].tobytes()
        assert (br + blo).tobytes() == got["j_b_row"][jlo:jhi].tobytes()
        assert bj.tobytes() == got["j_b_joined"][blo:bhi].tobytes()
        # the case the planted chain of test_gpu_pnp.py cannot show: the rows are not in pair-row order
        assert (np.diff(ar) < 0).any() and not np.array_equal(ar, br)
        Rp, tp, mp, ni = siftgpu.solvePnPRansac(xyz, xy, K, 8.0, 100, 0.99)
        assert Rp is not None and got["f3"][s] == 1 and got["ni"][s] == ni > 40
        assert np.c_[Rp, tp].tobytes() == got["pose3"][s].tobytes()
        assert mp.tobytes() == got["m3"][jlo:jhi].tobytes()
        print(f"scene {s}: {ahi - alo} + {bhi - blo} records, {jhi - jlo} joined, n_inliers {ni}, "
              f"|R - planted| {np.abs(Rp - R3).max():.3g}, |t - planted / |T|| {np.abs(tp - T3 / scale).max():.3g}")
        assert np.abs(Rp - R3).max() < 2e-2 and np.abs(tp - T3 / scale).max() < 5e-2
    assert (got["m3"][joff[nseg]:] == M_SENT).all() and (got["j_xyz"][joff[nseg]:] == D_SENT).all()
