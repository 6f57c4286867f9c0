"""The join of two match tables on a shared keypoint (include/sift_hip.h,
sift_join_matches) restated in numpy and plain loops, independent of the C
code: the checker of test_join.py and test_gpu_join.py.

A record is a row of siftgpu.MATCH_DTYPE (query, train, distance, segment); the
key of a record is its query (side 0) or its train (side 1)."""
import numpy as np

QUERY, TRAIN = 0, 1
FIELD = ("query", "train")


def rank_bits(distance):
    """bits(distance + 0.0f) of a float32 array as uint32: -0.0 becomes +0.0."""
    with np.errstate(invalid="ignore"):
        return (np.asarray(distance, np.float32) + np.float32(0.0)).view(np.uint32)


def winners(a, a_side, a_mask, n_keys):
    """{key: row} of table a: per key the candidate with the smallest (bits, row)."""
    best = {}
    keys = a[FIELD[a_side]]
    bits = rank_bits(a["distance"])
    for i in range(len(a)):
        k, d = int(keys[i]), a["distance"][i]
        if (a_mask is not None and a_mask[i] == 0) or not (0 <= k < n_keys) or not (d >= 0):
            continue
        r = (int(bits[i]), i)
        if k not in best or r < best[k]:
            best[k] = r
    return {k: r[1] for k, r in best.items()}


def join(a, a_xyz, a_mask, a_side, b, b_xy, b_mask, b_side, n_keys):
    """One segment -> dict(xyz [n, 3] float64, xy [n, 2] float32, a_row, b_row [n] int32, b_joined
    uint8[len(b)])."""
    win = winners(a, a_side, a_mask, n_keys)
    keys = b[FIELD[b_side]]
    a_row, b_row = [], []
    joined = np.zeros(len(b), np.uint8)
    for i in range(len(b)):
        k = int(keys[i])
        if (b_mask is not None and b_mask[i] == 0) or not (0 <= k < n_keys) or k not in win:
            continue
        joined[i] = 1
        a_row.append(win[k])
        b_row.append(i)
    a_row, b_row = np.array(a_row, np.int32), np.array(b_row, np.int32)
    xyz = np.zeros((0, 3)) if a_xyz is None else np.ascontiguousarray(a_xyz, np.float64).reshape(-1, 3)[a_row]
    xy = np.zeros((0, 2), np.float32) if b_xy is None else np.ascontiguousarray(b_xy, np.float32).reshape(-1, 2)[b_row]
    return {"xyz": xyz.reshape(-1, 3), "xy": xy.reshape(-1, 2), "a_row": a_row, "b_row": b_row, "b_joined": joined}


def clamp(v, cap):
    return min(max(int(v), 0), int(cap))


def join_segmented(a, a_off, a_cap, a_side, a_mask, a_xyz, b, b_off, b_cap, b_side, b_mask, b_xy, key_off, key_cap,
                   j_cap):
    """Every segment -> dict: xyz, xy, a_row, b_row (the first j_cap rows of all segments in order,
    rows absolute), j_offsets [n_segments + 1] (true counts), b_joined uint8[b_cap] with b_written
    bool[b_cap] (the bytes some segment owns), per_segment (join()'s dicts with absolute rows).
    A byte two overlapping segments own must get one value from both."""
    nseg = len(a_off) - 1
    parts, j_off = [], [0]
    joined, written = np.zeros(b_cap, np.uint8), np.zeros(b_cap, bool)
    for s in range(nseg):
        alo, ahi = clamp(a_off[s], a_cap), clamp(a_off[s + 1], a_cap)
        blo, bhi = clamp(b_off[s], b_cap), clamp(b_off[s + 1], b_cap)
        ahi, bhi = max(ahi, alo), max(bhi, blo)
        n_keys = clamp(key_off[s + 1], key_cap) - clamp(key_off[s], key_cap)
        r = join(a[alo:ahi], None if a_xyz is None else a_xyz[alo:ahi], None if a_mask is None else a_mask[alo:ahi],
                 a_side, b[blo:bhi], None if b_xy is None else b_xy[blo:bhi],
                 None if b_mask is None else b_mask[blo:bhi], b_side, n_keys)
        r["a_row"] = r["a_row"] + np.int32(alo)
        r["b_row"] = r["b_row"] + np.int32(blo)
        again = written[blo:bhi]
        assert (joined[blo:bhi][again] == r["b_joined"][again]).all(), "overlapping segments disagree on b_joined"
        joined[blo:bhi] = r["b_joined"]
        written[blo:bhi] = True
        parts.append(r)
        j_off.append(j_off[-1] + len(r["b_row"]))
    out = {k: np.concatenate([p[k] for p in parts])[:j_cap] for k in ("xyz", "xy", "a_row", "b_row")}
    out.update(j_offsets=np.array(j_off, np.int32), b_joined=joined, b_written=written, per_segment=parts)
    return out
