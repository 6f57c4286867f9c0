"""The join of two match tables on a shared keypoint (2-D / 3-D rows for PnP)
without a GPU: the entry points are declared, exported, wrapped and check their
arguments; the host sift_join_matches equals join_oracle.py byte for byte on
every segment of the census of join_inputs.py under the four settings of the key
sides; the census holds what the GPU test needs; the scratch layouts and the host
rule run as stand-alone programs under the address and undefined-behaviour
sanitizers.  The calls that need a context are in test_gpu_join.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import join_inputs as I
import join_oracle as JO

NEW = ["sift_join_matches", "sift_join_matches_segmented_device", "sift_join_matches_segmented"]


def test_entry_points_declared_exported_and_wrapped(siftgpu):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sift_hip.h")).read(), flags=re.S)
    L = ctypes.CDLL(siftgpu.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(L, name), name
        assert getattr(siftgpu.lib(), name).argtypes is not None, name
    for meth in ["join_matches_segmented_device", "joinMatchesSegmented"]:
        assert callable(getattr(siftgpu.Context, meth)), meth
    assert callable(siftgpu.joinMatches) and (siftgpu.JOIN_QUERY, siftgpu.JOIN_TRAIN) == (0, 1)
    assert re.search(r"#define SIFT_JOIN_QUERY 0\b", text) and re.search(r"#define SIFT_JOIN_TRAIN 1\b", text)
    assert b"join_matches\0" in open(siftgpu.LIB_PATH, "rb").read()           # the stage's name
    assert siftgpu.MATCH_DTYPE == I.MATCH and (JO.QUERY, JO.TRAIN) == (0, 1)
    # the block size the kernels are built with, as scratch.hpp states it
    sc = open(os.path.join(ROOT, "sift-gpu_amd", "csrc", "scratch.hpp")).read()
    assert re.search(r"constexpr int kJoinRows = 256;", sc) and I.KRB == 256
    mk = open(os.path.join(ROOT, "sift-gpu_amd", "Makefile")).read()
    assert "csrc/join.hip" in mk


def test_argument_checks(siftgpu):
    L, E = siftgpu.lib(), siftgpu.SIFT_E_INVALID
    rec = np.zeros(4, I.MATCH)
    xyz, xy = np.zeros((4, 3)), np.zeros((4, 2), np.float32)
    out = np.zeros(64)
    r, x, p, o = rec.ctypes.data, xyz.ctypes.data, xy.ctypes.data, out.ctypes.data
    call = lambda a=r, na=4, sa=0, b=r, nb=4, sb=1, nk=4, ax=x, bp=p, xo=o, po=o: L.sift_join_matches(  # noqa: E731
        a, na, sa, None, ax, b, nb, sb, None, bp, nk, xo, po, None, None, None)
    assert call() == 4                                              # every key 0, every distance 0: all four B rows join
    assert call(a=None) == E and call(b=None) == E                  # NULL records with n > 0
    assert call(a=None, na=0) == 0 and call(b=None, nb=0) == 0
    assert call(na=-1) == E and call(nb=-1) == E and call(nk=-1) == E
    for bad in (-1, 2, 7):
        assert call(sa=bad) == E and call(sb=bad) == E
    assert call(ax=None) == E and call(bp=None) == E                # an output without the rows it gathers from
    assert call(ax=None, xo=None) == 4 and call(bp=None, po=None) == 4
    # a null context, also with nothing to do
    for f in (L.sift_join_matches_segmented_device, L.sift_join_matches_segmented):
        assert f(None, r, r, 4, 0, None, x, r, r, 4, 1, None, p, r, 4, 1, o, o, None, None, None, 4, o) == E
        assert f(None, None, None, 0, 0, None, None, None, None, 0, 0, None, None, None, 0, 0, None, None, None, None,
                 None, 0, None) == E
    with pytest.raises(ValueError):
        siftgpu.joinMatches(rec, xyz[:3], rec, xy, 4, 0, 1)
    with pytest.raises(ValueError):
        siftgpu.joinMatches(rec, xyz, rec, xy, 4, 0, 1, a_mask=np.ones(3, np.uint8))
    with pytest.raises(siftgpu.SiftError):
        siftgpu.joinMatches(rec, xyz, rec, xy, 4, 0, 2)


def _host_segment(siftgpu, c, s, a_side, b_side, masks=True):
    """sift_join_matches on segment s into sentinel-filled outputs of exactly the size the rule may
    write -> join_oracle.join's dict with absolute rows."""
    alo, ahi, blo, bhi, nk = I.bounds(c, s)
    nb = bhi - blo
    xyz, xy = np.full((nb + 1, 3), -7.0), np.full((nb + 1, 2), -7.0, np.float32)
    ar, br, bj = np.full(nb + 1, -77, np.int32), np.full(nb + 1, -77, np.int32), np.full(nb + 1, 0xEE, np.uint8)
    a, b = np.ascontiguousarray(c.a[alo:ahi]), np.ascontiguousarray(c.b[blo:bhi])
    ax, bp = np.ascontiguousarray(c.a_xyz[alo:ahi]), np.ascontiguousarray(c.b_xy[blo:bhi])
    am, bm = np.ascontiguousarray(c.a_mask[alo:ahi]), np.ascontiguousarray(c.b_mask[blo:bhi])
    n = siftgpu.lib().sift_join_matches(
        a.ctypes.data, ahi - alo, a_side, am.ctypes.data if masks else None, ax.ctypes.data, b.ctypes.data, nb, b_side,
        bm.ctypes.data if masks else None, bp.ctypes.data, nk, xyz.ctypes.data, xy.ctypes.data, ar.ctypes.data,
        br.ctypes.data, bj.ctypes.data)
    assert 0 <= n <= nb, (s, n)
    assert (xyz[n:] == -7.0).all() and (xy[n:] == -7.0).all() and (ar[n:] == -77).all() and (br[n:] == -77).all() \
        and bj[nb] == 0xEE, f"segment {s}: a write past the joined rows"
    return {"xyz": xyz[:n], "xy": xy[:n], "a_row": ar[:n] + np.int32(alo), "b_row": br[:n] + np.int32(blo),
            "b_joined": bj[:nb]}


def test_host_matches_oracle_bytewise(siftgpu):
    """Every segment of the census under the four side settings, with and without the masks: the
    count, every gathered byte, the rows and b_joined."""
    c = I.call()
    for a_side, b_side in I.SIDES:
        for masks in (True, False):
            exp = I.expected(a_side, b_side, masks)
            for s, label in enumerate(c.labels):
                got, want = _host_segment(siftgpu, c, s, a_side, b_side, masks), exp["per_segment"][s]
                for k in ("xyz", "xy", "a_row", "b_row", "b_joined"):
                    assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), \
                        f"sides {a_side}{b_side} masks {masks} segment {s} ({label}): {k}"
            print(f"sides {a_side}{b_side} masks {masks}: joined per segment {np.diff(exp['j_offsets']).tolist()}")
    # the module-level wrapper returns the same
    alo, ahi, blo, bhi, nk = I.bounds(c, I.index("b600"))
    got = siftgpu.joinMatches(c.a[alo:ahi], c.a_xyz[alo:ahi], c.b[blo:bhi], c.b_xy[blo:bhi], nk, 1, 0,
                              c.a_mask[alo:ahi], c.b_mask[blo:bhi])
    want = JO.join(c.a[alo:ahi], c.a_xyz[alo:ahi], c.a_mask[alo:ahi], 1, c.b[blo:bhi], c.b_xy[blo:bhi], c.b_mask[blo:bhi],
                   0, nk)
    for g, k in zip(got, ("xyz", "xy", "a_row", "b_row", "b_joined")):
        assert g.tobytes() == want[k].tobytes(), k


def test_census(siftgpu):
    """The committed inputs are what the issue lists, counted on the oracle alone."""
    c = I.call()
    assert len(c.labels) == c.n_segments == 14 and len(c.a_off) == len(c.b_off) == len(c.k_off) == 15
    sizes = [I.bounds(c, s) for s in range(14)]
    assert [z[3] - z[2] for z in sizes][:6] == [0, 1, 255, 256, 257, 600]
    assert sizes[I.index("a0")][1] - sizes[I.index("a0")][0] == 0 and sizes[I.index("a0")][3] > sizes[I.index("a0")][2]
    bk = I.index("backwards")
    assert c.a_off[bk + 1] < c.a_off[bk] and c.b_off[bk + 1] < c.b_off[bk] and sizes[bk][1] == sizes[bk][0] \
        and sizes[bk][3] == sizes[bk][2]
    assert c.a_off[-1] > c.a_cap > c.a_off[-2] and c.b_off[-1] > c.b_cap > c.b_off[-2] \
        and c.k_off[-1] > c.key_cap > c.k_off[-2]
    assert len(c.a) == len(c.a_xyz) == len(c.a_mask) == c.a_cap and len(c.b) == len(c.b_xy) == len(c.b_mask) == c.b_cap
    for off, cap in ((c.a_off, c.a_cap), (c.b_off, c.b_cap)):       # several blocks, and the grid holds them
        used, most = I.tiles(off, cap)
        assert 10 < used <= most, (used, most)
    for a_side, b_side in I.SIDES:
        e = I.expected(a_side, b_side)
        per = e["per_segment"]
        loc = lambda s, k: (per[s][k] - sizes[s][0 if k == "a_row" else 2]).tolist()  # noqa: E731
        assert e["j_offsets"][-1] > c.j_cap > e["j_offsets"][6] and len(e["b_row"]) == c.j_cap       # rows are cut
        assert e["j_offsets"][1] == 0 and e["j_offsets"][bk + 1] == e["j_offsets"][bk]
        z = I.index("a0")
        assert e["j_offsets"][z + 1] == e["j_offsets"][z] and e["b_written"][sizes[z][2]:sizes[z][3]].all()
        for label, key_rows in (("dup_dist", {0: 20, 50: 20}), ("dup_equal", {3: 15}), ("dup_masked", {4: 70})):
            s = I.index(label)
            got = dict(zip(loc(s, "b_row"), loc(s, "a_row")))
            for brow, arow in key_rows.items():
                assert got[brow] == arow, (label, brow, got.get(brow))
        s = I.index("bad_keys")
        got = dict(zip(loc(s, "b_row"), loc(s, "a_row")))
        assert [got.get(r) for r in range(16)][:6] == [None] * 6                          # keys -1, n_keys, INT_MAX, INT_MIN
        assert [got.get(r) for r in range(10, 16)] == [11, 12, None, None, 16, 17]        # -0.0, +inf, NaN, -1, NaN|3, 0|-0.0
        s = I.index("dup_b")
        got = loc(s, "b_row")
        assert got[:8] == list(range(8)) and len(set(loc(s, "a_row")[:8])) == 1
        assert not e["b_written"][:0].any() and e["b_written"].all()                     # every B row has an owner here
        # one A row may serve several B rows, and some keys have several candidates
        assert len(set(e["a_row"].tolist())) < len(e["a_row"])
    assert I.expected(0, 1, False)["j_offsets"][-1] > I.expected(0, 1, True)["j_offsets"][-1]


def _program(tmp_path, name, ok):
    """tests/cpp/<name>.cpp as a program of its own, with the address and undefined-behaviour
    sanitizers (runtimes linked statically) where the host compiler has them."""
    src = os.path.join(ROOT, "tests", "cpp", name + ".cpp")
    exe = tmp_path / name
    cxx = shutil.which("g++") or "g++"
    base = [cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", src, "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and ok in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_join_layouts(tmp_path):
    _program(tmp_path, "join_layout", "join layouts ok")


def test_join_rule_program(tmp_path):
    _program(tmp_path, "join_rule", "join rule ok")
