#!/usr/bin/env python3
"""A/B of the epipolar matcher against the dense and the windowed segmented
matchers on a whole batch.

One child process per workload (its own timeout) detects the synthetic batch of
tools/bench_match_batch.py once, quantises the descriptors once, and then
times, alternating in that one process, with HIP events on the context's stream
(5 warm-up iterations, medians of 20, min and max), consecutive frames of the
batch (train = query, t_offsets = q_offsets + 1, keypoints aliased likewise)
under a planted F, the same for every pair:

  rect     rectified stereo, horizontal epipolar lines (Y = y);
  oblique  a pencil of lines at about 30 degrees, the epipole far off-image.

  D<m>             the unchanged dense segmented matcher of metric m, k = 2.
  W<m>r128         sift_knn_match_window_segmented_device at radius 128.
  E<m><F>b<B>r<R>  sift_knn_match_epipolar_segmented_device at band B in
                   {1, 3, 8} and radius R in {inf, 128}, k = 2, binning included.

Before anything is timed every E result is checked against D: where the dense
nearest neighbour is admissible (window and band, the rule restated in torch
float32), E's nearest neighbour is that row at that distance.
Also reported: the admissible rows per query (frame pair 0, brute force) and
the search grid.  --lib SCALE=PATH runs the same workload once more, in its own
child process, on another build of the library (the A/B of the grid's cell
side: -DSIFT_EPIPOLAR_CELL_SCALE=SCALE on apps.hip).

  python tools/bench_match_epipolar.py [--out profiles/match_epipolar_ab.txt]
"""
import argparse
import json
import math
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sift-gpu_amd")
WORKLOADS = {"1080p": (64, 1080, 1920, 16000, 1100)}  # B, R, C, rows/img, timeout s
METRICS = ["l1_f32", "l1_u8", "l2sqr_u8"]
BANDS = [1.0, 3.0, 8.0]
RADII = [math.inf, 128.0]
_c, _s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
# [e]_x with e = 1e6 (cos 30, sin 30) + (960, 540): every line passes through e, about 30 degrees in the image
_e = (1e6 * _c + 960.0, 1e6 * _s + 540.0)
MODELS = {"rect": [0, 0, 0, 0, 0, -1, 0, 1, 0],
          "oblique": [0, -1, _e[1], 1, 0, -_e[0], -_e[1], _e[0], 0]}


def rname(r):
    return "inf" if math.isinf(r) else str(int(r))


def worker(name, iters, warmup, lib):
    import numpy as np
    import torch
    sys.path.insert(0, PKG)
    import siftgpu
    if lib:
        siftgpu.LIB_PATH = os.path.abspath(lib)
    B, R, C, per_img, _ = WORKLOADS[name]
    cap = B * per_img
    strm = torch.cuda.Stream()
    ctx = siftgpu.Context(R, C, B, device=0)
    ctx.set_stream(strm.cuda_stream)
    with torch.cuda.stream(strm):
        imgs = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
        kpts = torch.empty((cap, 7), dtype=torch.int32, device="cuda")
        desc = torch.empty((cap, 128), dtype=torch.float32, device="cuda")
        d8 = torch.zeros((cap, 128), dtype=torch.uint8, device="cuda")
        offs = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
        ctx.synth_images(imgs.data_ptr(), B, R, C, C, R * C, seed_base=0)
        ctx.detect_compute_batch(imgs.data_ptr(), B, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                                 offs.data_ptr())
        ctx.descriptors_to_u8_device(desc.data_ptr(), offs.data_ptr() + 4 * B, cap, d8.data_ptr())
        ctx.sync()
        del imgs
        o = offs.cpu().numpy()
        assert o[-1] <= cap, f"{o[-1]} keypoints exceed the buffer ({cap})"
        seg = np.diff(o)
        n = int(o[B - 1])    # live query rows
        rows_of = [desc, d8, d8]
        dense_fn = [ctx.knn_match_segmented_device, ctx.knn_match_u8_segmented_device,
                    ctx.knn_match_l2sqr_u8_segmented_device]
        dF = {k: torch.tensor([v] * (B - 1), dtype=torch.float64, device="cuda") for k, v in MODELS.items()}
        out = {}

        def buf(key):
            if key not in out:
                out[key] = (torch.full((cap, 2), -1, dtype=torch.int32, device="cuda"),
                            torch.full((cap, 2), -1.0, dtype=torch.float32, device="cuda"))
            return out[key]

        def dense(m):
            i, d = buf(f"D{METRICS[m]}")
            dense_fn[m](rows_of[m].data_ptr(), offs.data_ptr(), B - 1, cap, rows_of[m].data_ptr(),
                        offs.data_ptr() + 4, cap, 2, i.data_ptr(), d.data_ptr())

        def window(m, r):
            i, d = buf(f"W{METRICS[m]}r{rname(r)}")
            ctx.knn_match_window_segmented_device(m, rows_of[m].data_ptr(), kpts.data_ptr(), offs.data_ptr(), B - 1, cap,
                                                  rows_of[m].data_ptr(), kpts.data_ptr(), offs.data_ptr() + 4, cap,
                                                  None, None, r, R, C, 2, i.data_ptr(), d.data_ptr())

        def epi(m, f, band, r):
            i, d = buf(f"E{METRICS[m]}{f}b{int(band)}r{rname(r)}")
            ctx.knn_match_epipolar_segmented_device(m, rows_of[m].data_ptr(), kpts.data_ptr(), offs.data_ptr(), B - 1,
                                                    cap, rows_of[m].data_ptr(), kpts.data_ptr(), offs.data_ptr() + 4,
                                                    cap, dF[f].data_ptr(), None, band, r, R, C, 2, i.data_ptr(),
                                                    d.data_ptr())

        legs = {}
        for m in range(3):
            legs[f"D{METRICS[m]}"] = (lambda m=m: dense(m))
            legs[f"W{METRICS[m]}r128"] = (lambda m=m: window(m, 128.0))
            for f in MODELS:
                for band in BANDS:
                    for r in RADII:
                        legs[f"E{METRICS[m]}{f}b{int(band)}r{rname(r)}"] = (lambda m=m, f=f, band=band, r=r: epi(m, f, band, r))
        for fn in legs.values():
            fn()
        ctx.sync()

        # the rule in torch float32 (no fused multiply-add: every product and sum is its own kernel)
        xy = kpts.view(torch.float32)[:, :2]

        def admissible(f9, x, y, X, Y, band, r):
            f = torch.tensor(f9, dtype=torch.float64).to(torch.float32).tolist()
            t = float(np.float32(band * band))
            a, b, c = f[0] * x + f[1] * y + f[2], f[3] * x + f[4] * y + f[5], f[6] * x + f[7] * y + f[8]
            d_dst = X * a + Y * b + c
            e_dst = d_dst * d_dst * (1.0 / (a * a + b * b))
            a2, b2, c2 = f[0] * X + f[3] * Y + f[6], f[1] * X + f[4] * Y + f[7], f[2] * X + f[5] * Y + f[8]
            d_src = x * a2 + y * b2 + c2
            e_src = d_src * d_src * (1.0 / (a2 * a2 + b2 * b2))
            return (e_dst <= t) & (e_src <= t) & ((X - x).abs() <= r) & ((Y - y).abs() <= r)

        row = torch.arange(cap, device="cuda")
        segid = torch.bucketize(row, offs[1:].to(torch.int64), right=True).clamp(max=B - 1)
        tbase = offs.to(torch.int64)[segid + 1]
        checked = {}
        for m in range(3):
            di, dd = out[f"D{METRICS[m]}"]
            j = (tbase + di[:, 0].to(torch.int64)).clamp(0, cap - 1)
            for f in MODELS:
                for band in BANDS:
                    for r in RADII:
                        key = f"{METRICS[m]}{f}b{int(band)}r{rname(r)}"
                        ei, ed = out["E" + key]
                        ok = admissible(MODELS[f], xy[:, 0], xy[:, 1], xy[j, 0], xy[j, 1], band, r) & (di[:, 0] >= 0) & (row < n)
                        same = bool(((ei[:, 0] == di[:, 0]) & (ed[:, 0] == dd[:, 0]))[ok].all())
                        assert same, f"{key}: E and D differ where the dense nearest neighbour is admissible"
                        assert bool((ed[:n, 0] >= dd[:n, 0]).all()), f"{key}: an E neighbour nearer than the dense one"
                        checked[key] = [int(ok.sum().item()), int((ei[:n, 0] >= 0).sum().item()),
                                        int((ei[:n, 1] >= 0).sum().item())]
        # admissible rows per query, frame pair 0, brute force
        q0, t0 = xy[o[0]:o[1]], xy[o[1]:o[2]]
        cand = {}
        for f in MODELS:
            for band in BANDS:
                for r in RADII:
                    c = admissible(MODELS[f], q0[:, None, 0], q0[:, None, 1], t0[None, :, 0], t0[None, :, 1], band, r)
                    c = c.sum(1).float()
                    cand[f"{f}b{int(band)}r{rname(r)}"] = [float(c.mean().item()), float(c.median().item()),
                                                           float(c.max().item())]
        ev = {k: [] for k in legs}
        for it in range(warmup + iters):
            for k, fn in legs.items():
                strm.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(strm)
                fn()
                b.record(strm)
                b.synchronize()
                if it >= warmup:
                    ev[k].append(a.elapsed_time(b))
    res = {"workload": name, "batch": B, "rows": R, "cols": C, "keypoints": int(o[-1]),
           "segment_rows": [int(seg.min()), int(statistics.median(seg.tolist())), int(seg.max())],
           "pairs": B - 1, "live_queries": n, "checked": checked, "candidates": cand, "iters": iters, "warmup": warmup,
           "event_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in ev.items()}}
    print("RESULT " + json.dumps(res), flush=True)
    ctx.close()


def resources():
    """Registers, LDS and private segment of the kernels of match_epipolar.hip, as the compiler reports them."""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fno-slp-vectorize", "-fno-gpu-rdc", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(PKG, "csrc", "match_epipolar.hip"), "-o",
                        os.devnull], capture_output=True, text=True, timeout=600)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|"
                      r"Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": re.sub(r"^_ZN4sift12_GLOBAL__N_1\d+", "", m.group(2))}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = m.group(2)
    return [f"{c['name']}: {c.get('VGPRs')} VGPRs, {c.get('TotalSGPRs')} SGPRs, LDS {c.get('LDS Size')} B, "
            f"private segment {c.get('ScratchSize')} B/lane, occupancy {c.get('Occupancy')} waves/SIMD"
            for c in rows if "kernel" in c["name"]]


def grid_line(R, C, t_cap, n_grids, scale):
    """scratch.hpp's epipolar_grid, restated for the report."""
    per = max(1, min((t_cap + n_grids - 1) // n_grids * 4, 4096))
    parts = []
    for band in BANDS:
        for r in RADII:
            cell = max(min(band, r), 1.0) * scale
            while math.ceil(C / cell) * math.ceil(R / cell) > per:
                cell *= 1.125
            parts.append(f"band {int(band)} radius {rname(r)}: {math.ceil(C / cell)} x {math.ceil(R / cell)} cells of {cell:.2f} px")
    return "; ".join(parts)


def table(r, scale):
    e = r["event_ms"]
    lines = [f"## {r['workload']}: {r['batch']} x {r['rows']}x{r['cols']}, {r['keypoints']} keypoints, "
             f"{r['pairs']} consecutive pairs, {r['live_queries']} live query rows, rows per segment min/median/max "
             f"{r['segment_rows']}",
             "k = 2; where the dense nearest neighbour is admissible, E's nearest neighbour is that row at that "
             "distance: True (asserted before timing)",
             f"grid (cell scale {scale:g}): " + grid_line(r["rows"], r["cols"], r["batch"] * 16000, r["pairs"], scale),
             f"medians of {r['iters']} iterations after {r['warmup']} warm-up [min, max], HIP events, ms; "
             "adm: admissible rows per query on frame pair 0, mean / median / max"]
    for m in METRICS:
        d, w = e[f"D{m}"], e[f"W{m}r128"]
        lines.append(f"D {m:9}                          {d[0]:10.3f} [{d[1]:9.3f}, {d[2]:9.3f}]  dense segmented matcher")
        lines.append(f"W {m:9} radius 128               {w[0]:10.3f} [{w[1]:9.3f}, {w[2]:9.3f}]  windowed matcher, D / W = {d[0] / w[0]:.2f}")
        for f in MODELS:
            for band in BANDS:
                for rad in RADII:
                    k = f"{m}{f}b{int(band)}r{rname(rad)}"
                    x, c, a = e["E" + k], r["checked"][k], r["candidates"][k[len(m):]]
                    lines.append(f"E {m:9} {f:7} band {int(band)} radius {rname(rad):>3} {x[0]:10.3f} [{x[1]:9.3f}, {x[2]:9.3f}]  "
                                 f"D / E = {d[0] / x[0]:7.2f}, W128 / E = {w[0] / x[0]:5.2f}; adm {a[0]:.1f} / {a[1]:.0f} / {a[2]:.0f}; "
                                 f"rows with a 1st / 2nd neighbour {c[1]} / {c[2]}, dense 1st admissible {c[0]}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_epipolar_ab.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--lib", action="append", default=[], help="SCALE=PATH: another build of the library, its cell scale")
    ap.add_argument("--worker", choices=sorted(WORKLOADS))
    ap.add_argument("--worker-lib", default="")
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.iters, a.warmup, a.worker_lib)
    parts = ["# Matching along epipolar lines (E) vs the dense (D) and the windowed (W) segmented matchers\n"
             "# written by tools/bench_match_epipolar.py\n"
             "# 8 lanes per query, 32 queries per workgroup; at most 4096 cells per grid, one grid per train segment"
             + ("" if a.no_resources else "\n# " + "\n# ".join(resources()))]
    builds = [(1.0, "")] + [(float(s.split("=", 1)[0]), s.split("=", 1)[1]) for s in a.lib]
    for scale, lib in builds:
        for name, w in WORKLOADS.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", name, "--iters", str(a.iters),
                                "--warmup", str(a.warmup), "--worker-lib", lib], capture_output=True, text=True,
                               timeout=w[4])
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(f"{name}: worker failed ({r.returncode}); nothing further is started")
            parts.append(table(json.loads(line[0][7:]), scale))
            print(parts[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n\n".join(parts) + "\n")


if __name__ == "__main__":
    main()
