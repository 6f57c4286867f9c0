#!/usr/bin/env python3
"""A/B of the windowed (spatially gated) matcher against the dense segmented
matchers on a whole batch.

One child process per workload (its own timeout) detects the synthetic batch of
tools/bench_match_batch.py once, quantises the descriptors once, and then
times, alternating, with HIP events on the context's stream (5 warm-up
iterations, medians, min and max), consecutive frames of the batch (train =
query, t_offsets = q_offsets + 1, keypoints aliased likewise) with the identity
prior (d_H = NULL):

  D<m>      the unchanged dense segmented matcher of metric m
            (l1_f32, l1_u8, l2sqr_u8), k = 2.
  W<m>r<R>  sift_knn_match_window_segmented_device of the same metric at
            radius R in {8, 32, 128}, k = 2, binning included.

Before anything is timed, every windowed result is checked against the dense
one: where the dense nearest neighbour lies inside the window, the windowed
nearest neighbour is the same row at the same distance.
Also reported: the admissible rows per query (frame pair 0, counted by brute
force), the search grid, and -- from a second context with SIFT_FLAG_PROFILE --
the binning's and the kNN kernel's share of a call.

  python tools/bench_match_window.py [--out profiles/match_window_ab.txt]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sift-gpu_amd")
WORKLOADS = {"1080p": (64, 1080, 1920, 16000, 1100)}  # B, R, C, rows/img, timeout s
METRICS = ["l1_f32", "l1_u8", "l2sqr_u8"]
RADII = [8.0, 32.0, 128.0]


def worker(name, iters, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, PKG)
    import siftgpu
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

        def window(m, r, c=ctx, key=None):
            i, d = buf(key or f"W{METRICS[m]}r{int(r)}")
            c.knn_match_window_segmented_device(m, rows_of[m].data_ptr(), kpts.data_ptr(), offs.data_ptr(), B - 1, cap,
                                                rows_of[m].data_ptr(), kpts.data_ptr(), offs.data_ptr() + 4, cap,
                                                None, None, r, R, C, 2, i.data_ptr(), d.data_ptr())

        legs = {}
        for m in range(3):
            legs[f"D{METRICS[m]}"] = (lambda m=m: dense(m))
            for r in RADII:
                legs[f"W{METRICS[m]}r{int(r)}"] = (lambda m=m, r=r: window(m, r))
        for fn in legs.values():
            fn()
        ctx.sync()
        # the check: where the dense nearest neighbour is inside the window, it is the windowed one too
        xy = kpts.view(torch.float32)[:, :2]
        row = torch.arange(cap, device="cuda")
        segid = torch.bucketize(row, offs[1:].to(torch.int64), right=True).clamp(max=B - 1)
        tbase = offs.to(torch.int64)[segid + 1]
        checked = {}
        for m in range(3):
            di, dd = out[f"D{METRICS[m]}"]
            for r in RADII:
                wi, wd = out[f"W{METRICS[m]}r{int(r)}"]
                j = (tbase + di[:, 0].to(torch.int64)).clamp(0, cap - 1)
                inside = ((xy[j] - xy).abs() <= r).all(1) & (di[:, 0] >= 0) & (row < n)
                ok = bool(((wi[:, 0] == di[:, 0]) & (wd[:, 0] == dd[:, 0]))[inside].all())
                assert ok, f"{METRICS[m]} radius {r}: the windowed and the dense nearest neighbour differ inside the window"
                assert bool((wd[:n, 0] >= dd[:n, 0]).all()), "a windowed neighbour nearer than the dense one"
                checked[f"{METRICS[m]}r{int(r)}"] = [int(inside.sum().item()), int((wi[:n, 0] >= 0).sum().item()),
                                                     int((wi[:n, 1] >= 0).sum().item())]
        # admissible rows per query, frame pair 0
        q0, t0 = xy[o[0]:o[1]], xy[o[1]:o[2]]
        cand = {}
        for r in RADII:
            c = (((q0[:, None, :] - t0[None, :, :]).abs() <= r).all(2)).sum(1).float()
            cand[int(r)] = [float(c.mean().item()), float(c.median().item()), float(c.max().item())]
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
        # the split of a windowed call, by stage events on a profiling context
        pctx = siftgpu.Context(64, 64, 1, device=0, flags=siftgpu.SIFT_FLAG_PROFILE)  # the matcher needs no image workspace
        pctx.set_stream(strm.cuda_stream)
        split = {}
        for m in range(3):
            for r in RADII:
                for _ in range(2):
                    window(m, r, pctx, "P")
                pctx.sync()
                pctx.stage_stats(reset=True)
                for _ in range(5):
                    window(m, r, pctx, "P")
                pctx.sync()
                st = pctx.stage_stats(reset=True)
                split[f"{METRICS[m]}r{int(r)}"] = [st["match_window_bin"]["ms"] / 5, st["match_window_segmented"]["ms"] / 5]
        pctx.close()
    res = {"workload": name, "batch": B, "rows": R, "cols": C, "keypoints": int(o[-1]),
           "segment_rows": [int(seg.min()), int(statistics.median(seg.tolist())), int(seg.max())],
           "pairs": B - 1, "live_queries": n, "checked": checked, "candidates": cand, "split": split, "iters": iters,
           "warmup": warmup, "event_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in ev.items()}}
    print("RESULT " + json.dumps(res), flush=True)
    ctx.close()


def resources():
    """Registers, LDS and private segment of the kernels of match_window.hip, as the compiler reports them."""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fno-slp-vectorize", "-fno-gpu-rdc", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(PKG, "csrc", "match_window.hip"), "-o",
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


def table(r):
    e = r["event_ms"]
    lines = [f"## {r['workload']}: {r['batch']} x {r['rows']}x{r['cols']}, {r['keypoints']} keypoints, "
             f"{r['pairs']} consecutive pairs, {r['live_queries']} live query rows, rows per segment min/median/max "
             f"{r['segment_rows']}",
             "identity prior (d_H = NULL), k = 2; where the dense nearest neighbour lies inside the window the "
             "windowed one is the same row at the same distance: True (asserted before timing)",
             "admissible rows per query, frame pair 0, mean / median / max: "
             + "; ".join(f"radius {k}: {v[0]:.1f} / {v[1]:.0f} / {v[2]:.0f}" for k, v in r["candidates"].items()),
             f"medians of {r['iters']} iterations after {r['warmup']} warm-up [min, max], HIP events, ms; "
             "bin / knn: the call's two stages on a profiling context (mean of 5)"]
    for m in METRICS:
        d = e[f"D{m}"]
        lines.append(f"D {m:9}            {d[0]:10.3f} [{d[1]:9.3f}, {d[2]:9.3f}]  dense segmented matcher")
        for rad in RADII:
            k = f"{m}r{int(rad)}"
            w, s, c = e["W" + k], r["split"][k], r["checked"][k]
            lines.append(f"W {m:9} radius {int(rad):3} {w[0]:10.3f} [{w[1]:9.3f}, {w[2]:9.3f}]  dense / windowed = "
                         f"{d[0] / w[0]:7.2f}; bin {s[0]:.3f} + knn {s[1]:.3f} ms (binning {100 * s[0] / (s[0] + s[1]):.0f} %); "
                         f"rows with a 1st / 2nd neighbour {c[1]} / {c[2]}, dense 1st inside the window {c[0]}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_window_ab.txt"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-resources", action="store_true")
    ap.add_argument("--worker", choices=sorted(WORKLOADS))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.iters, a.warmup)
    parts = ["# Matching within a search window (W) vs the dense segmented matchers (D)\n"
             "# written by tools/bench_match_window.py\n"
             "# 8 lanes per query, 32 queries per workgroup; at most 4096 cells per grid, one grid per train segment"
             + ("" if a.no_resources else "\n# " + "\n# ".join(resources()))]
    for name, w in WORKLOADS.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", name, "--iters", str(a.iters),
                            "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=w[4])
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"{name}: worker failed ({r.returncode}); nothing further is started")
        parts.append(table(json.loads(line[0][7:])))
        print(parts[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n\n".join(parts) + "\n")


if __name__ == "__main__":
    main()
