#!/usr/bin/env python3
"""A/B of the last stage of a batch: the segmented device homography against
the host loop it replaces.

For each workload one child process (its own timeout) detects a synthetic
batch, matches consecutive frames (segmented kNN + ratio test with keypoints)
once, then times, alternating, with HIP events on the context's stream
(5 warm-up iterations, medians of 20):

  A   sift_find_homography_segmented_device on the ratio stage's output
      (d_src_xy, d_dst_xy, d_m_offsets): one enqueue, no host value.
  B   the flow a caller has without it: m_offsets and the point pairs are
      copied to the host, the stream is waited for, and sift_find_homography
      runs per segment on the CPU.  The copy and the wait are inside B's
      window, because a caller pays them today.

A's H, found and inlier mask must equal B's byte for byte before anything is
timed.  A's latency is one segment's serial chain (the slowest segment); B's
is the sum of the segments' host RANSACs plus a round trip.

  python tools/bench_homography_batch.py [--out profiles/homography_batch_ab.txt]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {"1080p": (64, 1080, 1920, 16000, 420), "240x320": (64, 240, 320, 1500, 300)}  # B, R, C, rows/img, timeout s


def worker(name, iters, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "sift-gpu_amd"))
    import siftgpu
    B, R, C, per_img, _ = WORKLOADS[name]
    cap = B * per_img
    S = B - 1
    strm = torch.cuda.Stream()
    ctx = siftgpu.Context(R, C, B, device=0)
    ctx.set_stream(strm.cuda_stream)
    L = siftgpu.lib()
    with torch.cuda.stream(strm):
        imgs = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
        kpts = torch.empty((cap, 7), dtype=torch.int32, device="cuda")
        desc = torch.empty((cap, 128), dtype=torch.float32, device="cuda")
        offs = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
        idx = torch.empty((cap, 2), dtype=torch.int32, device="cuda")
        dist = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
        mt = torch.empty((cap, 4), dtype=torch.int32, device="cuda")
        sxy = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
        dxy = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
        moff = torch.empty((B,), dtype=torch.int32, device="cuda")
        dH = torch.zeros((S, 9), dtype=torch.float64, device="cuda")
        df = torch.zeros((S,), dtype=torch.int32, device="cuda")
        dm = torch.zeros((cap,), dtype=torch.uint8, device="cuda")
        ctx.synth_images(imgs.data_ptr(), B, R, C, C, R * C, seed_base=0)
        ctx.detect_compute_batch(imgs.data_ptr(), B, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                                 offs.data_ptr())
        ctx.knn_match_segmented_device(desc.data_ptr(), offs.data_ptr(), S, cap, desc.data_ptr(),
                                       offs.data_ptr() + 4, cap, 2, idx.data_ptr(), dist.data_ptr())
        ctx.ratio_matches_device(idx.data_ptr(), dist.data_ptr(), offs.data_ptr(), S, cap, 0.86, kpts.data_ptr(),
                                 kpts.data_ptr(), offs.data_ptr() + 4, mt.data_ptr(), sxy.data_ptr(), dxy.data_ptr(),
                                 cap, moff.data_ptr())
        ctx.sync()
        mo = moff.cpu().numpy()
        total = int(mo[-1])
        assert total <= cap
        seg = np.diff(mo)
        h_moff = torch.empty((B,), dtype=torch.int32).pin_memory()
        h_src = torch.empty((max(total, 1), 2), dtype=torch.float32).pin_memory()
        h_dst = torch.empty((max(total, 1), 2), dtype=torch.float32).pin_memory()
        bH = np.zeros((S, 9), np.float64)
        bf = np.zeros(S, np.int32)
        bm = np.zeros(max(total, 1), np.uint8)
        fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)

        def run_a():
            ctx.find_homography_segmented_device(sxy.data_ptr(), dxy.data_ptr(), moff.data_ptr(), S, cap,
                                                 dH.data_ptr(), df.data_ptr(), dm.data_ptr())

        def run_b():
            h_moff.copy_(moff, non_blocking=True)
            h_src.copy_(sxy[:max(total, 1)], non_blocking=True)   # the caller sized this from an earlier read of m_offsets
            h_dst.copy_(dxy[:max(total, 1)], non_blocking=True)
            strm.synchronize()
            ho = h_moff.numpy()
            s0, d0 = h_src.data_ptr(), h_dst.data_ptr()
            for b in range(S):
                lo, n = int(ho[b]), int(ho[b + 1] - ho[b])
                rc = L.sift_find_homography(ctypes.cast(s0 + lo * 8, fp), ctypes.cast(d0 + lo * 8, fp), n, 3.0, 2000,
                                            0.995, ctypes.cast(bH[b].ctypes.data, dp), bm.ctypes.data + lo)
                bf[b] = 1 if rc == 0 else 0
                if rc != 0:
                    bm[lo:lo + n] = 0

        legs = {"A": run_a, "B": run_b}
        run_a()
        run_b()
        ctx.sync()
        same = bool(dH.cpu().numpy().tobytes() == bH.tobytes() and df.cpu().numpy().tobytes() == bf.tobytes()
                    and dm.cpu().numpy()[:total].tobytes() == bm[:total].tobytes())
        assert same, "A and B differ"
        ev, wall = {k: [] for k in legs}, {k: [] for k in legs}
        for it in range(warmup + iters):
            for k, fn in legs.items():
                strm.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record(strm)
                fn()
                b.record(strm)
                b.synchronize()
                t1 = time.perf_counter()
                if it >= warmup:
                    ev[k].append(a.elapsed_time(b))
                    wall[k].append((t1 - t0) * 1e3)
    res = {"workload": name, "batch": B, "rows": R, "cols": C, "segments": S, "pairs_total": total,
           "segment_pairs": [int(seg.min()), int(statistics.median(seg.tolist())), int(seg.max())],
           "found": int(bf.sum()), "inliers": int(bm[:total].sum()), "a_equals_b": same, "iters": iters,
           "warmup": warmup,
           "event_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in ev.items()},
           "wall_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in wall.items()}}
    print("RESULT " + json.dumps(res), flush=True)
    ctx.close()


def table(r):
    lines = [f"## {r['workload']}: {r['batch']} x {r['rows']}x{r['cols']}, {r['segments']} consecutive pairs of frames, "
             f"{r['pairs_total']} point pairs, per segment min/median/max {r['segment_pairs']}",
             f"A == B byte for byte (H, found, mask): {r['a_equals_b']}; models found {r['found']} of {r['segments']}, "
             f"{r['inliers']} inliers",
             f"medians of {r['iters']} iterations after {r['warmup']} warm-up [min, max], ms",
             f"{'leg':4} {'HIP events':>32} {'host wall':>32}"]
    for k in ("A", "B"):
        e, w = r["event_ms"][k], r["wall_ms"][k]
        lines.append(f"{k:4} {e[0]:10.3f} [{e[1]:9.3f}, {e[2]:9.3f}] {w[0]:10.3f} [{w[1]:9.3f}, {w[2]:9.3f}]")
    ea, eb = r["event_ms"]["A"][0], r["event_ms"]["B"][0]
    lines.append(f"B / A = {eb / ea:.3f} (events), {r['wall_ms']['B'][0] / r['wall_ms']['A'][0]:.3f} (wall)"
                 + ("" if eb >= ea else "  -- A loses here; its point is that the stream never waits for the host"))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "homography_batch_ab.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--worker", choices=sorted(WORKLOADS))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.iters, a.warmup)
    parts = ["# Homography of a whole batch: segmented device call (A) vs copy to the host + loop of "
             "sift_find_homography (B)", "# written by tools/bench_homography_batch.py"]
    for name, w in WORKLOADS.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", name, "--iters", str(a.iters),
                            "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=w[4])
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
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
