#!/usr/bin/env python3
"""A/B of matching a whole batch: the segmented call against the per-pair loop.

For each workload one child process (its own timeout) detects a synthetic
batch once, then times, alternating, with HIP events on the context's stream
(5 warm-up iterations, medians):

  A   sift_knn_match_l1_segmented_device, consecutive frames of the batch
      (train = query, t_offsets = q_offsets + 1): one enqueue, no host value.
  A+  A followed by sift_ratio_matches_device with keypoints (the whole new
      sequence; B has no counterpart, its ratio test is host code).
  B   the same pairs through a loop of the unchanged sift_knn_match_l1_device:
      the offsets are copied to the host first (a synchronisation) and that
      copy is inside the timed window, because a caller pays it today.

A's idx / dist must equal B's byte for byte before anything is timed.  One
further pass under SIFT_FLAG_PROFILE gives the per-stage device time.

  python tools/bench_match_batch.py [--out profiles/match_batch_ab.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {"1080p": (64, 1080, 1920, 16000, 600), "240x320": (64, 240, 320, 1500, 300)}  # B, R, C, rows/img, timeout s


def worker(name, iters, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "sift-gpu_amd"))
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
        offs = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
        out = {k: (torch.empty((cap, 2), dtype=torch.int32, device="cuda"),
                   torch.empty((cap, 2), dtype=torch.float32, device="cuda")) for k in "AB"}
        mt = torch.empty((cap, 4), dtype=torch.int32, device="cuda")
        sxy = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
        dxy = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
        moff = torch.empty((B,), dtype=torch.int32, device="cuda")
        h_offs = torch.empty((B + 1,), dtype=torch.int32).pin_memory()
        ctx.synth_images(imgs.data_ptr(), B, R, C, C, R * C, seed_base=0)
        ctx.detect_compute_batch(imgs.data_ptr(), B, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                                 offs.data_ptr())
        ctx.sync()
        o = offs.cpu().numpy()
        assert o[-1] <= cap, f"{o[-1]} keypoints exceed the buffer ({cap})"
        seg = np.diff(o)

        def run_a(ratio=False):
            i, d = out["A"]
            ctx.knn_match_segmented_device(desc.data_ptr(), offs.data_ptr(), B - 1, cap, desc.data_ptr(),
                                           offs.data_ptr() + 4, cap, 2, i.data_ptr(), d.data_ptr())
            if ratio:
                ctx.ratio_matches_device(i.data_ptr(), d.data_ptr(), offs.data_ptr(), B - 1, cap, 0.86,
                                         kpts.data_ptr(), kpts.data_ptr(), offs.data_ptr() + 4, mt.data_ptr(),
                                         sxy.data_ptr(), dxy.data_ptr(), cap, moff.data_ptr())

        def run_b():
            i, d = out["B"]
            h_offs.copy_(offs, non_blocking=True)
            strm.synchronize()                       # the caller needs the row counts on the host
            ho = h_offs.numpy()
            for b in range(B - 1):
                q0, q1, t1 = int(ho[b]), int(ho[b + 1]), int(ho[b + 2])
                ctx.knn_match_device(desc.data_ptr() + q0 * 512, q1 - q0, desc.data_ptr() + q1 * 512, t1 - q1, 2,
                                     i.data_ptr() + q0 * 8, d.data_ptr() + q0 * 8)

        legs = {"A": run_a, "A+": lambda: run_a(True), "B": run_b}
        for k in "AB":
            out[k][0].fill_(-1)
            out[k][1].fill_(-1.0)
        run_a()
        run_b()
        ctx.sync()
        n = int(o[B - 1])
        same = bool(torch.equal(out["A"][0][:n], out["B"][0][:n]) and torch.equal(out["A"][1][:n], out["B"][1][:n]))
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
        ctx.set_flags(siftgpu.SIFT_FLAG_PROFILE)
        ctx.stage_stats(reset=True)
        run_a(True)
        sa = ctx.stage_stats(reset=True)
        run_b()
        sb = ctx.stage_stats(reset=True)
        ctx.sync()
        kept = int(moff.cpu().numpy()[-1])
    res = {"workload": name, "batch": B, "rows": R, "cols": C, "keypoints": int(o[-1]),
           "segment_rows": [int(seg.min()), int(statistics.median(seg.tolist())), int(seg.max())],
           "pairs": B - 1, "a_equals_b": same, "kept_matches": kept, "iters": iters, "warmup": warmup,
           "event_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in ev.items()},
           "wall_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in wall.items()},
           "stages_A+": {k: [v["launches"], v["ms"]] for k, v in sa.items()},
           "stages_B": {k: [v["launches"], v["ms"]] for k, v in sb.items()}}
    print("RESULT " + json.dumps(res), flush=True)
    ctx.close()


def table(r):
    lines = [f"## {r['workload']}: {r['batch']} x {r['rows']}x{r['cols']}, {r['keypoints']} keypoints, "
             f"{r['pairs']} consecutive pairs, rows per segment min/median/max {r['segment_rows']}",
             f"A == B byte for byte: {r['a_equals_b']}; matches kept by A+ at ratio 0.86: {r['kept_matches']}",
             f"medians of {r['iters']} iterations after {r['warmup']} warm-up [min, max], ms",
             f"{'leg':4} {'HIP events':>32} {'host wall':>32}"]
    for k in ("A", "A+", "B"):
        e, w = r["event_ms"][k], r["wall_ms"][k]
        lines.append(f"{k:4} {e[0]:10.3f} [{e[1]:9.3f}, {e[2]:9.3f}] {w[0]:10.3f} [{w[1]:9.3f}, {w[2]:9.3f}]")
    ea, eb = r["event_ms"]["A"][0], r["event_ms"]["B"][0]
    lines.append(f"B / A = {eb / ea:.3f} (events), {r['wall_ms']['B'][0] / r['wall_ms']['A'][0]:.3f} (wall)")
    for leg in ("A+", "B"):
        st = ", ".join(f"{k}: {v[0]} x, {v[1]:.3f} ms" for k, v in r["stages_" + leg].items())
        lines.append(f"stage stats (SIFT_FLAG_PROFILE, one pass) {leg}: {st}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_batch_ab.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--worker", choices=sorted(WORKLOADS))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.iters, a.warmup)
    parts = ["# Matching a whole batch: segmented call (A) vs per-pair loop of sift_knn_match_l1_device (B)",
             "# written by tools/bench_match_batch.py"]
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
