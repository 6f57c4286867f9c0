#!/usr/bin/env python3
"""What describing provided keypoints (sift_compute_batch) costs on the headline
batch: 64 synthetic 1080p images, exact mode, 5 octaves, one whole-batch context.

One child process (its own timeout).  It runs a detect step and then measures,
in that one process, with the keypoints and offsets the detect step left on the
device:

  (a) sift_detect_compute_batch
  (b) sift_compute_batch, max_layer = 3, on the detected keypoints
  (c) the same with max_layer = 4            ((c) - (b): the widest scale)
  (d) the only route without the call, per image and through the host:
      sift_build_gaussian_pyramid + sift_calc_descriptors on each image's
      keypoints, all 64 images once (not repeated: it takes seconds)
  (g) sift_compute_batch, max_layer = 1, on a dense grid: step 8, one size,
      octave 0 layer 1, 135 x 240 = 32,400 rows per image

  ms/step   wall clock per call + sift_sync over --steps steps after --warmup,
            median of --rounds interleaved rounds [min, max];
  stages    the same context under SIFT_FLAG_PROFILE (launches serial, HIP
            events per stage): device ms per step of every stage.

  python tools/bench_compute_batch.py [--out profiles/compute_batch_ab.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sift-gpu_amd")
B, R, C = 64, 1080, 1920
PER_IMG = 40000   # output rows per image, bench.py's sizing
GRID_STEP, GRID_SIZE = 8, 4.0
LEGS = ("detect", "compute3", "compute4", "grid")
WORKER_TIMEOUT = 540


def worker(a):
    import numpy as np
    import torch
    sys.path.insert(0, PKG)
    import siftgpu
    cap = B * PER_IMG
    imgs = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
    k = torch.zeros((cap, 7), dtype=torch.int32, device="cuda")
    d = torch.empty((cap, 128), dtype=torch.float32, device="cuda")
    d2 = torch.empty((cap, 128), dtype=torch.float32, device="cuda")
    o = torch.zeros((B + 1,), dtype=torch.int32, device="cuda")
    # the dense grid: the same rows for every image
    ys, xs = np.mgrid[GRID_STEP // 2:R:GRID_STEP, GRID_STEP // 2:C:GRID_STEP]
    g = np.zeros(xs.size, siftgpu.KEYPOINT_DTYPE)
    g["x"], g["y"], g["size"], g["octave"], g["class_id"] = xs.reshape(-1), ys.reshape(-1), GRID_SIZE, 1 << 8, -1
    g["angle"] = (np.arange(xs.size) * 37) % 360
    assert B * len(g) <= cap
    gk = torch.from_numpy(np.tile(g, B).view(np.int32).reshape(-1, 7)).cuda()
    go = torch.from_numpy((np.arange(B + 1) * len(g)).astype(np.int32)).cuda()
    torch.cuda.synchronize()
    ctx = siftgpu.Context(R, C, B, device=0)
    ctx.synth_images(imgs.data_ptr(), B, R, C, C, R * C, 0)
    ctx.sync()

    def leg(name):
        if name == "detect":
            ctx.detect_compute_batch(imgs.data_ptr(), B, R, C, C, R * C, k.data_ptr(), d.data_ptr(), cap, o.data_ptr())
        elif name == "grid":
            ctx.compute_batch(imgs.data_ptr(), B, R, C, C, R * C, gk.data_ptr(), go.data_ptr(), B * len(g),
                              d2.data_ptr(), 1)
        else:
            ctx.compute_batch(imgs.data_ptr(), B, R, C, C, R * C, k.data_ptr(), o.data_ptr(), cap, d2.data_ptr(),
                              3 if name == "compute3" else 4)

    def timed(name, steps):
        t0 = time.perf_counter()
        for _ in range(steps):
            leg(name)
            ctx.sync()
        return (time.perf_counter() - t0) * 1e3 / steps

    leg("detect")
    ctx.sync()
    offs = o.cpu().numpy()
    total = int(offs[B])
    assert 0 < total <= cap
    res = {"keypoints": total, "grid_rows": B * len(g), "ms_per_step": {}, "stages": {}, "equal": {}}
    # the compute legs reproduce the detect step's descriptors, bit for bit
    for name in ("compute3", "compute4"):
        d2.fill_(-1.0)
        torch.cuda.synchronize()
        leg(name)
        ctx.sync()
        res["equal"][name] = bool(torch.equal(d2[:total].view(torch.int32), d[:total].view(torch.int32)))
    rounds = {n: [] for n in LEGS}
    for n in LEGS:
        timed(n, a.warmup)
    for _ in range(a.rounds):
        for n in LEGS:
            rounds[n].append(timed(n, a.steps))
    for n in LEGS:
        res["ms_per_step"][n] = [statistics.median(rounds[n]), min(rounds[n]), max(rounds[n])]
    ctx.set_flags(siftgpu.SIFT_FLAG_PROFILE)
    for n in LEGS:
        timed(n, 1)
        ctx.stage_stats(reset=True)
        timed(n, a.steps)
        res["stages"][n] = {s: v["ms"] / a.steps for s, v in ctx.stage_stats(reset=True).items()}
    ctx.set_flags(0)
    # (d): per image through the host, on a one-image context as a caller without the batch call would
    leg("detect")
    ctx.sync()
    kh = k.cpu().numpy().view(siftgpu.KEYPOINT_DTYPE).reshape(-1)
    ih = imgs.cpu().numpy()
    dh = d.cpu().numpy()
    ctx.close()
    same = True
    with siftgpu.Context(R, C, 1, device=0) as one:
        one.calDescriptor(one.buildGaussianPyramid(ih[0], 5), kh[offs[0]:offs[1]], 0)   # warm-up
        t0 = time.perf_counter()
        for b in range(B):
            planes = one.buildGaussianPyramid(ih[b], 5)
            out = one.calDescriptor(planes, kh[offs[b]:offs[b + 1]], 0)
            same = same and out.tobytes() == dh[offs[b]:offs[b + 1]].tobytes()
        res["host_route_ms"] = (time.perf_counter() - t0) * 1e3
    res["equal"]["host_route"] = same
    print("RESULT " + json.dumps(res), flush=True)


def fmt3(v):
    return f"{v[0]:9.3f} [{v[1]:8.3f}, {v[2]:8.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compute_batch_ab.txt"))
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--commit", default=None, help="the commit the tree stands on (default: git rev-parse)")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--rounds", str(a.rounds)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=WORKER_TIMEOUT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(f"worker failed ({r.returncode})")
    res = json.loads(line[0][7:])
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                        text=True).stdout
    ms = res["ms_per_step"]
    out = [f"# Provided keypoints (sift_compute_batch) on {B} x {R}x{C}, exact mode, 5 octaves, one context of {B} images",
           f"# written by tools/bench_compute_batch.py (python tools/bench_compute_batch.py --steps {a.steps} "
           f"--warmup {a.warmup} --rounds {a.rounds}); one session, one device",
           f"# tree: the working tree on top of commit {commit.strip() or 'unknown'}",
           f"# ms/step: wall clock of call + sift_sync, {a.steps} steps after {a.warmup} warm-up, median of {a.rounds} "
           f"interleaved rounds [min, max]",
           f"# keypoints of the detect step: {res['keypoints']}; dense grid (step {GRID_STEP}, size {GRID_SIZE}, "
           f"max_layer 1): {res['grid_rows']} rows",
           "## ms/step",
           f"(a) sift_detect_compute_batch            {fmt3(ms['detect'])}",
           f"(b) sift_compute_batch, max_layer 3      {fmt3(ms['compute3'])}   bits equal to (a)'s descriptors: "
           f"{res['equal']['compute3']}",
           f"(c) sift_compute_batch, max_layer 4      {fmt3(ms['compute4'])}   bits equal to (a)'s descriptors: "
           f"{res['equal']['compute4']}",
           f"(c) - (b), the widest scale              {ms['compute4'][0] - ms['compute3'][0]:9.3f}",
           f"(d) per image through the host, 64 images {res['host_route_ms']:9.1f} ms, measured once "
           f"(buildGaussianPyramid + calDescriptor, packing included); bits equal to (a)'s descriptors: "
           f"{res['equal']['host_route']}",
           f"(b) / (d)                                {ms['compute3'][0] / res['host_route_ms']:9.5f}",
           f"(g) dense grid, sift_compute_batch       {fmt3(ms['grid'])}",
           "## per-stage device ms per step (SIFT_FLAG_PROFILE: launches serial)"]
    names = sorted({k for s in res["stages"].values() for k in s}, key=lambda k: -res["stages"]["detect"].get(k, 0.0))
    out.append(f"{'stage':>20} " + " ".join(f"{n:>10}" for n in LEGS))
    for k in names:
        out.append(f"{k:>20} " + " ".join(f"{res['stages'][n][k]:10.3f}" if k in res["stages"][n] else f"{'-':>10}"
                                          for n in LEGS))   # '-': the stage did not run
    out.append(f"{'sum':>20} " + " ".join(f"{sum(res['stages'][n].values()):10.3f}" for n in LEGS))
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
