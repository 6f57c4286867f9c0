#!/usr/bin/env python3
"""What the per-image keypoint budget (sift_set_max_features) costs and saves on
the headline batch: 64 synthetic 1080p images, exact mode, 5 octaves.

One child process per leg (its own timeout; nothing further is started after a
failure).  A leg measures, for each budget n in 0 (unlimited), 500, 2000, 8000:

  ms/step   wall clock over --steps steps after --warmup, the batch split over
            two contexts on two streams as bench.py's timed leg does; the legs
            of all budgets are interleaved over --rounds rounds and the median
            round is reported with [min, max];
  stages    one whole-batch context with SIFT_FLAG_PROFILE (launches run
            serially, HIP events per stage): ms per step of every stage;
  kept      the batch's keypoint total (d_img_offsets[batch]);
  match     the squared-L2 byte matcher on consecutive frames of the kept
            descriptors (sift_knn_match_l2sqr_u8_segmented_device), HIP events,
            median of 10 after 3.

--baseline-lib names a libsift_hip.so built from the parent commit: its
unlimited ms/step is measured in the same session, alternating with this
build's, as the A/B of "the option off changes nothing".

  python tools/bench_max_features.py [--baseline-lib PATH] [--out profiles/max_features_ab.txt]
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
BUDGETS = (0, 500, 2000, 8000)
PER_IMG = 40000   # output rows per image, bench.py's sizing
WORKER_TIMEOUT = 420


def worker(a):
    import numpy as np
    import torch
    sys.path.insert(0, PKG)
    import siftgpu
    if a.lib:
        siftgpu.LIB_PATH = a.lib
    budgets = (0,) if a.lib else BUDGETS
    imgs = torch.empty((B, R, C), dtype=torch.float32, device="cuda")

    class Part:
        def __init__(self, b0, nb, strm, flags=0):
            self.b0, self.nb, self.strm, self.cap = b0, nb, strm, nb * PER_IMG
            self.ctx = siftgpu.Context(R, C, nb, device=0, flags=flags)
            self.ctx.set_stream(strm.cuda_stream)
            self.k = torch.empty((self.cap, 7), dtype=torch.int32, device="cuda")
            self.d = torch.empty((self.cap, 128), dtype=torch.float32, device="cuda")
            self.o = torch.empty((nb + 1,), dtype=torch.int32, device="cuda")

        def step(self):
            self.ctx.detect_compute_batch(imgs[self.b0].data_ptr(), self.nb, R, C, C, R * C, self.k.data_ptr(),
                                          self.d.data_ptr(), self.cap, self.o.data_ptr())

        def budget(self, n):
            if n or not a.lib:   # the baseline library has no setter
                self.ctx.set_max_features(n)

    parts = [Part(0, B // 2, torch.cuda.Stream()), Part(B // 2, B - B // 2, torch.cuda.Stream())]
    for p in parts:
        p.ctx.synth_images(imgs[p.b0].data_ptr(), p.nb, R, C, C, R * C, seed_base=p.b0)
    torch.cuda.synchronize()

    def timed(n):
        for p in parts:
            p.budget(n)
        for _ in range(a.warmup):
            for p in parts:
                p.step()
        for p in parts:
            p.ctx.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            for p in parts:
                p.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        for p in parts:
            p.ctx.sync()   # raises if a capacity overflowed
        return 1e3 * dt / a.steps, sum(int(p.o[-1].item()) for p in parts)

    ms = {n: [] for n in budgets}
    kept = {}
    for _ in range(a.rounds):
        for n in budgets:
            t, kept[n] = timed(n)
            ms[n].append(t)
    res = {"lib": a.lib or "this build", "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "ms_per_step": {str(n): [statistics.median(v), min(v), max(v)] for n, v in ms.items()},
           "kept": {str(n): kept[n] for n in budgets}}
    for p in parts:
        p.ctx.close()
    del parts
    if not a.lib:
        # per-stage device times: one whole-batch context, launches serial
        prof = Part(0, B, torch.cuda.Stream(), flags=siftgpu.SIFT_FLAG_PROFILE)
        d8 = torch.zeros((prof.cap, 128), dtype=torch.uint8, device="cuda")
        mi = torch.empty((prof.cap, 2), dtype=torch.int32, device="cuda")
        md = torch.empty((prof.cap, 2), dtype=torch.float32, device="cuda")
        res["stages"], res["match_ms"] = {}, {}
        for n in budgets:
            prof.budget(n)
            for _ in range(2):
                prof.step()
            prof.ctx.sync()
            prof.ctx.stage_stats(reset=True)
            for _ in range(a.steps):
                prof.step()
            prof.ctx.sync()
            res["stages"][str(n)] = {k: v["ms"] / a.steps for k, v in prof.ctx.stage_stats(reset=True).items()}
            # the matcher on the kept rows: frame b against frame b + 1
            with torch.cuda.stream(prof.strm):
                prof.ctx.descriptors_to_u8_device(prof.d.data_ptr(), prof.o.data_ptr() + 4 * B, prof.cap, d8.data_ptr())
                ev = []
                for it in range(13):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(prof.strm)
                    prof.ctx.knn_match_l2sqr_u8_segmented_device(d8.data_ptr(), prof.o.data_ptr(), B - 1, prof.cap,
                                                                 d8.data_ptr(), prof.o.data_ptr() + 4, prof.cap, 2,
                                                                 mi.data_ptr(), md.data_ptr())
                    e1.record(prof.strm)
                    e1.synchronize()
                    if it >= 3:
                        ev.append(e0.elapsed_time(e1))
            prof.ctx.sync()
            prof.ctx.stage_stats(reset=True)   # the matcher's stages are not the detection's
            res["match_ms"][str(n)] = statistics.median(ev)
        seg = np.diff(prof.o.cpu().numpy())
        res["last_segments"] = [int(seg.min()), int(statistics.median(seg.tolist())), int(seg.max())]
        prof.ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(a, lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--rounds", str(a.rounds)] + (["--lib", lib] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=WORKER_TIMEOUT)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(f"worker failed ({r.returncode}); nothing further is started")
    return json.loads(line[0][7:])


def fmt3(v):
    return f"{v[0]:8.3f} [{v[1]:7.3f}, {v[2]:7.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "max_features_ab.txt"))
    ap.add_argument("--baseline-lib", default=None, help="libsift_hip.so of the parent commit (n = 0 A/B)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    out = [f"# Per-image keypoint budget (sift_set_max_features) on {B} x {R}x{C}, exact mode, 5 octaves\n"
           f"# written by tools/bench_max_features.py; one session, one device\n"
           f"# ms/step: wall clock, 2 contexts x {B // 2} images on 2 streams, {a.steps} steps after {a.warmup} warm-up, "
           f"median of {a.rounds} interleaved rounds [min, max]"]
    base = []
    if a.baseline_lib:
        # parent, this build, parent: each in its own process
        base.append(run_worker(a, os.path.abspath(a.baseline_lib)))
    new = run_worker(a, None)
    if a.baseline_lib:
        base.append(run_worker(a, os.path.abspath(a.baseline_lib)))
        out.append("## the option off (n = 0) against the parent commit's build")
        for i, b in enumerate(base):
            out.append(f"parent build, run {i + 1}   {fmt3(b['ms_per_step']['0'])} ms/step, {b['kept']['0']} keypoints")
        out.append(f"this build, n = 0      {fmt3(new['ms_per_step']['0'])} ms/step, {new['kept']['0']} keypoints")
        pm = statistics.mean(b["ms_per_step"]["0"][0] for b in base)
        out.append(f"this build / parent (mean of its runs) = {new['ms_per_step']['0'][0] / pm:.4f}")
    out.append("## ms/step and kept keypoints per budget")
    out.append(f"{'n':>6} {'ms/step  [min, max]':>28} {'vs n=0':>8} {'kept':>9} {'match l2sqr u8 ms':>18}")
    m0 = new["ms_per_step"]["0"][0]
    for n in BUDGETS:
        v = new["ms_per_step"][str(n)]
        out.append(f"{n:>6} {fmt3(v):>28} {v[0] / m0:8.4f} {new['kept'][str(n)]:>9} {new['match_ms'][str(n)]:18.3f}")
    out.append(f"# keypoints per image at the last budget: min/median/max {new['last_segments']}")
    out.append(f"## per-stage device ms per step (SIFT_FLAG_PROFILE: one context of {B} images, launches serial)")
    names = sorted({k for s in new["stages"].values() for k in s}, key=lambda k: -new["stages"]["0"].get(k, 0.0))
    out.append(f"{'stage':>20} " + " ".join(f"{'n=' + str(n):>10}" for n in BUDGETS))
    for k in names:
        out.append(f"{k:>20} " + " ".join(f"{new['stages'][str(n)][k]:10.3f}" if k in new["stages"][str(n)] else f"{'-':>10}"
                                          for n in BUDGETS))   # '-': the stage did not run
    out.append(f"{'sum':>20} " + " ".join(f"{sum(new['stages'][str(n)].values()):10.3f}" for n in BUDGETS))
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
