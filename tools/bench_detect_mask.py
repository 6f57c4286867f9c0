#!/usr/bin/env python3
"""What the detection mask (sift_detect_compute_batch_masked) costs and saves on
the headline batch: 64 synthetic 1080p images, exact mode, 5 octaves.

One child process per leg (its own timeout; nothing further is started after a
failure).  A leg measures, for each mask in none, ones (everything kept: the
cost of the stage alone), half (one shared mask keeping the left half plane,
mask_img_stride = 0) and window (a shared 480 x 640 window):

  ms/step   wall clock over --steps steps after --warmup, the batch split over
            two contexts on two streams as bench.py's timed leg does; the legs
            of all masks are interleaved over --rounds rounds and the median
            round is reported with [min, max];
  stages    one whole-batch context with SIFT_FLAG_PROFILE (launches run
            serially, HIP events per stage): ms per step of every stage;
  kept      the batch's keypoint total (d_img_offsets[batch]).

--baseline-lib names a libsift_hip.so built from the parent commit: its
unmasked ms/step is measured in the same session, alternating with this
build's, as the A/B of "no mask changes nothing".

  python tools/bench_detect_mask.py [--baseline-lib PATH] [--out profiles/detect_mask_ab.txt]
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
MASKS = ("none", "ones", "half", "window")
PER_IMG = 40000   # output rows per image, bench.py's sizing
WORKER_TIMEOUT = 420


def worker(a):
    import torch
    sys.path.insert(0, PKG)
    import siftgpu
    if a.lib:
        siftgpu.LIB_PATH = a.lib
    names = ("none",) if a.lib else MASKS   # the baseline library has no masked entry point
    imgs = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
    masks = {"none": None, "ones": torch.ones((R, C), dtype=torch.uint8, device="cuda"),
             "half": torch.zeros((R, C), dtype=torch.uint8, device="cuda"),
             "window": torch.zeros((R, C), dtype=torch.uint8, device="cuda")}
    masks["half"][:, :C // 2] = 1
    masks["window"][300:780, 640:1280] = 1

    class Part:
        def __init__(self, b0, nb, strm, flags=0):
            self.b0, self.nb, self.strm, self.cap = b0, nb, strm, nb * PER_IMG
            self.ctx = siftgpu.Context(R, C, nb, device=0, flags=flags)
            self.ctx.set_stream(strm.cuda_stream)
            self.k = torch.empty((self.cap, 7), dtype=torch.int32, device="cuda")
            self.d = torch.empty((self.cap, 128), dtype=torch.float32, device="cuda")
            self.o = torch.empty((nb + 1,), dtype=torch.int32, device="cuda")

        def step(self, name):
            m = masks[name]
            kw = {} if m is None else dict(masks_ptr=m.data_ptr(), mask_row_stride=C, mask_img_stride=0)
            self.ctx.detect_compute_batch(imgs[self.b0].data_ptr(), self.nb, R, C, C, R * C, self.k.data_ptr(),
                                          self.d.data_ptr(), self.cap, self.o.data_ptr(), **kw)

    parts = [Part(0, B // 2, torch.cuda.Stream()), Part(B // 2, B - B // 2, torch.cuda.Stream())]
    for p in parts:
        p.ctx.synth_images(imgs[p.b0].data_ptr(), p.nb, R, C, C, R * C, seed_base=p.b0)
    torch.cuda.synchronize()

    def timed(name):
        for _ in range(a.warmup):
            for p in parts:
                p.step(name)
        for p in parts:
            p.ctx.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            for p in parts:
                p.step(name)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        for p in parts:
            p.ctx.sync()   # raises if a capacity overflowed
        return 1e3 * dt / a.steps, sum(int(p.o[-1].item()) for p in parts)

    ms = {n: [] for n in names}
    kept = {}
    for _ in range(a.rounds):
        for n in names:
            t, kept[n] = timed(n)
            ms[n].append(t)
    res = {"lib": a.lib or "this build", "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "ms_per_step": {n: [statistics.median(v), min(v), max(v)] for n, v in ms.items()},
           "kept": {n: kept[n] for n in names}}
    for p in parts:
        p.ctx.close()
    del parts
    if not a.lib:
        # per-stage device times: one whole-batch context, launches serial
        prof = Part(0, B, torch.cuda.Stream(), flags=siftgpu.SIFT_FLAG_PROFILE)
        res["stages"] = {}
        for n in names:
            for _ in range(2):
                prof.step(n)
            prof.ctx.sync()
            prof.ctx.stage_stats(reset=True)
            for _ in range(a.steps):
                prof.step(n)
            prof.ctx.sync()
            res["stages"][n] = {k: v["ms"] / a.steps for k, v in prof.ctx.stage_stats(reset=True).items()}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_mask_ab.txt"))
    ap.add_argument("--baseline-lib", default=None, help="libsift_hip.so of the parent commit (unmasked A/B)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    out = [f"# Detection mask (sift_detect_compute_batch_masked) on {B} x {R}x{C}, exact mode, 5 octaves\n"
           f"# written by tools/bench_detect_mask.py; one session, one device\n"
           f"# masks (one shared by the batch): ones = all kept, half = columns < {C // 2}, window = rows 300..779 x "
           f"columns 640..1279\n"
           f"# ms/step: wall clock, 2 contexts x {B // 2} images on 2 streams, {a.steps} steps after {a.warmup} warm-up, "
           f"median of {a.rounds} interleaved rounds [min, max]"]
    base = []
    if a.baseline_lib:
        # parent, this build, parent: each in its own process
        base.append(run_worker(a, os.path.abspath(a.baseline_lib)))
    new = run_worker(a, None)
    if a.baseline_lib:
        base.append(run_worker(a, os.path.abspath(a.baseline_lib)))
        out.append("## no mask against the parent commit's build")
        for i, b in enumerate(base):
            out.append(f"parent build, run {i + 1}   {fmt3(b['ms_per_step']['none'])} ms/step, "
                       f"{b['kept']['none']} keypoints")
        out.append(f"this build, no mask    {fmt3(new['ms_per_step']['none'])} ms/step, {new['kept']['none']} keypoints")
        pm = statistics.mean(b["ms_per_step"]["none"][0] for b in base)
        out.append(f"this build / parent (mean of its runs) = {new['ms_per_step']['none'][0] / pm:.4f}")
    out.append("## ms/step and kept keypoints per mask")
    out.append(f"{'mask':>8} {'ms/step  [min, max]':>28} {'vs none':>8} {'kept':>9} {'share':>7}")
    m0, k0 = new["ms_per_step"]["none"][0], new["kept"]["none"]
    for n in MASKS:
        v = new["ms_per_step"][n]
        out.append(f"{n:>8} {fmt3(v):>28} {v[0] / m0:8.4f} {new['kept'][n]:>9} {new['kept'][n] / k0:7.3f}")
    out.append(f"## per-stage device ms per step (SIFT_FLAG_PROFILE: one context of {B} images, launches serial)")
    names = sorted({k for s in new["stages"].values() for k in s}, key=lambda k: -new["stages"]["none"].get(k, 0.0))
    out.append(f"{'stage':>20} " + " ".join(f"{n:>10}" for n in MASKS))
    for k in names:
        out.append(f"{k:>20} " + " ".join(f"{new['stages'][n][k]:10.3f}" if k in new["stages"][n] else f"{'-':>10}"
                                          for n in MASKS))   # '-': the stage did not run
    out.append(f"{'sum':>20} " + " ".join(f"{sum(new['stages'][n].values()):10.3f}" for n in MASKS))
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
