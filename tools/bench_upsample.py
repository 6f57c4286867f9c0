#!/usr/bin/env python3
"""What the upsampled first octave (sift_set_upsample) costs on the headline
batch: 64 synthetic 1080p images, exact mode, 5 octaves.

One child process per leg (its own timeout; nothing further is started after a
failure).  This build's leg measures:

  kernel    sift_upsample2x_device on the 64 images (HIP events around --reps
            launches), next to its byte floor of 20 B per source pixel, and a
            check that its output equals the same rule written in torch ops;
  plain     the setting off on the 1080p images -- bench.py's timed leg: wall
            clock over --steps steps after --warmup, the batch split over two
            contexts on two streams;
  up        the setting on, the same images;
  pre       the setting off on the images already doubled (2160 x 3840): the
            same work without the doubling kernel, so up - pre is what the
            feature costs;
  keypoints per image of plain and up (d_img_offsets[batch] / 64).

The legs are interleaved over --rounds rounds; the median round is reported
with [min, max].  --baseline-lib names a libsift_hip.so built from the parent
commit: its plain and pre legs are measured in the same session, before and
after this build's, as the A/B of "the setting off changes nothing" and of the
parent's pipeline on the doubled images.

  python tools/bench_upsample.py [--baseline-lib PATH] [--out profiles/upsample_ab.txt]
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
PER_IMG = 40000       # output rows per 1080p image, bench.py's sizing
PER_IMG_UP = 120000   # ... per doubled image
WORKER_TIMEOUT = 540


def double_torch(x):
    """The rule of sift_upsample2x in torch ops (each a * w0 + b * w1 unfused), [B, R, C] -> [B, 2R, 2C]."""
    import torch

    def axis(s, dim):
        s = s.movedim(dim, 0)
        n = s.shape[0]
        d = torch.empty((2 * n,) + tuple(s.shape[1:]), dtype=s.dtype, device=s.device)
        d[0] = s[0]
        d[2 * n - 1] = s[n - 1]
        if n > 1:
            d[1:2 * n - 1:2] = s[:-1] * 0.75 + s[1:] * 0.25   # odd d:  s = (d - 1) / 2
            d[2:2 * n - 1:2] = s[:-1] * 0.25 + s[1:] * 0.75   # even d: s = d / 2 - 1
        return d.movedim(0, dim)

    return axis(axis(x, 2), 1).contiguous()


def worker(a):
    import torch
    sys.path.insert(0, PKG)
    import siftgpu
    if a.lib:
        siftgpu.LIB_PATH = a.lib
    legs = ("plain", "pre") if a.lib else ("plain", "up", "pre")   # the baseline library has no such setting
    imgs = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
    res = {"lib": a.lib or "this build", "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds}

    class Part:
        def __init__(self, b0, nb, strm, rows, cols, per_img):
            self.b0, self.nb, self.strm, self.cap = b0, nb, strm, nb * per_img
            self.ctx = siftgpu.Context(rows, cols, nb, device=0)
            self.ctx.set_stream(strm.cuda_stream)
            self.k = torch.empty((self.cap, 7), dtype=torch.int32, device="cuda")
            self.d = torch.empty((self.cap, 128), dtype=torch.float32, device="cuda")
            self.o = torch.empty((nb + 1,), dtype=torch.int32, device="cuda")

        def step(self, leg):
            src, r, c = (big, 2 * R, 2 * C) if leg == "pre" else (imgs, R, C)
            self.ctx.detect_compute_batch(src[self.b0].data_ptr(), self.nb, r, c, c, r * c, self.k.data_ptr(),
                                          self.d.data_ptr(), self.cap, self.o.data_ptr())

    # plain runs on contexts of the 1080p shape, as bench.py's does; up and pre on contexts of the doubled shape
    strms = [torch.cuda.Stream(), torch.cuda.Stream()]
    halves = [(0, B // 2), (B // 2, B - B // 2)]
    small = [Part(b0, nb, st, R, C, PER_IMG) for (b0, nb), st in zip(halves, strms)]
    large = [Part(b0, nb, st, 2 * R, 2 * C, PER_IMG_UP) for (b0, nb), st in zip(halves, strms)]
    for p in small:
        p.ctx.synth_images(imgs[p.b0].data_ptr(), p.nb, R, C, C, R * C, seed_base=p.b0)
        p.ctx.sync()
    torch.cuda.synchronize()
    big = double_torch(imgs)
    torch.cuda.synchronize()

    if not a.lib:
        # (a) the doubling kernel alone, and its output against the torch statement of the rule
        ctx = large[0].ctx
        out = torch.empty((B, 2 * R, 2 * C), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(strms[0]):
            for _ in range(3):
                ctx.upsample2x_device(imgs.data_ptr(), B, R, C, C, R * C, out.data_ptr(), 2 * C, 4 * R * C)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                ctx.upsample2x_device(imgs.data_ptr(), B, R, C, C, R * C, out.data_ptr(), 2 * C, 4 * R * C)
            e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        floor_bytes = 20.0 * B * R * C
        res["kernel"] = {"ms": ms, "floor_bytes": floor_bytes, "tb_per_s": floor_bytes / (ms * 1e-3) / 1e12,
                         "equals_torch_rule": bool(torch.equal(out.view(torch.int32), big.view(torch.int32)))}
        del out

    def timed(leg):
        parts = small if leg == "plain" else large
        if not a.lib:
            for p in parts:
                p.ctx.set_upsample(leg == "up")
        for _ in range(a.warmup):
            for p in parts:
                p.step(leg)
        for p in parts:
            p.ctx.sync()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            for p in parts:
                p.step(leg)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        for p in parts:
            p.ctx.sync()   # raises if a capacity overflowed
        return 1e3 * dt / a.steps, sum(int(p.o[-1].item()) for p in parts)

    ms = {n: [] for n in legs}
    kept = {}
    for _ in range(a.rounds):
        for n in legs:
            t, kept[n] = timed(n)
            ms[n].append(t)
    res["ms_per_step"] = {n: [statistics.median(v), min(v), max(v)] for n, v in ms.items()}
    res["keypoints"] = kept
    for p in small + large:
        p.ctx.close()
    print("RESULT " + json.dumps(res), flush=True)


def run_worker(a, lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--steps", str(a.steps), "--warmup", str(a.warmup),
           "--rounds", str(a.rounds), "--reps", str(a.reps)] + (["--lib", lib] if lib else [])
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample_ab.txt"))
    ap.add_argument("--baseline-lib", default=None, help="libsift_hip.so of the parent commit")
    ap.add_argument("--box", default="unnamed", help="the machine's name, recorded in the file")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    out = [f"# Upsampled first octave (sift_set_upsample) on {B} x {R}x{C}, exact mode, 5 octaves; box: {a.box}\n"
           f"# written by tools/bench_upsample.py; one session, one device\n"
           f"# ms/step: wall clock, 2 contexts x {B // 2} images on 2 streams, {a.steps} steps after {a.warmup} warm-up, "
           f"median of {a.rounds} interleaved rounds [min, max]\n"
           f"# plain = setting off, 1080p; up = setting on, 1080p; pre = setting off, the images already doubled "
           f"({2 * R}x{2 * C})"]
    base = []
    if a.baseline_lib:
        base.append(run_worker(a, os.path.abspath(a.baseline_lib)))   # parent, this build, parent
    new = run_worker(a, None)
    if a.baseline_lib:
        base.append(run_worker(a, os.path.abspath(a.baseline_lib)))
    k = new["kernel"]
    out.append("## (a) the doubling kernel alone")
    out.append(f"upsample2x_kernel, {B} x {R}x{C} -> {2 * R}x{2 * C}: {k['ms']:.4f} ms; byte floor "
               f"{k['floor_bytes'] / 1e9:.3f} GB (20 B per source pixel) = {k['tb_per_s']:.2f} TB/s; "
               f"equals the rule in torch ops: {k['equals_torch_rule']}")
    out.append("## (b) an upsampled step against the pipeline on images doubled beforehand")
    m = new["ms_per_step"]
    out.append(f"this build, up      {fmt3(m['up'])} ms/step")
    out.append(f"this build, pre     {fmt3(m['pre'])} ms/step")
    for i, b in enumerate(base):
        out.append(f"parent run {i + 1}, pre   {fmt3(b['ms_per_step']['pre'])} ms/step")
    ref = statistics.mean(b["ms_per_step"]["pre"][0] for b in base) if base else m["pre"][0]
    out.append(f"up - pre (this build) = {m['up'][0] - m['pre'][0]:+.3f} ms/step; up / "
               f"{'parent pre (mean of its runs)' if base else 'pre'} = {m['up'][0] / ref:.4f}")
    out.append("## (c) keypoints per image")
    kp = new["keypoints"]
    out.append(f"setting off {kp['plain'] / B:.1f}, setting on {kp['up'] / B:.1f} ({kp['up'] / kp['plain']:.2f} x); "
               f"pre {kp['pre'] / B:.1f} (the same keypoints as on)")
    out.append("## (d) the setting off against the parent commit's build (bench.py's timed leg)")
    for i, b in enumerate(base):
        out.append(f"parent run {i + 1}, plain {fmt3(b['ms_per_step']['plain'])} ms/step, "
                   f"{b['keypoints']['plain']} keypoints")
    out.append(f"this build, plain   {fmt3(m['plain'])} ms/step, {kp['plain']} keypoints")
    if base:
        pm = statistics.mean(b["ms_per_step"]["plain"][0] for b in base)
        out.append(f"this build / parent (mean of its runs) = {m['plain'][0] / pm:.4f}")
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
