#!/usr/bin/env python3
"""What lens undistortion costs on the headline batch, against the library's own yardsticks.

Images: sift_undistort_batch_device on 64 x 1080x1920 -> 1080x1920, float32 and uint8 x 3, one
shared camera and a camera per image, zero distortion and k1 = -0.2.  Yardsticks, in the same
process on the same device: sift_warp_perspective_segmented_device with an identity H on the
same batch (the same algorithmic bytes: 8 B per float32 pixel, 6 B per uint8 x 3 pixel) and
sift_upsample2x_device (20 B per source pixel), as tools/bench_warp.py.

Points: sift_undistort_points_segmented_device on 64 segments of 300 and of 4000 rows against the
host loop a caller runs today: copy the rows to the host, wait, sift_undistort_points per segment.

Milliseconds are HIP events on the context stream around --reps launches; median [min, max] over
--rounds rounds after a warm-up.  Before anything is timed the device results are checked against
tests/undistort_oracle.py (image 0 of each pixel type and camera) and the host point path.

--lib NAME=PATH (repeatable) times further builds of the library (tools/build_var.sh on
csrc/undistort.hip: -DSIFT_UNDISTORT_GROUP=, -DSIFT_UNDISTORT_ROWS=), one child process each.

  python tools/bench_undistort.py [--lib group4=sift-gpu_amd/lib/libsift_hip_group4.so ...]
                                  [--out profiles/undistort_ab.txt]
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
WORKER_TIMEOUT = 400


def worker(a):
    import numpy as np
    import torch
    sys.path.insert(0, PKG)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import siftgpu
    if a.worker_lib:
        siftgpu.LIB_PATH = a.worker_lib
    import undistort_oracle as UO
    strm = torch.cuda.Stream()
    ctx = siftgpu.Context(R, C, B, device=0)
    ctx.set_stream(strm.cuda_stream)
    res = {"lib": a.worker_lib or "this build", "reps": a.reps, "rounds": a.rounds, "ok": True}

    def timed(fn, reps=a.reps):
        with torch.cuda.stream(strm):
            for _ in range(3):
                fn()
            ms = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / reps)
        return {"ms": statistics.median(ms), "min": min(ms), "max": max(ms)}

    with torch.cuda.stream(strm):
        f32 = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
        ctx.synth_images(f32.data_ptr(), B, R, C, C, R * C, seed_base=0)
        ctx.sync()
        u8 = (f32.clamp(0, 255)).to(torch.uint8).unsqueeze(-1).repeat(1, 1, 1, 3).contiguous()
        u8[..., 1] += 7
        u8[..., 2] += 19
    torch.cuda.synchronize()

    up = torch.empty((B, 2 * R, 2 * C), dtype=torch.float32, device="cuda")
    y = timed(lambda: ctx.upsample2x_device(f32.data_ptr(), B, R, C, C, R * C, up.data_ptr(), 2 * C, 4 * R * C))
    y["tb_per_s"] = 20.0 * B * R * C / (y["ms"] * 1e-3) / 1e12
    res["upsample2x"] = y
    del up

    K = np.array([[1500.0, 0, (C - 1) / 2], [0, 1500.0, (R - 1) / 2], [0, 0, 1]])
    dists = {"zero": np.zeros(8), "k1-0.2": np.array([-0.2, 0, 0, 0, 0, 0, 0, 0.0])}
    eye = torch.from_numpy(np.tile(np.eye(3).reshape(1, 9), (B, 1))).cuda()
    for kind, src, pixel, ch, bpp in (("f32", f32, 0, 1, 4), ("u8x3", u8, 1, 3, 3)):
        dst = torch.empty_like(src)
        nbytes = 2.0 * bpp * B * R * C
        t = timed(lambda: ctx.warp_perspective_segmented_device(pixel, ch, src.data_ptr(), R, C, 0, R * C * bpp,
                                                                eye.data_ptr(), 0, B, 0, dst.data_ptr(), R, C, 0, 0))
        t["tb_per_s"] = nbytes / (t["ms"] * 1e-3) / 1e12
        res[f"{kind} warp identity"] = t
        for dname, d in dists.items():
            for per in (0, 1):
                Kt = torch.from_numpy(np.tile(K.reshape(1, 9), (B if per else 1, 1))).cuda()
                dt = torch.from_numpy(np.tile(d.reshape(1, 8), (B if per else 1, 1))).cuda()

                def call():
                    ctx.undistort_batch_device(pixel, ch, src.data_ptr(), R, C, 0, R * C * bpp, Kt.data_ptr(),
                                               dt.data_ptr(), 0, per, B, dst.data_ptr(), R, C, 0, 0)
                with torch.cuda.stream(strm):
                    dst.fill_(1)
                    call()
                    ctx.sync()
                want = UO.undistort_ref(src[0].cpu().numpy(), K, d)
                same = dst[0].cpu().numpy().tobytes() == want.tobytes()
                if dname == "zero":
                    same = same and bool(torch.equal(dst.view(torch.uint8), src.view(torch.uint8)))
                name = f"{kind} {'per-image' if per else 'shared'} {dname}"
                if not same:
                    res["ok"] = False
                    res["failed"] = name
                    print("RESULT " + json.dumps(res))
                    return
                t = timed(call)
                t["tb_per_s"] = nbytes / (t["ms"] * 1e-3) / 1e12
                res[name] = t
        del dst

    # points: the device call against the host loop a caller runs today
    lib = siftgpu.lib()
    import ctypes
    pdbl = ctypes.POINTER(ctypes.c_double)
    d = np.array([-0.2, 0.05, 1e-3, -5e-4, 0, 0, 0, 0.0])
    for per_seg in (300, 4000):
        n = B * per_seg
        rng = np.random.default_rng(per_seg)
        xy = np.stack([rng.uniform(0, C - 1, n), rng.uniform(0, R - 1, n)], 1).astype(np.float32)
        offs = (np.arange(B + 1) * per_seg).astype(np.int32)
        dxy, dmo = torch.from_numpy(xy).cuda(), torch.from_numpy(offs).cuda()
        dK, dD = torch.from_numpy(K.reshape(9)).cuda(), torch.from_numpy(d).cuda()
        out, ok = torch.empty_like(dxy), torch.zeros(B, dtype=torch.int32, device="cuda")
        pinned, host_out = torch.empty((n, 2), dtype=torch.float32).pin_memory(), np.empty((n, 2), np.float32)

        def dev():
            ctx.undistort_points_segmented_device(dxy.data_ptr(), out.data_ptr(), 8, dmo.data_ptr(), B, n,
                                                  dK.data_ptr(), dD.data_ptr(), dK.data_ptr(), 0, 5, ok.data_ptr())

        def host():
            with torch.cuda.stream(strm):
                pinned.copy_(dxy, non_blocking=True)
            strm.synchronize()
            src = pinned.numpy()
            for b in range(B):
                lo = b * per_seg
                lib.sift_undistort_points(K.ctypes.data_as(pdbl), d.ctypes.data_as(pdbl), K.ctypes.data_as(pdbl), 5,
                                          src[lo:].ctypes.data, host_out[lo:].ctypes.data, 8, per_seg)
        with torch.cuda.stream(strm):
            dev()
            ctx.sync()
        host()
        if out.cpu().numpy().tobytes() != host_out.tobytes():
            res["ok"] = False
            res["failed"] = f"points {per_seg}"
            break
        res[f"points 64x{per_seg} device"] = timed(dev)
        w = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            host()
            w.append((time.perf_counter() - t0) * 1e3)
        res[f"points 64x{per_seg} host loop"] = {"ms": statistics.median(w), "min": min(w), "max": max(w)}
    ctx.close()
    print("RESULT " + json.dumps(res))


def run_child(a, lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--reps", str(a.reps), "--rounds", str(a.rounds)]
    if lib:
        cmd += ["--worker-lib", lib]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=WORKER_TIMEOUT)
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise SystemExit(f"worker failed ({r.returncode}) for {lib or 'this build'}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--worker-lib", default="")
    ap.add_argument("--lib", action="append", default=[], help="NAME=PATH of a further build to time")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--passes", type=int, default=1)
    ap.add_argument("--box", default="MI355X")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort_ab.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    builds = [("this build", "")] + [tuple(s.split("=", 1)) for s in a.lib]
    out = [f"# sift_undistort_batch_device on {B} x {R}x{C} -> {R}x{C}, and sift_undistort_points_segmented_device; "
           f"box: {a.box}",
           "# written by tools/bench_undistort.py; one session, one device; ms = median [min, max] of "
           f"{a.rounds} rounds of {a.reps} launches (host loop: wall clock of {a.rounds} runs)",
           "# TB/s = algorithmic bytes (f32 8 B, u8x3 6 B per destination pixel) per second; "
           "x warp = the identity warp's milliseconds over this line's", ""]
    for p in range(a.passes):
        for name, lib in builds:
            r = run_child(a, os.path.abspath(lib) if lib else "")
            y = r["upsample2x"]
            out.append(f"## pass {p + 1}: {name}" + (f" ({os.path.relpath(os.path.abspath(lib), ROOT)})" if lib else ""))
            out.append(f"upsample2x yardstick: {y['ms']:.4f} ms [{y['min']:.4f}, {y['max']:.4f}]  {y['tb_per_s']:.3f} TB/s")
            out.append(f"device results equal the restatement and the host path before timing: {r['ok']}"
                       + ("" if r["ok"] else f" (failed at {r.get('failed')})"))
            out.append(f"{'case':<30}{'ms':>10}{'[min':>10}{'max]':>10}{'TB/s':>9}{'x warp':>9}")
            for k, t in r.items():
                if not isinstance(t, dict) or k == "upsample2x":
                    continue
                kind = k.split()[0]
                ref = r.get(f"{kind} warp identity")
                tb = f"{t['tb_per_s']:>9.3f}" if "tb_per_s" in t else f"{'':>9}"
                xw = f"{ref['ms'] / t['ms']:>9.3f}" if ref and "tb_per_s" in t else f"{'':>9}"
                out.append(f"{k:<30}{t['ms']:>10.4f}{t['min']:>10.4f}{t['max']:>10.4f}{tb}{xw}")
            out.append("")
            print("\n".join(out[-24:]), flush=True)
            if not r["ok"]:
                raise SystemExit("a device result differs from the rule: nothing further is started")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
