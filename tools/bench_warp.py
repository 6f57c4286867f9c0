#!/usr/bin/env python3
"""What sift_warp_perspective_segmented_device costs on the headline batch:
64 x 1080p warped to 64 x 1080p, float32 and uint8 x 3, one launch per call.

Three homography sets (H maps source to destination, one H per image):

  identity  every pixel reads its own position: the streaming case;
  motion    small inter-frame motions, seeded: a shift of up to 8 pixels, a
            rotation of up to half a degree and a scale within 0.5 % about the
            image centre, and perspective terms up to 1e-6 -- what registering
            frame b to frame b + 1 looks like;
  rot30     a 30 degree rotation about the centre: the worst locality (a
            destination row crosses a source row every two pixels, and a third
            of the destination falls outside the source).

For each: milliseconds (HIP events on the context stream around --reps
launches; median [min, max] over --rounds rounds after a warm-up), algorithmic
bytes per second (8 B per float32 destination pixel, 6 B per uint8 x 3 pixel)
and the ratio to sift_upsample2x_device's bandwidth (20 B per source pixel on
64 x 1080p -> 2160 x 3840), the library's streaming image kernel, measured in
the same process on the same device.  Before anything is timed the identity
warp is checked to reproduce the source bytes.

--lib NAME=PATH (repeatable) times further builds of the library -- the tile
shapes and orderings of csrc/warp.hip built with tools/build_var.sh -- one child
process each (its own timeout; nothing further is started after a failure); the
whole list is run --passes times so that drift shows.

  python tools/bench_warp.py [--lib rows8=sift-gpu_amd/lib/libsift_hip_warp_rows8.so ...]
                             [--out profiles/warp_ab.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sift-gpu_amd")
B, R, C = 64, 1080, 1920
WORKER_TIMEOUT = 240
SETS = ("identity", "motion", "rot30")


def homography_sets():
    import numpy as np

    def about_centre(A):
        t = np.array([[1, 0, (C - 1) / 2], [0, 1, (R - 1) / 2], [0, 0, 1.0]])
        return t @ A @ np.linalg.inv(t)

    def rot(deg, s=1.0):
        a = np.deg2rad(deg)
        return np.array([[s * np.cos(a), -s * np.sin(a), 0], [s * np.sin(a), s * np.cos(a), 0], [0, 0, 1.0]])

    r = np.random.default_rng(0)
    motion = []
    for _ in range(B):
        H = about_centre(rot(r.uniform(-0.5, 0.5), r.uniform(0.995, 1.005)))
        H[:2, 2] += r.uniform(-8, 8, 2)
        H[2, :2] = r.uniform(-1e-6, 1e-6, 2)
        motion.append(H)
    return {"identity": np.stack([np.eye(3)] * B), "motion": np.stack(motion),
            "rot30": np.stack([about_centre(rot(30.0))] * B)}


def worker(a):
    import numpy as np
    import torch
    sys.path.insert(0, PKG)
    import siftgpu
    if a.worker_lib:
        siftgpu.LIB_PATH = a.worker_lib
    strm = torch.cuda.Stream()
    ctx = siftgpu.Context(R, C, B, device=0)
    ctx.set_stream(strm.cuda_stream)
    res = {"lib": a.worker_lib or "this build", "reps": a.reps, "rounds": a.rounds}
    sets = {k: torch.from_numpy(v.reshape(B, 9).copy()).cuda() for k, v in homography_sets().items()}

    def timed(fn):
        with torch.cuda.stream(strm):
            for _ in range(3):
                fn()
            ms = []
            for _ in range(a.rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.reps):
                    fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1) / a.reps)
        return {"ms": statistics.median(ms), "min": min(ms), "max": max(ms)}

    with torch.cuda.stream(strm):
        f32 = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
        ctx.synth_images(f32.data_ptr(), B, R, C, C, R * C, seed_base=0)
        ctx.sync()
        u8 = (f32.clamp(0, 255)).to(torch.uint8).unsqueeze(-1).repeat(1, 1, 1, 3).contiguous()
        u8[..., 1] += 7
        u8[..., 2] += 19
    torch.cuda.synchronize()

    # the yardstick: the streaming image kernel on the same device, the same process
    up = torch.empty((B, 2 * R, 2 * C), dtype=torch.float32, device="cuda")
    y = timed(lambda: ctx.upsample2x_device(f32.data_ptr(), B, R, C, C, R * C, up.data_ptr(), 2 * C, 4 * R * C))
    y["bytes"] = 20.0 * B * R * C
    y["tb_per_s"] = y["bytes"] / (y["ms"] * 1e-3) / 1e12
    res["upsample2x"] = y
    del up

    for kind, src, pixel, ch, bpp in (("f32", f32, 0, 1, 4), ("u8x3", u8, 1, 3, 3)):
        dst = torch.empty_like(src)

        def call(H):
            ctx.warp_perspective_segmented_device(pixel, ch, src.data_ptr(), R, C, 0, R * C * bpp, H.data_ptr(), 0, B,
                                                  0, dst.data_ptr(), R, C, 0, 0)
        with torch.cuda.stream(strm):
            dst.fill_(1)
            call(sets["identity"])
            ctx.sync()
        ok = bool(torch.equal(dst.view(torch.uint8), src.view(torch.uint8)))
        res[f"{kind}_identity_equals_source"] = ok
        if not ok:
            break
        for name in SETS:
            H = sets[name]
            t = timed(lambda: call(H))
            t["bytes"] = 2.0 * bpp * B * R * C
            t["tb_per_s"] = t["bytes"] / (t["ms"] * 1e-3) / 1e12
            t["of_upsample2x"] = t["tb_per_s"] / y["tb_per_s"]
            res[f"{kind}_{name}"] = t
        del dst
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
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--box", default="MI355X")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_ab.txt"))
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    builds = [("this build", "")] + [tuple(s.split("=", 1)) for s in a.lib]
    out = [f"# sift_warp_perspective_segmented_device on {B} x {R}x{C} -> {R}x{C}; box: {a.box}",
           "# written by tools/bench_warp.py; one session, one device; ms = median [min, max] of "
           f"{a.rounds} rounds of {a.reps} launches",
           "# TB/s = algorithmic bytes (f32 8 B, u8x3 6 B per destination pixel) per second; "
           "x up2x = that over sift_upsample2x_device's TB/s in the same process", ""]
    for p in range(a.passes):
        for name, lib in builds:
            r = run_child(a, os.path.abspath(lib) if lib else "")
            y = r["upsample2x"]
            out.append(f"## pass {p + 1}: {name}" + (f" ({os.path.relpath(os.path.abspath(lib), ROOT)})" if lib else ""))
            out.append(f"upsample2x yardstick: {y['ms']:.4f} ms [{y['min']:.4f}, {y['max']:.4f}]  {y['tb_per_s']:.3f} TB/s")
            ok = all(r.get(f"{k}_identity_equals_source") for k in ("f32", "u8x3"))
            out.append(f"identity warp reproduces the source bytes (f32, u8x3): {ok}")
            out.append(f"{'case':<16}{'ms':>10}{'[min':>10}{'max]':>10}{'TB/s':>9}{'x up2x':>9}")
            for kind in ("f32", "u8x3"):
                for s in SETS:
                    t = r.get(f"{kind}_{s}")
                    if t:
                        out.append(f"{kind + ' ' + s:<16}{t['ms']:>10.4f}{t['min']:>10.4f}{t['max']:>10.4f}"
                                   f"{t['tb_per_s']:>9.3f}{t['of_upsample2x']:>9.3f}")
            out.append("")
            print("\n".join(out[-10:]), flush=True)
            if not ok:
                raise SystemExit("the identity warp does not reproduce its source: nothing further is started")
    with open(a.out, "w") as f:
        f.write("\n".join(out))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
