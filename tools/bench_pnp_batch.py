#!/usr/bin/env python3
"""A/B of the absolute pose of a batch (PnP RANSAC over P3P): the segmented
device call against the host loop it replaces, beside the fundamental-matrix
estimate on the same rows for scale, and the round size kPnpRound across saved
builds.

The workload is synthetic: 64 segments of 300 and of 4000 rows.  The first two
views are bench_pose_batch.py's scene (bench_fundamental_batch.py's two_views:
0.5 px of jitter, 30 % outliers); F, the relative pose, d_xyz and d_mask_out are
the segmented calls' own, left on the device.  A third view under a planted pose
sees point i in row i, with 0.5 px of jitter and 30 % of its rows moved 50 to
300 px away.  One child process per library (its own timeout) times,
alternating, with HIP events on the context's stream (5 warm-up iterations,
medians of 20):

  PNP        sift_solve_pnp_segmented_device on the device-resident d_xyz,
             d_mask_out and third-view pixels: one enqueue, no host value
  PNP_HOST   the flow a caller has without it: offsets, d_xyz, the mask and the
             pixels are copied to the host, the stream is waited for, and
             sift_solve_pnp runs per segment on the CPU (copy and wait inside
             the window)
  FUND       sift_find_fundamental_segmented_device on the same rows

The device leg's pose, found, n_inliers and mask must equal the host loop's byte
for byte before anything is timed.  --variant NAME=PATH (repeatable) adds a child
that loads that library -- a build with another SIFT_PNP_ROUND -- and times PNP;
--resources FILE copies the compiler's kernel-resource-usage remarks into the
report.

  python tools/bench_pnp_batch.py [--variant R64=PATH ...] [--resources FILE] [--out profiles/pnp_batch_ab.txt]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
S, TIMEOUT = 64, 420
WORKLOADS = (("300 rows", 300), ("4000 rows", 4000))
THR, MAX_ITERS, CONF = 8.0, 100, 0.99     # OpenCV's defaults for solvePnPRansac


def third_view(np, seed, n, out_frac, noise=0.5):
    """The pixels of two_views' 3-D points (its first draws) in a third camera."""
    K = np.array([[1200.0, 0, 960], [0, 1200, 540], [0, 0, 1]])
    ay, ax = np.deg2rad(-6.0), np.deg2rad(3.0)
    R = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]]) @ \
        np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    t = np.array([0.8, -0.15, 0.3])
    rng = np.random.default_rng(seed)
    P = np.c_[rng.uniform(-3, 3, n), rng.uniform(-1.7, 1.7, n), rng.uniform(4, 10, n)]
    rng = np.random.default_rng(seed + 100000)
    c = (P @ R.T + t) @ K.T
    xy = c[:, :2] / c[:, 2:] + rng.uniform(-noise, noise, (n, 2))
    bad = rng.permutation(n)[:int(round(n * out_frac))]
    ang = rng.uniform(0, 2 * np.pi, len(bad))
    xy[bad] += rng.uniform(50, 300, len(bad))[:, None] * np.c_[np.cos(ang), np.sin(ang)]
    return xy.astype(np.float32)


def worker(lib_path, iters, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "sift-gpu_amd"))
    import siftgpu
    from bench_fundamental_batch import two_views
    variant = bool(lib_path)
    if variant:
        siftgpu.LIB_PATH = lib_path
    K = np.array([1200.0, 0, 960, 0, 1200, 540, 0, 0, 1])
    strm = torch.cuda.Stream()
    ctx = siftgpu.Context(64, 64, 1, device=0)
    ctx.set_stream(strm.cuda_stream)
    L = siftgpu.lib()
    out = {}
    fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    with torch.cuda.stream(strm):
        for name, per in WORKLOADS:
            cap = S * per
            pairs = [two_views(np, 1000 + b, per, 0.3) for b in range(S)]
            sxy = torch.from_numpy(np.concatenate([p[0] for p in pairs])).cuda()
            dxy = torch.from_numpy(np.concatenate([p[1] for p in pairs])).cuda()
            xy3 = torch.from_numpy(np.concatenate([third_view(np, 1000 + b, per, 0.3) for b in range(S)])).cuda()
            moff = torch.from_numpy(np.arange(S + 1, dtype=np.int32) * per).cuda()
            dK = torch.from_numpy(K).cuda()
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
            dF, df, dm = z((S, 9), torch.float64), z((S,), torch.int32), z((cap,), torch.uint8)
            dP, dpf, dng = z((S, 12), torch.float64), z((S,), torch.int32), z((S,), torch.int32)
            dmo, dxyz = z((cap,), torch.uint8), z((cap, 3), torch.float64)
            d3, d3f, d3n, d3m = z((S, 12), torch.float64), z((S,), torch.int32), z((S,), torch.int32), z((cap,), torch.uint8)
            pin = lambda shape, dt: torch.empty(shape, dtype=dt).pin_memory()  # noqa: E731
            h_moff, h_xyz, h_xy = pin((S + 1,), torch.int32), pin((cap, 3), torch.float64), pin((cap, 2), torch.float32)
            h_m = pin((cap,), torch.uint8)
            b3, b3f, b3n, b3m = np.zeros((S, 12)), np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(cap, np.uint8)
            strm.synchronize()

            def fund():
                ctx.find_fundamental_segmented_device(sxy.data_ptr(), dxy.data_ptr(), moff.data_ptr(), S, cap,
                                                      dF.data_ptr(), df.data_ptr(), dm.data_ptr())

            def pose():
                ctx.recover_pose_segmented_device(sxy.data_ptr(), dxy.data_ptr(), moff.data_ptr(), S, cap,
                                                  dF.data_ptr(), df.data_ptr(), dK.data_ptr(), dK.data_ptr(),
                                                  dP.data_ptr(), dpf.data_ptr(), dng.data_ptr(), 0, dm.data_ptr(),
                                                  50.0, None, dmo.data_ptr(), dxyz.data_ptr())

            def device():
                ctx.solve_pnp_segmented_device(dxyz.data_ptr(), xy3.data_ptr(), moff.data_ptr(), S, cap, dK.data_ptr(),
                                               d3.data_ptr(), d3f.data_ptr(), d3n.data_ptr(), 0, dmo.data_ptr(), THR,
                                               MAX_ITERS, CONF, d3m.data_ptr())

            def host():
                for h, d in ((h_moff, moff), (h_xyz, dxyz), (h_xy, xy3), (h_m, dmo)):
                    h.copy_(d, non_blocking=True)
                strm.synchronize()
                ho = h_moff.numpy()
                x0, p0, m0 = h_xyz.data_ptr(), h_xy.data_ptr(), h_m.data_ptr()
                ni = ctypes.c_int(0)
                for b in range(S):
                    lo, n = int(ho[b]), int(ho[b + 1] - ho[b])
                    rc = L.sift_solve_pnp(ctypes.cast(x0 + lo * 24, dp), ctypes.cast(p0 + lo * 8, fp), n, m0 + lo,
                                          K.ctypes.data_as(dp), THR, MAX_ITERS, CONF,
                                          ctypes.cast(b3[b].ctypes.data, dp), b3m.ctypes.data + lo, ctypes.byref(ni))
                    b3f[b], b3n[b] = (1, ni.value) if rc == 0 else (0, 0)

            fund()
            pose()
            device()
            host()
            ctx.sync()
            g = lambda t: t.cpu().numpy().tobytes()  # noqa: E731
            same = bool(g(d3) == b3.tobytes() and g(d3f) == b3f.tobytes() and g(d3n) == b3n.tobytes()
                        and g(d3m) == b3m.tobytes())
            assert same, f"{name}: the device call and the host loop differ"
            census = {"found": int(b3f.sum()), "inliers": int(b3n.sum()), "rows": int(dmo.sum().item())}
            legs = {"PNP": device} if variant else {"PNP": device, "PNP_HOST": host, "FUND": fund}
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
            out[name] = {"census": census,
                         "event_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in ev.items()},
                         "wall_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in wall.items()}}
    print("RESULT " + json.dumps({"iters": iters, "warmup": warmup, "workloads": out}), flush=True)
    ctx.close()


def run_worker(args, lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--iters", str(args.iters), "--warmup",
           str(args.warmup)] + (["--lib", lib] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=TIMEOUT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(f"worker failed ({r.returncode}); nothing further is started")
    return json.loads(line[0][7:])


def rows(w, names, tag=""):
    out = []
    for k in names:
        e, wl = w["event_ms"][k], w["wall_ms"][k]
        out.append(f"{tag + k:16} {e[0]:10.3f} [{e[1]:9.3f}, {e[2]:9.3f}] {wl[0]:10.3f} [{wl[1]:9.3f}, {wl[2]:9.3f}]")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_batch_ab.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of a saved libsift_hip.so")
    ap.add_argument("--resources", default="", help="a file of kernel-resource-usage remarks to copy in")
    ap.add_argument("--lib", default="")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.lib, a.iters, a.warmup)
    r = run_worker(a, "")
    variants = [(v.split("=", 1)[0], run_worker(a, v.split("=", 1)[1])) for v in a.variant]
    parts = ["# Absolute pose of a whole batch: segmented device call (PNP) vs copy to the host + loop of",
             "# sift_solve_pnp (PNP_HOST), and the fundamental-matrix estimate on the same rows (FUND)",
             "# written by tools/bench_pnp_batch.py", "",
             f"{S} segments; d_xyz and the row mask from the segmented pose recovery, a third view with 0.5 px of jitter "
             f"and 30 % outliers; thr {THR}, max_iters {MAX_ITERS}, confidence {CONF}",
             "the device leg == the host loop byte for byte (pose, found, n_inliers, mask): True",
             f"medians of {r['iters']} iterations after {r['warmup']} warm-up [min, max], ms",
             "round-size variants: " + (", ".join(t for t, _ in variants) if variants else "not measured in this run")]
    for name, per in WORKLOADS:
        w = r["workloads"][name]
        c = w["census"]
        parts += ["", f"## {S} x {name}: models found {c['found']} of {S}, inliers {c['inliers']} of {c['rows']} "
                      f"unmasked rows of {S * per}", f"{'leg':16} {'HIP events':>32} {'host wall':>32}"]
        parts += rows(w, ["PNP", "PNP_HOST", "FUND"])
        e = w["event_ms"]
        parts.append(f"PNP_HOST / PNP = {e['PNP_HOST'][0] / e['PNP'][0]:.1f}; host per segment "
                     f"{e['PNP_HOST'][0] / S:.3f} ms; PNP / FUND = {e['PNP'][0] / e['FUND'][0]:.3f} (events)")
        for tag, v in variants:
            parts += rows(v["workloads"][name], ["PNP"], tag + " ")
    if a.resources:
        parts += ["", "## pnp_ransac_kernel, -Rpass-analysis=kernel-resource-usage (gfx950)"]
        parts += [ln.strip() for ln in open(a.resources).read().splitlines() if "remark:" in ln]
    text = "\n".join(parts) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
