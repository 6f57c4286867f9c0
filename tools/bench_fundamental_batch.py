#!/usr/bin/env python3
"""A/B of the fundamental matrix of a batch: the segmented device estimate
against the host loop it replaces, beside the segmented homography on the same
pairs for scale, and the round size kFundRound across saved builds.

The workload is synthetic: 64 segments of 300 two-view point pairs each (two
pinhole cameras with a baseline and a rotation, 3-D points with depth spread,
0.5 px of jitter; an outlier's dst point is moved off its epipolar line by 50 to
300 px), once with 30 % outliers (the loop ends within one round) and once with
50 % (it runs all max_iters).  One child process per library (its own timeout)
times, alternating, with HIP events on the context's stream (5 warm-up
iterations, medians of 20):

  FUND       sift_find_fundamental_segmented_device on device-resident pairs:
             one enqueue, no host value
  FUND_HOST  the flow a caller has without it: m_offsets and the point pairs are
             copied to the host, the stream is waited for, and
             sift_find_fundamental runs per segment on the CPU (copy and wait
             inside the window)
  HOM        sift_find_homography_segmented_device on the same pairs

The device leg's F, found and mask must equal the host loop's byte for byte
before anything is timed.  --variant NAME=PATH (repeatable) adds a child that
loads that library -- a build with another kFundRound -- and times FUND and HOM.

  python tools/bench_fundamental_batch.py [--variant R64=PATH ...] [--out profiles/fundamental_batch_ab.txt]
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
S, PER, TIMEOUT = 64, 300, 420
THR, MAX_ITERS, CONF = 3.0, 1000, 0.99     # OpenCV's defaults for findFundamentalMat
WORKLOADS = (("30% outliers", 0.3), ("50% outliers", 0.5))


def two_views(np, seed, n, out_frac, noise=0.5):
    K = np.array([[1200.0, 0, 960], [0, 1200, 540], [0, 0, 1]])
    ay = np.deg2rad(8.0)
    R = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    t = np.array([-1.0, 0.1, 0.2])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    F = np.linalg.inv(K).T @ tx @ R @ np.linalg.inv(K)
    rng = np.random.default_rng(seed)
    P = np.c_[rng.uniform(-3, 3, n), rng.uniform(-1.7, 1.7, n), rng.uniform(4, 10, n)]
    a, b = P @ K.T, (P @ R.T + t) @ K.T
    src = a[:, :2] / a[:, 2:] + rng.uniform(-noise, noise, (n, 2))
    dst = b[:, :2] / b[:, 2:] + rng.uniform(-noise, noise, (n, 2))
    bad = np.zeros(n, bool)
    bad[rng.permutation(n)[:int(round(n * out_frac))]] = True
    line = np.c_[src, np.ones(n)] @ F.T
    normal = line[:, :2] / np.hypot(line[:, 0], line[:, 1])[:, None]
    move = rng.uniform(50, 300, n) * rng.choice([-1.0, 1.0], n)
    dst = np.where(bad[:, None], dst + normal * move[:, None], dst)
    return src.astype(np.float32), dst.astype(np.float32)


def worker(lib_path, iters, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "sift-gpu_amd"))
    import siftgpu
    variant = bool(lib_path)
    if variant:
        siftgpu.LIB_PATH = lib_path
    cap = S * PER
    strm = torch.cuda.Stream()
    ctx = siftgpu.Context(64, 64, 1, device=0)
    ctx.set_stream(strm.cuda_stream)
    L = siftgpu.lib()
    out = {}
    fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    with torch.cuda.stream(strm):
        for name, frac in WORKLOADS:
            pairs = [two_views(np, 1000 + b, PER, frac) for b in range(S)]
            sxy = torch.from_numpy(np.concatenate([p[0] for p in pairs])).cuda()
            dxy = torch.from_numpy(np.concatenate([p[1] for p in pairs])).cuda()
            moff = torch.from_numpy(np.arange(S + 1, dtype=np.int32) * PER).cuda()
            dF = torch.zeros((S, 9), dtype=torch.float64, device="cuda")
            df = torch.zeros((S,), dtype=torch.int32, device="cuda")
            dm = torch.zeros((cap,), dtype=torch.uint8, device="cuda")
            h_moff = torch.empty((S + 1,), dtype=torch.int32).pin_memory()
            h_src = torch.empty((cap, 2), dtype=torch.float32).pin_memory()
            h_dst = torch.empty((cap, 2), dtype=torch.float32).pin_memory()
            bF, bf, bm = np.zeros((S, 9), np.float64), np.zeros(S, np.int32), np.zeros(cap, np.uint8)
            strm.synchronize()

            def device():
                ctx.find_fundamental_segmented_device(sxy.data_ptr(), dxy.data_ptr(), moff.data_ptr(), S, cap,
                                                      dF.data_ptr(), df.data_ptr(), dm.data_ptr(), THR, MAX_ITERS, CONF)

            def host():
                h_moff.copy_(moff, non_blocking=True)
                h_src.copy_(sxy, non_blocking=True)
                h_dst.copy_(dxy, non_blocking=True)
                strm.synchronize()
                ho = h_moff.numpy()
                s0, d0 = h_src.data_ptr(), h_dst.data_ptr()
                for b in range(S):
                    lo, n = int(ho[b]), int(ho[b + 1] - ho[b])
                    rc = L.sift_find_fundamental(ctypes.cast(s0 + lo * 8, fp), ctypes.cast(d0 + lo * 8, fp), n, THR,
                                                 MAX_ITERS, CONF, ctypes.cast(bF[b].ctypes.data, dp),
                                                 bm.ctypes.data + lo)
                    bf[b] = 1 if rc == 0 else 0

            def homography():
                ctx.find_homography_segmented_device(sxy.data_ptr(), dxy.data_ptr(), moff.data_ptr(), S, cap,
                                                     dF.data_ptr(), df.data_ptr(), dm.data_ptr())

            device()
            host()
            ctx.sync()
            same = bool(dF.cpu().numpy().tobytes() == bF.tobytes() and df.cpu().numpy().tobytes() == bf.tobytes()
                        and dm.cpu().numpy().tobytes() == bm.tobytes())
            assert same, f"{name}: the device call and the host loop differ"
            census = {"found": int(bf.sum()), "inliers": int(bm.sum())}
            legs = {"FUND": device, "HOM": homography} if variant else \
                {"FUND": device, "FUND_HOST": host, "HOM": homography}
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
    print("RESULT " + json.dumps({"round": getattr(siftgpu, "FUND_ROUND", None), "iters": iters, "warmup": warmup,
                                  "workloads": out}), flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fundamental_batch_ab.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--variant", action="append", default=[], help="NAME=PATH of a saved libsift_hip.so")
    ap.add_argument("--lib", default="")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.lib, a.iters, a.warmup)
    r = run_worker(a, "")
    variants = [(v.split("=", 1)[0], run_worker(a, v.split("=", 1)[1])) for v in a.variant]
    parts = ["# Fundamental matrix of a whole batch: segmented device estimate (FUND) vs copy to the host + loop of",
             "# sift_find_fundamental (FUND_HOST), beside the segmented homography on the same pairs (HOM)",
             "# written by tools/bench_fundamental_batch.py", "",
             f"{S} segments x {PER} synthetic two-view pairs; thr {THR}, max_iters {MAX_ITERS}, confidence {CONF} "
             "(the homography: 3, 2000, 0.995)",
             f"this build: kFundRound = {r['round']}; the device leg == the host loop byte for byte (F, found, mask): True",
             f"medians of {r['iters']} iterations after {r['warmup']} warm-up [min, max], ms"]
    for name, _ in WORKLOADS:
        w = r["workloads"][name]
        parts += ["", f"## {name}: models found {w['census']['found']} of {S}, inliers {w['census']['inliers']} of {S * PER}",
                  f"{'leg':16} {'HIP events':>32} {'host wall':>32}"] + rows(w, ["FUND", "FUND_HOST", "HOM"])
        e = w["event_ms"]
        parts.append(f"FUND_HOST / FUND = {e['FUND_HOST'][0] / e['FUND'][0]:.1f}; host per segment "
                     f"{e['FUND_HOST'][0] / S:.3f} ms; FUND / HOM = {e['FUND'][0] / e['HOM'][0]:.3f} (events)")
        for tag, v in variants:
            parts += rows(v["workloads"][name], ["FUND", "HOM"], tag + " ")
    text = "\n".join(parts) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
