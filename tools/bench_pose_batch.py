#!/usr/bin/env python3
"""A/B of the relative pose of a batch: the segmented device call against the
host loop it replaces, beside the fundamental-matrix estimate on the same pairs
for scale, and the triangulation call alone.

The workload is synthetic: 64 segments of 300 and of 4000 two-view point pairs
(bench_fundamental_batch.py's scene: two pinhole cameras with a baseline and a
rotation, 3-D points with depth spread, 0.5 px of jitter, 30 % outliers).  F,
found and the inlier mask are the segmented estimate's own, left on the device.
One process times, alternating, with HIP events on the context's stream (5
warm-up iterations, medians of 20):

  POSE       sift_recover_pose_segmented_device on the device-resident pairs, F,
             found and mask: one enqueue, no host value
  POSE_HOST  the flow a caller has without it: offsets, pairs, F, found and mask
             are copied to the host, the stream is waited for, and
             sift_recover_pose runs per segment on the CPU (copy and wait inside
             the window)
  TRI        sift_triangulate_points_segmented_device under [I | 0] and the poses
  FUND       sift_find_fundamental_segmented_device on the same pairs

The device leg's pose, found, n_good, mask and xyz must equal the host loop's
byte for byte before anything is timed.

  python tools/bench_pose_batch.py [--out profiles/pose_batch_ab.txt]
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
WORKLOADS = (("300 pairs", 300), ("4000 pairs", 4000))
THRESH = 50.0


def worker(iters, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "sift-gpu_amd"))
    import siftgpu
    from bench_fundamental_batch import two_views
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
            moff = torch.from_numpy(np.arange(S + 1, dtype=np.int32) * per).cuda()
            dK = torch.from_numpy(K).cuda()
            dI = torch.from_numpy(np.tile(np.array([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]), (S, 1))).cuda()
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
            dF, df, dm = z((S, 9), torch.float64), z((S,), torch.int32), z((cap,), torch.uint8)
            dP, dpf, dng = z((S, 12), torch.float64), z((S,), torch.int32), z((S,), torch.int32)
            dmo, dxyz, dq = z((cap,), torch.uint8), z((cap, 3), torch.float64), z((cap, 4), torch.float64)
            pin = lambda shape, dt: torch.empty(shape, dtype=dt).pin_memory()  # noqa: E731
            h_moff, h_src, h_dst = pin((S + 1,), torch.int32), pin((cap, 2), torch.float32), pin((cap, 2), torch.float32)
            h_F, h_f, h_m = pin((S, 9), torch.float64), pin((S,), torch.int32), pin((cap,), torch.uint8)
            bP, bpf, bng = np.zeros((S, 12)), np.zeros(S, np.int32), np.zeros(S, np.int32)
            bmo, bxyz = np.zeros(cap, np.uint8), np.zeros((cap, 3))
            strm.synchronize()

            def fund():
                ctx.find_fundamental_segmented_device(sxy.data_ptr(), dxy.data_ptr(), moff.data_ptr(), S, cap,
                                                      dF.data_ptr(), df.data_ptr(), dm.data_ptr())

            def device():
                ctx.recover_pose_segmented_device(sxy.data_ptr(), dxy.data_ptr(), moff.data_ptr(), S, cap,
                                                  dF.data_ptr(), df.data_ptr(), dK.data_ptr(), dK.data_ptr(),
                                                  dP.data_ptr(), dpf.data_ptr(), dng.data_ptr(), 0, dm.data_ptr(),
                                                  THRESH, None, dmo.data_ptr(), dxyz.data_ptr())

            def tri():
                ctx.triangulate_points_segmented_device(sxy.data_ptr(), dxy.data_ptr(), moff.data_ptr(), S, cap,
                                                        dI.data_ptr(), dP.data_ptr(), dq.data_ptr())

            def host():
                for h, d in ((h_moff, moff), (h_src, sxy), (h_dst, dxy), (h_F, dF), (h_f, df), (h_m, dm)):
                    h.copy_(d, non_blocking=True)
                strm.synchronize()
                ho, hf = h_moff.numpy(), h_f.numpy()
                s0, d0, F0, m0 = h_src.data_ptr(), h_dst.data_ptr(), h_F.data_ptr(), h_m.data_ptr()
                ng = ctypes.c_int(0)
                for b in range(S):
                    lo, n = int(ho[b]), int(ho[b + 1] - ho[b])
                    rc = -1
                    if hf[b]:
                        rc = L.sift_recover_pose(ctypes.cast(F0 + b * 72, dp), K.ctypes.data_as(dp), K.ctypes.data_as(dp),
                                                 ctypes.cast(s0 + lo * 8, fp), ctypes.cast(d0 + lo * 8, fp), n,
                                                 m0 + lo, THRESH, ctypes.cast(bP[b].ctypes.data, dp), None,
                                                 bmo.ctypes.data + lo, bxyz.ctypes.data + lo * 24, ctypes.byref(ng))
                    bpf[b], bng[b] = (1, ng.value) if rc == 0 else (0, 0)

            fund()
            device()
            host()
            ctx.sync()
            g = lambda t: t.cpu().numpy().tobytes()  # noqa: E731
            same = bool(g(dP) == bP.tobytes() and g(dpf) == bpf.tobytes() and g(dng) == bng.tobytes()
                        and g(dmo) == bmo.tobytes() and g(dxyz) == bxyz.tobytes())
            assert same, f"{name}: the device call and the host loop differ"
            census = {"found": int(bpf.sum()), "good": int(bng.sum()), "inliers": int(dm.sum().item())}
            legs = {"POSE": device, "POSE_HOST": host, "TRI": tri, "FUND": fund}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_batch_ab.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.iters, a.warmup)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--iters", str(a.iters), "--warmup", str(a.warmup)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=TIMEOUT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(f"worker failed ({r.returncode}); nothing further is started")
    res = json.loads(line[0][7:])
    parts = ["# Relative pose of a whole batch: segmented device call (POSE) vs copy to the host + loop of",
             "# sift_recover_pose (POSE_HOST), the triangulation call alone (TRI), and the fundamental-matrix",
             "# estimate on the same pairs (FUND)", "# written by tools/bench_pose_batch.py", "",
             f"{S} segments of synthetic two-view pairs, 30 % outliers; F, found and the inlier mask from the segmented "
             f"estimate; distance_thresh {THRESH}",
             "the device leg == the host loop byte for byte (pose, found, n_good, mask, xyz): True",
             f"medians of {res['iters']} iterations after {res['warmup']} warm-up [min, max], ms"]
    for name, per in WORKLOADS:
        w = res["workloads"][name]
        c = w["census"]
        parts += ["", f"## {S} x {name}: poses found {c['found']} of {S}, good rows {c['good']} of {c['inliers']} "
                      f"inliers of {S * per} pairs", f"{'leg':16} {'HIP events':>32} {'host wall':>32}"]
        for k in ("POSE", "POSE_HOST", "TRI", "FUND"):
            e, wl = w["event_ms"][k], w["wall_ms"][k]
            parts.append(f"{k:16} {e[0]:10.3f} [{e[1]:9.3f}, {e[2]:9.3f}] {wl[0]:10.3f} [{wl[1]:9.3f}, {wl[2]:9.3f}]")
        e = w["event_ms"]
        parts.append(f"POSE_HOST / POSE = {e['POSE_HOST'][0] / e['POSE'][0]:.1f}; host per segment "
                     f"{e['POSE_HOST'][0] / S:.3f} ms; POSE / FUND = {e['POSE'][0] / e['FUND'][0]:.3f} (events)")
    text = "\n".join(parts) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
