#!/usr/bin/env python3
"""A/B of the motion model of a batch: the segmented device estimate of an
affine or a similarity transform against the host loop it replaces, and against
the segmented homography on the same pairs.

The workload is tools/bench_homography_batch.py's: 64 x 1080p synthetic frames,
consecutive frames matched once (segmented kNN + ratio test with keypoints).
One child process (its own timeout) then times, alternating, with HIP events on
the context's stream (5 warm-up iterations, medians of 20):

  AFF   sift_estimate_affine_segmented_device, SIFT_MODEL_AFFINE, on the ratio
        stage's output (d_src_xy, d_dst_xy, d_m_offsets): one enqueue, no host value
  SIM   the same with SIFT_MODEL_SIMILARITY
  AFF_HOST / SIM_HOST
        the flow a caller has without it: m_offsets and the point pairs are
        copied to the host, the stream is waited for, and sift_estimate_affine
        runs per segment on the CPU (copy and wait inside the window)
  HOM   sift_find_homography_segmented_device on the same pairs

With --parent-lib, a second child loads that library (a build of the parent
commit) and times HOM alone: the homography call this change must not be slower
than.  Each device leg's H, found and mask must equal its host loop's byte for
byte before anything is timed.

  python tools/bench_affine_batch.py [--parent-lib PATH] [--out profiles/affine_batch_ab.txt]
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
B, R, C, PER_IMG, TIMEOUT = 64, 1080, 1920, 16000, 420
THR, MAX_ITERS, CONF = 3.0, 2000, 0.99     # OpenCV's defaults for estimateAffine2D


def worker(lib_path, iters, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "sift-gpu_amd"))
    import siftgpu
    parent = bool(lib_path)
    if parent:
        siftgpu.LIB_PATH = lib_path
    cap, S = B * PER_IMG, B - 1
    strm = torch.cuda.Stream()
    ctx = siftgpu.Context(R, C, B, device=0)
    ctx.set_stream(strm.cuda_stream)
    L = siftgpu.lib()
    with torch.cuda.stream(strm):
        imgs = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
        kpts = torch.empty((cap, 7), dtype=torch.int32, device="cuda")
        desc = torch.empty((cap, 128), dtype=torch.float32, device="cuda")
        offs = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
        idx = torch.empty((cap, 2), dtype=torch.int32, device="cuda")
        dist = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
        mt = torch.empty((cap, 4), dtype=torch.int32, device="cuda")
        sxy = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
        dxy = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
        moff = torch.empty((B,), dtype=torch.int32, device="cuda")
        dH = torch.zeros((S, 9), dtype=torch.float64, device="cuda")
        df = torch.zeros((S,), dtype=torch.int32, device="cuda")
        dm = torch.zeros((cap,), dtype=torch.uint8, device="cuda")
        ctx.synth_images(imgs.data_ptr(), B, R, C, C, R * C, seed_base=0)
        ctx.detect_compute_batch(imgs.data_ptr(), B, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                                 offs.data_ptr())
        ctx.knn_match_segmented_device(desc.data_ptr(), offs.data_ptr(), S, cap, desc.data_ptr(),
                                       offs.data_ptr() + 4, cap, 2, idx.data_ptr(), dist.data_ptr())
        ctx.ratio_matches_device(idx.data_ptr(), dist.data_ptr(), offs.data_ptr(), S, cap, 0.86, kpts.data_ptr(),
                                 kpts.data_ptr(), offs.data_ptr() + 4, mt.data_ptr(), sxy.data_ptr(), dxy.data_ptr(),
                                 cap, moff.data_ptr())
        ctx.sync()
        mo = moff.cpu().numpy()
        total = int(mo[-1])
        assert total <= cap
        seg = np.diff(mo)
        h_moff = torch.empty((B,), dtype=torch.int32).pin_memory()
        h_src = torch.empty((max(total, 1), 2), dtype=torch.float32).pin_memory()
        h_dst = torch.empty((max(total, 1), 2), dtype=torch.float32).pin_memory()
        bH = np.zeros((S, 9), np.float64)
        bf = np.zeros(S, np.int32)
        bm = np.zeros(max(total, 1), np.uint8)
        fp, dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)

        def device(model):
            def run():
                ctx.estimate_affine_segmented_device(sxy.data_ptr(), dxy.data_ptr(), moff.data_ptr(), S, cap, model,
                                                     dH.data_ptr(), df.data_ptr(), dm.data_ptr(), THR, MAX_ITERS, CONF)
            return run

        def host(model):
            def run():
                h_moff.copy_(moff, non_blocking=True)
                h_src.copy_(sxy[:max(total, 1)], non_blocking=True)   # sized from an earlier read of m_offsets
                h_dst.copy_(dxy[:max(total, 1)], non_blocking=True)
                strm.synchronize()
                ho = h_moff.numpy()
                s0, d0 = h_src.data_ptr(), h_dst.data_ptr()
                bH[:] = 0
                for b in range(S):
                    lo, n = int(ho[b]), int(ho[b + 1] - ho[b])
                    rc = L.sift_estimate_affine(ctypes.cast(s0 + lo * 8, fp), ctypes.cast(d0 + lo * 8, fp), n, model,
                                                THR, MAX_ITERS, CONF, ctypes.cast(bH[b].ctypes.data, dp),
                                                bm.ctypes.data + lo)
                    bf[b] = 1 if rc == 0 else 0
                    bH[b, 8] = bf[b]
            return run

        def homography():
            ctx.find_homography_segmented_device(sxy.data_ptr(), dxy.data_ptr(), moff.data_ptr(), S, cap,
                                                 dH.data_ptr(), df.data_ptr(), dm.data_ptr())

        legs, census = {"HOM": homography}, {}
        if not parent:
            legs = {"AFF": device(0), "SIM": device(1), "AFF_HOST": host(0), "SIM_HOST": host(1), "HOM": homography}
            for k, model in (("AFF", 0), ("SIM", 1)):
                legs[k]()
                legs[k + "_HOST"]()
                ctx.sync()
                same = bool(dH.cpu().numpy().tobytes() == bH.tobytes() and df.cpu().numpy().tobytes() == bf.tobytes()
                            and dm.cpu().numpy()[:total].tobytes() == bm[:total].tobytes())
                assert same, f"{k}: the device call and the host loop differ"
                census[k] = {"found": int(bf.sum()), "inliers": int(bm[:total].sum())}
        homography()
        ctx.sync()
        census["HOM"] = {"found": int(df.cpu().numpy().sum()), "inliers": int(dm.cpu().numpy()[:total].sum())}
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
    res = {"parent": parent, "segments": S, "pairs_total": total,
           "segment_pairs": [int(seg.min()), int(statistics.median(seg.tolist())), int(seg.max())],
           "census": census, "iters": iters, "warmup": warmup,
           "event_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in ev.items()},
           "wall_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in wall.items()}}
    print("RESULT " + json.dumps(res), flush=True)
    ctx.close()


def run_worker(args, lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--iters", str(args.iters), "--warmup",
           str(args.warmup)] + (["--parent-lib", lib] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=TIMEOUT)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout + r.stderr)
        sys.exit(f"worker failed ({r.returncode}); nothing further is started")
    return json.loads(line[0][7:])


def rows(r, names):
    out = []
    for k in names:
        e, w = r["event_ms"][k], r["wall_ms"][k]
        out.append(f"{k:12} {e[0]:10.3f} [{e[1]:9.3f}, {e[2]:9.3f}] {w[0]:10.3f} [{w[1]:9.3f}, {w[2]:9.3f}]")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_batch_ab.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.parent_lib, a.iters, a.warmup)
    r = run_worker(a, "")
    c = r["census"]
    parts = ["# Motion model of a whole batch: segmented device estimate of an affine (AFF) or similarity (SIM) transform",
             "# vs copy to the host + loop of sift_estimate_affine (*_HOST), and vs the segmented homography (HOM)",
             "# written by tools/bench_affine_batch.py", "",
             f"## 1080p: {B} x {R}x{C}, {r['segments']} consecutive pairs of frames, {r['pairs_total']} point pairs, "
             f"per segment min/median/max {r['segment_pairs']}",
             "each device leg == its host loop byte for byte (H, found, mask): True",
             "models found / inliers: " + ", ".join(f"{k} {c[k]['found']} of {r['segments']} / {c[k]['inliers']}"
                                                    for k in ("AFF", "SIM", "HOM")),
             f"thr {THR}, max_iters {MAX_ITERS}, confidence {CONF} (the homography: 3, 2000, 0.995)",
             f"medians of {r['iters']} iterations after {r['warmup']} warm-up [min, max], ms",
             f"{'leg':12} {'HIP events':>32} {'host wall':>32}"] + rows(r, ["AFF", "SIM", "AFF_HOST", "SIM_HOST", "HOM"])
    hom = r["event_ms"]["HOM"][0]
    if a.parent_lib:
        p = run_worker(a, a.parent_lib)
        parts += ["", "the parent commit's build, its own process:"] + rows(p, ["HOM"])
        parts.append(f"HOM here / HOM parent = {hom / p['event_ms']['HOM'][0]:.3f} (events)")
        hom = p["event_ms"]["HOM"][0]
    for k in ("AFF", "SIM"):
        e = r["event_ms"][k][0]
        parts.append(f"{k} / HOM{' parent' if a.parent_lib else ''} = {e / hom:.4f} (events); "
                     f"{k}_HOST / {k} = {r['event_ms'][k + '_HOST'][0] / e:.1f}")
    text = "\n".join(parts) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
