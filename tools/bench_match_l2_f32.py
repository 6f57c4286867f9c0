#!/usr/bin/env python3
"""A/B of the squared-L2 float matcher (f32 MFMA) against the L1 float matcher.

For each workload one child process (its own timeout) detects a synthetic
batch once, then times, alternating, with HIP events on the context's stream
(5 warm-up iterations, medians of 20), consecutive frames of the batch (train =
query, t_offsets = q_offsets + 1) on the same float rows:

  A   sift_knn_match_l2sqr_f32_segmented_device (match_l2_f32.hip), its norms
      pre-kernel included.
  B   sift_knn_match_l1_segmented_device (match.hip) on the same rows.
  C   information: sift_descriptors_to_u8_device and
      sift_knn_match_l2sqr_u8_segmented_device (the quantised route).

The metrics differ, so B is the cost baseline, not an equality check.  Before
anything is timed, A's idx / dist on the first, the last and four random rows of
every segment must equal, bit for bit, the oracle of tests/match_l2_f32_inputs.py
(the rule of sift_hip.h walked with a correctly rounded float32 fma) computed on
the host from the copied-back rows.
Reported: B / A, and A against the matrix-pipe bound of the pairs actually scored
(256 FLOP a pair at 155 TFLOP/s; 17.8 ms for the 1.08e10 pairs of the design
estimate).  The header lists each kernel's registers, LDS and private segment
from -Rpass-analysis=kernel-resource-usage.

  python tools/bench_match_l2_f32.py [--out profiles/match_l2_f32_ab.txt]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sift-gpu_amd")
WORKLOADS = {"1080p": (64, 1080, 1920, 16000, 900), "240x320": (64, 240, 320, 1500, 300)}  # B, R, C, rows/img, timeout s
SAMPLE_PER_SEGMENT = 4
PEAK_TFLOPS = 155.0


def worker(name, iters, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, PKG)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import match_l2_f32_inputs as F
    import siftgpu
    B, R, C, per_img, _ = WORKLOADS[name]
    cap = B * per_img
    strm = torch.cuda.Stream()
    ctx = siftgpu.Context(R, C, B, device=0)
    ctx.set_stream(strm.cuda_stream)
    with torch.cuda.stream(strm):
        imgs = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
        kpts = torch.empty((cap, 7), dtype=torch.int32, device="cuda")
        desc = torch.zeros((cap, 128), dtype=torch.float32, device="cuda")
        d8 = torch.zeros((cap, 128), dtype=torch.uint8, device="cuda")
        offs = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
        out = {k: (torch.empty((cap, 2), dtype=torch.int32, device="cuda"),
                   torch.empty((cap, 2), dtype=torch.float32, device="cuda")) for k in ("A", "B", "C")}
        ctx.synth_images(imgs.data_ptr(), B, R, C, C, R * C, seed_base=0)
        ctx.detect_compute_batch(imgs.data_ptr(), B, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                                 offs.data_ptr())
        ctx.sync()
        del imgs
        o = offs.cpu().numpy()
        assert o[-1] <= cap, f"{o[-1]} keypoints exceed the buffer ({cap})"
        seg = np.diff(o)
        n = int(o[B - 1])    # live query rows
        pairs = int((seg[:-1].astype(np.int64) * seg[1:].astype(np.int64)).sum())

        def match(key):
            i, d = out[key]
            if key == "C":
                ctx.descriptors_to_u8_device(desc.data_ptr(), offs.data_ptr() + 4 * B, cap, d8.data_ptr())
                ctx.knn_match_l2sqr_u8_segmented_device(d8.data_ptr(), offs.data_ptr(), B - 1, cap, d8.data_ptr(),
                                                        offs.data_ptr() + 4, cap, 2, i.data_ptr(), d.data_ptr())
                return
            fn = ctx.knn_match_l2sqr_f32_segmented_device if key == "A" else ctx.knn_match_segmented_device
            fn(desc.data_ptr(), offs.data_ptr(), B - 1, cap, desc.data_ptr(), offs.data_ptr() + 4, cap, 2,
               i.data_ptr(), d.data_ptr())

        legs = {k: (lambda k=k: match(k)) for k in ("A", "B", "C")}
        for v in out.values():
            v[0].fill_(-1)
            v[1].fill_(-1.0)
        for fn in legs.values():
            fn()
        ctx.sync()
        # the oracle on a sample of rows of every segment
        h = desc.cpu().numpy()
        ai, ad = out["A"][0].cpu().numpy(), out["A"][1].cpu().numpy()
        rng = np.random.default_rng(0)
        sampled = 0
        for b in range(B - 1):
            if o[b + 1] == o[b]:
                continue
            rows = np.unique(np.r_[o[b], o[b + 1] - 1, rng.integers(o[b], o[b + 1], SAMPLE_PER_SEGMENT)])
            want_i, want_d = F.knn_ref(h[rows], h[o[b + 1]:o[b + 2]], 2)
            for j, r in enumerate(rows):
                assert (ai[r] == want_i[j]).all() and (ad[r].view(np.int32) == want_d[j].view(np.int32)).all(), \
                    f"row {r} of segment {b}: {ai[r]} {ad[r]} != {want_i[j]} {want_d[j]}"
                sampled += 1
        del h
        agree = {k: float((out["A"][0][:n, 0] == out[k][0][:n, 0]).float().mean().item()) for k in ("B", "C")}
        ev = {k: [] for k in legs}
        for it in range(warmup + iters):
            for k, fn in legs.items():
                strm.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(strm)
                fn()
                b.record(strm)
                b.synchronize()
                if it >= warmup:
                    ev[k].append(a.elapsed_time(b))
    res = {"workload": name, "batch": B, "rows": R, "cols": C, "keypoints": int(o[-1]),
           "segment_rows": [int(seg.min()), int(statistics.median(seg.tolist())), int(seg.max())],
           "pairs": B - 1, "scored_pairs": pairs, "sampled_rows_equal_oracle": sampled, "nn_agreement": agree,
           "iters": iters, "warmup": warmup,
           "event_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in ev.items()}}
    print("RESULT " + json.dumps(res), flush=True)
    ctx.close()


def resources():
    """Registers, LDS and private segment of the kernels of match_l2_f32.hip, as the compiler reports them."""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fno-slp-vectorize", "-fno-gpu-rdc", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(PKG, "csrc", "match_l2_f32.hip"), "-o",
                        os.devnull], capture_output=True, text=True, timeout=600)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|"
                      r"LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": re.sub(r"^_ZN4sift12_GLOBAL__N_1\d+", "", m.group(2))}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = m.group(2)
    return [f"{c['name']}: {c.get('VGPRs')} VGPRs + {c.get('AGPRs')} AGPRs, {c.get('TotalSGPRs')} SGPRs, "
            f"LDS {c.get('LDS Size')} B, private segment {c.get('ScratchSize')} B/lane, "
            f"occupancy {c.get('Occupancy')} waves/SIMD" for c in rows if "kernel" in c["name"]]


def table(r):
    e = r["event_ms"]
    bound = r["scored_pairs"] * 256 / (PEAK_TFLOPS * 1e12) * 1e3
    lines = [f"## {r['workload']}: {r['batch']} x {r['rows']}x{r['cols']}, {r['keypoints']} keypoints, "
             f"{r['pairs']} consecutive pairs, rows per segment min/median/max {r['segment_rows']}, "
             f"{r['scored_pairs']:.4g} (query, train) pairs",
             f"squared-L2 f32 matcher == the oracle on {r['sampled_rows_equal_oracle']} sampled rows "
             f"(first, last and {SAMPLE_PER_SEGMENT} random rows of every segment), idx and dist bit for bit",
             f"medians of {r['iters']} iterations after {r['warmup']} warm-up [min, max], HIP events, ms"]
    for k, what in (("A", "squared-L2 f32 matcher (f32 MFMA), norms kernel included"),
                    ("B", "L1 f32 matcher (match.hip) on the same rows"),
                    ("C", "information: quantiser + squared-L2 u8 matcher (i8 MFMA)")):
        lines.append(f"{k:5} {e[k][0]:10.3f} [{e[k][1]:9.3f}, {e[k][2]:9.3f}]  {what}")
    lines.append(f"B / A = {e['B'][0] / e['A'][0]:.3f}")
    lines.append(f"matrix-pipe bound of these pairs (256 FLOP a pair at {PEAK_TFLOPS:.0f} TFLOP/s): {bound:.3f} ms; "
                 f"A / bound = {e['A'][0] / bound:.2f} (the design estimate's 1.08e10 pairs: 17.8 ms)")
    lines.append(f"accuracy (information): A's nearest neighbour equals the L1 matcher's on "
                 f"{100 * r['nn_agreement']['B']:.2f} % of the live rows and the quantised squared-L2 matcher's on "
                 f"{100 * r['nn_agreement']['C']:.2f} %")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_l2_f32_ab.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--worker", choices=sorted(WORKLOADS))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.iters, a.warmup)
    parts = ["# Matching a whole batch of float descriptors: squared L2 on f32 MFMA (A) vs float L1 (B)\n"
             "# written by tools/bench_match_l2_f32.py\n"
             "# 256 queries per workgroup (2 x 32 per wave, match_l2_f32.hip), 64 train rows per step through LDS\n# "
             + "\n# ".join(resources())]
    for name, w in WORKLOADS.items():
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", name, "--iters", str(a.iters),
                            "--warmup", str(a.warmup)], capture_output=True, text=True, timeout=w[4])
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"{name}: worker failed ({r.returncode}); nothing further is started")
        parts.append(table(json.loads(line[0][7:])))
        print(parts[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n\n".join(parts) + "\n")


if __name__ == "__main__":
    main()
