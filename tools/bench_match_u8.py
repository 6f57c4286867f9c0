#!/usr/bin/env python3
"""A/B of matching a whole batch on 8-bit descriptors against the float matcher.

For each workload one child process (its own timeout) detects a synthetic
batch once, then times, alternating, with HIP events on the context's stream
(5 warm-up iterations, medians), consecutive frames of the batch (train =
query, t_offsets = q_offsets + 1):

  Q     sift_descriptors_to_u8_device alone (d_n_rows = d_img_offsets + batch).
  A     Q followed by sift_knn_match_l1_u8_segmented_device, train rows by
        scalar loads (the route the library ships).
  Alds  the same with SIFT_HIP_U8_ROUTE=lds: train rows from LDS chunks.
  B     the unchanged sift_knn_match_l1_segmented_device on the float rows.

Before anything is timed, A's idx / dist on both routes must equal, byte for
byte, the float matcher run on the quantised bytes converted to float32.
Accuracy (information): the share of live rows whose nearest neighbour is the
same in A and B, and the rows the 0.86 ratio test keeps after each.
The header lists each kernel's registers, LDS and private segment from
-Rpass-analysis=kernel-resource-usage.

  python tools/bench_match_u8.py [--out profiles/match_u8_ab.txt]
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


def worker(name, iters, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, PKG)
    import siftgpu
    B, R, C, per_img, _ = WORKLOADS[name]
    cap = B * per_img
    strm = torch.cuda.Stream()
    ctx = siftgpu.Context(R, C, B, device=0)
    ctx.set_stream(strm.cuda_stream)
    with torch.cuda.stream(strm):
        imgs = torch.empty((B, R, C), dtype=torch.float32, device="cuda")
        kpts = torch.empty((cap, 7), dtype=torch.int32, device="cuda")
        desc = torch.empty((cap, 128), dtype=torch.float32, device="cuda")
        d8 = torch.zeros((cap, 128), dtype=torch.uint8, device="cuda")
        offs = torch.empty((B + 1,), dtype=torch.int32, device="cuda")
        out = {k: (torch.empty((cap, 2), dtype=torch.int32, device="cuda"),
                   torch.empty((cap, 2), dtype=torch.float32, device="cuda")) for k in ("A", "Alds", "B", "ref")}
        mt = torch.empty((cap, 4), dtype=torch.int32, device="cuda")
        moff = torch.empty((B,), dtype=torch.int32, device="cuda")
        ctx.synth_images(imgs.data_ptr(), B, R, C, C, R * C, seed_base=0)
        ctx.detect_compute_batch(imgs.data_ptr(), B, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                                 offs.data_ptr())
        ctx.sync()
        del imgs
        o = offs.cpu().numpy()
        assert o[-1] <= cap, f"{o[-1]} keypoints exceed the buffer ({cap})"
        seg = np.diff(o)
        n = int(o[B - 1])    # live query rows

        def quant():
            ctx.descriptors_to_u8_device(desc.data_ptr(), offs.data_ptr() + 4 * B, cap, d8.data_ptr())

        def match_u8(key, route):
            if route:
                os.environ["SIFT_HIP_U8_ROUTE"] = route
            else:
                os.environ.pop("SIFT_HIP_U8_ROUTE", None)
            i, d = out[key]
            ctx.knn_match_u8_segmented_device(d8.data_ptr(), offs.data_ptr(), B - 1, cap, d8.data_ptr(),
                                              offs.data_ptr() + 4, cap, 2, i.data_ptr(), d.data_ptr())

        def match_f(key, rows):
            i, d = out[key]
            ctx.knn_match_segmented_device(rows.data_ptr(), offs.data_ptr(), B - 1, cap, rows.data_ptr(),
                                           offs.data_ptr() + 4, cap, 2, i.data_ptr(), d.data_ptr())

        def kept(key):
            i, d = out[key]
            ctx.ratio_matches_device(i.data_ptr(), d.data_ptr(), offs.data_ptr(), B - 1, cap, 0.86, None, None, None,
                                     mt.data_ptr(), None, None, cap, moff.data_ptr())
            ctx.sync()
            return int(moff.cpu().numpy()[-1])

        legs = {"Q": quant, "A": lambda: (quant(), match_u8("A", None)),
                "Alds": lambda: (quant(), match_u8("Alds", "lds")), "B": lambda: match_f("B", desc)}
        for v in out.values():
            v[0].fill_(-1)
            v[1].fill_(-1.0)
        for fn in legs.values():
            fn()
        ctx.sync()
        as_float = d8.to(torch.float32)
        strm.synchronize()
        match_f("ref", as_float)
        ctx.sync()
        del as_float
        same = all(bool(torch.equal(out[k][0][:n], out["ref"][0][:n]) and torch.equal(out[k][1][:n], out["ref"][1][:n]))
                   for k in ("A", "Alds"))
        assert same, "the u8 matcher and the float matcher on the same bytes differ"
        agree = float((out["A"][0][:n, 0] == out["B"][0][:n, 0]).float().mean().item())
        kept_a, kept_b = kept("A"), kept("B")
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
           "pairs": B - 1, "u8_equals_float_on_bytes": same, "nn_agreement": agree, "kept_u8": kept_a,
           "kept_float": kept_b, "iters": iters, "warmup": warmup,
           "event_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in ev.items()}}
    print("RESULT " + json.dumps(res), flush=True)
    ctx.close()


def resources():
    """Registers, LDS and private segment of the kernels of match_u8.hip, as the compiler reports them."""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fno-slp-vectorize", "-fno-gpu-rdc", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(PKG, "csrc", "match_u8.hip"), "-o",
                        os.devnull], capture_output=True, text=True, timeout=600)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|"
                      r"Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": re.sub(r"^_ZN4sift12_GLOBAL__N_1\d+", "", m.group(2))}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = m.group(2)
    return [f"{c['name']}: {c.get('VGPRs')} VGPRs, {c.get('TotalSGPRs')} SGPRs, LDS {c.get('LDS Size')} B, "
            f"private segment {c.get('ScratchSize')} B/lane, occupancy {c.get('Occupancy')} waves/SIMD"
            for c in rows if "kernel" in c["name"]]


def table(r):
    e = r["event_ms"]
    lines = [f"## {r['workload']}: {r['batch']} x {r['rows']}x{r['cols']}, {r['keypoints']} keypoints, "
             f"{r['pairs']} consecutive pairs, rows per segment min/median/max {r['segment_rows']}",
             f"u8 matcher (both routes) == float matcher on the same bytes, byte for byte: "
             f"{r['u8_equals_float_on_bytes']}",
             f"medians of {r['iters']} iterations after {r['warmup']} warm-up [min, max], HIP events, ms"]
    for k, what in (("Q", "quantiser"), ("A", "quantiser + u8 matcher, scalar-load route"),
                    ("Alds", "quantiser + u8 matcher, LDS route"), ("B", "float matcher")):
        lines.append(f"{k:5} {e[k][0]:10.3f} [{e[k][1]:9.3f}, {e[k][2]:9.3f}]  {what}")
    lines.append(f"B / A = {e['B'][0] / e['A'][0]:.3f}; B / Alds = {e['B'][0] / e['Alds'][0]:.3f}; "
                 f"u8 matcher alone (A - Q) = {e['A'][0] - e['Q'][0]:.3f} ms")
    lines.append(f"accuracy (information): nearest neighbour equal to the float matcher's on "
                 f"{100 * r['nn_agreement']:.2f} % of the live rows; ratio 0.86 keeps {r['kept_u8']} rows after u8, "
                 f"{r['kept_float']} after float")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_u8_ab.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--worker", choices=sorted(WORKLOADS))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.iters, a.warmup)
    parts = ["# Matching a whole batch on 8-bit descriptors (A) vs the float matcher (B)\n"
             "# written by tools/bench_match_u8.py\n"
             "# Q = 4 queries per lane (kU8Q, match_u8.hip); the library ships the scalar-load route\n# "
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
