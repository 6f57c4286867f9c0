#!/usr/bin/env python3
"""A/B of cross-check matching against today's ratio-test flow, per metric.

For each workload one child process (its own timeout) detects a synthetic
batch once and quantises its descriptors, then, for each of the three metrics
(float L1, byte L1, byte squared L2), times, alternating, with HIP events on
the context's stream (5 warm-up iterations, medians), consecutive frames of the
batch (train = query, t_offsets = q_offsets + 1):

  A    sift_cross_match_segmented_device with ratio = 0: forward k = 1, reverse
       k = 1 and the cross-check stage.
  B    the forward k = 2 matcher followed by sift_ratio_matches_device (ratio
       0.86, 0.86^2 on squared distances): today's flow.
  As   the cross-check stage alone (sift_cross_check_matches_device) on a
       forward k = 2 and a reverse k = 1 table.
  Bs   the ratio stage alone on the same forward table.

A does one matcher pass more than B; the stages are small beside a pass.
Before anything is timed, A's records on sampled segments (the first, the
middle and the last) must equal a numpy reference: the keep rule restated, on
the separately computed forward and reverse tables copied back, of which
sampled rows must equal a brute-force matcher on the copied-back descriptors:
int64 sums for the byte metrics, oracle/match.py's float32 distance (the
matcher's summation order) for the float metric.
Kept counts (information): A, B, and A with the ratio test.
The header lists each new kernel's registers, LDS and private segment from
-Rpass-analysis=kernel-resource-usage.

  python tools/bench_cross_check.py [--out profiles/cross_check_ab.txt]
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
METRICS = ["l1_f32", "l1_u8", "l2sqr_u8"]
SAMPLE_SEGMENTS = 3
SAMPLE_ROWS = 8     # random rows per table and sampled segment, besides the first and the last


def keep_ref(idx, ridx, qlo, qhi, tlo, thi):
    """Local (query, train) pairs of one segment by the keep rule, ratio 0."""
    out = []
    for i in range(qlo, qhi):
        j = int(idx[i])
        if j >= 0 and tlo + j < thi and int(ridx[tlo + j]) == i - qlo:
            out.append((i - qlo, j))
    return out


def brute(q, t, metric):
    """Nearest train row per query row (the lower index at equal distance): int64 on bytes; on
    floats the float32 L1 distance in the matcher's summation order, as oracle/match.py states it."""
    import numpy as np
    out = np.full(len(q), -1, np.int64)
    if len(t) == 0:
        return out
    if metric == 0:
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import match as M
        return np.argmin(M.l1_distances(q, t), axis=1)      # the first minimum
    ti = t.astype(np.int64)
    for s in range(0, len(q), 64):
        e = q[s:s + 64, None, :].astype(np.int64) - ti[None, :, :]
        d = np.abs(e).sum(-1) if metric == 1 else (e * e).sum(-1)
        out[s:s + 64] = np.argmin(d, axis=1)        # the first minimum
    return out


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
        idx = torch.empty((cap, 2), dtype=torch.int32, device="cuda")
        dist = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
        ridx = torch.empty((cap, 1), dtype=torch.int32, device="cuda")
        rdist = torch.empty((cap, 1), dtype=torch.float32, device="cuda")
        mt = {k: torch.empty((cap, 4), dtype=torch.int32, device="cuda") for k in "AB"}
        src = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
        dst = torch.empty((cap, 2), dtype=torch.float32, device="cuda")
        moff = {k: torch.empty((B,), dtype=torch.int32, device="cuda") for k in "AB"}
        ctx.synth_images(imgs.data_ptr(), B, R, C, C, R * C, seed_base=0)
        ctx.detect_compute_batch(imgs.data_ptr(), B, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                                 offs.data_ptr())
        ctx.descriptors_to_u8_device(desc.data_ptr(), offs.data_ptr() + 4 * B, cap, d8.data_ptr())
        ctx.sync()
        del imgs
        o = offs.cpu().numpy()
        assert o[-1] <= cap, f"{o[-1]} keypoints exceed the buffer ({cap})"
        seg = np.diff(o)
        op, kp = offs.data_ptr(), kpts.data_ptr()
        res = {"workload": name, "batch": B, "rows": R, "cols": C, "keypoints": int(o[-1]),
               "segment_rows": [int(seg.min()), int(statistics.median(seg.tolist())), int(seg.max())],
               "pairs": B - 1, "iters": iters, "warmup": warmup, "metrics": {}}
        for metric, mname in enumerate(METRICS):
            rows = desc if metric == 0 else d8
            rp = rows.data_ptr()
            knn = [ctx.knn_match_segmented_device, ctx.knn_match_u8_segmented_device,
                   ctx.knn_match_l2sqr_u8_segmented_device][metric]
            ratio = 0.86 * 0.86 if metric == 2 else 0.86

            def one_call(r, k="A"):
                ctx.cross_match_segmented_device(metric, rp, op, B - 1, cap, rp, op + 4, cap, r, kp, kp,
                                                 mt[k].data_ptr(), src.data_ptr(), dst.data_ptr(), cap,
                                                 moff[k].data_ptr())

            def forward2():
                knn(rp, op, B - 1, cap, rp, op + 4, cap, 2, idx.data_ptr(), dist.data_ptr())

            def ratio_stage():
                ctx.ratio_matches_device(idx.data_ptr(), dist.data_ptr(), op, B - 1, cap, ratio, kp, kp, op + 4,
                                         mt["B"].data_ptr(), src.data_ptr(), dst.data_ptr(), cap, moff["B"].data_ptr())

            def cross_stage():
                ctx.cross_check_matches_device(idx.data_ptr(), dist.data_ptr(), 2, op, B - 1, cap, ridx.data_ptr(), 1,
                                               op + 4, cap, 0.0, kp, kp, mt["A"].data_ptr(), src.data_ptr(),
                                               dst.data_ptr(), cap, moff["A"].data_ptr())

            def today():
                forward2()
                ratio_stage()

            # tables for the stage-alone legs and the check; then A once
            forward2()
            knn(rp, op + 4, B - 1, cap, rp, op, cap, 1, ridx.data_ptr(), rdist.data_ptr())
            one_call(0.0)
            ctx.sync()
            ma = mt["A"].cpu().numpy().view(siftgpu.MATCH_DTYPE).reshape(-1)
            oa = moff["A"].cpu().numpy()
            hi, hr = idx.cpu().numpy()[:, 0], ridx.cpu().numpy()[:, 0]
            hrows = rows.cpu().numpy()
            checked = brute_rows = 0
            rng = np.random.default_rng(metric)
            for b in sorted({0, (B - 1) // 2, B - 2})[:SAMPLE_SEGMENTS]:
                qlo, qhi, tlo, thi = int(o[b]), int(o[b + 1]), int(o[b + 1]), int(o[b + 2])
                if qhi > qlo and thi > tlo:      # sampled rows of both tables against the brute-force matcher
                    qs = np.unique(np.r_[qlo, qhi - 1, rng.integers(qlo, qhi, SAMPLE_ROWS)])
                    ts = np.unique(np.r_[tlo, thi - 1, rng.integers(tlo, thi, SAMPLE_ROWS)])
                    assert (brute(hrows[qs], hrows[tlo:thi], metric) == hi[qs]).all() and \
                        (brute(hrows[ts], hrows[qlo:qhi], metric) == hr[ts]).all(), \
                        f"{mname}: segment {b}: the device tables differ from the brute-force matcher"
                    brute_rows += len(qs) + len(ts)
                want = keep_ref(hi, hr, qlo, qhi, tlo, thi)
                got = ma[oa[b]:oa[b + 1]]
                assert (got["segment"] == b).all() and list(zip(got["query"].tolist(), got["train"].tolist())) == want, \
                    f"{mname}: segment {b}: records differ from the reference"
                checked += len(want)
            kept_a = int(oa[-1])
            one_call(ratio)
            today()
            ctx.sync()
            kept_ar, kept_b = int(moff["A"].cpu().numpy()[-1]), int(moff["B"].cpu().numpy()[-1])
            legs = {"A": lambda: one_call(0.0), "B": today, "As": cross_stage, "Bs": ratio_stage}
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
            res["metrics"][mname] = {"checked_records": checked, "brute_rows": brute_rows, "kept_cross": kept_a,
                                     "kept_ratio": kept_b,
                                     "kept_cross_and_ratio": kept_ar,
                                     "event_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in ev.items()}}
    print("RESULT " + json.dumps(res), flush=True)
    ctx.close()


def resources():
    """Registers, LDS and private segment of the kernels of cross_check.hip, as the compiler reports them."""
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                        "-fno-slp-vectorize", "-fno-gpu-rdc", "--cuda-device-only", "-c",
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(PKG, "csrc", "cross_check.hip"), "-o",
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
    lines = [f"## {r['workload']}: {r['batch']} x {r['rows']}x{r['cols']}, {r['keypoints']} keypoints, "
             f"{r['pairs']} consecutive pairs, rows per segment min/median/max {r['segment_rows']}",
             f"medians of {r['iters']} iterations after {r['warmup']} warm-up [min, max], HIP events, ms"]
    for mname, m in r["metrics"].items():
        e = m["event_ms"]
        lines.append(f"### {mname}: A == numpy reference on {SAMPLE_SEGMENTS} sampled segments "
                     f"({m['checked_records']} records; both tables == brute force on {m['brute_rows']} sampled rows)")
        for k, what in (("A", "one call: forward k=1 + reverse k=1 + cross-check stage"),
                        ("B", "forward k=2 + ratio stage (today's flow)"),
                        ("As", "cross-check stage alone"), ("Bs", "ratio stage alone")):
            lines.append(f"{k:5} {e[k][0]:10.3f} [{e[k][1]:9.3f}, {e[k][2]:9.3f}]  {what}")
        lines.append(f"A / B = {e['A'][0] / e['B'][0]:.3f}   As / Bs = {e['As'][0] / e['Bs'][0]:.3f}")
        lines.append(f"kept: cross-check {m['kept_cross']}, ratio test {m['kept_ratio']}, "
                     f"cross-check and ratio test {m['kept_cross_and_ratio']}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_check_ab.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--worker", choices=sorted(WORKLOADS))
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.iters, a.warmup)
    parts = ["# Cross-check matching of a whole batch (A) vs the ratio-test flow (B), consecutive frames, per metric\n"
             "# written by tools/bench_cross_check.py\n# " + "\n# ".join(resources())]
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
