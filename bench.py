#!/usr/bin/env python3
"""bench.py -- SIFT detect+compute throughput on MI355X (BASELINE.json metric
"Mpix/s + keypoints/s, 1920x1080 grayscale, 1/2/4/8 MI355X vs CPU ref").

Workload (one "step"): the full SIFT_NCL hot path -- Gaussian pyramid, DoG,
extrema + refinement + orientation, 128-D descriptors -- over one batch of
--batch synthetic 1920x1080 grayscale images per GPU (default 64:
BASELINE.json configs[2] at N=1; at N=8 the 8 x 64 = 512 images are
configs[3]).  Inputs are generated on device (integer-exact generator,
SURVEY.md 8(d) d2) before the timed region; every rank has its own images
(weak scaling).  The timed step runs the per-GPU batch as --streams (default
2) sub-batches, one library context and HIP stream each, with no
synchronisation between them inside the timed region (graph replay; the
streams' stages overlap).  For N > 1 each sub-batch's keypoints are gathered
to rank 0 over RCCL one step behind the compute (sift-gpu_amd/sift_dist.py),
and the last step's gather is inside the timed region.

A plain run does only that: set-up, --warmup steps, --steps timed steps, the
--dump-outputs files if asked for (what the last timed step computed, as .npy:
see dump_outputs), and the one JSON line with the headline (`value`,
`ms_per_step`, ...).  Everything below runs only with --full.

Stage times and the per-kernel rooflines come from a separate serial leg (one
context, the whole batch, HIP events around every stage).

Outside the timed region rank 0 checks its image 0 (seed 0) -- and seeds 31
and 63 at the default shape -- against the CPU path's SHA-256 digests
(tests/golden) and reports "output_verified".  Further legs (rank 0, N=1
unless noted): SIFT_FLAG_FAST (separable pyramid, HBM roofline), configs[1]
single-image latency (hipGraph replay, 4 octaves), configs[4] (one 8K image,
output checked, pyramid rooflines at C5), the knnMatch leg, and the CPU
baseline (oracle, 1 thread + image-parallel on the host's cores).

Launch: python bench.py [--gpus N --steps K --warmup W] [--full]
[--dump-outputs DIR].  At N > 1 without a
launcher, bench.py starts `python -m torch.distributed.run --nproc-per-node N
--master-addr 127.0.0.1 ... bench.py <same args>` as a child process (one rank
per GPU, RCCL) and exits with its code; under a launcher WORLD_SIZE must equal
--gpus.  Rank 0 prints one JSON line.  Exit codes: 0 ok; 3 a device (HIP)
error was caught in an optional leg; 4 the headline's output check failed
(the line is printed first in both cases).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import platform
import subprocess
import sys
import time

import numpy as np
import torch  # first: its HIP runtime becomes the process-wide one
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "sift-gpu_amd"))
import siftgpu  # noqa: E402
import sift_dist  # noqa: E402

METRIC = "Mpix/s + keypoints/s, 1920×1080 grayscale, 1/2/4/8 MI355X vs CPU ref"
FP32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: FP32 vector peak (FMA = 2 flops, 2-cycle wave64 issue)
VALU_OP_PEAK_T = 78.65     # non-FMA fp32 lane-ops/s: 256 CU x 4 SIMD x 32 lanes x 2.4 GHz
VALU_ISSUE_PEAK_G = 1228.8  # wave64 VALU instructions/s (G): 256 CU x 4 SIMD x 2.4 GHz / 2 cycles
HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
GOLDEN = os.path.join(ROOT, "tests", "golden")
TRAFFIC_JSON = os.path.join(ROOT, "profiles", "traffic.json")


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--batch", type=int, default=64, help="images per GPU per step")
    p.add_argument("--rows", type=int, default=1080)
    p.add_argument("--cols", type=int, default=1920)
    p.add_argument("--octaves", type=int, default=5)
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-gather", action="store_true")
    p.add_argument("--no-fast", action="store_true", help="skip the SIFT_FLAG_FAST leg")
    p.add_argument("--no-match", action="store_true", help="skip the knnMatch leg (SURVEY 8(f) f2)")
    p.add_argument("--no-single", action="store_true", help="skip the configs[1] single-image leg")
    p.add_argument("--streams", type=int, default=2,
                   help="timed legs: the per-GPU batch as this many sub-batches, one context + HIP stream each")
    p.add_argument("--no-8k", action="store_true", help="skip the configs[4] 7680x4320 leg")
    p.add_argument("--no-multi", action="store_true", help="skip the C-ABI multi-GPU (sift_multi_*) leg")
    p.add_argument("--only", default=None, choices=[None, "exact", "fast", "single", "8k", "multi"],
                   help="profiling runs: time only this leg")
    p.add_argument("--profile-json", default=None, help="also write per-stage stats here (needs --full)")
    p.add_argument("--full", action="store_true",
                   help="besides the headline: its output check, the serial profiled leg (stage times, "
                        "rooflines), the CPU baselines and the fast / match / single / 8k / multi legs "
                        "(--only LEG implies it)")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="after the timed steps, write what the last step computed as DIR/<name>.npy")
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0:
        p.error("--steps must be >= 1 and --warmup >= 0")
    a.full = a.full or a.only is not None
    return a


# ---- CPU baseline (oracle = C restatement of the reference path) ------------
def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or "unknown"


def _oracle():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O  # the checker / CPU baseline only
    O.build()
    return O


ORACLE_NOTE = ("oracle/sift_oracle.c: SIFT_NCL restated in C, gcc -O3 -ffp-contract=off, no -march "
               "(reference makefile:25 flags); its blur tests the zero-padding bounds inline instead of "
               "copying each ksize^2 neighbourhood through getSubMatrix (src/sift.cpp:110-120), so it is "
               "faster than the reference's own loop (conservative for speed-up claims)")


def cpu_baseline(rows, cols, threads=1, min_seconds=0.0, max_images=8):
    """`threads` OpenMP threads (the reference's own split: the descriptor
    loop, src/sift.cpp:738; the rest of the path is serial there) over
    synthetic images of seeds 0, 1, ... until at least `min_seconds` of CPU
    work (one image at least, `max_images` at most): the bounded sample the
    rate is measured on."""
    O = _oracle()
    O.set_threads(threads)
    dt, nkp, n = 0.0, 0, 0
    while n < max(1, max_images) and (n == 0 or dt < min_seconds):
        img = O.synth_image(n, rows, cols)
        t0 = time.perf_counter()
        kps, _ = O.sift(img, 5)
        dt += time.perf_counter() - t0
        nkp += len(kps)
        n += 1
    O.set_threads(1)
    mpix = n * rows * cols / 1e6
    return {"value": round(mpix / dt, 4), "unit": "Mpix/s", "cores": threads, "kind": "port",
            "keypoints_per_s": round(nkp / dt, 1), "seconds": round(dt, 3),
            "sample": f"{n} synthetic {cols}x{rows} image(s) (seeds 0..{n - 1}), {threads} thread(s)"
                      f"{' (OpenMP over descriptors, as the reference)' if threads > 1 else ''}, "
                      f"{nkp} keypoints",
            "note": ORACLE_NOTE}


_WORKER = r"""
import sys, time
sys.path.insert(0, sys.argv[1])
import oracle as O
O.set_threads(1)
img = O.synth_image(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
t0 = time.perf_counter()
k, _ = O.sift(img, 5)
print(len(k), time.perf_counter() - t0)
"""


def cpu_baseline_parallel(rows, cols, workers):
    """Image-parallel rate on the GPU's share of the host (SURVEY.md 8(d) d4
    item 2): `workers` (16: an eighth of the GPU box's CPUs) independent
    processes, one image each, one thread each; rate = images / wall.  Child
    processes import only the oracle (no GPU)."""
    O = _oracle()
    del O
    t0 = time.perf_counter()
    procs = [subprocess.Popen([sys.executable, "-c", _WORKER, os.path.join(ROOT, "oracle"), str(100 + i),
                               str(rows), str(cols)], stdout=subprocess.PIPE, text=True,
                              env=dict(os.environ, OMP_NUM_THREADS="1", HIP_VISIBLE_DEVICES="",
                                       CUDA_VISIBLE_DEVICES=""))
             for i in range(workers)]
    try:
        outs = [p.communicate(timeout=600)[0].split() for p in procs]
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
            p.wait()
        raise
    wall = time.perf_counter() - t0
    if any(p.returncode for p in procs):
        return None
    nkp = sum(int(o[0]) for o in outs)
    per_img = [float(o[1]) for o in outs]
    mpix = workers * rows * cols / 1e6
    nproc = os.cpu_count() or workers
    return {"value": round(mpix / wall, 4), "unit": "Mpix/s", "cores": workers, "kind": "port",
            "cores_note": f"{workers} of {nproc} host CPUs: the per-GPU share of an 8-GPU node, not all cores",
            "keypoints_per_s": round(nkp / wall, 1), "seconds_wall": round(wall, 3),
            "seconds_per_image_median": round(float(np.median(per_img)), 3),
            "sample": f"{workers} synthetic {cols}x{rows} images (seeds 100..{99 + workers}), one process and "
                      f"one thread per image, all started together",
            "note": ORACLE_NOTE}


# ---- output check -----------------------------------------------------------
def _sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def verify_outputs(parts, R, C, octaves, seed_base):
    """Digest check of this rank's outputs against the CPU path's
    (tests/golden/make_golden.py).  parts: (first image, images, kpts, desc,
    offs) per sub-batch.  Returns (verified seeds, failures)."""
    if octaves != 5 or (R, C) != (1080, 1920):
        return [], ["no golden digests for this shape / octave count"]
    gold = {}
    g0 = np.load(os.path.join(GOLDEN, "synth0_1080x1920.npz"), allow_pickle=False)
    gold[0] = (int(g0["n"]), str(g0["kp_sha"]), str(g0["desc_sha"]))
    gb = np.load(os.path.join(GOLDEN, "batch_1080x1920.npz"), allow_pickle=False)
    for s, n, ks, ds in zip(gb["seeds"], gb["n"], gb["kp_sha"], gb["desc_sha"]):
        gold[int(s)] = (int(n), str(ks), str(ds))
    ok, bad = [], []
    for seed, (n, ks, ds) in sorted(gold.items()):
        for b0, nb, kpts, desc, offs in parts:
            b = seed - seed_base - b0
            if not 0 <= b < nb:
                continue
            o = offs.cpu().numpy().astype(np.int64)
            a, e = int(o[b]), int(o[b + 1])
            k = kpts[a:e].cpu().numpy()
            d = desc[a:e].cpu().numpy()
            if e - a == n and _sha(k) == ks and _sha(d) == ds:
                ok.append(seed)
            else:
                bad.append(seed)
    return ok, bad


def load_traffic():
    try:
        with open(TRAFFIC_JSON) as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


def traffic_of(tr, kernel):
    k = tr.get("kernels", {}).get(kernel)
    if not k:
        return None, None
    return k["read_bytes"] + k["write_bytes"], tr.get("source")


def valu_issue_frac(tr, kernel, launch_ms):
    """SQ_INSTS_VALU per launch (committed PMC pass) / the live launch time,
    as a fraction of the wave64 VALU issue peak (VALU_ISSUE_PEAK_G)."""
    valu = tr.get("kernels", {}).get(kernel, {}).get("valu_insts")
    if not valu or not launch_ms:
        return None
    return round(valu / (launch_ms * 1e-3) / 1e9 / VALU_ISSUE_PEAK_G, 4)


def descriptor_roofline(tr, d):
    """descriptor_kernel against the VALU issue ceiling: its work is integer /
    float bookkeeping per window sample (gather, exp32f, trilinear weights, bin
    hand-off), no FMA stream, so the bound is wave-instructions issued.
    achieved = SQ_INSTS_VALU per launch (committed rocprofv3 SQ pass over
    tools/stage_bench.py, same 64 x 1080p batch) / the live average launch
    time; peak = 256 CU x 4 SIMD x 2.4 GHz / 2 cycles per wave64 VALU
    instruction (MI355X_MICROARCH.md)."""
    launches = max(d["launches"], 1)
    ms = d["ms"] / launches
    k = tr.get("kernels", {}).get("descriptor_kernel", {})
    valu = k.get("valu_insts")
    out = {"bound": "valu", "unit": "Ginstr/s", "peak": VALU_ISSUE_PEAK_G, "kernel": "descriptor_kernel",
           "avg_launch_ms": round(ms, 4), "valu_insts_per_launch": valu, "lds_insts_per_launch": k.get("lds_insts"),
           "traffic": (k["read_bytes"] + k["write_bytes"]) if "read_bytes" in k else None,
           "traffic_source": tr.get("source")}
    if valu and ms:
        g = valu / (ms * 1e-3) / 1e9
        out.update({"achieved": round(g, 1), "frac": round(g / VALU_ISSUE_PEAK_G, 4)})
    else:
        out.update({"achieved": None, "frac": None})
    return out


# ---- single image (configs[1]) ------------------------------------------------
def single_image_leg(R, C, steps, warmup, octaves=4):
    """configs[1]: one 1920x1080 image, 4 octaves x 5 scales.
    device: image resident in HBM, sift_detect_compute_batch(batch 1) = the
      captured hipGraph of the whole sequence, each call followed by
      sift_sync (per-image latency incl. the wait);
    host: SIFT_NCL from a host numpy image to host keypoints/descriptors
      (upload, graphed compute, one wait for the count, one copy of n results)."""
    out = {}
    with siftgpu.Context(R, C, 1, device=torch.cuda.current_device()) as ctx:
        ctx.set_octaves(octaves)
        img = torch.empty((1, R, C), dtype=torch.float32, device="cuda")
        ctx.synth_images(img.data_ptr(), 1, R, C, C, R * C, seed_base=0)
        cap = 40000
        kpts = torch.empty((cap, 7), dtype=torch.int32, device="cuda")
        desc = torch.empty((cap, 128), dtype=torch.float32, device="cuda")
        offs = torch.empty((2,), dtype=torch.int32, device="cuda")
        for mode, flags in (("graph", 0), ("no_graph", siftgpu.SIFT_FLAG_NO_GRAPH)):
            ctx.set_flags(flags)

            def call():
                ctx.detect_compute_batch(img.data_ptr(), 1, R, C, C, R * C, kpts.data_ptr(), desc.data_ptr(), cap,
                                         offs.data_ptr())
                ctx.sync()
            for _ in range(warmup + 1):
                call()
            ts = []
            for _ in range(max(steps, 10)):
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
            out[f"device_{mode}_ms"] = round(float(np.median(ts)) * 1e3, 4)
        n = int(offs[1].item())
        ctx.set_flags(0)
        host = img[0].cpu().numpy()
        for _ in range(warmup + 1):
            kps, dsc = ctx.SIFT_NCL(host)
        ts = []
        for _ in range(max(steps, 10)):
            t0 = time.perf_counter()
            kps, dsc = ctx.SIFT_NCL(host)
            ts.append(time.perf_counter() - t0)
        out["host_ms"] = round(float(np.median(ts)) * 1e3, 4)
        # H2D / D2H separately: the host call's upload and
        # download stages, HIP events on the context stream (PROFILE mode)
        ctx.set_flags(siftgpu.SIFT_FLAG_PROFILE)
        ctx.stage_stats(reset=True)
        reps = max(steps, 10)
        for _ in range(reps):
            ctx.SIFT_NCL(host)
        st = ctx.stage_stats(reset=True)
        ctx.set_flags(0)
        for k in ("upload", "download"):
            if k in st and st[k]["ms"] > 0:
                ms = st[k]["ms"] / reps
                out[f"{k}_ms"] = round(ms, 4)
                out[f"{k}_GBs"] = round(st[k]["bytes"] / reps / (ms * 1e-3) / 1e9, 2)
        gb = np.load(os.path.join(GOLDEN, "batch_1080x1920.npz"), allow_pickle=False)
        verified = (R, C) == (1080, 1920) and octaves == 4 and len(kps) == int(gb["oct4_n"]) and \
            _sha(kps) == str(gb["oct4_kp_sha"]) and _sha(dsc) == str(gb["oct4_desc_sha"])
    lat = out["device_graph_ms"]
    out.update({
        "config": f"configs[1]: one {C}x{R} synthetic image (seed 0), {octaves} octaves x 5 scales, exact mode",
        "keypoints": n, "output_verified": bool(verified),
        "latency_ms": lat, "Mpix_per_s": round(R * C / 1e6 / (lat * 1e-3), 2),
        "keypoints_per_s": round(n / (lat * 1e-3), 1),
        "keypoints_per_s_host_to_host": round(n / (out["host_ms"] * 1e-3), 1),
        "note": "latency = median wall time of one call + sift_sync, image resident in HBM; host_ms = "
                "SIFT_NCL from host memory to host memory (H2D 8.3 MB, graphed compute, one wait, D2H of n "
                "records); upload/download = the H2D image copy and D2H result copy of that call alone "
                "(pageable host memory, HIP events); output_verified = the host call's keypoints/descriptors "
                "equal the CPU path's "
                "(5-octave output filtered to octave <= 3, tests/golden/batch_1080x1920.npz)"})
    return out


# ---- 8K single image (configs[4]) ---------------------------------------------
def eightk_leg(steps, warmup, R8=4320, C8=7680):
    """configs[4]: one 7680x4320 synthetic image (seed 0), 5 octaves, exact
    mode, resident in HBM: graph replay + sift_sync latency, output checked
    against the CPU path's digests (tests/golden/synth0_4320x7680.npz).  Then
    the pyramid rooflines SURVEY 8(d) d3 asks for at C5: the exact octave blur
    and the SIFT_FLAG_FAST separable pyramid, from PROFILE-mode HIP events."""
    out = {}
    g = np.load(os.path.join(GOLDEN, "synth0_4320x7680.npz"), allow_pickle=False)
    with siftgpu.Context(R8, C8, 1, device=torch.cuda.current_device()) as ctx:
        img = torch.empty((1, R8, C8), dtype=torch.float32, device="cuda")
        ctx.synth_images(img.data_ptr(), 1, R8, C8, C8, R8 * C8, seed_base=0)
        cap = 400000
        kpts = torch.empty((cap, 7), dtype=torch.int32, device="cuda")
        desc = torch.empty((cap, 128), dtype=torch.float32, device="cuda")
        offs = torch.empty((2,), dtype=torch.int32, device="cuda")

        def call():
            ctx.detect_compute_batch(img.data_ptr(), 1, R8, C8, C8, R8 * C8, kpts.data_ptr(), desc.data_ptr(), cap,
                                     offs.data_ptr())
            ctx.sync()
        for _ in range(warmup + 1):
            call()
        ts = []
        for _ in range(max(steps, 5)):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        lat = float(np.median(ts))
        n = int(offs[1].item())
        verified = n == int(g["n"]) and _sha(kpts[:n].cpu().numpy()) == str(g["kp_sha"]) and \
            _sha(desc[:n].cpu().numpy()) == str(g["desc_sha"])
        px = sum((R8 >> o) * (C8 >> o) for o in range(5))
        roof = {}
        for name, flags, stage in (("exact_blur_octave", siftgpu.SIFT_FLAG_PROFILE, "blur_octave"),
                                   ("fast_pyramid", siftgpu.SIFT_FLAG_PROFILE | siftgpu.SIFT_FLAG_FAST,
                                    "pyramid_fast")):
            ctx.set_flags(flags)
            call()
            ctx.stage_stats(reset=True)
            reps = max(steps, 5)
            for _ in range(reps):
                call()
            sts = ctx.stage_stats(reset=True)
            st = sts.get(stage)
            if stage == "blur_octave" and "blur_octave_sym" in sts:  # both blur forms: one figure
                st = {k: (st or {}).get(k, 0) + sts["blur_octave_sym"][k] for k in ("ms", "flops")}
            if not st or not st["ms"]:
                continue
            if stage == "blur_octave":
                tf = st["flops"] / (st["ms"] * 1e-3) / 1e12
                roof[name] = {"bound": "valu", "achieved": round(tf, 2), "peak": FP32_PEAK_TFLOPS,
                              "unit": "TFLOP/s", "frac": round(tf / FP32_PEAK_TFLOPS, 4),
                              "ms_per_image": round(st["ms"] / reps, 4)}
            else:
                gbs = st["bytes"] / (st["ms"] * 1e-3) / 1e9
                roof[name] = {"bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": round(gbs / HBM_PEAK_GBS, 4), "ms_per_image": round(st["ms"] / reps, 4),
                              "algorithmic_bytes": round(24.0 * px)}
        ctx.set_flags(0)
    out.update({"config": f"configs[4]: one {C8}x{R8} synthetic image (seed 0), 5 octaves x 5 scales, exact mode",
                "latency_ms": round(lat * 1e3, 3), "Mpix_per_s": round(R8 * C8 / 1e6 / lat, 1),
                "keypoints": n, "keypoints_per_s": round(n / lat, 1), "output_verified": bool(verified),
                "roofline": roof,
                "note": "latency = median wall time of sift_detect_compute_batch(batch 1) + sift_sync, image "
                        "resident in HBM (graph replay); roofline legs use PROFILE-mode HIP events per stage"})
    return out


# ---- the C-ABI multi-GPU path (sift_multi_*, csrc/multi.hip) at n = 1 ----------
def c_abi_multi_leg(env, steps, warmup):
    """configs[3]'s C++-host path on this GPU alone: the headline batch
    (--batch images, this rank's synthetic images) through sift_multi_step on
    one device -- --streams contexts and HIP streams as in the headline, graph
    replay, the records gathered one step behind (device 0's own pieces by
    DMA copy) -- timed like a leg (flush inside the timed region).  The rate beside `value` shows what the C ABI's multi path
    costs against bench.py's two-stream Python driver."""
    a = env.a
    B, R, C = env.B, env.R, env.C
    with siftgpu.MultiContext([env.dev], R, C, B, B * 40000, streams_per_device=env.S) as m:
        m.set_octaves(env.octaves)
        ptr = env.imgs.data_ptr()
        for _ in range(warmup):
            m.step([ptr], [B], R, C, C, R * C)
        m.flush()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            m.step([ptr], [B], R, C, C, R * C)
        m.flush()
        dt = time.perf_counter() - t0
        _, _, offs, _ = m.gathered(B + 1)
        st = m.stats()
    return {"n_devices": 1, "streams_per_device": env.S, "Mpix_per_s": round(B * R * C * steps / 1e6 / dt, 2),
            "ms_per_step": round(dt / steps * 1e3, 3), "keypoints_per_step": int(offs[-1]),
            "rccl_version": siftgpu.rccl_version(), "rccl_p2p_transfers": st["transfers"],
            "records_gathered": st["records"],
            "note": "sift_multi_create/_step/_flush (include/sift_hip.h) on this one GPU: the shard as "
                    "streams_per_device sub-batches on their own contexts and HIP streams, the 28-B records "
                    "gathered to device 0 one step behind (other devices over RCCL p2p; device 0's own by DMA "
                    "copy, so no RCCL transfer at n = 1); tests/cpp/multi_gpu.cpp is the same path from C++"}


# ---- knnMatch leg ---------------------------------------------
def match_leg(ctx, a, desc, offs):
    """src/main.cpp:27 on the batch's own output: knnMatch(k=2) of image 1's
    descriptors (queries) against image 0's (train), device buffers, W + K
    launches timed with the context's HIP events (rank 0 only; not in `value`)."""
    o = [int(x) for x in offs[:3].tolist()]
    nt, nq = o[1] - o[0], o[2] - o[1]
    train, query = desc[o[0]:o[1]], desc[o[1]:o[2]]
    idx = torch.empty((nq, 2), dtype=torch.int32, device="cuda")
    dst = torch.empty((nq, 2), dtype=torch.float32, device="cuda")
    ctx.set_flags(siftgpu.SIFT_FLAG_PROFILE)

    def run():
        ctx.knn_match_device(query.data_ptr(), nq, train.data_ptr(), nt, 2, idx.data_ptr(), dst.data_ptr())
    for _ in range(a.warmup):
        run()
    ctx.sync()
    ctx.stage_stats(reset=True)
    for _ in range(a.steps):
        run()
    st = ctx.stage_stats(reset=True)["match"]
    ms = st["ms"] / max(st["launches"], 1)
    return {"n_query": nq, "n_train": nt, "ms": ms, "flops": st["flops"] / max(st["launches"], 1),
            "idx": idx, "dist": dst, "query": query, "train": train}


def match_cpu_baseline(m, n_sample=64):
    """oracle/match.py (numpy, this process's BLAS-free float32 ops) on a sample
    of the leg's queries against the full train set."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import match as M  # the checker / CPU baseline only
    q = m["query"][:n_sample].cpu().numpy()
    t = m["train"].cpu().numpy()
    t0 = time.perf_counter()
    ridx, rdist = M.knn_match(q, t, 2)
    dt = time.perf_counter() - t0
    same = bool((ridx == m["idx"][:n_sample].cpu().numpy()).all() and
                (rdist.view("u4") == m["dist"][:n_sample].cpu().numpy().view("u4")).all())
    return {"value": round(len(q) * len(t) / dt / 1e6, 2), "unit": "Mpairs/s", "cores": 1, "kind": "port",
            "sample": f"{len(q)} queries x {len(t)} train rows (oracle/match.py, numpy float32, normL1_ order)",
            "gpu_equals_oracle_on_sample": same}


def is_gpu_error(e) -> bool:
    """A device-side failure: the library's HIP error code, or torch's
    accelerator error (a HIP runtime error raised by torch)."""
    if isinstance(e, siftgpu.SiftError) and e.code == siftgpu.SIFT_E_HIP:
        return True
    acc = getattr(torch, "AcceleratorError", None)
    if acc is not None and isinstance(e, acc):
        return True
    return isinstance(e, RuntimeError) and str(e).startswith(("HIP error", "CUDA error"))


GPU_ERROR_LEGS = set()   # legs whose caught exception was a device-side failure


def guarded(errors, name, fn, *args, **kw):
    """Runs one optional leg; a failure is recorded as errors[name] and the
    leg's block as {"error": ...} instead of costing the headline line."""
    try:
        return fn(*args, **kw)
    except Exception as e:  # noqa: BLE001 -- any failure of an optional leg
        errors[name] = f"{type(e).__name__}: {e}"[:400]
        if is_gpu_error(e):
            GPU_ERROR_LEGS.add(name)
        print(f"bench.py: leg {name} failed: {errors[name]}", file=sys.stderr, flush=True)
        return None


def cpu_legs(a, errors):
    """1 thread, OpenMP over descriptors, image-parallel."""
    nthr = min(16, int(os.environ.get("OMP_NUM_THREADS", "16")))
    cpu = {}
    # the 1-thread baseline: about 10 s of CPU work (3 images at ~3.2 s each)
    one = guarded(errors, "cpu_baseline", cpu_baseline, a.rows, a.cols, 1, 9.0)
    if one is not None:
        cpu["cpu_baseline"] = one
    omp = guarded(errors, "cpu_baseline_omp", cpu_baseline, a.rows, a.cols, nthr)
    if omp is not None:
        cpu["cpu_baseline_omp"] = omp
    par = guarded(errors, "cpu_baseline_gpu_share", cpu_baseline_parallel, a.rows, a.cols, nthr)
    if par:
        cpu["cpu_baseline_gpu_share"] = par
    cpu["cpu_host"] = {"nproc": os.cpu_count(), "model": _cpu_model(), "share_used": nthr,
                       "compiler_flags": "gcc -O3 -ffp-contract=off -fno-fast-math"}
    return cpu


class Part:
    """One context on one stream over images [b0, b0 + nb) of this rank's
    batch; with `gather`, its results go to rank 0 one step behind
    (sift_dist.PipelinedSteps, two result slots)."""

    def __init__(self, env, b0, nb, strm, gather):
        self.env, self.b0, self.nb, self.stream = env, b0, nb, strm
        R, C = env.R, env.C
        self.ctx = siftgpu.Context(R, C, nb, device=env.dev)
        self.ctx.set_stream(strm.cuda_stream)
        self.ctx.set_octaves(env.octaves)
        self.cap = nb * 40000
        self.bufs = [(torch.empty((self.cap, 7), dtype=torch.int32, device="cuda"),
                      torch.empty((self.cap, 128), dtype=torch.float32, device="cuda"),
                      torch.empty((nb + 1,), dtype=torch.int32, device="cuda")) for _ in range(2 if gather else 1)]
        self.runner = self.pipe = None
        if gather:
            def on_result(step, out, first=(b0 == 0)):
                env.gathered["steps"] += 1 if first else 0
                env.gathered["keypoints"] += sum(int(o[-1]) for o in out[1])
            self.pipe = sift_dist.GatherPipeline(env.shard_batches(nb), self.cap, dst=0, timing=True)
            self.runner = sift_dist.PipelinedSteps(self.pipe, self.bufs, with_desc=False, on_result=on_result)

    def compute(self, k, d, o):
        e = self.env
        self.ctx.detect_compute_batch(e.imgs[self.b0].data_ptr(), self.nb, e.R, e.C, e.C, e.R * e.C, k.data_ptr(),
                                      d.data_ptr(), self.cap, o.data_ptr())

    def step(self):
        with torch.cuda.stream(self.stream):
            if self.runner is not None:
                self.runner.step(self.compute)
            else:
                self.compute(*self.bufs[0])

    def flush(self):
        if self.runner is not None:
            with torch.cuda.stream(self.stream):
                self.runner.flush()

    def last_bufs(self):
        """The (kpts, desc, offs) the last timed step wrote: with a gather,
        step i of a leg uses slot i % 2."""
        return self.bufs[(self.env.a.steps - 1) % 2 if self.runner is not None else 0]

    def close(self):
        self.ctx.close()


class Env:
    """This rank's device state: the synthetic batch, the timed parts and the
    serial (profiled) part."""

    def __init__(self, a, world, rank):
        self.a, self.world, self.rank = a, world, rank
        self.dev = torch.cuda.current_device()
        self.B, self.R, self.C, self.octaves = a.batch, a.rows, a.cols, a.octaves
        self.S = max(1, min(a.streams, self.B // 2))
        self.seed_base = rank * self.B
        self.imgs = torch.empty((self.B, self.R, self.C), dtype=torch.float32, device="cuda")
        self.gathering = world > 1 and not a.no_gather
        self.gathered = {"steps": 0, "keypoints": 0}
        B, S = self.B, self.S
        self.parts = [Part(self, B * s // S, B * (s + 1) // S - B * s // S,
                           torch.cuda.Stream() if S > 1 else torch.cuda.current_stream(), self.gathering)
                      for s in range(S)]
        # the serial (profiled) part holds a whole-batch context: --full only
        self.serial = Part(self, 0, B, torch.cuda.current_stream(), False) if a.full else None
        for p in self.parts:   # image b of this rank is seed seed_base + b, whichever part generates it
            p.ctx.synth_images(self.imgs[p.b0].data_ptr(), p.nb, self.R, self.C, self.C, self.R * self.C,
                               seed_base=self.seed_base + p.b0)
        torch.cuda.synchronize()

    def shard_batches(self, nb):
        return [nb] * self.world   # every rank runs the same --batch / --streams split

    def leg(self, ps, flags):
        """W warmup + K timed steps of parts ps in one mode; returns (max-over-
        ranks seconds, per-stage device stats of this rank (one part), keypoints
        per step summed over ranks)."""
        a, world = self.a, self.world
        for p in ps:
            p.ctx.set_flags(flags)
        for _ in range(a.warmup):
            for p in ps:
                p.step()
        for p in ps:
            p.flush()
        for p in ps:
            p.ctx.sync()  # sticky device status: candidate / keypoint capacity
            p.ctx.stage_stats(reset=True)
            if p.pipe is not None:
                p.pipe.reset_stats()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            for p in ps:
                p.step()
        for p in ps:
            p.flush()   # the last step's gather is part of the timed work
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        dt = time.perf_counter() - t0
        stats = {}
        for p in ps:
            p.ctx.sync()  # raises if any timed step overflowed a capacity
            stats = p.ctx.stage_stats(reset=True)
        kp_step = torch.tensor([float(sum(int(p.bufs[0][2][-1].item()) for p in ps))], dtype=torch.float64,
                               device="cuda")
        t = torch.tensor([dt], dtype=torch.float64, device="cuda")
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dist.all_reduce(kp_step, op=dist.ReduceOp.SUM)
        return float(t.item()), stats, float(kp_step.item())

    def gather_evidence(self, dt):
        """N > 1: per-rank gather statistics of the timed exact leg, collected
        on rank 0 (gloo metadata group): backend, world size, records each rank
        sent / rank 0 received, and the side-stream transfer time as a share of
        the timed region."""
        mine = {"sent_records": 0, "received_records_per_rank": [0] * self.world, "transfer_ms": 0.0,
                "gathers": 0}
        for p in self.parts:
            if p.pipe is None:
                continue
            st = p.pipe.stats()
            mine["sent_records"] += st["sent_records"]
            mine["gathers"] += st["gathers"]
            mine["received_records_per_rank"] = [x + y for x, y in zip(mine["received_records_per_rank"],
                                                                      st["received_records_per_rank"])]
            mine["transfer_ms"] += st["transfer_ms"] or 0.0
        allst = [None] * self.world
        dist.all_gather_object(allst, mine, group=sift_dist._meta_group())
        if self.rank != 0:
            return None
        recv = allst[0]["received_records_per_rank"]
        sent = [s["sent_records"] for s in allst]
        return {"backend": dist.get_backend(), "world_size": dist.get_world_size(),
                "steps_gathered": self.gathered["steps"],
                "keypoints_gathered_per_step": self.gathered["keypoints"] / max(self.gathered["steps"], 1),
                "received_records_per_rank": recv, "sent_records_per_rank": sent,
                "sent_equals_received": all(recv[r] == sent[r] for r in range(1, self.world)),
                "transfer_ms_per_rank": [round(s["transfer_ms"], 3) for s in allst],
                "transfer_share_of_timed_region": [round(s["transfer_ms"] / (dt * 1e3), 4) for s in allst],
                "note": "keypoint records (28 B) of every rank's sub-batches gathered to rank 0 one step "
                        "behind compute (batch_isend_irecv on a side stream); transfer_ms = device time of "
                        "those transfer groups summed over the timed leg, overlapped with compute"}

    def close(self):
        for p in self.parts + ([self.serial] if self.serial is not None else []):
            p.close()


DUMP_BYTES = 48 << 20   # --dump-outputs: budget for the sampled records (the whole dump stays under 64 MB)


def dump_outputs(path, env):
    """--dump-outputs: what the timed parts hold after the last timed step,
    as a caller of sift_detect_compute_batch receives it.  offsets.npy: the
    B + 1 per-image keypoint offsets of the whole batch.  The keypoint
    records (x, y, size, angle, response as stored; octave, class_id as
    numbers) and the 128-float descriptors are written for a fixed sample of
    whole images (seeded order, as many as fit DUMP_BYTES; of an image that
    alone is larger, its leading rows): sample_images.npy names them,
    sample_offsets.npy delimits their rows in keypoints.npy / descriptors.npy."""
    os.makedirs(path, exist_ok=True)
    counts, images = [], {}
    for p in env.parts:
        k, d, o = p.last_bufs()
        o = o.cpu().numpy().astype(np.int64)
        counts.extend(np.diff(o).tolist())
        for b in range(p.nb):
            images[p.b0 + b] = (k, d, int(o[b]), int(o[b + 1]))
    max_rows = DUMP_BYTES // (7 * 8 + siftgpu.DESC_LEN * 4)
    chosen, rows = [], 0
    for b in np.random.default_rng(0).permutation(env.B).tolist():
        if rows + counts[b] > max_rows:
            break
        chosen.append(b)
        rows += counts[b]
    kps, descs, soffs = [], [], [0]
    for b in chosen or [0]:
        k, d, lo, hi = images[b]
        hi = min(hi, lo + max_rows)
        rec = k[lo:hi].cpu().numpy()
        kp = np.empty((hi - lo, 7), dtype=np.float64)
        kp[:, :5] = rec[:, :5].view(np.float32)
        kp[:, 5:] = rec[:, 5:]
        kps.append(kp)
        descs.append(d[lo:hi].cpu().numpy().astype(np.float32, copy=False))
        soffs.append(soffs[-1] + hi - lo)
    np.save(os.path.join(path, "offsets.npy"), np.concatenate([[0], np.cumsum(counts)]).astype(np.float64))
    np.save(os.path.join(path, "sample_images.npy"), np.asarray(chosen or [0], dtype=np.float64))
    np.save(os.path.join(path, "sample_offsets.npy"), np.asarray(soffs, dtype=np.float64))
    np.save(os.path.join(path, "keypoints.npy"), np.concatenate(kps))
    np.save(os.path.join(path, "descriptors.npy"), np.concatenate(descs))


def run_exact(env):
    """The headline: the exact leg (timed streams); with --full its output
    check and the serial profiled leg (stage times, rooflines) as well."""
    exact = env.leg(env.parts, 0)
    if env.a.dump_outputs and env.rank == 0:
        dump_outputs(env.a.dump_outputs, env)
    verified = failed = prof = None
    if env.a.full and env.rank == 0:
        verified, failed = verify_outputs([(p.b0, p.nb) + p.bufs[0] for p in env.parts], env.R, env.C,
                                          env.octaves, env.seed_base)
    gather = env.gather_evidence(exact[0]) if env.gathering else None
    if env.a.full:
        prof = env.leg([env.serial], siftgpu.SIFT_FLAG_PROFILE)
    return {"exact": exact, "prof": prof, "verified": verified, "failed": failed, "gather": gather}


def run_fast(env):
    # the same --streams split as the exact leg (2 streams: 12.8-12.9 vs
    # 13.2-13.4 ms per step on one stream, round 2 final tree)
    fast = env.leg(env.parts, siftgpu.SIFT_FLAG_FAST)
    fast_prof = env.leg([env.serial], siftgpu.SIFT_FLAG_PROFILE | siftgpu.SIFT_FLAG_FAST)
    return fast, fast_prof


def run_match(env):
    s = env.serial
    s.ctx.set_flags(0)
    s.compute(*s.bufs[0])
    s.ctx.sync()
    return match_leg(s.ctx, env.a, s.bufs[0][1], s.bufs[0][2])


def profile_block(a, world, B, R, C, res, tr):
    """--full: stage times and rooflines from run_exact's serial profiled leg."""
    out = {}
    kp_total_step = res["exact"][2]
    pdt, stats, _ = res["prof"]
    mpix = world * B * R * C * a.steps / 1e6

    # roofline of the dominant kernel: the exact octave blur -- octave 0
    # in scatter form (blur_sym_kernel) when the library chose it for
    # this launch size, the 2-D tiles (blur_octave_kernel) otherwise
    def blur_roof(stage, kernel):
        bo = stats.get(stage)
        if not bo or not bo["launches"]:
            return None
        per_launch_ms = bo["ms"] / bo["launches"]
        tflops = (bo["flops"] / bo["launches"]) / (per_launch_ms * 1e-3) / 1e12 if per_launch_ms else 0.0
        traffic, tsrc = traffic_of(tr, kernel)
        r = {"bound": "valu", "achieved": round(tflops, 2), "peak": FP32_PEAK_TFLOPS, "unit": "TFLOP/s",
             "frac": round(tflops / FP32_PEAK_TFLOPS, 4), "traffic": traffic,
             "traffic_algorithmic": round(bo["bytes"] / bo["launches"]),
             "traffic_source": tsrc, "kernel": kernel, "launches_per_step": bo["launches"] // a.steps,
             "avg_launch_ms": round(per_launch_ms, 4),
             "valu_issue_frac": valu_issue_frac(tr, kernel, per_launch_ms),
             "note": "exact-mode 2-D blur is fp32-VALU bound, no MFMA; peak = the fp32 vector peak "
                     "(FMA counted as 2 flops); flops = 2 x taps per launch, algorithmic (the "
                     "reference's chain: one multiply + one add per tap, FMA forbidden by the parity "
                     "contract), 4 scales x the whole batch; traffic = HBM bytes per launch from the "
                     "committed rocprofv3 PMC pass (calibrated FETCH_SIZE/WRITE_SIZE); valu_issue_frac = "
                     "SQ_INSTS_VALU per launch (same PMC pass) / launch time / the wave64 VALU issue peak "
                     "(256 CU x 4 SIMD x 2.4 GHz / 2 cycles)"}
        if kernel == "blur_sym_kernel":
            r["note"] += ("; scatter form: K[a][b] = K[-a][b], so each multiply serves kernel rows +a "
                          "and -a of two outputs -- (2w+1)(w+1) multiplies + (2w+1)^2 adds per output "
                          "instead of 2(2w+1)^2, same chain, bit-exact -- which is why frac can pass 0.5")
        return r
    sym_used = "blur_octave_sym" in stats
    roof = blur_roof("blur_octave_sym", "blur_sym_kernel") if sym_used else \
        blur_roof("blur_octave", "blur_octave_kernel")
    roof_gather = blur_roof("blur_octave", "blur_octave_kernel") if sym_used else None
    pyr_ms = sum(stats[k]["ms"] for k in ("blur_base", "blur_octave", "blur_octave_sym", "decimate", "dog")
                 if k in stats)
    pyr_bytes = 24.0 * sum(sum((R >> o) * (C >> o) for o in range(a.octaves)) for _ in range(B)) * a.steps
    out.update({
        "roofline": roof,
        "roofline_octaves_2d_tiles": roof_gather,
        "pyramid": {"ms_per_step": round(pyr_ms / a.steps, 3),
                    "algorithmic_GBs": round(pyr_bytes / (pyr_ms * 1e-3) / 1e9, 1) if pyr_ms else None,
                    "note": "B_pyr = 24 B x sum of octave pixels (1 read + 5 plane writes), SURVEY.md 8(d)"},
        "stages_ms_per_step": {k: round(v["ms"] / a.steps, 3) for k, v in stats.items()},
        "serial_leg": {"ms_per_step": round(pdt / a.steps * 1e3, 3),
                       "Mpix_per_s": round(mpix / pdt, 2),
                       "note": "one context, the whole batch on one stream, HIP events around every "
                               "stage (SIFT_FLAG_PROFILE, no graph): the source of stages_ms_per_step, "
                               "roofline and descriptor; value is the streams leg (graph replay, no "
                               "events)"},
    })
    d = stats.get("descriptor")
    if d:
        out["descriptor"] = {"ms_per_step": round(d["ms"] / a.steps, 3),
                             "keypoints_per_s_kernel": round(kp_total_step / world * a.steps /
                                                             (d["ms"] * 1e-3), 1),
                             "roofline": descriptor_roofline(tr, d)}
    return out


def exact_block(a, world, B, R, C, S, res, tr):
    """The headline fields from run_exact's result; with --full the output
    check's verdict in front and profile_block's fields behind them."""
    out = {}
    dt, _, kp_total_step = res["exact"]
    verified, failed = res["verified"], res["failed"]
    mpix = world * B * R * C * a.steps / 1e6
    value = mpix / dt
    gathering = res.get("gather") is not None
    backend = (res.get("gather") or {}).get("backend")
    if verified is not None:
        # first after the metric: the driver's record keeps only the line's head
        out.update({"output_verified": bool(verified) and not failed,
                    "output_verified_seeds": verified})
    out.update({
        "value": round(value, 2),
        "unit": "Mpix/s",
        "n_gpus": world,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": round(dt / a.steps * 1e3, 3),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic: integer-exact 1920x1080 textures (SURVEY.md 8(d) d2) generated on device",
        "config": {"workload": f"configs[2]: batch of {B} x {C}x{R} synthetic grayscale per GPU "
                               f"(N=8 x 64 = configs[3]), {a.octaves} octaves x 5 scales, exact mode",
                   "global_batch": world * B, "rows": R, "cols": C, "octaves": a.octaves,
                   "mode": "exact (bit-identical to the CPU path)",
                   "parallelism": f"image-sharded x{world}, {S} HIP streams x {B // S} images per GPU" +
                                  (f", keypoint gather to rank 0 one step behind over {gather_label(backend)}"
                                   if gathering else "")},
        "keypoints_per_s": round(kp_total_step * a.steps / dt, 1),
        "keypoints_per_step": int(kp_total_step),
    })
    if res["prof"] is not None:
        out.update(profile_block(a, world, B, R, C, res, tr))
    if failed:
        out["output_failed_seeds"] = failed
    if gathering:
        out["gather"] = res["gather"]
    return out


def gather_label(backend) -> str:
    """What actually carried the keypoint gather: torch.distributed's "nccl"
    backend is RCCL on ROCm; anything else (the shared-GPU gloo rehearsal)
    is named as what it is."""
    if backend == "nccl":
        return "RCCL (torch.distributed nccl backend, xGMI p2p)"
    return f"{backend} (host-staged; not RCCL)"


def fast_kernel():
    """The SIFT_FLAG_FAST pyramid kernel (sift-gpu_amd/csrc/pyramid_pc.hip)."""
    return "pyr_pc_kernel", "pyramid_pc.hip"


def fast_block(a, world, B, R, C, fast_res, tr):
    (fdt, _, fkp), fast_prof = fast_res
    kname, kfile = fast_kernel()
    fst = fast_prof[1]
    mpix = world * B * R * C * a.steps / 1e6
    pf = fst.get("pyramid_fast", {"ms": 0.0, "bytes": 0.0, "launches": 0})
    gbs = pf["bytes"] / (pf["ms"] * 1e-3) / 1e9 if pf["ms"] else 0.0
    traffic, tsrc = traffic_of(tr, kname)
    fm = {
        "value": round(mpix / fdt, 2), "unit": "Mpix/s", "ms_per_step": round(fdt / a.steps * 1e3, 3),
        "keypoints_per_s": round(fkp * a.steps / fdt, 1), "keypoints_per_step": int(fkp),
        "stages_ms_per_step": {k: round(v["ms"] / a.steps, 3) for k, v in fst.items()},
        "note": "the exact leg's stream split (--streams), graph replay; SIFT_FLAG_FAST: separable row/column "
                f"Gaussian pyramid ({kfile}) in front of the same exact DoG/extrema/orientation/"
                "descriptor kernels; not bit-exact (float rounding of the pyramid), keypoint/descriptor "
                "match rates vs the CPU path are in tests/test_gpu_fast.py"}
    roof = {
        "bound": "hbm", "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
        "frac": round(gbs / HBM_PEAK_GBS, 4), "traffic": traffic,
        "traffic_algorithmic": round(pf["bytes"] / max(pf["launches"], 1)),
        "traffic_source": tsrc, "kernel": kname,
        "avg_launch_ms": round(pf["ms"] / max(pf["launches"], 1), 4),
        "pyramid_ms_per_step": round(pf["ms"] / a.steps, 4),
        "note": "algorithmic bytes B_pyr = 24 B x sum of octave pixels (1 read + 5 plane writes, "
                "SURVEY.md 8(d)) over the per-octave launches of one step, / their summed "
                "HIP-event time; north_star target frac >= 0.6"}
    return fm, roof


def match_block(a, world, match):
    pairs = match["n_query"] * match["n_train"]
    lane_ops = match["flops"] / (match["ms"] * 1e-3) / 1e12 if match["ms"] else 0.0
    m = {
        "metric": "knnMatch(k=2) L1 distance pairs/s, image 1 vs image 0 of the batch",
        "value": round(pairs / (match["ms"] * 1e-3) / 1e9, 3) if match["ms"] else None,
        "unit": "Gpairs/s", "ms": round(match["ms"], 4),
        "n_query": match["n_query"], "n_train": match["n_train"],
        "roofline": {"bound": "valu", "achieved": round(lane_ops, 2), "peak": VALU_OP_PEAK_T,
                     "unit": "Tlane-op/s", "frac": round(lane_ops / VALU_OP_PEAK_T, 4),
                     "kernel": "knn_l1_kernel",
                     "note": "2 VALU lane-ops (v_sub, v_add |x|) per descriptor element per pair; "
                             "peak = 256 CU x 4 SIMD x 32 lanes x 2.4 GHz"},
        "note": "SURVEY 8(f) f2 (src/main.cpp:25-27); bit-exact vs oracle/match.py"}
    if not a.no_cpu_baseline:
        m["cpu_baseline"] = match_cpu_baseline(match)
    return m


def assemble(a, world, env_shape, res, cpu, errors):
    """The one JSON line.  Every optional block is built under its own guard:
    a failure there becomes {"error": ...} and the headline fields stay."""
    B, R, C, S = env_shape
    tr = load_traffic()
    out = {"metric": METRIC}
    if res.get("exact") is not None:
        out.update(exact_block(a, world, B, R, C, S, res["exact"], tr))
    if res.get("fast") is not None:
        fb = guarded(errors, "fast_block", fast_block, a, world, B, R, C, res["fast"], tr)
        if fb is not None:
            out["fast_mode"], out["roofline_pyramid_fast"] = fb
    if res.get("match") is not None:
        mb = guarded(errors, "match_block", match_block, a, world, res["match"])
        if mb is not None:
            out["match"] = mb
    if res.get("single") is not None:
        out["single_image"] = res["single"]
    if res.get("eightk") is not None:
        out["image_8k"] = res["eightk"]
    if res.get("multi") is not None:
        out["c_abi_multi"] = res["multi"]
    if cpu:
        out.update(cpu)
        cb = cpu.get("cpu_baseline")
        if cb and "value" in out:
            out["speedup_vs_cpu_1thread"] = {"Mpix/s": round(out["value"] / cb["value"], 1),
                                             "keypoints/s": round(out["keypoints_per_s"] / cb["keypoints_per_s"], 1)}
        if cb and res.get("single") is not None:
            res["single"]["speedup_vs_cpu_1thread_keypoints_per_s"] = round(
                res["single"]["keypoints_per_s"] / cb["keypoints_per_s"], 1)
    for name in errors:
        block = {"fast": "fast_mode", "fast_block": "fast_mode", "match": "match", "match_block": "match",
                 "single": "single_image", "eightk": "image_8k", "multi": "c_abi_multi"}.get(name)
        if block and block not in out:
            out[block] = {"error": errors[name]}
    if errors:
        out["leg_errors"] = dict(errors)
    return out


def free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


CPU_JSON_ENV = "SIFT_BENCH_CPU_JSON"


def wants_cpu_legs(a) -> bool:
    return a.full and not a.no_cpu_baseline and a.only is None


def save_cpu_legs(cpu, errors, path):
    with open(path, "w") as f:
        json.dump({"cpu": cpu, "errors": errors}, f)


def load_cpu_legs(path, errors):
    """Rank 0 of an N > 1 run: the CPU legs its launching parent measured
    (launch_ranks) -- merged into the line exactly as at N = 1."""
    with open(path) as f:
        d = json.load(f)
    errors.update(d.get("errors") or {})
    return d.get("cpu") or None


def launch_ranks(a, argv=None) -> int:
    """`--gpus N > 1` without a launcher: run N ranks of this script under
    torch.distributed.run as a CHILD process (never an exec: nothing here has
    touched the GPU, and the child's ranks initialise their own devices), one
    rank per GPU, rendezvous on 127.0.0.1.  The CPU baselines (SURVEY 8(d) d4:
    the reference path on the node's own cores, in the same run at every GPU
    count) are measured here first, while no process of the run holds a GPU,
    and reach rank 0 as a JSON file named by SIFT_BENCH_CPU_JSON.  Rank 0's
    line reaches our stdout through the inherited descriptor; returns the
    child's exit code."""
    argv = sys.argv[1:] if argv is None else argv
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    tmp = None
    if wants_cpu_legs(a):
        import tempfile
        errors = {}
        cpu = cpu_legs(a, errors)
        fd, tmp = tempfile.mkstemp(prefix="sift_bench_cpu_", suffix=".json")
        os.close(fd)
        save_cpu_legs(cpu, errors, tmp)
        env[CPU_JSON_ENV] = tmp
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr=127.0.0.1", f"--master-port={free_port()}", os.path.abspath(__file__)] + list(argv)
    print(f"bench.py: launching {a.gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    try:
        return subprocess.run(cmd, env=env).returncode
    finally:
        if tmp is not None:
            try:
                os.unlink(tmp)
            except OSError:
                pass


def rehearsal():
    """SIFT_BENCH_SHARE_GPU=1 (rehearsal only, never a reported run): N ranks
    may share the visible devices (rank r on device r % count) and talk over
    SIFT_BENCH_DIST_BACKEND (gloo: the gather stages through host memory), so
    the N > 1 orchestration -- launcher, barriers, max-over-ranks timing, the
    keypoint gather and rank 0's line -- runs on a one-GPU box, where RCCL
    refuses two ranks on one device."""
    return os.environ.get("SIFT_BENCH_SHARE_GPU", "0") == "1"


def dist_backend():
    return os.environ.get("SIFT_BENCH_DIST_BACKEND", "nccl") if rehearsal() else "nccl"


def check_world(a):
    """The rank count the launcher gave us must be the one --gpus asks for,
    and the node must have that many devices (device_count does not
    initialise the GPU on this image).  Returns an error message or None."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" in os.environ and world != a.gpus:
        return f"WORLD_SIZE={world} but --gpus {a.gpus}: launch one rank per requested GPU"
    if a.gpus > 1 and not rehearsal():
        n = torch.cuda.device_count()
        if a.gpus > n:
            return f"--gpus {a.gpus} but only {n} HIP device(s) visible"
    return None


def main():
    a = parse()
    if a.gpus < 1:
        sys.exit("bench.py: --gpus must be >= 1")
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        n = torch.cuda.device_count()
        if a.gpus > n and not rehearsal():
            sys.exit(f"bench.py: --gpus {a.gpus} but only {n} HIP device(s) visible")
        sys.exit(launch_ranks(a))
    GPU_ERROR_LEGS.clear()
    msg = check_world(a)
    if msg:
        sys.exit(f"bench.py: {msg}")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    errors = {}
    cpu = None
    if rank == 0 and wants_cpu_legs(a):
        if world > 1 and os.environ.get(CPU_JSON_ENV):
            # measured by launch_ranks before any rank started
            cpu = guarded(errors, "cpu_legs", load_cpu_legs, os.environ[CPU_JSON_ENV], errors)
        else:
            # N = 1, or ranks started by an outside launcher: rank 0 measures
            # them before this process touches the GPU (the image-parallel leg
            # starts child processes); the other ranks wait at the rendezvous
            cpu = cpu_legs(a, errors)
    if world > 1:
        dev = local % torch.cuda.device_count() if rehearsal() else local
        torch.cuda.set_device(dev)
        if dist_backend() == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev))
        else:
            dist.init_process_group(dist_backend())
    else:
        torch.cuda.set_device(0)
    env = Env(a, world, rank)
    res = {}
    if a.only in (None, "exact"):
        res["exact"] = run_exact(env)   # the headline: not guarded
    # every further leg is a run of its own: --full (or --only LEG) asks for it
    want = (lambda leg_name: a.full and a.only in (None, leg_name))
    # the fast leg only at N = 1: with collectives inside, a failure caught on
    # one rank would leave the others waiting in that collective;
    # the multi-GPU line is the exact path's
    if not a.no_fast and want("fast") and world == 1:
        res["fast"] = guarded(errors, "fast", run_fast, env)
    if not (a.no_match or rank != 0 or env.B < 2 or res.get("exact") is None or not a.full):
        res["match"] = guarded(errors, "match", run_match, env)
    if rank == 0 and world == 1 and not a.no_single and want("single"):
        res["single"] = guarded(errors, "single", single_image_leg, env.R, env.C, a.steps, a.warmup)
    if rank == 0 and world == 1 and not a.no_8k and want("8k"):
        res["eightk"] = guarded(errors, "eightk", eightk_leg, a.steps, a.warmup)
    if rank == 0 and world == 1 and not a.no_multi and want("multi"):
        res["multi"] = guarded(errors, "multi", c_abi_multi_leg, env, a.steps, a.warmup)
    verified_ok = True
    if rank == 0:
        out = assemble(a, world, (env.B, env.R, env.C, env.S), res, cpu, errors)
        out["distributed"] = {"world_size": world, "backend": dist.get_backend() if world > 1 else None,
                              "launcher": "torch.distributed.run" if "WORLD_SIZE" in os.environ else "none"}
        if rehearsal():
            out["distributed"]["rehearsal"] = ("SIFT_BENCH_SHARE_GPU=1: ranks share devices; not a "
                                               "multi-GPU measurement")
        if a.profile_json and res.get("exact") is not None and res["exact"]["prof"] is not None:
            with open(a.profile_json, "w") as f:
                json.dump(res["exact"]["prof"][1], f, indent=1)
        print(json.dumps(out), flush=True)
        verified_ok = output_check_passed(a, out, res)
    env.close()
    if world > 1:
        dist.destroy_process_group()
    # a GPU error caught in an optional leg leaves the line printed but the
    # run marked failed: the context that raised it is not trusted further
    if GPU_ERROR_LEGS:
        sys.exit(3)
    if not verified_ok:
        print("bench.py: output check failed (output_verified false or a seed differs from the CPU path's "
              "digests)", file=sys.stderr, flush=True)
        sys.exit(4)


def output_check_passed(a, out, res) -> bool:
    """The headline's output check (--full) must pass for the run to pass: at the
    golden shape every checked seed must equal the CPU path's digest (count,
    keypoint bytes, descriptor bytes) and none may fail.  Shapes without
    digests (--rows/--cols/--octaves changed) are not checked."""
    if res.get("exact") is None or res["exact"]["verified"] is None:   # no headline, or no --full
        return True
    if a.octaves != 5 or (a.rows, a.cols) != (1080, 1920):
        return True
    return bool(out.get("output_verified")) and not out.get("output_failed_seeds")


if __name__ == "__main__":
    main()
