#!/usr/bin/env python3
"""A/B of the join of two match tables on a shared keypoint: the segmented device
call against the flow a caller has without it.

The workload is synthetic: 64 segments of 300 and of 4000 records in each table.
A shared view has 1.25 keypoints per record; 30 % of table A's records name a
keypoint another record names too, 20 % of its mask bytes are zero, and table B
names a keypoint of the shared view per record in query order, as the ratio stage
leaves a table.  One child process (its own timeout) times, alternating, with HIP
events on the context's stream (5 warm-up iterations, medians of 20):

  JOIN        sift_join_matches_segmented_device on the device-resident tables,
              d_xyz and mask: one enqueue, no host value
  JOIN_HOST   the flow a caller has without it: both tables, their offsets, d_xyz,
              the mask and the pixels are copied to the host, the stream is waited
              for, sift_join_matches runs per segment on the CPU, and the joined
              rows and offsets are copied back (copies and wait inside the window)

The device leg's rows, offsets and b_joined must equal the host loop's byte for
byte before anything is timed.  The report also counts the bytes the call and its
emit kernel must move; --kernel-ms FILE copies per-kernel times measured in a run
of their own (rocprofv3 --kernel-trace --stats) into the report.

  python tools/bench_join.py [--kernel-ms FILE] [--out profiles/join_ab.txt]
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
S, TIMEOUT = 64, 420
WORKLOADS = (("300 records", 300), ("4000 records", 4000))


def tables(np, seed, per):
    """(A records, B records, keys per segment) of one workload, MATCH_DTYPE layout as int32 [n, 4]."""
    rng = np.random.default_rng(seed)
    nk = per * 5 // 4
    a, b = np.zeros((S * per, 4), np.int32), np.zeros((S * per, 4), np.int32)
    for s in range(S):
        rows = slice(s * per, (s + 1) * per)
        train = rng.permutation(nk)[:per]
        dup = rng.permutation(per)[:per * 3 // 10]
        train[dup] = train[(dup + 1) % per]                       # one train keypoint from several queries
        a[rows, 0], a[rows, 1] = np.sort(rng.permutation(nk)[:per]), train
        b[rows, 0], b[rows, 1] = np.sort(rng.permutation(nk)[:per]), rng.permutation(nk)[:per]
    a[:, 2] = rng.integers(1, 400, len(a)).astype(np.float32).view(np.int32)
    b[:, 2] = rng.integers(1, 400, len(b)).astype(np.float32).view(np.int32)
    return a, b, nk


def worker(iters, warmup):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "sift-gpu_amd"))
    import siftgpu
    strm = torch.cuda.Stream()
    ctx = siftgpu.Context(64, 64, 1, device=0)
    ctx.set_stream(strm.cuda_stream)
    L = siftgpu.lib()
    out = {}
    vp = ctypes.c_void_p
    with torch.cuda.stream(strm):
        for name, per in WORKLOADS:
            cap = S * per
            a, b, nk = tables(np, 7000 + per, per)
            rng = np.random.default_rng(per)
            dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
            da, db = dev(a), dev(b)
            off = dev(np.arange(S + 1, dtype=np.int32) * per)
            koff = dev(np.arange(S + 1, dtype=np.int32) * nk)
            dxyz, dmask = dev(rng.standard_normal((cap, 3))), dev((rng.random(cap) < 0.8).astype(np.uint8))
            dbxy = dev((rng.random((cap, 2)) * 1000).astype(np.float32))
            z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
            oxyz, oxy, oar, obr = z((cap, 3), torch.float64), z((cap, 2), torch.float32), z((cap,), torch.int32), \
                z((cap,), torch.int32)
            obj, ojo = z((cap,), torch.uint8), z((S + 1,), torch.int32)
            pin = lambda t: torch.empty(t.shape, dtype=t.dtype).pin_memory()  # noqa: E731
            ha, hb, hoff, hkoff, hxyz, hmask, hbxy = (pin(t) for t in (da, db, off, koff, dxyz, dmask, dbxy))
            rxyz, rxy, rar, rbr, rbj, rjo = (pin(t) for t in (oxyz, oxy, oar, obr, obj, ojo))
            bxyz, bxy, bar, bbr, bjo = z((cap, 3), torch.float64), z((cap, 2), torch.float32), z((cap,), torch.int32), \
                z((cap,), torch.int32), z((S + 1,), torch.int32)
            strm.synchronize()

            def device():
                ctx.join_matches_segmented_device(
                    da.data_ptr(), off.data_ptr(), cap, siftgpu.JOIN_TRAIN, dxyz.data_ptr(), db.data_ptr(),
                    off.data_ptr(), cap, siftgpu.JOIN_QUERY, dbxy.data_ptr(), koff.data_ptr(), S * nk, S, cap,
                    ojo.data_ptr(), oxyz.data_ptr(), oxy.data_ptr(), oar.data_ptr(), obr.data_ptr(), obj.data_ptr(),
                    dmask.data_ptr(), None)

            def host():
                for h, d in ((ha, da), (hb, db), (hoff, off), (hkoff, koff), (hxyz, dxyz), (hmask, dmask), (hbxy, dbxy)):
                    h.copy_(d, non_blocking=True)
                strm.synchronize()
                ho, hk = hoff.numpy(), hkoff.numpy()
                jo = rjo.numpy()
                jo[0] = 0
                for s in range(S):
                    lo, n, j = int(ho[s]), int(ho[s + 1] - ho[s]), int(jo[s])
                    m = L.sift_join_matches(
                        vp(ha.data_ptr() + lo * 16), n, siftgpu.JOIN_TRAIN, vp(hmask.data_ptr() + lo),
                        vp(hxyz.data_ptr() + lo * 24), vp(hb.data_ptr() + lo * 16), n, siftgpu.JOIN_QUERY, None,
                        vp(hbxy.data_ptr() + lo * 8), int(hk[s + 1] - hk[s]), vp(rxyz.data_ptr() + j * 24),
                        vp(rxy.data_ptr() + j * 8), vp(rar.data_ptr() + j * 4), vp(rbr.data_ptr() + j * 4),
                        vp(rbj.data_ptr() + lo))
                    rar.numpy()[j:j + m] += lo                   # rows of the whole tables, as the device call gives
                    rbr.numpy()[j:j + m] += lo
                    jo[s + 1] = j + m
                total = int(jo[S])
                for d, h in ((bxyz, rxyz), (bxy, rxy), (bar, rar), (bbr, rbr)):
                    d[:total].copy_(h[:total], non_blocking=True)
                bjo.copy_(rjo, non_blocking=True)

            device()
            host()
            ctx.sync()
            strm.synchronize()
            total = int(rjo.numpy()[S])
            g = lambda t, n=None: t[:n].cpu().numpy().tobytes()  # noqa: E731
            same = bool(g(ojo) == g(rjo) and g(obj) == g(rbj) and
                        all(g(d, total) == g(h, total) for d, h in ((oxyz, rxyz), (oxy, rxy), (oar, rar), (obr, rbr))))
            assert same, f"{name}: the device call and the host loop differ"
            cand = int(dmask.sum().item())
            legs = {"JOIN": device, "JOIN_HOST": host}
            ev, wall = {k: [] for k in legs}, {k: [] for k in legs}
            for it in range(warmup + iters):
                for k, fn in legs.items():
                    strm.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record(strm)
                    fn()
                    e1.record(strm)
                    e1.synchronize()
                    t1 = time.perf_counter()
                    if it >= warmup:
                        ev[k].append(e0.elapsed_time(e1))
                        wall[k].append((t1 - t0) * 1e3)
            out[name] = {"census": {"joined": total, "candidates": cand, "keys": S * nk},
                         "event_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in ev.items()},
                         "wall_ms": {k: [statistics.median(v), min(v), max(v)] for k, v in wall.items()}}
    print("RESULT " + json.dumps({"iters": iters, "warmup": warmup, "workloads": out}), flush=True)
    ctx.close()


def traffic(per, joined, keys):
    """(bytes the whole call must move, bytes the emit kernel must move): records 16 B and a mask
    byte per A row, 16 B per B row in two kernels, the lookup filled (8 B per key), bid for (8 B per
    candidate, not counted: it depends on the data) and read (8 B per B row, twice), the counts, and
    per joined row 24 + 8 B gathered and 24 + 8 + 4 + 4 B written, a b_joined byte per B row."""
    rows = S * per
    emit = rows * (16 + 8 + 1) + joined * (24 + 8 + 24 + 8 + 4 + 4)
    return rows * 17 + keys * 8 + rows * (16 + 8) + emit, emit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join_ab.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-ms", default="", help="a file of per-kernel times from a profiler run of its own")
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
    r = json.loads(line[0][7:])
    parts = ["# The join of two match tables on a shared keypoint: segmented device call (JOIN) vs copy to the host +",
             "# loop of sift_join_matches + copy back (JOIN_HOST)", "# written by tools/bench_join.py", "",
             f"{S} segments; 1.25 keypoints of the shared view per record, 30 % of table A's records on a keypoint "
             "another record names, 20 % of its mask bytes zero",
             "the device leg == the host loop byte for byte (rows, offsets, b_joined): True",
             f"medians of {r['iters']} iterations after {r['warmup']} warm-up [min, max], ms"]
    for name, per in WORKLOADS:
        w = r["workloads"][name]
        c, e = w["census"], w["event_ms"]
        call_b, emit_b = traffic(per, c["joined"], c["keys"])
        parts += ["", f"## {S} x {name} per table: {c['joined']} rows joined of {S * per}, {c['candidates']} unmasked A "
                      f"rows, {c['keys']} keys", f"{'leg':16} {'HIP events':>32} {'host wall':>32}"]
        for k in ("JOIN", "JOIN_HOST"):
            ee, wl = e[k], w["wall_ms"][k]
            parts.append(f"{k:16} {ee[0]:10.3f} [{ee[1]:9.3f}, {ee[2]:9.3f}] {wl[0]:10.3f} [{wl[1]:9.3f}, {wl[2]:9.3f}]")
        parts.append(f"JOIN_HOST / JOIN = {e['JOIN_HOST'][0] / e['JOIN'][0]:.1f} (events); host per segment "
                     f"{e['JOIN_HOST'][0] / S:.3f} ms")
        parts.append(f"bytes the call must move {call_b} ({call_b / e['JOIN'][0] / 1e6:.2f} GB/s over the whole call, "
                     f"seven launches); of them the emit kernel {emit_b}")
    if a.kernel_ms:
        parts += ["", "## per-kernel times, from a profiler run of its own"] + open(a.kernel_ms).read().splitlines()
    else:
        parts += ["", "per-kernel times: not measured in this run"]
    text = "\n".join(parts) + "\n"
    print(text, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
