"""hrt_denoise timed alone: device_ms (HIP events around the denoise kernels) at the defaults on config 2, 2 spp, for the internal sizes
   858x482, 1286x724, 1920x1080, 2573x1447,
median of --reps with min and max, beside the floor it is judged against: a device-to-device copy of the compulsory bytes of the
record layout (csrc/hrt_denoise.hpp), timed with events in the same process.  Per pixel: prepare reads 56 B (radiance, normal,
position, albedo, depth, hit mask) and writes 48 B (guide + colour); an iteration reads 48 B and writes 16 B; the last one also reads
the albedo (12 B) and writes 12 + 4 B instead: 104 + 64 (iterations - 1) + 76 B, of which a copy of half as many bytes reads one
half and writes the other.  For context, at 858x482 -> 1280x720: the frame's own kernels (2 spp, reuse on) and hrt_present mode 1.
   python tools/denoise_bench.py [--reps 20] [--warmup 3] [--out profiles/denoise_bench.json]
HRT_LIB=<variant library> times another kernel shape (make variant NAME=dn_global DEFS=-DHRT_DENOISE_SHAPE=0).
--trace: one size, no floor, for a `rocprofv3 --kernel-trace --stats -- python tools/denoise_bench.py --trace` run; --kernels CSV
prints the per-step times of such a run's kernel trace (the kernels of one denoise are prepare, then one pass per step 1, 2, 4 ...)."""
import argparse
import csv
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="profiles/denoise_bench.json")
ap.add_argument("--trace", action="store_true")
ap.add_argument("--kernels", default=None)
args = ap.parse_args()

ITER = 5


def per_step(path):
    rows = list(csv.DictReader(open(path)))
    rows = [r for r in rows if "hrt_denoise" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = [rows[i:i + 1 + ITER] for i in range(0, len(rows) - ITER, 1 + ITER)]
    calls = [c for c in calls if "prepare" in c[0]["Kernel_Name"]]
    us = np.array([[(int(k["End_Timestamp"]) - int(k["Start_Timestamp"])) / 1000.0 for k in c] for c in calls[2:]])
    med = np.median(us, axis=0)
    return {"calls": len(us), "prepare_us": round(float(med[0]), 2), "step_us": {str(1 << i): round(float(med[1 + i]), 2) for i in range(ITER)}}


if args.kernels:
    print(json.dumps(per_step(args.kernels)))
    sys.exit(0)
if args.reps < 20 and not args.trace:
    sys.exit("--reps must be at least 20: the figure is a median")

import torch                                           # before the library: torch's HIP runtime is then the process's
from ilgpu_raytracing_amd import _types as T, scenes, engine

SIZES = [(1920, 1080)] if args.trace else [(858, 482), (1286, 724), (1920, 1080), (2573, 1447)]
CFG = scenes.CONFIGS[2]
BYTES_PER_PIXEL = 104 + 64 * (ITER - 1) + 76

torch.cuda.set_device(0)
r = engine.RTRenderer([0])
s = engine.Scene(); scenes.build_config2(s); r.commit(s)


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def frame(w, h, f, reuse=False):
    cfg = scenes.Config("dn", w, h, 2, CFG.cam_origin, CFG.cam_lookat, extra=CFG.extra)
    return r.render_params(scenes.frame_params(cfg, engine.camera_look_at, engine.bake_camera_derived, engine.sun_direction, frame=f, reuse=reuse))


res = {"scene": "config2", "spp": 2, "iterations": ITER, "reps": args.reps, "warmup": args.warmup, "library": os.path.basename(engine.LIB_PATH),
       "bytes_per_pixel": BYTES_PER_PIXEL, "sizes": {}}
for w, h in SIZES:
    frame(w, h, 0)
    ms = []
    for i in range(args.warmup + args.reps):
        r.denoise(slot=0)
        if i >= args.warmup:
            ms.append(r.last_query_ms)
    entry = {"denoise_ms": stats(ms)}
    if not args.trace:
        n = w * h * BYTES_PER_PIXEL // 2
        src, dst = torch.zeros(n, dtype=torch.uint8, device="cuda:0"), torch.empty(n, dtype=torch.uint8, device="cuda:0")
        fl = []
        for i in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
            if i >= args.warmup:
                fl.append(e0.elapsed_time(e1))
        entry["floor_copy_ms"] = stats(fl)
        entry["denoise_over_floor"] = round(entry["denoise_ms"]["median"] / entry["floor_copy_ms"]["median"], 2)
        del src, dst
    res["sizes"]["%dx%d" % (w, h)] = entry
if not args.trace:
    w, h, ow, oh = 858, 482, 1280, 720
    k, pm = [], []
    for f in range(args.warmup + args.reps):
        st = frame(w, h, f, reuse=True)
        r.present(ow, oh, taau=True)
        if f >= args.warmup:
            k.append(st.kernel_ms[0] + st.kernel_ms[1]); pm.append(r.present_ms())
    res["context_858x482_to_1280x720"] = {"frame_kernels_ms": stats(k), "present_mode1_ms": stats(pm)}
r.close()
line = json.dumps(res)
print(line)
if not args.trace:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
