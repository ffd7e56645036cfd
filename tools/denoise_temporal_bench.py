"""hrt_denoise_temporal timed alone: device_ms (HIP events around its kernels) at the defaults on config 2, 2 spp, for the internal
sizes of tools/denoise_bench.py (858x482, 1286x724, 1920x1080, 2573x1447), median of --reps with min and max, in the steady state (a
history older than four frames: the variance comes from the moments), once under a static camera, which is the cheapest case (fx =
fy = 0: one of the four history taps has a weight and is fetched), and once under a pan of 1.37 pixels per frame, where every pixel
fetches four taps and a strip at the border restarts each frame; beside
  (a) hrt_denoise on the same frames, and
  (b) a device-to-device copy of the compulsory bytes of the record layout (csrc/hrt_denoise_temporal.hpp).  Per pixel: the temporal
      step reads the frame (56 B) and four history taps, of which one pixel's worth is compulsory (32 B guides + 16 B colour + 16 B
      moments), and writes guides, colour and moments (32 + 16 + 16 B): 56 + 64 + 64 = 184 B; the variance step reads the moments and
      the hit word (16 + 16 B) and writes 4 B: 36 B; an iteration reads 48 B and writes 16 B, iteration 0 writes the history colour as
      well (16 B), the last one reads the albedo (12 B) and writes 12 + 4 B instead of 16: 184 + 36 + 64 iterations + 16 + 12 B = 568 B
      at 5 iterations.  A copy of half as many bytes reads one half and writes the other.
   python tools/denoise_temporal_bench.py [--reps 20] [--warmup 6] [--out profiles/denoise_temporal_bench.json]
--trace: one size, no floor, for a `rocprofv3 --kernel-trace --stats -- python tools/denoise_temporal_bench.py --trace` run."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=6)
ap.add_argument("--out", default="profiles/denoise_temporal_bench.json")
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
if args.reps < 20 and not args.trace:
    sys.exit("--reps must be at least 20: the figure is a median")
if args.warmup < 4:
    sys.exit("--warmup must be at least 4: the steady state starts with a history of four frames")

import torch                                           # before the library: torch's HIP runtime is then the process's
from ilgpu_raytracing_amd import scenes, engine

ITER = 5
SIZES = [(1920, 1080)] if args.trace else [(858, 482), (1286, 724), (1920, 1080), (2573, 1447)]
CFG = scenes.CONFIGS[2]
BYTES_PER_PIXEL = 184 + 36 + 64 * ITER + 16 + 12

torch.cuda.set_device(0)
r = engine.RTRenderer([0])
s = engine.Scene(); scenes.build_config2(s); r.commit(s)


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


DIST = float(np.linalg.norm(np.subtract(CFG.cam_origin, CFG.cam_lookat)))


def frame(w, h, f, pixels=0.0):
    """Frame f; the camera moved sideways by `pixels` pixels at the look-at distance."""
    shift = pixels * 2.0 * DIST * np.tan(np.radians(CFG.vfov) / 2) / h
    o, l = CFG.cam_origin, CFG.cam_lookat
    cfg = scenes.Config("dt", w, h, 2, (o[0] + shift, o[1], o[2]), (l[0] + shift, l[1], l[2]), extra=CFG.extra)
    return r.render_params(scenes.frame_params(cfg, engine.camera_look_at, engine.bake_camera_derived, engine.sun_direction, frame=f))


res = {"scene": "config2", "spp": 2, "iterations": ITER, "reps": args.reps, "warmup": args.warmup, "library": os.path.basename(engine.LIB_PATH),
       "bytes_per_pixel": BYTES_PER_PIXEL, "sizes": {}}
for w, h in SIZES:
    r.reset_history()
    tm, sm, first = [], [], None
    for i in range(args.warmup + args.reps):
        frame(w, h, i)                                 # one temporal call per frame
        r.denoise(slot=0)
        spatial = r.last_query_ms
        r.denoise_temporal(slot=0)
        if i == 0:
            first = r.last_query_ms                    # an empty history: every workgroup runs the 7x7 variance window
        if i >= args.warmup:
            sm.append(spatial); tm.append(r.last_query_ms)
    pm = []
    for i in range(args.warmup + args.reps):          # the same history, now under the pan
        frame(w, h, 1000 + i, pixels=1.37 * (i + 1))
        r.denoise_temporal(slot=0)
        if i >= args.warmup:
            pm.append(r.last_query_ms)
    entry = {"temporal_ms": stats(tm), "temporal_pan_ms": stats(pm), "denoise_ms": stats(sm), "temporal_first_frame_ms": round(first, 4)}
    entry["temporal_over_denoise"] = round(entry["temporal_ms"]["median"] / entry["denoise_ms"]["median"], 2)
    entry["temporal_pan_over_denoise"] = round(entry["temporal_pan_ms"]["median"] / entry["denoise_ms"]["median"], 2)
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
        entry["temporal_over_floor"] = round(entry["temporal_ms"]["median"] / entry["floor_copy_ms"]["median"], 2)
        entry["temporal_pan_over_floor"] = round(entry["temporal_pan_ms"]["median"] / entry["floor_copy_ms"]["median"], 2)
        del src, dst
    res["sizes"]["%dx%d" % (w, h)] = entry
r.close()
line = json.dumps(res)
print(line)
if not args.trace:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
