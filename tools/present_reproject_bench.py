"""The TAAU resolve timed alone: HIP-event time of the kernel of hrt_present (hrt_present_time), mode 1 (HRT_PRESENT_TAAU) and mode 2
(HRT_PRESENT_TAAU_REPROJECT) alternating frame by frame in one process on one history, on the textured test scene with a camera that
moves about three display pixels per frame (so the history taps of mode 2 really scatter), at
   858x482 -> 1280x720,  1286x724 -> 1920x1080,  2573x1447 -> 3840x2160.
The yardstick of mode 2 is mode 1 in the same run, never a stored number.  One process on GPU 0; prints one JSON line and writes it
to --out.
   python tools/present_reproject_bench.py [--reps 20] [--warmup 4] [--out profiles/present_bench.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ilgpu_raytracing_amd import _types as T, scenes, engine

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--out", default="profiles/present_reproject_bench.json")
args = ap.parse_args()
if args.reps < 20:
    sys.exit("--reps must be at least 20: the figure is a median")

SIZES = [((858, 482), (1280, 720)), ((1286, 724), (1920, 1080)), ((2573, 1447), (3840, 2160))]
ORIGIN, LOOKAT, VFOV = (0.3, 1.3, 4.2), (0.0, 0.7, 0.0), 60.0

r = engine.RTRenderer([0])
s = engine.Scene(); scenes.build_textured_test_scene(s); r.commit(s)
res = {"scene": "textured_test_scene", "reps": args.reps, "warmup": args.warmup, "sizes": {}}
for (iw, ih), (ow, oh) in SIZES:
    dist = float(np.linalg.norm(np.subtract(ORIGIN, LOOKAT)))
    step = 3.0 * 2.0 * dist * np.tan(np.radians(VFOV) / 2) * (ow / oh) / ow          # three display pixels at the look-at distance
    r.reset_history()
    ms = {1: [], 2: []}
    for f in range(2 * (args.warmup + args.reps)):
        cfg = scenes.Config("pan", iw, ih, 1, (ORIGIN[0] + step * f, ORIGIN[1] + 0.4 * step * f, ORIGIN[2]), (LOOKAT[0] + step * f, LOOKAT[1] + 0.4 * step * f, LOOKAT[2]))
        r.render_params(scenes.frame_params(cfg, engine.camera_look_at, engine.bake_camera_derived, engine.sun_direction, frame=f))
        mode = 1 + (f & 1)
        out = r.present(ow, oh, taau=True, reproject=(mode == 2))
        if f >= 2 * args.warmup:
            ms[mode].append(r.present_ms())
    mv = r.motion_vectors(from_cam=None)            # prevCam == cam here: only that the call works at this size
    m1, m2 = float(np.median(ms[1])), float(np.median(ms[2]))
    res["sizes"]["%dx%d->%dx%d" % (iw, ih, ow, oh)] = {
        "mode1_ms_median": round(m1, 4), "mode1_ms_min": round(float(np.min(ms[1])), 4), "mode1_ms_max": round(float(np.max(ms[1])), 4),
        "mode2_ms_median": round(m2, 4), "mode2_ms_min": round(float(np.min(ms[2])), 4), "mode2_ms_max": round(float(np.max(ms[2])), 4),
        "mode2_over_mode1": round(m2 / m1, 3), "calls_per_mode": len(ms[1]), "motion_vectors_ms": round(r.last_query_ms, 4)}
r.close()
line = json.dumps(res)
print(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(line + "\n")
