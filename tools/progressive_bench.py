"""Cost of progressive frames (hrt_render_progressive) against one hrt_render_frame, configs 2-5 at their stated size and spp:
time to the first preview, ms per call and the total of a schedule of cumulative sample counts.  Before anything is printed the
last call's frame is checked to equal the one-shot frame bit for bit (every output array).  Blocking calls, host wall time (the
frames stay on the device), median over --reps runs after one warm-up run; the HIP-event time of the path stage is reported too.
Prints one JSON object (and writes it to --json).
   python tools/progressive_bench.py [--configs 2,3,4,5] [--reps 3] [--json FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ilgpu_raytracing_amd import _types as T, engine, scenes

SCHEDULES = {
    2: [(1, 4), (2, 4)],
    3: [(1, 4, 16), (4, 16)],
    4: [(4, 16, 64), (8, 16, 32, 64), (16, 32, 48, 64)],
    5: [(8, 16, 32, 64, 128, 256), (8, 24, 96, 256), (32, 64, 128, 192, 256)],
}


def with_spp(p, spp):
    q = T.FrameParams.from_buffer_copy(p)
    q.spp = spp
    return q


def same(a, b):
    if a.dtype == np.float32:
        return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def timed(fn):
    t0 = time.perf_counter()
    st = fn()
    return (time.perf_counter() - t0) * 1e3, st


def run_config(r, cid, reps):
    cfg = scenes.CONFIGS[cid]
    s = engine.Scene()
    scenes.build(cid, s)
    r.commit(s)
    w, h, spp = cfg.width, cfg.height, cfg.spp
    p = scenes.frame_params(cfg, engine.camera_look_at, engine.bake_camera_derived, engine.sun_direction, width=w, height=h, spp=spp)
    # bit-exactness first: the last call of every schedule against the one-shot frame, every array
    r.reset_history()
    want, o = T.alloc_outputs(w, h)
    r.render_params(p, o)
    for sched in SCHEDULES[cid]:
        r.reset_history()
        got, og = T.alloc_outputs(w, h)
        begin = 0
        for k in sched:
            r.render_progressive(with_spp(p, k), begin, og if k == sched[-1] else None)
            begin = k
        bad = [n for n in want if not same(want[n], got[n])]
        assert not bad, "config %d schedule %s: the final frame differs from the one-shot frame in %s" % (cid, sched, bad)
    del want, got
    # timing
    one = []
    for i in range(reps + 1):
        ms, st = timed(lambda: r.render_params(p, None))
        if i:
            one.append((ms, st.kernel_ms[0], st.kernel_ms[1]))
    one_ms = float(np.median([x[0] for x in one]))
    out = {"config": cid, "size": "%dx%d" % (w, h), "spp": spp,
           "one_shot_ms": round(one_ms, 2), "one_shot_path_stage_ms": round(float(np.median([x[2] for x in one])), 2),
           "schedules": []}
    for sched in SCHEDULES[cid]:
        runs = []
        for i in range(reps + 1):
            calls, begin = [], 0
            for k in sched:
                ms, st = timed(lambda: r.render_progressive(with_spp(p, k), begin, None))
                calls.append((ms, st.kernel_ms[1]))
                begin = k
            if i:
                runs.append(calls)
        per_call = [float(np.median([run[j][0] for run in runs])) for j in range(len(sched))]
        per_call_dev = [float(np.median([run[j][1] for run in runs])) for j in range(len(sched))]
        total = float(np.median([sum(c[0] for c in run) for run in runs]))
        out["schedules"].append({
            "schedule": list(sched), "first_preview_ms": round(per_call[0], 2),
            "ms_per_call": [round(x, 2) for x in per_call], "path_stage_ms_per_call": [round(x, 2) for x in per_call_dev],
            "total_ms": round(total, 2), "total_over_one_shot": round(total / one_ms, 4),
            "samples_per_call_min": min(b - a for a, b in zip((0,) + tuple(sched), sched)),
            "final_frame_bit_identical": True})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,3,4,5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    r = engine.RTRenderer([0])
    try:
        res = {"what": "progressive frames vs one hrt_render_frame (blocking calls, host wall ms, median of %d runs)" % a.reps,
               "configs": [run_config(r, int(c), a.reps) for c in a.configs.split(",")]}
    finally:
        r.close()
    txt = json.dumps(res)
    if a.json:
        with open(a.json, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(txt)


if __name__ == "__main__":
    main()
