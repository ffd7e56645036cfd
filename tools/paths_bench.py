"""Radiance queries (hrt_trace_paths) against frames (hrt_render_frame) on configs 2-5 at their stated size and spp.

Per config: the frame's own camera rays through trace_paths against the same frame through render_params (checked bit-equal in
radiance, color, depth and objectId before timing) and against the same frame forced into the fused organisation
(HRT_FLAG_MEGAKERNEL, the organisation every query runs), and for configs 3 and 4 a 2048x1024 equirectangular probe from the camera's
look-at point (checked: a call equals itself and a slice of it equals a call on the slice).  Times are medians over --steps calls
after --warmup: HIP-event device time (frame: its two launches; query: primary + path stage, copies excluded) and wall time
(query: host path, with the ray upload and result download).

    python tools/paths_bench.py --steps 5 --warmup 1 --out profiles/paths_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ilgpu_raytracing_amd import _types as T, engine, scenes          # noqa: E402


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(ref, res):
    rad = np.stack([res["radiance"][a] for a in ("X", "Y", "Z")], 1).astype(np.float32)
    return (np.array_equal(_bits(ref["radiance"]), _bits(rad)) and np.array_equal(ref["color"], res["color"])
            and np.array_equal(_bits(ref["depth"]), _bits(res["depth"].astype(np.float32))) and np.array_equal(ref["objectId"], res["objId"]))


def _probe(centre, w, h):
    j = np.arange(w * h)
    phi = ((j % w) + 0.5) / w * 2 * np.pi
    th = ((j // w) + 0.5) / h * np.pi
    d = np.stack([np.sin(th) * np.cos(phi), np.cos(th), np.sin(th) * np.sin(phi)], 1).astype(np.float32)
    return np.broadcast_to(np.asarray(centre, np.float32), d.shape).copy(), d


def _median_times(fn, steps, warmup):
    dev, wall = [], []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        ms = fn()
        t1 = time.perf_counter()
        if i >= warmup:
            dev.append(ms)
            wall.append((t1 - t0) * 1e3)
    return statistics.median(dev), statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,3,4,5")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="profiles/paths_bench.json")
    a = ap.parse_args()
    r = engine.RTRenderer([0])
    out = {"tool": "tools/paths_bench.py", "steps": a.steps, "warmup": a.warmup, "configs": {}}
    try:
        for cid in [int(c) for c in a.configs.split(",")]:
            cfg = scenes.CONFIGS[cid]
            s = engine.Scene()
            scenes.build(cid, s)
            r.commit(s)
            r.reset_history()
            p = scenes.frame_params(cfg, engine.camera_look_at, engine.bake_camera_derived, engine.sun_direction, reuse=False)
            W, H_ = p.width, p.height
            o, d = r.camera_rays(p)
            ref, outs = T.alloc_outputs(W, H_, names=("color", "depth", "objectId", "radiance"))
            r.render_params(p, outs)
            res = r.trace_paths(o, d, p)
            assert _same(ref, res), "config %d: camera rays differ from the frame" % cid

            mega, outm = T.alloc_outputs(W, H_, names=("color", "depth", "objectId", "radiance"))
            r.render_params(p, outm, flags=T.FLAG_MEGAKERNEL)
            assert all(np.array_equal(_bits(ref[k]), _bits(mega[k])) for k in ref), "config %d: MEGAKERNEL frame differs" % cid

            def frame(flags=0):
                st = r.render_params(p, flags=flags)
                return st.kernel_ms[0] + st.kernel_ms[1]

            def query():
                r.trace_paths(o, d, p)
                return r.last_query_ms

            f_dev, f_wall = _median_times(frame, a.steps, a.warmup)
            m_dev, _ = _median_times(lambda: frame(T.FLAG_MEGAKERNEL), a.steps, a.warmup)       # the control: the frame in the fused organisation
            q_dev, q_wall = _median_times(query, a.steps, a.warmup)
            e = {"size": [W, H_], "spp": p.spp, "maxDepth": p.maxDepth, "equal": True,
                 "frame_device_ms": round(f_dev, 3), "frame_wall_ms": round(f_wall, 3),
                 "camera_paths_device_ms": round(q_dev, 3), "camera_paths_wall_ms": round(q_wall, 3),
                 "ratio_device": round(q_dev / f_dev, 3),
                 "frame_megakernel_device_ms": round(m_dev, 3), "ratio_to_megakernel_frame": round(q_dev / m_dev, 3)}
            if cid in (3, 4):
                po, pd = _probe(cfg.cam_lookat, 2048, 1024)
                pp = T.FrameParams.from_buffer_copy(p)
                pp.width, pp.height = 2048, 1024
                a1 = r.trace_paths(po, pd, pp)
                a2 = r.trace_paths(po, pd, pp)
                k0, k1 = 700000, 760000
                sl = r.trace_paths(po[k0:k1], pd[k0:k1], pp, first_key=k0)
                assert a1.tobytes() == a2.tobytes() and a1[k0:k1].tobytes() == sl.tobytes(), "probe not reproducible"

                def probe():
                    r.trace_paths(po, pd, pp)
                    return r.last_query_ms

                p_dev, p_wall = _median_times(probe, a.steps, a.warmup)
                e["probe_2048x1024"] = {"device_ms": round(p_dev, 3), "wall_ms": round(p_wall, 3), "spp": pp.spp, "from": list(cfg.cam_lookat)}
            out["configs"][str(cid)] = e
            print(json.dumps({str(cid): e}), flush=True)
    finally:
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
