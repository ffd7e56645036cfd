"""Multi-hit queries (hrt_trace_hits) timed alone: on the scenes of configs 2-5, three seeded sets of 1920x1080 rays each (those of
tools/query_bench.py), k in {1, 4, 16} with totals off and on, and CLOSEST and OCCLUDED on the same rays in the same process, the
calls alternating rep by rep.  One process on GPU 0; prints one JSON line and writes it to --out.
   python tools/hits_bench.py [--configs 2,3,4,5] [--reps 5] [--warmup 1] [--out profiles/hits_bench.json]
Ray sets (seeded):
   primary  pixel-centre camera rays of every pixel, tMax = +inf
   diffuse  cosine-distributed directions from primary hit points (normal offset as the path tracer's, RTRay.cs:552-558), tMax = +inf
   shadow   from the same hit points toward the sun, tMax = 1e29 (the path tracer's sun shadow rays)
Times are the library's HIP-event times of the device work (copies excluded)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ilgpu_raytracing_amd import _types as T, scenes, engine

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="2,3,4,5")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default="profiles/hits_bench.json")
args = ap.parse_args()
W, H = 1920, 1080
f32 = np.float32


def camera_rays(p):
    """Frame.primary_ray (RTRay.cs:120-126, Ray.GenerateRay RTUtils.cs:13-17) of every pixel, float32, the kernel's operation order."""
    cam = p.cam
    v3 = lambda a: np.array([a.X, a.Y, a.Z], np.float32)
    idx = np.arange(p.width * p.height)
    x, y = (idx % p.width).astype(np.float32), (idx // p.width).astype(np.float32)
    u = (x + f32(0.5)) / f32(p.width)
    v = (y + f32(0.5)) / f32(p.height)
    ll, hz, vt, org = v3(cam.lowerLeft), v3(cam.horizontal), v3(cam.vertical), v3(cam.origin)
    d = ((ll[None, :] + hz[None, :] * u[:, None]) + vt[None, :] * v[:, None]) - org[None, :]
    s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    d = d * (f32(1.0) / np.sqrt(np.maximum(f32(1e-20), s)))[:, None]
    return np.broadcast_to(org, d.shape).astype(np.float32), d.astype(np.float32)


def cosine_dirs(n, rng):
    """Cosine-distributed directions about the normals n (Malley: uniform disc lifted to the hemisphere)."""
    r1, r2 = rng.random(len(n)), rng.random(len(n))
    phi, rr = 2.0 * np.pi * r1, np.sqrt(r2)
    lx, ly, lz = rr * np.cos(phi), rr * np.sin(phi), np.sqrt(np.maximum(0.0, 1.0 - r2))
    a = np.where(np.abs(n[:, 0:1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    t = np.cross(n, a)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(n, t)
    return (t * lx[:, None] + b * ly[:, None] + n * lz[:, None]).astype(np.float32)


def stats(ms, n):
    ms = np.asarray(ms, np.float64)
    mr = n / (ms * 1e3)
    return {"mrays_s_median": round(float(np.median(mr)), 1), "mrays_s_min": round(float(mr.min()), 1), "mrays_s_max": round(float(mr.max()), 1),
            "ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(ms.min()), 4), "ms_max": round(float(ms.max()), 4), "calls": len(ms)}


KS = (1, 4, 16)


def timed_all(r, o, d, tmax):
    """Every variant once per rep, in turn: drift of the clock or the machine spreads over all of them alike."""
    calls = [("closest", lambda: r.trace_rays(o, d, query="closest")), ("occluded", lambda: r.trace_rays(o, d, tmax, query="occluded"))]
    for k in KS:
        for tot in (False, True):
            calls.append(("k%d%s" % (k, "_totals" if tot else ""), lambda k=k, tot=tot: r.trace_hits(o, d, k, tmax, totals=tot)))
    for _ in range(args.warmup):
        for _, f in calls:
            f()
    ms = {name: [] for name, _ in calls}
    for _ in range(args.reps):
        for name, f in calls:
            f()
            ms[name].append(r.last_query_ms)
    return {name: stats(v, len(o)) for name, v in ms.items()}


r = engine.RTRenderer([0])
out = {"tool": "tools/hits_bench.py", "rays_per_set": W * H, "reps": args.reps, "warmup": args.warmup, "device": "GPU 0", "cases": []}
for cid in [int(c) for c in args.configs.split(",")]:
    s = engine.Scene()
    cfg = scenes.build(cid, s)
    r.commit(s)
    p = scenes.frame_params(cfg, engine.camera_look_at, engine.bake_camera_derived, engine.sun_direction, width=W, height=H, spp=1)
    o, d = camera_rays(p)
    hits = r.trace_rays(o, d)
    hit = hits["t"] < f32(1e29)
    nrm = np.stack([hits["normal"][a] for a in "XYZ"], 1).astype(np.float32)
    pos = (o + d * hits["t"][:, None]).astype(np.float32)
    rng = np.random.default_rng(1000 + cid)
    k = rng.choice(np.flatnonzero(hit), W * H, replace=True)
    hp, hn = pos[k], nrm[k]
    dd = cosine_dirs(hn.astype(np.float64), rng)
    sgn = np.where((hn * dd).sum(1) >= 0, f32(1.0), f32(-1.0))[:, None]
    do = (hp + hn * (f32(0.0025) * sgn)).astype(np.float32)
    sun = np.array([p.dirLightDir.X, p.dirLightDir.Y, p.dirLightDir.Z], np.float32)
    sun = (sun / np.sqrt((sun * sun).sum())).astype(np.float32)
    sd = np.broadcast_to(sun, hp.shape).astype(np.float32)
    so = (hp + hn * (f32(0.0025) * np.where((hn * sd).sum(1) >= 0, f32(1.0), f32(-1.0))[:, None])).astype(np.float32)
    for name, ro, rd, tm in (("primary", o, d, f32(np.inf)), ("diffuse", do, dd, f32(np.inf)), ("shadow", so, sd, f32(1e29))):
        t = timed_all(r, ro, rd, tm)
        _, cnt, tot = r.trace_hits(ro, rd, 1, tm, totals=True)
        case = {"config": cid, "rays": name, "mean_accepted_hits": round(float(tot.mean()), 3), "times": t,
                "k1_over_closest": round(t["k1"]["ms_median"] / t["closest"]["ms_median"], 3),
                "k1_totals_over_occluded": round(t["k1_totals"]["ms_median"] / t["occluded"]["ms_median"], 3)}
        out["cases"].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
r.close()
line = json.dumps(out)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
