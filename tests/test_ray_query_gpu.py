"""Ray queries on the uploaded scene (hrt_trace_rays): TraceClosest / ShadowOcclusion over caller rays, bit for bit against the
oracle (oracle.orc.trace_rays) and the independent restatement (oracle.orc_indep.Views), on the packed walkers and on TracerRef."""
import ctypes as C

import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, engine, scenes
from oracle import orc_indep as OI
from tests import helpers as H

pytestmark = pytest.mark.gpu
f32 = np.float32
NAN, INF = np.float32(np.nan), np.float32(np.inf)


# ------------------------------------------------------------------ scenes and rays
def _oracle_scene(orc, builder, **kw):
    so = orc.OrcScene()
    builder(so, **kw) if kw else builder(so)
    return so.arrays()


def _commit(renderer, arrs):
    desc, keep = T.scene_desc_from_arrays(arrs)
    renderer.commit(desc)
    return desc, keep


def _params(cfg, w, h):
    return scenes.frame_params(cfg, *H.host_funcs("hrt"), width=w, height=h, spp=1)


def _camera_rays(p, idx):
    """Frame.primary_ray (RTRay.cs:120-126, RTUtils.cs:13-17) over pixel indices, vectorised in float32 with the same operation order."""
    cam = p.cam
    v3 = lambda a: np.array([a.X, a.Y, a.Z], np.float32)
    x, y = (idx % p.width).astype(np.float32), (idx // p.width).astype(np.float32)
    u = (x + f32(0.5)) / f32(max(1, p.width))
    v = (y + f32(0.5)) / f32(max(1, p.height))
    ll, hz, vt, org = v3(cam.lowerLeft), v3(cam.horizontal), v3(cam.vertical), v3(cam.origin)
    d = ((ll[None, :] + hz[None, :] * u[:, None]) + vt[None, :] * v[:, None]) - org[None, :]
    s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    inv = f32(1.0) / np.sqrt(np.maximum(f32(1e-20), s))
    d = d * inv[:, None]
    o = np.broadcast_to(org, d.shape).copy()
    return o, d.astype(np.float32)


def _check_camera_rays_match_frame(p, idx):
    K = OI.Frame(p)
    o, d = _camera_rays(p, idx)
    for k, i in enumerate(idx):
        ro, rd, _ = K.primary_ray(int(i))
        assert H.bits_equal(np.array(ro, np.float32), o[k]).all() and H.bits_equal(np.array(rd, np.float32), d[k]).all(), int(i)


def _bounds(arrs):
    r = arrs["tlasNodes"][0]
    lo = np.array([r["boundsMin"][a] for a in "XYZ"], np.float32)
    hi = np.array([r["boundsMax"][a] for a in "XYZ"], np.float32)
    return lo, hi


def _hostile(rng, lo, hi, surf_o, n):
    o = (lo + (hi - lo) * rng.random((n, 3), dtype=np.float32)).astype(np.float32)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    specials = np.array([NAN, INF, -INF, 0.0, -0.0, 1e-40, -1e-42, 1e19, -1e19, 1e-45], np.float32)
    k = np.arange(n)
    # a special value in one component of the origin or the direction, cycling through all of them
    pick = specials[k % len(specials)]
    comp = (k // len(specials)) % 3
    where = (k // (3 * len(specials))) % 2
    o[where == 0, comp[where == 0]] = pick[where == 0]
    d[where == 1, comp[where == 1]] = pick[where == 1]
    d[::17] = 0.0                                            # zero direction
    d[5::23] = -0.0
    d[7::29] *= f32(1e19)                                    # huge magnitudes
    o[11::31] *= f32(1e19)
    d[13::37] = np.array([0.0, -1.0, 0.0], np.float32)       # axis-aligned
    if len(surf_o):
        m = min(len(surf_o), n // 4)
        o[:m] = surf_o[:m]                                   # origins exactly on surfaces (no normal offset)
    return o, d


def _ray_sets(orc, arrs, desc, p, n, seed):
    """camera, random-in-bounds, from earlier hit points, hostile: (name, origins, dirs)."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(p.width * p.height, size=min(n, p.width * p.height), replace=False)
    co, cd = _camera_rays(p, idx)
    lo, hi = _bounds(arrs)
    ro = (lo + (hi - lo) * rng.random((n, 3), dtype=np.float32)).astype(np.float32)
    rd = rng.standard_normal((n, 3)).astype(np.float32) * rng.uniform(0.1, 4.0, (n, 1)).astype(np.float32)    # not normalised
    ref = orc.trace_rays(desc, co, cd)
    hit = ref["hit"] != 0
    po = (co[hit] + cd[hit] * ref["t"][hit][:, None]).astype(np.float32)
    pn = ref["normal"][hit]
    if len(po) == 0:
        po, pn = ro[:1], np.array([[0, 1, 0]], np.float32)
    k = rng.integers(0, len(po), n)
    bo = (po[k] + pn[k] * f32(0.0025)).astype(np.float32)                                   # the kernels' normal offset
    bd = (pn[k] + rng.standard_normal((n, 3)).astype(np.float32)).astype(np.float32)
    ho, hd = _hostile(rng, lo, hi, po, n)
    return [("camera", co, cd), ("random", ro, rd), ("bounce", bo, bd), ("hostile", ho, hd)]


# ------------------------------------------------------------------ checks
def _unpack(h):
    g = lambda f: np.stack([h[f][a] for a in "XYZ"], 1).astype(np.float32)
    return dict(t=h["t"].astype(np.float32), normal=g("normal"), albedo=g("albedo"), objId=h["objId"], shade=h["shade"],
                ior=h["ior"].astype(np.float32), instance=h["instance"], prim=h["prim"])


def _cut_tlas(arrs, inst):
    """The same arrays with the TLAS cut to one leaf that holds only instance `inst` (root box kept: every walk tests it first)."""
    a = dict(arrs)
    nodes = np.array(arrs["tlasNodes"][:1], copy=True)
    nodes[0]["left"] = nodes[0]["right"] = -1
    nodes[0]["first"], nodes[0]["count"], nodes[0]["skipIndex"] = 0, 1, -1
    a["tlasNodes"] = nodes
    a["tlasInstanceIndices"] = np.array([inst], np.int32)
    return a


def _aff(m):
    return tuple(f32(m[k]) for k in ("m00", "m01", "m02", "m03", "m10", "m11", "m12", "m13", "m20", "m21", "m22", "m23"))


def check_closest(orc, arrs, desc, o, d, got, what, max_instance_checks=200):
    ref = orc.trace_rays(desc, o, d)
    g = _unpack(got)
    for k in ("t", "normal", "albedo", "objId", "shade"):
        eq = H.bits_equal(ref[k], g[k])
        eq = eq.all(axis=1) if eq.ndim > 1 else eq
        assert eq.all(), "%s: %s differs from the oracle at %d of %d rays (first %s)" % (what, k, int((~eq).sum()), len(eq), np.flatnonzero(~eq)[:5])
    hit = ref["hit"] != 0
    miss = ~hit
    assert (g["instance"][miss] == -1).all() and (g["prim"][miss] == -1).all() and (g["ior"][miss] == 1.0).all(), what
    assert (g["instance"][hit] >= 0).all() and (g["prim"][hit] >= 0).all(), what
    tri = hit & (g["objId"] >= 0)
    sph = hit & (g["objId"] < 0)
    # prim: the triangle index of a triangle hit (== objId); ior: 1 for triangles, the sphere's (> 0 ? ior : 1) for spheres
    assert (g["prim"][tri] == g["objId"][tri]).all() and (g["ior"][tri] == 1.0).all(), what
    sp = arrs["spheres"]
    if sph.any():
        sior = sp["ior"][g["prim"][sph]].astype(np.float32)
        assert H.bits_equal(np.where(sior > 0, sior, f32(1.0)).astype(np.float32), g["ior"][sph]).all(), what
        assert (g["shade"][sph] == sp["shading"][g["prim"][sph]]).all(), what
    # prim of a sphere hit: the sphere's own intersection in the instance's object space gives the same world t
    inst = arrs["instances"]
    for i in np.flatnonzero(sph)[:max_instance_checks]:
        rec = inst[g["instance"][i]]
        s = sp[g["prim"][i]]
        w = (tuple(map(f32, o[i])), tuple(map(f32, d[i])), OI.inv_dir(tuple(map(f32, d[i]))))
        oray = OI.transform_ray(_aff(rec["worldToObject"]), w)
        ok, t, _ = OI.intersect_sphere(oray, tuple(f32(s["center"][a]) for a in "XYZ"), f32(s["radius"]))
        us = f32(rec["uniformScale"])
        assert ok and H.bits_equal(np.array([t / (us if us > 0 else f32(1.0))], np.float32), g["t"][i:i + 1]).all(), (what, int(i))
    # instance: the oracle on a TLAS that holds only that instance finds the same t
    sel = np.flatnonzero(hit)[:max_instance_checks]
    for inst_id in np.unique(g["instance"][sel]):
        rs = sel[g["instance"][sel] == inst_id]
        cd, keep = T.scene_desc_from_arrays(_cut_tlas(arrs, int(inst_id)))
        one = orc.trace_rays(cd, o[rs], d[rs])
        assert H.bits_equal(one["t"], g["t"][rs]).all(), "%s: instance %d does not give the hit t" % (what, inst_id)


def _math(orc):
    def m(name, x, y=None):
        return orc.math_eval(name, np.array([x], np.float32), None if y is None else np.array([y], np.float32))[0]
    return m


def check_occluded(orc, arrs, o, d, tmax, got, what):
    V = OI.Views(arrs)
    V.math = _math(orc)
    ref = np.array([1 if V.shadow_occlusion((tuple(map(f32, o[i])), tuple(map(f32, d[i])), OI.inv_dir(tuple(map(f32, d[i])))), f32(tmax[i])) else 0
                    for i in range(len(o))], np.int32)
    bad = np.flatnonzero(ref != got)
    assert len(bad) == 0, "%s: occlusion differs at %d of %d rays (first %s)" % (what, len(bad), len(o), bad[:5])


def _tmax_mix(rng, n):
    choices = np.array([1e29, 0.0, -1.0, np.nan, np.inf, -np.inf], np.float32)
    t = choices[rng.integers(0, len(choices), n)]
    fin = rng.random(n) < 0.4
    t[fin] = rng.uniform(0.0, 30.0, fin.sum()).astype(np.float32)
    return t.astype(np.float32)


# ------------------------------------------------------------------ 1. closest vs the oracle
CLOSEST_SCENES = [
    ("default", lambda b: b.build_default_scene(), scenes.Config("d", 0, 0, 0, (0.0, 1.4, 4.5), (0.0, 0.5, 0.0)), 4000),
    ("config1", scenes.build_config1, scenes.CONFIGS[1], 4000),
    ("config2", scenes.build_config2, scenes.CONFIGS[2], 8000),
    ("config3", scenes.build_config3, scenes.CONFIGS[3], 20000),
    ("textured", scenes.build_textured_test_scene, scenes.Config("t", 0, 0, 0, (0.0, 1.2, 4.0), (0.0, 0.6, 0.0)), 8000),
    ("rotated", scenes.build_rotated_instances_scene, scenes.Config("r", 0, 0, 0, (0.0, 1.5, 5.0), (0.0, 0.8, 0.0)), 8000),
    ("config4", scenes.build_config4, scenes.CONFIGS[4], 30000),
    ("config5", scenes.build_config5, scenes.CONFIGS[5], 30000),
]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name,builder,cfg,n", CLOSEST_SCENES, ids=[s[0] for s in CLOSEST_SCENES])
def test_closest_matches_oracle(orc, renderer, name, builder, cfg, n):
    arrs = _oracle_scene(orc, builder)
    desc, keep = _commit(renderer, arrs)
    p = _params(cfg, 320, 180)
    _check_camera_rays_match_frame(p, np.arange(0, p.width * p.height, 997))
    for what, o, d in _ray_sets(orc, arrs, desc, p, n, seed=len(name)):
        got = renderer.trace_rays(o, d)
        check_closest(orc, arrs, desc, o, d, got, "%s/%s" % (name, what))


# ------------------------------------------------------------------ 2. occluded vs the independent restatement
OCCL_SCENES = [
    ("default", lambda b: b.build_default_scene(), scenes.Config("d", 0, 0, 0, (0.0, 1.4, 4.5), (0.0, 0.5, 0.0))),
    ("config1", scenes.build_config1, scenes.CONFIGS[1]),
    ("config2", scenes.build_config2, scenes.CONFIGS[2]),
    ("textured", scenes.build_textured_test_scene, scenes.Config("t", 0, 0, 0, (0.0, 1.2, 4.0), (0.0, 0.6, 0.0))),
    ("rotated", scenes.build_rotated_instances_scene, scenes.Config("r", 0, 0, 0, (0.0, 1.5, 5.0), (0.0, 0.8, 0.0))),
    ("config4_small", lambda b: scenes.build_config4(b, nu=48, nv=48), scenes.CONFIGS[4]),
    ("config5_small", lambda b: scenes.build_config5(b, n=96), scenes.CONFIGS[5]),
]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name,builder,cfg", OCCL_SCENES, ids=[s[0] for s in OCCL_SCENES])
def test_occluded_matches_restatement(orc, renderer, name, builder, cfg):
    arrs = _oracle_scene(orc, builder)
    desc, keep = _commit(renderer, arrs)
    p = _params(cfg, 160, 90)
    rng = np.random.default_rng(7)
    for what, o, d in _ray_sets(orc, arrs, desc, p, 1000, seed=3):
        tm = _tmax_mix(rng, len(o))
        got = renderer.trace_rays(o, d, tm, query="occluded")
        assert got.dtype == np.int32 and set(np.unique(got)) <= {0, 1}
        check_occluded(orc, arrs, o, d, tm, got, "%s/%s" % (name, what))


# ------------------------------------------------------------------ 3. scenes the packed layout refuses: TracerRef
def _big_leaf_scene(orc, leaf_size):
    """tests/test_hostile_gpu.py::test_one_big_tlas_leaf's scene: one TLAS leaf of leaf_size instances."""
    so = orc.OrcScene()
    rng = scenes.XorShift32(4242)
    ids = [so.add_sphere(scenes.sphere((0.0, -1000.0, 0.0), 1000.0, (0.6, 0.6, 0.6)))]
    for i in range(leaf_size):
        ids.append(so.add_sphere(scenes.sphere((rng.uniform(-3, 3), rng.uniform(0.2, 1.6), rng.uniform(-3, 3)), rng.uniform(0.2, 0.5),
                                               (rng.uniform(0.2, 0.9), rng.uniform(0.2, 0.9), rng.uniform(0.2, 0.9)),
                                               [T.SHADING_LAMBERT, T.SHADING_MIRROR, T.SHADING_GLASS][i % 3], 1.5 if i % 2 else 0.0)))
    for i in ids:
        so.build_sphere_instance([i])
    so.rebuild_tlas()
    arrs = so.arrays()
    inst = arrs["instances"]
    n = len(inst)
    nodes = np.zeros(3, dtype=arrs["tlasNodes"].dtype)

    def put(k, ids, **kw):
        for a in "XYZ":
            nodes[k]["boundsMin"][a] = min(float(inst[i]["worldBoundsMin"][a]) for i in ids)
            nodes[k]["boundsMax"][a] = max(float(inst[i]["worldBoundsMax"][a]) for i in ids)
        for f, v in kw.items():
            nodes[k][f] = v
    put(0, range(n), left=1, right=2, first=-1, count=0, skipIndex=-1)
    put(1, range(1, n), left=-1, right=-1, first=0, count=leaf_size, skipIndex=2)
    put(2, [0], left=-1, right=-1, first=leaf_size, count=1, skipIndex=-1)
    arrs["tlasNodes"] = nodes
    arrs["tlasInstanceIndices"] = np.array(list(range(1, n)) + [0], np.int32)
    return arrs


@pytest.mark.timeout(600)
@pytest.mark.parametrize("leaf_size", [15, 20])
def test_reference_layout_scenes(orc, renderer, leaf_size):
    arrs = _big_leaf_scene(orc, leaf_size)
    desc, keep = _commit(renderer, arrs)
    p = _params(scenes.Config("big", 0, 0, 0, (0.0, 2.5, 8.0), (0.0, 0.7, 0.0)), 160, 90)
    rng = np.random.default_rng(11)
    for what, o, d in _ray_sets(orc, arrs, desc, p, 3000, seed=5):
        check_closest(orc, arrs, desc, o, d, renderer.trace_rays(o, d), "big%d/%s" % (leaf_size, what))
        tm = _tmax_mix(rng, len(o))
        check_occluded(orc, arrs, o[:800], d[:800], tm[:800], renderer.trace_rays(o[:800], d[:800], tm[:800], query="occluded"), "big%d/%s" % (leaf_size, what))


# ------------------------------------------------------------------ 4. after scene updates
def _device_arrays(renderer, arrs):
    """The scene as it is on the device now: every array (hrt_scene_download_array), the TLAS in the reference's layout
    (hrt_scene_download_tlas)."""
    a = {name: renderer.download_array(name) for name, _ in T.SCENE_ARRAYS}
    nodes, idx, inst, cnt = renderer.download_tlas()
    a["tlasNodes"] = np.frombuffer(bytes(nodes), dtype=T.np_dtype(T.BvhNode), count=cnt[0]).copy()
    a["tlasInstanceIndices"] = np.frombuffer(bytes(idx), dtype=np.int32, count=cnt[1]).copy()
    a["instances"] = np.frombuffer(bytes(inst), dtype=T.np_dtype(T.InstanceRecord), count=cnt[2]).copy()
    return a


def _update_check(orc, renderer, arrs, cfg, what, n=6000):
    a = _device_arrays(renderer, arrs)
    desc, keep = T.scene_desc_from_arrays(a)
    p = _params(cfg, 160, 90)
    rng = np.random.default_rng(13)
    for rs, o, d in _ray_sets(orc, a, desc, p, n, seed=9):
        check_closest(orc, a, desc, o, d, renderer.trace_rays(o, d), "%s/%s" % (what, rs))
        tm = _tmax_mix(rng, len(o))
        got = renderer.trace_rays(o[:400], d[:400], tm[:400], query="occluded")
        check_occluded(orc, a, o[:400], d[:400], tm[:400], got, "%s/%s" % (what, rs))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("policy", [T.REBUILD_FORCE_REFIT, T.REBUILD_FORCE_REBUILD])
def test_after_instance_updates(orc, renderer, policy):
    arrs = _oracle_scene(orc, scenes.build_rotated_instances_scene)
    _commit(renderer, arrs)
    n = len(arrs["instances"])
    ids = np.arange(0, n, 2, dtype=np.int32)
    xf = np.array([_aff(arrs["instances"][i]["objectToWorld"]) for i in ids], np.float32)      # each keeps its rotation / scale and moves
    xf[:, 3] += np.float32(0.3) * (ids % 3 - 1)
    xf[:, 7] += np.float32(0.1) * (ids % 2)
    xf[:, 11] -= np.float32(0.2) * (ids % 4)
    renderer.update_instances(ids, xf, policy)
    _update_check(orc, renderer, arrs, scenes.Config("r", 0, 0, 0, (0.0, 1.5, 5.0), (0.0, 0.8, 0.0)), "instances%d" % policy)


@pytest.mark.timeout(900)
def test_after_sphere_updates(orc, renderer):
    arrs = _oracle_scene(orc, scenes.build_config2)
    _commit(renderer, arrs)
    sp = np.array(arrs["spheres"], copy=True)
    sp["center"]["Y"][1:] += np.float32(0.25)
    sp["radius"][1:] *= np.float32(0.9)
    renderer.update_spheres(0, sp, T.REBUILD_AUTO)
    _update_check(orc, renderer, arrs, scenes.CONFIGS[2], "spheres")


@pytest.mark.timeout(900)
@pytest.mark.parametrize("policy", [T.REBUILD_AUTO, T.REBUILD_AUTO | T.REBUILD_BLAS])
def test_after_vertex_updates(orc, renderer, policy):
    arrs = _oracle_scene(orc, lambda b: scenes.build_config4(b, nu=64, nv=64))
    _commit(renderer, arrs)
    pos = np.stack([arrs["meshPositions"][a] for a in "XYZ"], 1).astype(np.float32)
    pos[:, 1] += np.float32(0.05) * np.sin(np.float32(3.0) * pos[:, 0]).astype(np.float32)
    renderer.update_positions(0, pos, policy)
    _update_check(orc, renderer, arrs, scenes.CONFIGS[4], "positions%d" % policy)


# ------------------------------------------------------------------ 5. full size against the frame's G-buffer
def _pack_matid(shade, ior):
    """StoreHit (RTRay.cs:90-98): (shade & 0xFFFF) | (FloatToI16(ior) << 16)."""
    uniq, inv = np.unique(np.ascontiguousarray(ior).view(np.uint32), return_inverse=True)
    i16 = np.array([OI.float_to_i16(f32(v)) for v in uniq.view(np.float32)], np.int64)[inv.reshape(-1)]
    return ((shade.astype(np.int64) & 0xFFFF) | (i16 << 16)).astype(np.uint32).view(np.int32)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("cfg_id", [2, 4])
def test_full_size_matches_gbuffer(orc, renderer, cfg_id):
    arrs = _oracle_scene(orc, lambda b: scenes.build(cfg_id, b))
    _commit(renderer, arrs)
    cfg = scenes.CONFIGS[cfg_id]
    w, h = 1920, 1080
    p = _params(cfg, w, h)
    renderer.reset_history()
    out, og = T.alloc_outputs(w, h, names=["gb_hitMask", "gb_normalWS", "gb_baseColor", "gb_objId", "gb_matId", "gb_worldPos"])
    renderer.render_params(p, og)
    idx = np.arange(w * h)
    rng = np.random.default_rng(1)
    _check_camera_rays_match_frame(p, rng.choice(w * h, 3000, replace=False))
    o, d = _camera_rays(p, idx)
    g = _unpack(renderer.trace_rays(o, d))
    hit = g["t"] < f32(1e29)
    assert (out["gb_hitMask"] == hit.astype(np.int32)).all()
    assert H.bits_equal(out["gb_normalWS"][hit], g["normal"][hit]).all()
    assert H.bits_equal(out["gb_baseColor"][hit], g["albedo"][hit]).all()
    assert (out["gb_objId"][hit] == g["objId"][hit]).all()
    assert (out["gb_matId"][hit] == _pack_matid(g["shade"][hit], g["ior"][hit])).all()
    with np.errstate(all="ignore"):
        pos = (o + d * g["t"][:, None]).astype(np.float32)           # numpy: separate multiply and add, no FMA
    assert H.bits_equal(out["gb_worldPos"][hit], pos[hit]).all()
    assert (out["gb_objId"][~hit] == -1).all()
    renderer.camera = engine.copy_camera(p.cam)         # pick casts from the camera of the last make_params
    renderer.make_params(w, h, 0)
    for k in rng.choice(w * h, 8, replace=False):
        x, y = int(k % w), int(k // w)
        r = renderer.pick(w, h, x, y)
        assert H.bits_equal(np.array([r["t"]], np.float32), g["t"][k:k + 1]).all() and int(r["objId"]) == int(g["objId"][k])
        assert int(r["instance"]) == int(g["instance"][k]) and int(r["prim"]) == int(g["prim"][k])


# ------------------------------------------------------------------ 6. the product against itself
def _as_records(g):
    return np.concatenate([g["t"][:, None], g["normal"], g["albedo"], g["ior"][:, None],
                           np.stack([g["objId"], g["shade"], g["instance"], g["prim"]], 1).view(np.float32)], 1).astype(np.float32)


DEVICE_WORKER = r'''
import sys
sys.path.insert(0, %(root)r)
import torch                                        # first: its HIP runtime is the one the process uses
import ctypes as C
import numpy as np
from ilgpu_raytracing_amd import _types as T, engine, scenes
from oracle import orc
from tests import helpers as H
from tests.test_ray_query_gpu import _oracle_scene, _commit, _params, _ray_sets, _unpack, _tmax_mix, _as_records

orc.build()
torch.cuda.set_device(0)
r = engine.RTRenderer([0])
arrs = _oracle_scene(orc, scenes.build_config3)
desc, keep = _commit(r, arrs)
p = _params(scenes.CONFIGS[3], 320, 180)
rng = np.random.default_rng(3)
for what, o, d in _ray_sets(orc, arrs, desc, p, 20000, seed=1):
    hh = r.trace_rays(o, d)
    to, td = torch.from_numpy(o).cuda(0), torch.from_numpy(d).cuda(0)
    dh = r.trace_rays(to, td)
    assert dh["t"].device.type == "cuda" and dh["objId"].dtype == torch.int32
    rec = torch.cat([dh["t"][:, None], dh["normal"], dh["albedo"], dh["ior"][:, None],
                     torch.stack([dh["objId"], dh["shade"], dh["instance"], dh["prim"]], 1).view(torch.float32)], 1).cpu().numpy()
    assert H.bits_equal(_as_records(_unpack(hh)), rec).all(), what
    tm = _tmax_mix(rng, len(o))
    ho = r.trace_rays(o, d, tm, query="occluded")
    do = r.trace_rays(to, td, torch.from_numpy(tm).cuda(0), query="occluded")
    assert do.device.type == "cuda" and (do.cpu().numpy() == ho).all(), what
# the device path's pointer checks
L, ctx = r._L, r._ctx
rays = torch.zeros((4, 8), dtype=torch.float32, device="cuda:0")
hits = torch.zeros((4, 12), dtype=torch.float32, device="cuda:0")
host_hits = (T.RayHit * 4)()
assert L.hrt_trace_rays(ctx, 0, rays.data_ptr(), 4, host_hits, 0, None) == -1        # device rays, host results
assert L.hrt_trace_rays(ctx, 0, rays.data_ptr(), 4, hits.data_ptr(), 0, None) == 0
assert L.hrt_trace_rays(ctx, 0, rays.data_ptr() + 4, 3, hits.data_ptr(), 0, None) == -1   # not 16-byte aligned
assert L.hrt_trace_rays(ctx, 0, rays.data_ptr(), 4, hits.data_ptr(), -1, None) == -1     # device memory on the host path
r.close()
print("DEVICE_PATH_OK")
'''


@pytest.mark.timeout(600)
def test_device_pointers_equal_host_pointers(tmp_path):
    """torch tensors on the GPU (device path, no host copy) give the bits numpy arrays (host path) give."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "device_worker.py"
    script.write_text(DEVICE_WORKER % {"root": root})
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=540, cwd=root)
    assert out.returncode == 0 and "DEVICE_PATH_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.timeout(900)
def test_two_slots_equal_one_and_chunk_edges(orc, renderer):
    arrs = _oracle_scene(orc, scenes.build_config2)
    desc, keep = _commit(renderer, arrs)
    two = engine.RTRenderer([0, 0])
    try:
        two.commit(desc)
        p = _params(scenes.CONFIGS[2], 1920, 1200)
        rng = np.random.default_rng(5)
        for n in (1, 63, 65, 4097, T.QUERY_CHUNK + 17):
            idx = rng.integers(0, p.width * p.height, n)
            o, d = _camera_rays(p, idx)
            d[::3] = rng.standard_normal((len(d[::3]), 3)).astype(np.float32)
            a, b = renderer.trace_rays(o, d), two.trace_rays(o, d)
            assert H.bits_equal(_as_records(_unpack(a)), _as_records(_unpack(b))).all(), n
            if n < 100000:
                check_closest(orc, arrs, desc, o, d, a, "n=%d" % n, max_instance_checks=50)
            else:       # several chunks on one slot: each ray's result is the one it gets alone in a small batch
                sub = rng.choice(n, 2000, replace=False)
                sub = np.concatenate([sub, [0, T.QUERY_CHUNK - 1, T.QUERY_CHUNK, n - 1]])
                c = renderer.trace_rays(o[sub], d[sub])
                assert H.bits_equal(_as_records(_unpack(a[sub])), _as_records(_unpack(c))).all()
            tm = _tmax_mix(rng, n)
            oa, ob = renderer.trace_rays(o, d, tm, query="occluded"), two.trace_rays(o, d, tm, query="occluded")
            assert (oa == ob).all(), n
        assert two.trace_rays(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)).shape == (0,)
    finally:
        two.close()


# ------------------------------------------------------------------ 7. frame state untouched
@pytest.mark.timeout(600)
def test_queries_leave_frame_state_alone(orc, renderer):
    arrs = _oracle_scene(orc, scenes.build_textured_test_scene)
    desc, keep = _commit(renderer, arrs)
    cfg = scenes.Config("t", 0, 0, 0, (0.0, 1.2, 4.0), (0.0, 0.6, 0.0))
    w, h = 160, 96
    ps = [scenes.frame_params(cfg, *H.host_funcs("hrt"), width=w, height=h, spp=2, frame=f, reuse=True, rng_lock_noise=1234) for f in (0, 1)]
    rng = np.random.default_rng(2)
    o, d = _camera_rays(ps[0], rng.integers(0, w * h, 5000))
    tm = _tmax_mix(rng, len(o))

    def run(with_queries):
        renderer.reset_history()
        a0, o0 = T.alloc_outputs(w, h)
        renderer.render_params(ps[0], o0)
        views0 = renderer.device_views()
        times0 = renderer.frame_times(0).copy(), renderer.frame_times(1).copy()
        if with_queries:
            renderer.trace_rays(o, d)
            renderer.trace_rays(o, d, tm, query="occluded")
            v = renderer.device_views()
            for f in ("color", "gb_worldPos", "gb_normalWS", "gb_matId", "present_color"):
                assert getattr(v, f) == getattr(views0, f), f
            assert list(v.res_a) == list(views0.res_a) and list(v.res_b) == list(views0.res_b)
            assert (renderer.frame_times(0) == times0[0]).all() and (renderer.frame_times(1) == times0[1]).all()
        a1, o1 = T.alloc_outputs(w, h)
        renderer.render_params(ps[1], o1)
        col = renderer.present(w * 2, h * 2, taau=True)
        return a0, a1, col

    ref = run(False)
    got = run(True)
    for x, y in zip(ref[:2], got[:2]):
        for k in x:
            assert H.bits_equal(x[k], y[k]).all(), k
    assert (ref[2] == got[2]).all()

    # queries while frames enqueued with HRT_FLAG_NO_SYNC are in flight
    hits_alone = renderer.trace_rays(o, d)
    occ_alone = renderer.trace_rays(o, d, tm, query="occluded")
    renderer.reset_history()
    p = scenes.frame_params(cfg, *H.host_funcs("hrt"), width=w, height=h, spp=2)
    for _ in range(3):
        renderer.render_params(p, None, flags=T.FLAG_NO_SYNC)
    hq = renderer.trace_rays(o, d)
    oq = renderer.trace_rays(o, d, tm, query="occluded")
    st = renderer.synchronize()
    assert st.frames == 3 and len(renderer.frame_times(1)) == 3
    assert H.bits_equal(_as_records(_unpack(hq)), _as_records(_unpack(hits_alone))).all() and (oq == occ_alone).all()
    check_closest(orc, arrs, desc, o, d, hq, "no-sync", max_instance_checks=30)


# ------------------------------------------------------------------ 8. error codes
def test_error_codes(renderer, hrt_lib):
    L = hrt_lib
    ray = (T.Ray * 4)()
    hits = (T.RayHit * 4)()
    ms = C.c_float(-1.0)
    assert L.hrt_trace_rays(None, 0, ray, 4, hits, -1, None) == -1
    fresh = engine.RTRenderer([0])
    try:
        ctx = fresh._ctx
        assert L.hrt_trace_rays(ctx, 0, ray, 4, hits, -1, None) == -2          # no scene uploaded
        assert L.hrt_trace_rays(ctx, 0, ray, 0, hits, -1, C.byref(ms)) == 0 and ms.value == 0.0
    finally:
        fresh.close()
    s = engine.Scene()
    s.build_default_scene()
    renderer.commit(s)
    ctx = renderer._ctx
    assert L.hrt_trace_rays(ctx, 0, ray, -1, hits, -1, None) == -1             # n < 0
    assert L.hrt_trace_rays(ctx, 0, None, 4, hits, -1, None) == -1             # NULL rays
    assert L.hrt_trace_rays(ctx, 0, ray, 4, None, -1, None) == -1              # NULL results
    assert L.hrt_trace_rays(ctx, 2, ray, 4, hits, -1, None) == -1              # unknown query
    assert L.hrt_trace_rays(ctx, -7, ray, 4, hits, -1, None) == -1
    assert L.hrt_trace_rays(ctx, 0, ray, 4, hits, 1, None) == -1               # slot out of range (one slot)
    assert L.hrt_trace_rays(ctx, 0, ray, 4, hits, 99, None) == -1
    assert L.hrt_trace_rays(ctx, 0, ray, 4, hits, 0, None) == -1               # dev >= 0 with host memory
    assert L.hrt_trace_rays(ctx, 1, ray, 4, hits, 0, None) == -1
    assert L.hrt_trace_rays(ctx, 0, None, 0, None, -1, None) == 0              # n == 0: nothing to do
    assert L.hrt_trace_rays(ctx, 0, ray, 4, hits, -1, C.byref(ms)) == 0 and ms.value >= 0.0


# ------------------------------------------------------------------ 9. the staging the three caller-ray queries share
def _pack(o, d, tmax):
    rays = np.zeros((len(o), 8), np.float32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 3] = o, d, tmax
    return rays


def _three_queries(L, ctx, p, rays, n, k, nh, out=None):
    """hrt_trace_rays (both queries) and hrt_trace_paths over the first n of rays, hrt_trace_hits with totals over the first nh, through
    the C entry points with the caller's own arrays; returns them (freshly allocated unless `out` passes a set in)."""
    res = out or dict(closest=np.zeros(n, T.np_dtype(T.RayHit)), occluded=np.zeros(n, np.int32), hits=np.zeros((nh, k), T.np_dtype(T.RayHit)),
                      counts=np.zeros(nh, np.int32), totals=np.zeros(nh, np.int32), paths=np.zeros(n, T.np_dtype(T.PathResult)))
    ptr = lambda name: res[name].ctypes.data
    assert L.hrt_trace_rays(ctx, T.QUERY_CLOSEST, rays.ctypes.data, n, ptr("closest"), -1, None) == 0
    assert L.hrt_trace_hits(ctx, rays.ctypes.data, nh, k, ptr("hits"), ptr("counts"), ptr("totals"), -1, None) == 0
    assert L.hrt_trace_paths(ctx, C.byref(p), 0, rays.ctypes.data, n, 0, ptr("paths"), -1, None) == 0
    assert L.hrt_trace_rays(ctx, T.QUERY_OCCLUDED, rays.ctypes.data, n, ptr("occluded"), -1, None) == 0
    return res


def _assert_same_bytes(a, b, what):
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), "%s: %s" % (what, name)


def _staging_case(rng, n):
    p = scenes.frame_params(scenes.CONFIGS[2], *H.host_funcs("hrt"), width=1920, height=1200, spp=4)
    o, d = _camera_rays(p, rng.integers(0, p.width * p.height, n))
    d[::3] = rng.standard_normal((len(d[::3]), 3)).astype(np.float32)
    return p, _pack(o, d, _tmax_mix(rng, n))


@pytest.mark.timeout(900)
def test_registered_host_arrays_give_the_same_bytes(orc, renderer, hrt_lib):
    """A host-path call whose arrays the caller page-locked (hrt_host_register) copies straight from and into them, without the pinned
    staging: the same bytes as the pageable call, for the three queries, with more rays (and, at k = 4, more hit slots) than a chunk."""
    _commit(renderer, _oracle_scene(orc, scenes.build_config2))
    n, nh = T.QUERY_CHUNK + 777, T.QUERY_CHUNK // 4 + 777
    p, rays = _staging_case(np.random.default_rng(21), n)
    ref = _three_queries(hrt_lib, renderer._ctx, p, rays, n, 4, nh)
    got = {name: np.zeros_like(a) for name, a in ref.items()}
    pinned = [rays] + list(got.values())
    renderer.register_host(pinned)
    try:
        _three_queries(hrt_lib, renderer._ctx, p, rays, n, 4, nh, out=got)
    finally:
        renderer.unregister_host(pinned)
    assert ref["counts"].any() and ref["occluded"].any()
    _assert_same_bytes(ref, got, "registered")
    # only some of a call's arrays registered: each array decides for itself
    some = {name: np.zeros_like(a) for name, a in ref.items()}
    pinned = [some["hits"], some["paths"]]
    renderer.register_host(pinned)
    try:
        _three_queries(hrt_lib, renderer._ctx, p, rays, n, 4, nh, out=some)
    finally:
        renderer.unregister_host(pinned)
    _assert_same_bytes(ref, some, "partly registered")


@pytest.mark.timeout(900)
def test_alternating_queries_share_one_context(orc, renderer, hrt_lib):
    """One context calling the three queries in turn, small then large then small (k = 16 after hrt_trace_rays, radiance after both),
    gives what a fresh context gives for each size: the staging is carved anew for every chunk of every query."""
    desc, keep = _commit(renderer, _oracle_scene(orc, scenes.build_config2))
    sizes = (300, T.QUERY_CHUNK // 16 + 4097, 65)
    p, rays = _staging_case(np.random.default_rng(22), max(sizes))
    got = [_three_queries(hrt_lib, renderer._ctx, p, rays, n, 16, n) for n in sizes]
    for n, g in zip(sizes, got):
        fresh = engine.RTRenderer([0])
        try:
            fresh.commit(desc)
            _assert_same_bytes(_three_queries(hrt_lib, fresh._ctx, p, rays, n, 16, n), g, "n=%d" % n)
        finally:
            fresh.close()
