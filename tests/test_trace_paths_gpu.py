"""Radiance queries (hrt_trace_paths) on the GPU.  The contract's testable property: the frame's own camera rays in pixel order, with
first_key 0 and the frame's width, give the frame's radiance, color, depth and objectId bit for bit, whatever the scene, the path
flags, spp, maxDepth, frame and lock.  Arbitrary and hostile rays are checked against the CPU oracle (primary vertex from
oracle.orc.trace_rays, path stage from oracle.orc.render_frame with the row's origin as camera origin); then the invariances and the
state rules of the call."""
import ctypes as C

import numpy as np
import pytest
import torch          # before libhip_raytrace.so is loaded: torch brings its own HIP runtime of the same soname

from ilgpu_raytracing_amd import _types as T, engine, scenes, tiling
from oracle import orc_indep as OI
from tests import helpers as H

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID_ARG, INVALID_STATE = -1, -2


def _default_scene(b):
    b.build_default_scene()


DEFAULT = scenes.Config("default", 0, 0, 0, (0.0, 1.4, 4.5), (0.0, 0.5, 0.0))
TEXTURED = scenes.Config("textured", 0, 0, 0, (0.3, 1.3, 4.2), (0.0, 0.7, 0.0))
BUILDERS = {
    "default": (_default_scene, DEFAULT),
    "config1": (scenes.build_config1, scenes.CONFIGS[1]),
    "config2": (scenes.build_config2, scenes.CONFIGS[2]),
    "config3": (scenes.build_config3, scenes.CONFIGS[3]),
    "config4": (scenes.build_config4, scenes.CONFIGS[4]),
    "config5": (scenes.build_config5, scenes.CONFIGS[5]),
    "textured": (scenes.build_textured_test_scene, TEXTURED),
}
# the path flags that select another organisation or tracer (TREELETS changes only scenes with big triangle meshes)
FLAGS = {name: [0, T.FLAG_MEGAKERNEL, T.FLAG_STREAMED, T.FLAG_REFERENCE_LAYOUT] for name in BUILDERS}
for _n in ("config4", "config5"):
    FLAGS[_n] = FLAGS[_n] + [T.FLAG_TREELETS | T.FLAG_STREAMED]
_SCENES = {}


def _scene(name):
    if name not in _SCENES:
        s = engine.Scene()
        BUILDERS[name][0](s)
        _SCENES[name] = s
    return _SCENES[name]


def _commit(r, name):
    r.commit(_scene(name))
    r.reset_history()


def _params(name, w, h, spp, frame=0, lock=0, depth=None):
    cfg = BUILDERS[name][1]
    c2 = scenes.Config(cfg.name, w, h, spp, cfg.cam_origin, cfg.cam_lookat, extra=cfg.extra)
    p = scenes.frame_params(c2, *H.host_funcs("hrt"), frame=frame, reuse=False, rng_lock_noise=lock)
    if depth is not None:
        p.maxDepth = depth
    return p


def _frame(r, p, flags=0):
    arrs, o = T.alloc_outputs(p.width, p.height, names=("color", "depth", "objectId", "radiance"))
    r.render_params(p, o, flags=flags)
    return arrs


def _as_frame(res):
    """hrt_path_result records (host structured array, or the dict of the device path) as the frame's four arrays"""
    if isinstance(res, dict):
        return dict(radiance=res["radiance"].cpu().numpy(), color=res["color"].cpu().numpy(), depth=res["depth"].cpu().numpy(),
                    objectId=res["objId"].cpu().numpy())
    assert (res["reserved"] == 0).all()
    rad = np.stack([res["radiance"][a] for a in ("X", "Y", "Z")], 1).astype(np.float32)
    return dict(radiance=rad, color=res["color"], depth=res["depth"].astype(np.float32), objectId=res["objId"])


def _same(ref, got, what):
    for k in ("radiance", "color", "depth", "objectId"):
        eq = H.bits_equal(np.ascontiguousarray(ref[k]), np.ascontiguousarray(got[k]))
        eq = eq.all(axis=1) if eq.ndim > 1 else eq
        assert eq.all(), "%s: %s differs at %d of %d keys (first %s)" % (what, k, int((~eq).sum()), len(eq), np.flatnonzero(~eq)[:5])


def _probe_rays(centre, w, h):
    """equirectangular directions over rows of w keys, all from `centre`"""
    j = np.arange(w * h)
    phi = ((j % w) + 0.5) / w * 2 * np.pi
    th = ((j // w) + 0.5) / h * np.pi
    d = np.stack([np.sin(th) * np.cos(phi), np.cos(th), np.sin(th) * np.sin(phi)], 1).astype(np.float32)
    return np.broadcast_to(np.asarray(centre, np.float32), d.shape).copy(), d


@pytest.fixture(scope="module")
def rnd(hrt_lib):
    r = engine.RTRenderer([0])
    yield r
    r.close()


# ------------------------------------------------------------------ 1. frame equivalence
CASES = [(1, 0, 0, 0), (3, 5, 0, 0), (3, 1, 1, 1), (1, 5, 1, 0)]      # (spp, maxDepth, frame, lock)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_camera_rays_give_the_frame(rnd, name):
    _commit(rnd, name)
    for flags in FLAGS[name]:
        for spp, depth, frame, lock in CASES:
            p = _params(name, 40, 28, spp, frame=frame, lock=lock, depth=depth)
            ref = _frame(rnd, p, flags)
            o, d = rnd.camera_rays(p)
            got = _as_frame(rnd.trace_paths(o, d, p, flags=flags))
            _same(ref, got, "%s flags=%#x spp=%d depth=%d frame=%d lock=%d" % (name, flags, spp, depth, frame, lock))


def test_headline_frame_config2_1080p(rnd):
    _commit(rnd, "config2")
    p = _params("config2", 1920, 1080, 4)
    ref = _frame(rnd, p)
    o, d = rnd.camera_rays(p)
    _same(ref, _as_frame(rnd.trace_paths(o, d, p)), "config2 1920x1080 4 spp")


# ------------------------------------------------------------------ 2. / 3. arbitrary and hostile rays against the oracle
def _closest_ior(orc, arrs, o, d):
    """TraceClosest's bestIor per ray (SceneDeviceViews.cs:30-86), which oracle.orc.trace_rays does not return: the independent
    restatement oracle.orc_indep.Views.trace_closest.  Also its hit flag and t, to be checked against oracle.orc."""
    V = OI.Views(arrs)
    V.math = lambda name, x, y=None: orc.math_eval(name, np.array([x], np.float32), None if y is None else np.array([y], np.float32))[0]
    hit, t, ior = np.zeros(len(o), bool), np.zeros(len(o), np.float32), np.ones(len(o), np.float32)
    with np.errstate(all="ignore"):
        for i in range(len(o)):
            oo, dd = tuple(map(f32, o[i])), tuple(map(f32, d[i]))
            h, tt, _, _, _, _, ii = V.trace_closest((oo, dd, OI.inv_dir(dd)))
            hit[i], t[i], ior[i] = h, tt, ii
    return hit, t, ior


def _oracle_paths(orc, desc, p, o, d, ior):
    """Expected results of rays whose rows (p.width keys from key 0) each share one origin; ior from _closest_ior."""
    W, n = p.width, len(o)
    rows = (n + W - 1) // W
    ref = orc.trace_rays(desc, o, d)
    hit = ref["hit"] != 0
    with np.errstate(all="ignore"):
        wp = np.where(hit[:, None], o + d * ref["t"][:, None], o + d * f32(1e6)).astype(np.float32)      # pos / StoreMiss
        i16 = np.clip(ior.astype(np.float32) * f32(1000.0), f32(0), f32(65535)).astype(np.int64) & 0xFFFF   # FloatToI16
    arrs, out = T.alloc_outputs(W, rows)
    arrs["gb_worldPos"][:n] = wp
    arrs["gb_normalWS"][:n] = np.where(hit[:, None], ref["normal"], np.array([0, 1, 0], np.float32))
    arrs["gb_baseColor"][:n] = np.where(hit[:, None], ref["albedo"], f32(0))
    arrs["gb_matId"][:n] = np.where(hit, (ref["shade"].astype(np.int64) & 0xFFFF) | (i16 << 16), -1).astype(np.int32)
    arrs["gb_objId"][:n] = np.where(hit, ref["objId"], -1)
    arrs["gb_hitMask"][:n] = hit.astype(np.int32)
    q = T.FrameParams.from_buffer_copy(p)
    q.height = rows
    for r in range(rows):
        q.cam.origin = T.f3(*o[r * W])
        orc.render_frame(desc, q, out, row_begin=r, row_end=r + 1, run_primary=False)
    res = {k: arrs[k][:n].copy() for k in ("radiance", "color", "depth", "objectId")}
    K = OI.Frame(p)
    spp = max(1, p.spp)
    for i in np.flatnonzero(~hit):            # a missed caller ray: SafeColor(SkyWeighted(ray.dir)), spp times in order, scaled
        c = OI.safe_color(K.sky(tuple(f32(v) for v in d[i])))
        acc = (f32(0), f32(0), f32(0))
        for _ in range(spp):
            acc = tuple(f32(a + b) for a, b in zip(acc, c))
        L = np.array([f32(a * (f32(1.0) / f32(spp))) for a in acc], np.float32)
        res["radiance"][i] = L
        res["color"][i] = orc.lib().orc_pack_rgba8(*[float(v) for v in L])
    return res


def _oracle_scene(orc, builder):
    so = orc.OrcScene()
    builder(so)
    return so.arrays()


def _ray_set(cfg, W, rng):
    """rows of W keys with one origin each: equirectangular probe rows from inside the scene, a fisheye row, rows from random
    origins with unnormalised directions, a row from inside the first sphere, hostile rows"""
    po, pd = _probe_rays(cfg.cam_lookat, W, 3)
    a = (np.arange(W) + 0.5) / W * np.pi * 0.95                                 # fisheye: equidistant angle across the row
    fd = np.stack([np.sin(a - np.pi * 0.475), np.zeros(W), -np.cos(a - np.pi * 0.475)], 1).astype(np.float32)
    fo = np.repeat(np.asarray(cfg.cam_origin, np.float32)[None], W, 0)
    ro = np.repeat(rng.uniform(-2, 2, (2, 3)).astype(np.float32) + np.asarray(cfg.cam_lookat, np.float32), W, 0)
    rd = (rng.standard_normal((2 * W, 3)) * rng.uniform(0.2, 3.0, (2 * W, 1))).astype(np.float32)
    ho = np.repeat(np.asarray(cfg.cam_lookat, np.float32)[None], W, 0)
    hd = rng.standard_normal((W, 3)).astype(np.float32)
    hd[0::6, 0] = np.nan
    hd[1::6, 1] = np.inf
    hd[2::6, 2] = -np.inf
    hd[3::6] = 0.0
    hd[4::6, 0] = f32(1e-40)
    hd[5::6, 1] = f32(-1e-42)
    spec = np.array([np.nan, np.inf, -np.inf, 0.0, 1e-40], np.float32)
    xo = []
    for v in spec:                                                              # one hostile origin component per row
        oo = np.repeat(np.asarray(cfg.cam_lookat, np.float32)[None], W, 0)
        oo[:, 0] = v
        xo.append(oo)
    xo = np.concatenate(xo)
    xd = np.tile(pd[:W], (len(spec), 1))
    return np.concatenate([po, fo, ro, ho, xo]), np.concatenate([pd, fd, rd, hd, xd])


@pytest.mark.parametrize("name,builder,cfg", [
    ("config2", scenes.build_config2, scenes.CONFIGS[2]),                              # sphere scene (glass spheres)
    ("config3", scenes.build_config3, scenes.CONFIGS[3]),                              # sphere instances
    ("rotated", scenes.build_rotated_instances_scene, scenes.CONFIGS[2]),              # rotated / scaled instances
    ("textured", scenes.build_textured_test_scene, TEXTURED),                          # alpha-textured mesh
])
def test_arbitrary_rays_against_the_oracle(orc, rnd, name, builder, cfg):
    arrs = _oracle_scene(orc, builder)
    desc, keep = T.scene_desc_from_arrays(arrs)
    rnd.commit(desc)
    rnd.reset_history()
    W = 24
    rng = np.random.default_rng(11)
    o, d = _ray_set(cfg, W, rng)
    if name == "config2":                                                      # a row from inside a glass sphere
        sp = arrs["spheres"]
        g = np.flatnonzero(sp["shading"] == T.SHADING_GLASS)
        c = sp["center"][g[0] if len(g) else 0]
        o = np.concatenate([o, np.repeat(np.array([[c["X"], c["Y"], c["Z"]]], np.float32), W, 0)])
        d = np.concatenate([d, _probe_rays((0, 0, 0), W, 1)[1]])
    ihit, it, ior = _closest_ior(orc, arrs, o, d)
    oref = orc.trace_rays(desc, o, d)
    assert (ihit == (oref["hit"] != 0)).all() and H.bits_equal(it[ihit], oref["t"][ihit]).all()
    for spp, depth in ((2, 4), (1, 1)):
        p = _params("config2", W, 4, spp, depth=depth, frame=1)
        ref = _oracle_paths(orc, desc, p, o, d, ior)
        _same(ref, _as_frame(rnd.trace_paths(o, d, p)), "%s spp=%d depth=%d" % (name, spp, depth))


# ------------------------------------------------------------------ 4. invariance
def test_invariance_keys_chunks_device_path(rnd):
    _commit(rnd, "config2")
    p = _params("config2", 64, 48, 2, depth=3)
    o, d = _probe_rays((0.0, 1.0, 0.0), 64, 48)
    full = _as_frame(rnd.trace_paths(o, d, p))
    a, b = 1000, 2100                                         # a slice of a call equals a call on the slice, keys shifted
    _same({k: v[a:b] for k, v in full.items()}, _as_frame(rnd.trace_paths(o[a:b], d[a:b], p, first_key=a)), "first_key slice")
    got = rnd.trace_paths(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), p)
    _same(full, _as_frame(got), "device path")
    # more keys than one chunk, in rows of 4096 keys and in one row wider than a chunk
    n = T.QUERY_CHUNK + 777
    rng = np.random.default_rng(3)
    big_o = np.repeat(np.array([[0.0, 1.0, 0.0]], np.float32), n, 0)
    big_d = rng.standard_normal((n, 3)).astype(np.float32)
    for w in (4096, T.QUERY_CHUNK + 100):
        pw = _params("config2", w, 8, 1, depth=2)
        big = _as_frame(rnd.trace_paths(big_o, big_d, pw))
        for s in (0, T.QUERY_CHUNK - 5, n - 300):
            sl = _as_frame(rnd.trace_paths(big_o[s:s + 300], big_d[s:s + 300], pw, first_key=s))
            _same({k: v[s:s + 300] for k, v in big.items()}, sl, "width %d, keys at %d" % (w, s))


def test_two_slots_equal_one(hrt_lib):
    a, b = engine.RTRenderer([0]), engine.RTRenderer([0, 0])
    try:
        for r in (a, b):
            _commit(r, "config4")
        p = _params("config4", 48, 40, 2, depth=3)
        o, d = _probe_rays((0.0, 1.0, 0.0), 48, 40)
        _same(_as_frame(a.trace_paths(o, d, p)), _as_frame(b.trace_paths(o, d, p)), "two slots")
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 5. state
def test_frame_state_left_alone(rnd):
    _commit(rnd, "config1")
    p = _params("config1", 48, 32, 2)
    arrs, out = T.alloc_outputs(48, 32)
    rnd.render_params(p, out)
    before = {k: v.copy() for k, v in arrs.items()}
    views = bytes(rnd.device_views())
    times = rnd.frame_times(1)
    o, d = _probe_rays((0.0, 1.0, 0.0), 48, 32)
    rnd.trace_paths(o, d, p)
    assert bytes(rnd.device_views()) == views
    assert rnd.frame_times(1) == times
    for k in before:
        assert H.bits_equal(before[k], arrs[k]).all(), k                   # host outputs untouched
    # the path stage again from the resident G-buffer and resPrev: the same frame iff the query left the device state alone
    again, out2 = T.alloc_outputs(48, 32)
    rnd.render_params(p, out2, flags=T.FLAG_SKIP_PRIMARY)
    for k in ("color", "depth", "objectId", "radiance", "gb_worldPos", "gb_normalWS", "gb_objId", "gb_matId", "res_w", "res_wSum", "res_m"):
        assert H.bits_equal(before[k], again[k]).all(), k


def test_progressive_continuation_survives(hrt_lib):
    a, b = engine.RTRenderer([0]), engine.RTRenderer([0])
    try:
        for r in (a, b):
            _commit(r, "config2")
        p = _params("config2", 40, 24, 4)
        q2 = T.FrameParams.from_buffer_copy(p)
        q2.spp = 2
        a.render_progressive(q2, 0)
        o, d = a.camera_rays(p)
        a.trace_paths(o, d, p)
        got, out = T.alloc_outputs(40, 24)
        a.render_progressive(p, 2, out)
        ref, out_b = T.alloc_outputs(40, 24)
        b.render_params(p, out_b)
        H.assert_outputs_equal(ref, got)
    finally:
        a.close()
        b.close()


def test_no_sync_frames_stay_correct(hrt_lib):
    a, b = engine.RTRenderer([0]), engine.RTRenderer([0])
    try:
        for r in (a, b):
            _commit(r, "config2")
        p = _params("config2", 64, 40, 3)
        q = _params("config2", 64, 40, 2, frame=5, depth=4)                 # the query: other params than the enqueued frame
        a.render_params(p, None, flags=T.FLAG_NO_SYNC)
        o, d = a.camera_rays(q)
        got = _as_frame(a.trace_paths(o, d, q))
        st = a.synchronize()
        assert st.frames == 1
        _same(_frame(b, q), got, "query after an enqueued frame")
        ref = _frame(b, p)
        v = a.device_views()                                  # the enqueued frame as it is on the device after the query
        P = 64 * 40
        dev = {"color": (v.color, (P,), np.int32), "depth": (v.depth, (P,), np.float32), "objectId": (v.objectId, (P,), np.int32),
               "radiance": (v.radiance, (P, 3), np.float32)}
        enq = {k: torch.as_tensor(tiling._DeviceArray(ptr, shape, dt), device="cuda").cpu().numpy() for k, (ptr, shape, dt) in dev.items()}
        _same(ref, enq, "the enqueued frame after the query")
    finally:
        a.close()
        b.close()


def test_query_sees_scene_updates(rnd):
    _commit(rnd, "config3")
    p = _params("config3", 40, 28, 2)
    xf = np.tile(np.array([1, 0, 0, 0.3, 0, 1, 0, 0.2, 0, 0, 1, -0.1], np.float32), (2, 1))
    rnd.update_instances([0, 5], xf)
    o, d = rnd.camera_rays(p)
    _same(_frame(rnd, p), _as_frame(rnd.trace_paths(o, d, p)), "after update_instances")
    _commit(rnd, "config2")
    sp = rnd.download_array("spheres")[:2].copy()
    sp["center"]["Y"] += f32(0.25)
    rnd.update_spheres(0, sp)
    p2 = _params("config2", 40, 28, 2)
    o, d = rnd.camera_rays(p2)
    _same(_frame(rnd, p2), _as_frame(rnd.trace_paths(o, d, p2)), "after update_spheres")


# ------------------------------------------------------------------ 6. errors
def test_errors(rnd, hrt_lib):
    _commit(rnd, "config2")
    p = _params("config2", 16, 8, 1)
    L = hrt_lib
    rays = np.zeros((4, 8), np.float32)
    res = np.zeros(4, T.np_dtype(T.PathResult))
    q = T.FrameParams.from_buffer_copy(p)
    q.enableSpatialReuse = 1
    ms = C.c_float(1.0)
    assert L.hrt_trace_paths(rnd._ctx, C.byref(q), 0, rays.ctypes.data, 4, 0, res.ctypes.data, -1, C.byref(ms)) == INVALID_ARG
    q = T.FrameParams.from_buffer_copy(p)
    q.enableTemporalReuse = 1
    assert L.hrt_trace_paths(rnd._ctx, C.byref(q), 0, rays.ctypes.data, 4, 0, res.ctypes.data, -1, None) == INVALID_ARG
    assert L.hrt_trace_paths(rnd._ctx, C.byref(p), T.FLAG_COUNTERS, rays.ctypes.data, 4, 0, res.ctypes.data, -1, None) == INVALID_ARG
    assert L.hrt_trace_paths(rnd._ctx, C.byref(p), 0, rays.ctypes.data, 4, 0x7FFFFFFF - 3, res.ctypes.data, -1, None) == INVALID_ARG
    assert L.hrt_trace_paths(rnd._ctx, C.byref(p), 0, None, 4, 0, res.ctypes.data, -1, None) == INVALID_ARG
    ms = C.c_float(1.0)
    assert L.hrt_trace_paths(rnd._ctx, C.byref(p), 0, None, 0, 0, None, -1, C.byref(ms)) == 0 and ms.value == 0.0
    fresh = engine.RTRenderer([0])
    try:
        assert L.hrt_trace_paths(fresh._ctx, C.byref(p), 0, rays.ctypes.data, 4, 0, res.ctypes.data, -1, None) == INVALID_STATE
    finally:
        fresh.close()
