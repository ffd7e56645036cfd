"""Guard bands: no entry point writes outside the caller's buffers.

Every destination (and every input) goes to the raw C ABI as the middle of a larger allocation pre-filled with 0xA5 (tests/guards.py),
at the weakest alignment include/hip_raytrace.h allows: 16 bytes for rays and result records, 8 for motion vectors, 4 for counts, totals
and the frame's planes.  Every case asserts BOTH: the payload equals what the suite already trusts for that call (the oracle and the
restatements, through the helpers of the neighbouring GPU tests), and every guard byte on both sides still holds 0xA5.  A guard check
alone would pass a call that did nothing; a payload check alone is the rest of the suite.

References are computed once per module and shared; results of ray queries depend on the ray alone (radiance queries: on ray and key),
so the 4097-ray reference is a random draw from 640 distinct rays whose restatement runs once."""
import ctypes as C

import numpy as np
import pytest
import torch          # before libhip_raytrace.so is loaded: torch brings its own HIP runtime of the same soname

from ilgpu_raytracing_amd import _types as T, engine, scenes, tiling
from oracle import orc_indep as OI
from tests import denoise_ref as R
from tests import denoise_temporal_ref as DT
from tests import guards as G
from tests import helpers as H
from tests import hits_ref as HR
from tests.test_denoise_gpu import _render as render_guides
from tests.test_present_reproject import make_taa
from tests.test_present_reproject_gpu import RefHistory
from tests.test_ray_query_gpu import _ray_sets, _tmax_mix, _math, check_closest, _device_arrays
from tests.test_trace_paths_gpu import _closest_ior, _oracle_paths, _as_frame, _same as same_frame

pytestmark = pytest.mark.gpu
f32 = np.float32
OK, INVALID_ARG = 0, -1

TEXTURED = scenes.Config("t", 0, 0, 0, (0.3, 1.3, 4.2), (0.0, 0.7, 0.0))
SCENES = {"config2": (scenes.build_config2, scenes.CONFIGS[2]), "textured": (scenes.build_textured_test_scene, TEXTURED)}
NS = [1, 63, 64, 65, 255, 257, 4097]
N_MAX, N_DISTINCT = 4097, 640
RAYHIT, PATHRES = T.np_dtype(T.RayHit), T.np_dtype(T.PathResult)
PAD = f32(123.0)                 # hrt_ray.pad: ignored, and not rewritten


@pytest.fixture(scope="module")
def one(hrt_lib):
    r = engine.RTRenderer([0])
    yield r
    r.close()


def _commit(r, name):
    s = engine.Scene()
    SCENES[name][0](s)
    r.commit(s)
    r.reset_history()


def _ok(r, rc):
    assert rc == OK, (rc, r._L.hrt_last_error(r._ctx))


# ====================================================================== ray queries
_RAYS = {}


def _ray_case(orc, name):
    """Per scene, once: 4097 rays drawn from 640 distinct ones (camera, random, bounce and hostile rays of tests/test_ray_query_gpu.py)
    and the references of all four queries over them.  Every smaller n is a prefix."""
    if name in _RAYS:
        return _RAYS[name]
    builder, cfg = SCENES[name]
    so = orc.OrcScene()
    builder(so)
    arrs = so.arrays()
    desc, keep = T.scene_desc_from_arrays(arrs)
    p = scenes.frame_params(cfg, *H.host_funcs("hrt"), width=160, height=90, spp=1)
    rng = np.random.default_rng(len(name))
    sets = _ray_sets(orc, arrs, desc, p, N_DISTINCT // 4, seed=17)
    uo, ud = np.concatenate([s[1] for s in sets]), np.concatenate([s[2] for s in sets])
    utm = _tmax_mix(rng, len(uo))
    utm[: len(uo) // 4] = np.inf
    V = HR.views(orc, arrs)
    uhits, ucnt, utot = HR.trace_hits(V, uo, ud, T.HITS_MAX, utm)
    W = OI.Views(arrs)
    W.math = _math(orc)
    uocc = np.array([1 if W.shadow_occlusion((tuple(map(f32, uo[i])), tuple(map(f32, ud[i])), OI.inv_dir(tuple(map(f32, ud[i])))), f32(utm[i])) else 0
                     for i in range(len(uo))], np.int32)
    pick = rng.integers(0, len(uo), N_MAX)
    pick[:len(uo)] = rng.permutation(len(uo))                  # every distinct ray occurs
    o, d, tm = uo[pick], ud[pick], utm[pick]
    rays = np.zeros((N_MAX, 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, tm, d, PAD
    # radiance queries: one origin for the whole row of 4097 keys (tests/test_trace_paths_gpu.py::_oracle_paths), distinct directions
    po = np.repeat(np.asarray(cfg.cam_lookat, np.float32)[None] + f32(0.25), N_MAX, 0).astype(np.float32)
    pd = ud[pick]
    _, _, uior = _closest_ior(orc, arrs, po[:len(ud)], ud)
    pp = scenes.frame_params(cfg, *H.host_funcs("hrt"), width=N_MAX, height=1, spp=2, frame=1)
    pp.enableTemporalReuse = pp.enableSpatialReuse = 0
    pp.maxDepth = 3
    pref = _oracle_paths(orc, desc, pp, po, pd, uior[pick])
    prays = np.zeros((N_MAX, 8), np.float32)
    prays[:, 0:3], prays[:, 3], prays[:, 4:7], prays[:, 7] = po, f32(np.nan), pd, PAD     # tMax and pad are ignored by hrt_trace_paths
    case = dict(orc=orc, arrs=arrs, desc=desc, keep=keep, o=o, d=d, tm=tm, rays=rays, occ=uocc[pick], hits=uhits[pick], tot=utot[pick],
                pp=pp, prays=prays, pref=pref)
    _RAYS[name] = case
    return case


class _Mem:
    """Guarded buffers of one memory kind: host numpy arrays, or torch tensors on slot 0's device."""

    def __init__(self, dev):
        self.dev = dev                       # -1: host path, 0: device path

    def new(self, shape, dtype, align, lead):
        if self.dev < 0:
            return G.host(shape, dtype, align, lead)
        dt = np.dtype(dtype)
        shape = (shape,) if np.isscalar(shape) else tuple(shape)
        if dt.names:                         # records on the device: rows of 32-bit words
            return G.device(torch, shape + (dt.itemsize // 4,), torch.float32, align, lead)
        return G.device(torch, shape, {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32}[dt], align, lead)

    def put(self, buf, values):
        if self.dev < 0:
            buf[...] = values
        else:
            buf.copy_(torch.from_numpy(np.ascontiguousarray(values)).view(buf.dtype).reshape(buf.shape))
            torch.cuda.synchronize()

    def ptr(self, buf):
        return buf.ctypes.data if self.dev < 0 else buf.data_ptr()

    def get(self, buf, dtype=None):
        """The payload as a numpy array (of structured dtype `dtype` where records were rows of words)."""
        a = buf if self.dev < 0 else buf.cpu().numpy()
        if dtype is not None and a.dtype != np.dtype(dtype):
            a = np.ascontiguousarray(a).view(dtype).reshape(a.shape[:-1])
        return a

    def bytes(self, buf):
        return np.ascontiguousarray(self.get(buf)).tobytes()


def _rays_in(mem, rays):
    buf = mem.new(rays.shape, np.float32, 16, 16)
    mem.put(buf, rays)
    return buf, mem.bytes(buf)


def _inputs_unchanged(mem, buf, before, what):
    assert mem.bytes(buf) == before, "%s: the ray array was modified" % what
    G.check(buf, what + ": rays")


def _run_closest(r, mem, case, n, what):
    rb, before = _rays_in(mem, case["rays"][:n])
    out = mem.new((n,), RAYHIT, 16, 16)
    _ok(r, r._L.hrt_trace_rays(r._ctx, T.QUERY_CLOSEST, mem.ptr(rb), n, mem.ptr(out), mem.dev, None))
    got = mem.get(out, RAYHIT)
    assert G.written(out), what
    check_closest(case["orc"], case["arrs"], case["desc"], case["o"][:n], case["d"][:n], got, what, max_instance_checks=0)
    G.check(out, what + ": hits")
    _inputs_unchanged(mem, rb, before, what)


def _run_occluded(r, mem, case, n, what):
    rb, before = _rays_in(mem, case["rays"][:n])
    align = 16 if mem.dev >= 0 else 4              # the header: device rays and results 16-byte aligned, whatever the record
    out = mem.new((n,), np.int32, align, align)
    _ok(r, r._L.hrt_trace_rays(r._ctx, T.QUERY_OCCLUDED, mem.ptr(rb), n, mem.ptr(out), mem.dev, None))
    got = mem.get(out)
    bad = np.flatnonzero(got != case["occ"][:n])
    assert len(bad) == 0, "%s: occlusion differs at %d of %d rays (first %s)" % (what, len(bad), n, bad[:5])
    G.check(out, what + ": results")
    _inputs_unchanged(mem, rb, before, what)


def _run_hits(r, mem, case, n, k, with_totals, what):
    rb, before = _rays_in(mem, case["rays"][:n])
    hits, counts = mem.new((n, k), RAYHIT, 16, 16), mem.new((n,), np.int32, 4, 4)
    totals = mem.new((n,), np.int32, 4, 4) if with_totals else None
    _ok(r, r._L.hrt_trace_hits(r._ctx, mem.ptr(rb), n, k, mem.ptr(hits), mem.ptr(counts), mem.ptr(totals) if with_totals else None, mem.dev, None))
    assert G.written(hits), what
    HR.assert_same(HR.unpack(mem.get(hits, RAYHIT)), {f: a[:, :k] for f, a in HR.unpack(case["hits"][:n]).items()}, what)
    assert (mem.get(counts) == np.minimum(case["tot"][:n], k)).all(), what
    G.check(hits, what + ": hits")
    G.check(counts, what + ": counts")
    if with_totals:
        assert (mem.get(totals) == case["tot"][:n]).all(), what
        G.check(totals, what + ": totals")
    _inputs_unchanged(mem, rb, before, what)


def _run_paths(r, mem, case, n, what):
    rb, before = _rays_in(mem, case["prays"][:n])
    out = mem.new((n,), PATHRES, 16, 16)
    _ok(r, r._L.hrt_trace_paths(r._ctx, C.byref(case["pp"]), 0, mem.ptr(rb), n, 0, mem.ptr(out), mem.dev, None))
    assert G.written(out), what
    same_frame({k: v[:n] for k, v in case["pref"].items()}, _as_frame(mem.get(out, PATHRES)), what)
    G.check(out, what + ": results")
    _inputs_unchanged(mem, rb, before, what)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dev", [0, -1], ids=["device", "host"])
@pytest.mark.parametrize("entry", ["closest", "occluded", "paths"])
def test_ray_queries(orc, one, entry, dev, n):
    """hrt_trace_rays (both queries) and hrt_trace_paths on one slot: device path (rays and results 16-byte aligned and no better) on the textured scene, host path on config2."""
    name = "textured" if dev == 0 else "config2"
    case = _ray_case(orc, name)
    _commit(one, name)
    what = "%s dev=%d n=%d" % (entry, dev, n)
    {"closest": _run_closest, "occluded": _run_occluded, "paths": _run_paths}[entry](one, _Mem(dev), case, n, what)


@pytest.mark.parametrize("with_totals", [False, True], ids=["no-totals", "totals"])
@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dev", [0, -1], ids=["device", "host"])
def test_trace_hits(orc, one, dev, n, k, with_totals):
    name = "textured" if dev == 0 else "config2"
    case = _ray_case(orc, name)
    _commit(one, name)
    _run_hits(one, _Mem(dev), case, n, k, with_totals, "hits dev=%d n=%d k=%d totals=%d" % (dev, n, k, with_totals))


@pytest.mark.parametrize("n", [65, 4097])
def test_ray_queries_over_three_slots(orc, hrt_lib, n):
    """The host path's contiguous per-slot split has ragged pieces: 65 = 22 + 22 + 21 rays."""
    case = _ray_case(orc, "textured")
    r = engine.RTRenderer([0, 0, 0])
    try:
        _commit(r, "textured")
        mem = _Mem(-1)
        _run_closest(r, mem, case, n, "3 slots closest n=%d" % n)
        _run_occluded(r, mem, case, n, "3 slots occluded n=%d" % n)
        _run_paths(r, mem, case, n, "3 slots paths n=%d" % n)
        for k in (1, 3, 16):
            _run_hits(r, mem, case, n, k, k != 3, "3 slots hits n=%d k=%d" % (n, k))
    finally:
        r.close()


def test_ray_queries_in_registered_ranges(orc, one):
    """Rays and results inside ranges registered with hrt_host_register: the "straight from / to a registered range" branch.  Each
    registration covers exactly the payload; the guards lie outside it."""
    case = _ray_case(orc, "textured")
    _commit(one, "textured")
    L, ctx, n, k = one._L, one._ctx, N_MAX, 3
    rays, prays = G.host((n, 8), np.float32, 16, 16), G.host((n, 8), np.float32, 16, 16)
    rays[...], prays[...] = case["rays"], case["prays"]
    out = dict(closest=G.host((n,), RAYHIT, 16, 16), occluded=G.host((n,), np.int32, 4, 4), hits=G.host((n, k), RAYHIT, 16, 16),
               counts=G.host((n,), np.int32, 4, 4), totals=G.host((n,), np.int32, 4, 4), paths=G.host((n,), PATHRES, 16, 16))
    pinned = [rays, prays] + list(out.values())
    one.register_host(pinned)
    try:
        ptr = lambda name: out[name].ctypes.data
        _ok(one, L.hrt_trace_rays(ctx, T.QUERY_CLOSEST, rays.ctypes.data, n, ptr("closest"), -1, None))
        _ok(one, L.hrt_trace_rays(ctx, T.QUERY_OCCLUDED, rays.ctypes.data, n, ptr("occluded"), -1, None))
        _ok(one, L.hrt_trace_hits(ctx, rays.ctypes.data, n, k, ptr("hits"), ptr("counts"), ptr("totals"), -1, None))
        _ok(one, L.hrt_trace_paths(ctx, C.byref(case["pp"]), 0, prays.ctypes.data, n, 0, ptr("paths"), -1, None))
    finally:
        one.unregister_host(pinned)
    check_closest(orc, case["arrs"], case["desc"], case["o"], case["d"], out["closest"], "registered closest", max_instance_checks=0)
    assert (out["occluded"] == case["occ"]).all()
    HR.assert_same(HR.unpack(out["hits"]), {f: a[:, :k] for f, a in HR.unpack(case["hits"]).items()}, "registered hits")
    assert (out["counts"] == np.minimum(case["tot"], k)).all() and (out["totals"] == case["tot"]).all()
    same_frame(case["pref"], _as_frame(out["paths"]), "registered paths")
    assert rays.tobytes() == case["rays"].tobytes() and prays.tobytes() == case["prays"].tobytes()
    for name, a in list(out.items()) + [("rays", rays), ("path rays", prays)]:
        G.check(a, "registered " + name)


@pytest.mark.parametrize("entry", ["closest", "occluded", "hits", "paths"])
def test_ray_queries_across_the_chunk_seam(orc, one, entry):
    """HRT_QUERY_CHUNK + 17 rays (hits: k = 16, HRT_QUERY_CHUNK // 16 + 17 rays) on one slot: the staged copy-back of the second chunk
    ends 17 records after the seam.  CLOSEST, OCCLUDED and hits are compared with the oracle's answers on every ray (each is a draw
    from the 4097 rays of the shared reference); a radiance query depends on its key, so, as tests/test_trace_paths_gpu.py does, the keys
    around the seam, at both ends and in 40 windows elsewhere are compared with the same keys traced alone in small calls."""
    case = _ray_case(orc, "config2")
    _commit(one, "config2")
    L, ctx = one._L, one._ctx
    k = 16
    n = T.QUERY_CHUNK // 16 + 17 if entry == "hits" else T.QUERY_CHUNK + 17
    rng = np.random.default_rng(23)
    pick = rng.integers(0, N_MAX, n)
    rays = G.host((n, 8), np.float32, 16, 16)
    rays[...] = (case["prays"] if entry == "paths" else case["rays"])[pick]
    before = rays.tobytes()
    what = "%s n=%d" % (entry, n)
    if entry == "closest":
        out = [G.host((n,), RAYHIT, 16, 16)]
        _ok(one, L.hrt_trace_rays(ctx, T.QUERY_CLOSEST, rays.ctypes.data, n, out[0].ctypes.data, -1, None))
        ref = np.zeros(N_MAX, RAYHIT)
        _ok(one, L.hrt_trace_rays(ctx, T.QUERY_CLOSEST, case["rays"].ctypes.data, N_MAX, ref.ctypes.data, -1, None))
        check_closest(orc, case["arrs"], case["desc"], case["o"], case["d"], ref, what + " (4097)", max_instance_checks=0)
        assert H.canon(out[0]).tobytes() == H.canon(ref[pick]).tobytes(), what
    elif entry == "occluded":
        out = [G.host((n,), np.int32, 4, 4)]
        _ok(one, L.hrt_trace_rays(ctx, T.QUERY_OCCLUDED, rays.ctypes.data, n, out[0].ctypes.data, -1, None))
        assert (out[0] == case["occ"][pick]).all(), what
    elif entry == "hits":
        out = [G.host((n, k), RAYHIT, 16, 16), G.host((n,), np.int32, 4, 4), G.host((n,), np.int32, 4, 4)]
        _ok(one, L.hrt_trace_hits(ctx, rays.ctypes.data, n, k, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, -1, None))
        HR.assert_same(HR.unpack(out[0]), HR.unpack(case["hits"][pick]), what)
        assert (out[1] == np.minimum(case["tot"][pick], k)).all() and (out[2] == case["tot"][pick]).all(), what
    else:
        pp = T.FrameParams.from_buffer_copy(case["pp"])
        pp.width, pp.spp, pp.maxDepth = 4096, 1, 2
        out = [G.host((n,), PATHRES, 16, 16)]
        _ok(one, L.hrt_trace_paths(ctx, C.byref(pp), 0, rays.ctypes.data, n, 0, out[0].ctypes.data, -1, None))
        got = _as_frame(out[0])
        for s in (0, T.QUERY_CHUNK - 150, n - 300):
            m = min(300, n - s)
            alone = np.zeros(m, PATHRES)
            part = np.ascontiguousarray(rays[s:s + m])
            _ok(one, L.hrt_trace_paths(ctx, C.byref(pp), 0, part.ctypes.data, m, s, alone.ctypes.data, -1, None))
            same_frame({f: v[s:s + m] for f, v in got.items()}, _as_frame(alone), "%s keys at %d" % (what, s))
        for s in rng.integers(0, n - 64, 40):               # 40 more windows of 64 keys anywhere
            s = int(s)
            alone = np.zeros(64, PATHRES)
            part = np.ascontiguousarray(rays[s:s + 64])
            _ok(one, L.hrt_trace_paths(ctx, C.byref(pp), 0, part.ctypes.data, 64, s, alone.ctypes.data, -1, None))
            same_frame({f: v[s:s + 64] for f, v in got.items()}, _as_frame(alone), "%s keys at %d" % (what, s))
    assert rays.tobytes() == before, what
    G.check(rays, what + ": rays")
    for i, a in enumerate(out):
        assert G.written(a), what
        G.check(a, "%s: output %d" % (what, i))


@pytest.mark.parametrize("dev", [0, -1], ids=["device", "host"])
def test_zero_rays_write_nothing(orc, one, dev):
    case = _ray_case(orc, "config2")
    _commit(one, "config2")
    L, ctx, mem = one._L, one._ctx, _Mem(dev)
    rb, before = _rays_in(mem, case["rays"][:4])
    bufs = dict(closest=mem.new((4,), RAYHIT, 16, 16), occluded=mem.new((4,), np.int32, 16, 16), hits=mem.new((4, 3), RAYHIT, 16, 16),
                counts=mem.new((4,), np.int32, 4, 4), totals=mem.new((4,), np.int32, 4, 4), paths=mem.new((4,), PATHRES, 16, 16))
    ptr = lambda name: mem.ptr(bufs[name])
    _ok(one, L.hrt_trace_rays(ctx, T.QUERY_CLOSEST, mem.ptr(rb), 0, ptr("closest"), dev, None))
    _ok(one, L.hrt_trace_rays(ctx, T.QUERY_OCCLUDED, mem.ptr(rb), 0, ptr("occluded"), dev, None))
    _ok(one, L.hrt_trace_hits(ctx, mem.ptr(rb), 0, 3, ptr("hits"), ptr("counts"), ptr("totals"), dev, None))
    _ok(one, L.hrt_trace_paths(ctx, C.byref(case["pp"]), 0, mem.ptr(rb), 0, 0, ptr("paths"), dev, None))
    for name, a in bufs.items():
        assert G.untouched(a), name
        G.check(a, "n = 0: " + name)
    _inputs_unchanged(mem, rb, before, "n = 0")


# ====================================================================== frames
def guarded_outputs(w, h):
    """All 18 arrays of hrt_outputs, each in a guarded buffer of its own (cameraId with its one element), 4-byte aligned and no better."""
    arrs, o = {}, T.Outputs()
    for name, dt, k in T.OUTPUT_ARRAYS:
        cnt = 1 if name == "cameraId" else w * h
        arrs[name] = G.host((cnt, k) if k > 1 else (cnt,), dt, 4, 4)
        setattr(o, name, arrs[name].ctypes.data)
    return arrs, o


def check_all(arrs, what):
    for name, a in arrs.items():
        G.check(a, "%s: %s" % (what, name))


_FRAMES = {}


def _oracle(orc, name, w, h, spp=2):
    key = (name, w, h, spp)
    if key not in _FRAMES:
        _FRAMES[key] = H.oracle_frame(orc, SCENES[name][0], SCENES[name][1], w, h, spp)[0]
    return _FRAMES[key]


def _params(name, w, h, spp=2, **kw):
    return scenes.frame_params(SCENES[name][1], *H.host_funcs("hrt"), width=w, height=h, spp=spp, **kw)


def _render(r, p, o, flags=0, rows=None, strips=None):
    opts = T.RenderOpts(flags, rows[0] if rows else 0, rows[1] if rows else 0, strips[0] if strips else 1, strips[1] if strips else 0)
    _ok(r, r._L.hrt_render_frame(r._ctx, C.byref(p), C.byref(opts), C.byref(o) if o is not None else None, None))


def _tile_rows(h, rows, strips):
    if rows:
        return np.arange(rows[0], rows[1])
    if strips:
        return tiling.strip_rows(h, *strips)
    return np.arange(h)


def _check_tile(ref, arrs, w, h, inside, what):
    """Rows `inside` of every array equal the full frame's; every other row of the payload still holds 0xA5."""
    outside = np.setdiff1d(np.arange(h), inside)
    for name, a in arrs.items():
        if name == "cameraId":                         # one element, in no row: the tile that holds row 0 delivers it, the others leave it
            assert (a == ref[name]).all() if 0 in inside else G.untouched(a), "%s: cameraId" % what
            continue
        got, want = a.reshape(h, -1), ref[name].reshape(h, -1)
        assert H.bits_equal(got[inside], want[inside]).all(), "%s: %s differs inside the tile" % (what, name)
        assert (np.ascontiguousarray(got[outside]).view(np.uint8) == G.FILL).all(), "%s: %s was written outside the tile" % (what, name)


ORGS = {"auto": 0, "streamed": T.FLAG_STREAMED, "counting": T.FLAG_COUNTERS}
LAYOUTS = [((33, 9), None, None), ((1, 1), None, None), ((200, 125), None, None),
           ((200, 125), (16, 32), None), ((200, 125), (0, 1), None), ((200, 125), (124, 125), None),
           ((200, 125), None, (3, 0)), ((200, 125), None, (3, 1)), ((200, 125), None, (3, 2))]     # strip (3, 2) ends in the ragged 5-row strip


@pytest.mark.parametrize("org", list(ORGS))
@pytest.mark.parametrize("size,rows,strips", LAYOUTS, ids=lambda v: "-" if v is None else "x".join(map(str, v)))
def test_frames(orc, one, size, rows, strips, org):
    w, h = size
    name = "textured" if (w, h) != (33, 9) else "config2"
    ref = _oracle(orc, name, w, h)
    _commit(one, name)
    arrs, o = guarded_outputs(w, h)
    what = "%s %dx%d rows=%s strips=%s %s" % (name, w, h, rows, strips, org)
    _render(one, _params(name, w, h), o, ORGS[org], rows, strips)
    if rows is None and strips is None:
        H.assert_outputs_equal(ref, arrs)
        assert all(G.written(a) for a in arrs.values()), what
    else:
        _check_tile(ref, arrs, w, h, _tile_rows(h, rows, strips), what)
    check_all(arrs, what)


@pytest.mark.parametrize("slots", [2, 3])
def test_frames_gathered_from_several_slots(orc, hrt_lib, slots):
    """Each slot gathers its own 8-row strips into the same arrays (strided 2-D copies); also once into registered arrays, the
    asynchronous-DMA gather a host with pinned framebuffers gets."""
    w, h = 200, 125
    ref = _oracle(orc, "textured", w, h)
    r = engine.RTRenderer([0] * slots)
    try:
        _commit(r, "textured")
        arrs, o = guarded_outputs(w, h)
        _render(r, _params("textured", w, h), o)
        H.assert_outputs_equal(ref, arrs)
        check_all(arrs, "%d slots" % slots)
        r.reset_history()
        pinned, o2 = guarded_outputs(w, h)
        r.register_host(pinned)                            # each registration covers exactly one payload
        try:
            _render(r, _params("textured", w, h), o2)
        finally:
            r.unregister_host(pinned)
        H.assert_outputs_equal(ref, pinned)
        assert all(G.written(a) for a in pinned.values())
        check_all(pinned, "%d slots, registered" % slots)
    finally:
        r.close()


def test_frames_registered_on_one_slot(orc, one):
    w, h = 33, 9
    ref = _oracle(orc, "textured", w, h)
    _commit(one, "textured")
    arrs, o = guarded_outputs(w, h)
    one.register_host(arrs)
    try:
        _render(one, _params("textured", w, h), o)
    finally:
        one.unregister_host(arrs)
    H.assert_outputs_equal(ref, arrs)
    check_all(arrs, "registered 33x9")


def test_progressive_frames(orc, one):
    """Samples [0, 2) then [2, 5) at 33x9: after each call the outputs are the frame at that many samples."""
    w, h = 33, 9
    _commit(one, "textured")
    p = _params("textured", w, h, spp=2)
    opts = T.RenderOpts(0, 0, 0, 1, 0)
    for begin, spp in ((0, 2), (2, 5)):
        p.spp = spp
        arrs, o = guarded_outputs(w, h)
        _ok(one, one._L.hrt_render_progressive(one._ctx, C.byref(p), C.byref(opts), begin, C.byref(o), None))
        H.assert_outputs_equal(_oracle(orc, "textured", w, h, spp), arrs)
        assert all(G.written(a) for a in arrs.values())
        check_all(arrs, "progressive [%d, %d)" % (begin, spp))


def test_reuse_frames(orc, one):
    """Two frames of tests/test_parity_gpu.py::test_restir_reuse_over_frames' recipe at 64x44 (5 full strips and a ragged one), res_*
    included."""
    builder, cfg = SCENES["textured"]
    w, h, spp = 64, 44, 2
    _commit(one, "textured")
    A, B = H.new_reservoirs(w, h), H.new_reservoirs(w, h)
    for f in range(2):
        prev, cur = (B, A) if f % 2 == 0 else (A, B)
        ref, _, _ = H.oracle_frame(orc, builder, cfg, w, h, spp, frame=f, reuse=True, prev=prev, cur=cur)
        arrs, o = guarded_outputs(w, h)
        _render(one, _params("textured", w, h, spp, frame=f, reuse=True), o, T.FLAG_COUNTERS | T.FLAG_STREAMED)
        H.assert_outputs_equal(ref, arrs)
        check_all(arrs, "reuse frame %d" % f)


# ====================================================================== presentation and post
PRESENT_SIZES = [((131, 77), (66, 39)), ((257, 3), (172, 2)), ((1, 1), (1, 1)), ((64, 48), (96, 72))]     # (display, frame); the last display is smaller


_PRESENT_DENOISED = {}


@pytest.mark.parametrize("denoised", [False, True], ids=["frame", "denoised"])
@pytest.mark.parametrize("mode", [T.PRESENT_RESAMPLE, T.PRESENT_TAAU, T.PRESENT_TAAU_REPROJECT])
@pytest.mark.parametrize("display,frame", PRESENT_SIZES, ids=lambda v: "x".join(map(str, v)))
def test_present(orc, one, display, frame, mode, denoised):
    """Three panned frames per case.  The frames' arrays and their denoised colour (the inputs of the reference present) are the same
    for the six cases of a size pair and are kept; the reference present itself depends on mode and history and runs per case."""
    (ow, oh), (w, h) = display, frame
    _commit(one, "textured")
    ref = RefHistory(orc, make_taa(orc))
    pp = T.PresentParams(ow, oh, mode | (T.PRESENT_DENOISED if denoised else 0), 0.0, 0.0, 0.0)
    for f in range(3):
        p, low = render_guides(one, TEXTURED, w, h, frame=f, pan=0.06)
        if denoised:
            one.denoise()
            if (w, h, f) not in _PRESENT_DENOISED:
                _PRESENT_DENOISED[(w, h, f)] = R.denoise(low, w, h, R.make_fns(orc))[1]
            low = dict(low, color=_PRESENT_DENOISED[(w, h, f)])
        out = G.host((ow * oh,), np.int32, 4, 4)
        _ok(one, one._L.hrt_present(one._ctx, C.byref(pp), out.ctypes.data))
        want = ref.present(mode, low, p.cam, w, h, ow, oh)
        assert np.array_equal(out, want), "frame %d: %d words differ" % (f, int((out != want).sum()))
        G.check(out, "present %dx%d <- %dx%d mode %d frame %d" % (ow, oh, w, h, pp.mode, f))


def _mv_frames(r, w, h):
    p0, _ = render_guides(r, TEXTURED, w, h, frame=0, pan=0.06, names=["gb_worldPos"])
    cam0 = engine.copy_camera(p0.cam)
    p, low = render_guides(r, TEXTURED, w, h, frame=3, pan=0.06, names=["gb_worldPos"])
    return cam0, p, low


@pytest.mark.parametrize("size", [(33, 9), (200, 125)], ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("slots", [1, 3])
def test_motion_vectors_host(orc, hrt_lib, slots, size):
    w, h = size
    r = engine.RTRenderer([0] * slots)
    try:
        _commit(r, "textured")
        cam0, p, low = _mv_frames(r, w, h)
        mv = G.host((w * h, 2), np.float32, 8, 8)
        _ok(r, r._L.hrt_motion_vectors(r._ctx, C.byref(cam0), mv.ctypes.data, -1, None))
        want = make_taa(orc).motion_vectors(low["gb_worldPos"], w, h, cam0, p.cam)
        assert H.bits_equal(mv, want).all() and G.written(mv)
        G.check(mv, "motion vectors, %d slots, %dx%d" % (slots, w, h))
    finally:
        r.close()


@pytest.mark.parametrize("size", [(33, 9), (200, 125)], ids=lambda v: "x".join(map(str, v)))
def test_motion_vectors_device(orc, one, size):
    """Device path: 8-byte aligned and no better."""
    w, h = size
    _commit(one, "textured")
    cam0, p, low = _mv_frames(one, w, h)
    mv = G.device(torch, (w * h, 2), torch.float32, 8, 8)
    torch.cuda.synchronize()
    _ok(one, one._L.hrt_motion_vectors(one._ctx, C.byref(cam0), mv.data_ptr(), 0, None))
    want = make_taa(orc).motion_vectors(low["gb_worldPos"], w, h, cam0, p.cam)
    assert H.bits_equal(mv.cpu().numpy(), want).all() and G.written(mv)
    G.check(mv, "motion vectors on the device, %dx%d" % (w, h))


POINTERS = {"both": (True, True), "radiance only": (True, False), "colour only": (False, True)}
DENOISE_SIZES = [(33, 9), (200, 125), (1, 1)]
_DENOISED = {}


def _denoise_out(w, h, which):
    rad = G.host((w * h, 3), np.float32, 4, 4) if which[0] else None
    col = G.host((w * h,), np.int32, 4, 4) if which[1] else None
    return rad, col


def _check_denoised(rad, col, want_rad, want_col, what):
    if rad is not None:
        assert H.bits_equal(rad, want_rad).all(), "%s: radiance differs" % what
        G.check(rad, what + ": radiance")
    if col is not None:
        assert np.array_equal(col, want_col), "%s: colour differs" % what
        G.check(col, what + ": colour")


@pytest.mark.parametrize("pointers", list(POINTERS))
@pytest.mark.parametrize("size", DENOISE_SIZES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("slots", [1, 3])
def test_denoise(orc, hrt_lib, slots, size, pointers):
    w, h = size
    r = engine.RTRenderer([0] * slots)
    try:
        _commit(r, "textured")
        _, low = render_guides(r, TEXTURED, w, h)
        if size not in _DENOISED:                          # a frame is the same bits on any number of slots (tests/test_multidevice_gpu.py)
            _DENOISED[size] = R.denoise(low, w, h, R.make_fns(orc))
        rad, col = _denoise_out(w, h, POINTERS[pointers])
        dp = T.DenoiseParams(0, 0, 0.0, 0.0, 0.0)
        _ok(r, r._L.hrt_denoise(r._ctx, C.byref(dp), rad.ctypes.data if rad is not None else None, col.ctypes.data if col is not None else None, None))
        _check_denoised(rad, col, *_DENOISED[size], "denoise %dx%d, %d slots, %s" % (w, h, slots, pointers))
    finally:
        r.close()


_TEMPORAL = {}


def _temporal_reference(orc, r, size):
    """Per size, once: the restatement's outputs after each of three panned frames, and its history after the third."""
    w, h = size
    if size not in _TEMPORAL:
        ref = DT.Temporal(DT.make_fns(orc))
        steps = []
        for f in range(3):
            p, low = render_guides(r, TEXTURED, w, h, frame=f, pan=0.04)
            steps.append(ref.step(low, w, h, p.cam))
        _TEMPORAL[size] = (steps, ref.history())
        r.reset_history()
    return _TEMPORAL[size]


@pytest.mark.parametrize("pointers", list(POINTERS))
@pytest.mark.parametrize("size", DENOISE_SIZES, ids=lambda v: "x".join(map(str, v)))
@pytest.mark.parametrize("slots", [1, 3])
def test_denoise_temporal_and_history_read(orc, hrt_lib, slots, size, pointers):
    """hrt_denoise_temporal over three panned frames, then hrt_denoise_history_read with the same choice of pointers."""
    w, h = size
    r = engine.RTRenderer([0] * slots)
    try:
        _commit(r, "textured")
        steps, hist = _temporal_reference(orc, r, size)
        tp = T.DenoiseTemporalParams()
        for f in range(3):
            render_guides(r, TEXTURED, w, h, frame=f, pan=0.04)
            rad, col = _denoise_out(w, h, POINTERS[pointers])
            _ok(r, r._L.hrt_denoise_temporal(r._ctx, C.byref(tp), rad.ctypes.data if rad is not None else None,
                                              col.ctypes.data if col is not None else None, None))
            _check_denoised(rad, col, *steps[f], "temporal %dx%d, %d slots, %s, frame %d" % (w, h, slots, pointers, f))
        hc = G.host((w * h, 4), np.float32, 4, 4) if POINTERS[pointers][0] else None
        hm = G.host((w * h, 4), np.float32, 4, 4) if POINTERS[pointers][1] else None
        _ok(r, r._L.hrt_denoise_history_read(r._ctx, hc.ctypes.data if hc is not None else None, hm.ctypes.data if hm is not None else None))
        same = lambda a, b: H.bits_equal(np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)).all()
        if hc is not None:
            assert same(hc[:, :3], hist["color"]) and same(hc[:, 3], hist["variance"]) and G.written(hc)
            G.check(hc, "history colour")
        if hm is not None:
            assert same(hm[:, :2], hist["moments"]) and same(hm[:, 2], hist["length"]) and (hm[:, 3] == 0).all() and G.written(hm)
            G.check(hm, "history moments")
    finally:
        r.close()


# ====================================================================== read-backs with a capacity
def _uploaded(orc, name):
    so = orc.OrcScene()
    SCENES[name][0](so)
    return so.arrays()


@pytest.mark.parametrize("array", range(15), ids=[n for n, _ in T.SCENE_ARRAYS])
def test_scene_download_array(orc, one, array):
    name, t = T.SCENE_ARRAYS[array]
    arrs = _uploaded(orc, "textured")
    desc, keep = T.scene_desc_from_arrays(arrs)
    one.commit(desc)
    L, ctx, dt = one._L, one._ctx, T.np_dtype(t)
    want = one.download_array(name)
    count = len(want)
    if array >= 3:
        assert count == len(arrs[name]) and want.tobytes() == arrs[name].tobytes()      # what was uploaded
    assert count >= 1
    for cap in (count, count + 1000):
        dst, cnt = G.host((cap,), dt, 4, 4), C.c_int64(-1)
        _ok(one, L.hrt_scene_download_array(ctx, 0, array, dst.ctypes.data, cap, C.byref(cnt)))
        assert cnt.value == count and dst[:count].tobytes() == want.tobytes()
        assert (np.ascontiguousarray(dst[count:]).view(np.uint8) == G.FILL).all(), "elements past count were written"
        G.check(dst, "%s cap=%d" % (name, cap))
    dst = G.host((count,), dt, 4, 4)                          # room for count, told count - 1
    assert L.hrt_scene_download_array(ctx, 0, array, dst.ctypes.data, count - 1, None) == INVALID_ARG
    assert G.untouched(dst)
    G.check(dst, "%s cap=count-1" % name)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["tlasNodes", "tlasInstanceIndices", "instances"])
def test_scene_download_tlas(orc, one, which):
    _commit(one, "textured")
    L, ctx = one._L, one._ctx
    nodes, idx, inst, cnt = one.download_tlas()
    want = [bytes(nodes)[:cnt[0] * 44], bytes(idx)[:cnt[1] * 4], bytes(inst)[:cnt[2] * 144]][which]
    dt = [T.np_dtype(T.BvhNode), np.dtype(np.int32), T.np_dtype(T.InstanceRecord)][which]
    count = cnt[which]
    assert count >= 1

    def call(dst, cap):
        a = [None, 0, None, 0, None, 0]
        a[2 * which], a[2 * which + 1] = dst.ctypes.data, cap
        counts = (C.c_int64 * 3)()
        return L.hrt_scene_download_tlas(ctx, 0, *a, counts), tuple(counts)

    for cap in (count, count + 1000):
        dst = G.host((cap,), dt, 4, 4)
        rc, counts = call(dst, cap)
        assert rc == OK and counts == tuple(cnt) and dst[:count].tobytes() == want
        assert (np.ascontiguousarray(dst[count:]).view(np.uint8) == G.FILL).all()
        G.check(dst, "tlas array %d cap=%d" % (which, cap))
    dst = G.host((count,), dt, 4, 4)
    assert call(dst, count - 1)[0] == INVALID_ARG and G.untouched(dst)
    G.check(dst, "tlas array %d cap=count-1" % which)


def test_frame_times(one):
    _commit(one, "config2")
    p = _params("config2", 64, 40)
    for _ in range(5):
        _render(one, p, None, T.FLAG_NO_SYNC)
    assert one.synchronize().frames == 5
    for launch in (0, 1):
        want = one.frame_times(launch)
        assert len(want) == 5 and (want > 0).all()
        for cap in (0, 2, 5, 9):
            ms, n = G.host((9,), np.float32, 4, 4), C.c_int(-1)
            _ok(one, one._L.hrt_frame_times(one._ctx, 0, launch, ms.ctypes.data, cap, C.byref(n)))
            m = min(cap, 5)
            assert n.value == 5 and (ms[:m] == want[:m]).all()
            assert (np.ascontiguousarray(ms[m:]).view(np.uint8) == G.FILL).all(), "more than min(cap, 5) floats changed"
            G.check(ms, "frame times cap=%d" % cap)


# ====================================================================== inputs are inputs
def _guarded_copy(a, align=4):
    a = np.ascontiguousarray(a)
    g = G.host(a.shape, a.dtype, align, align)
    g[...] = a
    return g


def _frame_matches_oracle_on_device_scene(orc, r, cfg, what):
    """A small frame on the scene as it is on the device now equals the oracle's on the downloaded arrays (tests/test_bvh_update_gpu.py)."""
    desc, keep = T.scene_desc_from_arrays(_device_arrays(r, None))
    w, h = 48, 30
    p = scenes.frame_params(cfg, *H.host_funcs("hrt"), width=w, height=h, spp=1)
    ref, oo = T.alloc_outputs(w, h)
    orc.render_frame(desc, p, oo, None)
    r.reset_history()
    got, og = T.alloc_outputs(w, h)
    _render(r, p, og)
    H.assert_outputs_equal(ref, got, names=[n for n in ref if not n.startswith("res_")])


def test_scene_upload_leaves_its_arrays_alone(orc, one):
    arrs = _uploaded(orc, "textured")
    guarded = {name: _guarded_copy(a) for name, a in arrs.items() if len(a)}
    d = T.SceneDesc()
    for name, t in T.SCENE_ARRAYS:
        if name in guarded:
            setattr(d, name, C.cast(guarded[name].ctypes.data, C.POINTER(t)))
            setattr(d, "n_" + name, len(guarded[name]))
    _ok(one, one._L.hrt_scene_upload(one._ctx, C.byref(d)))
    _frame_matches_oracle_on_device_scene(orc, one, TEXTURED, "upload")
    for name, g in guarded.items():
        assert g.tobytes() == arrs[name].tobytes(), name
        G.check(g, "hrt_scene_upload: " + name)


def test_scene_updates_leave_their_arrays_alone(orc, one):
    """hrt_scene_update_instances and _spheres on tests/test_bvh_update_gpu.py's smallest scene (60 one-sphere instances), _positions
    on the textured scene's mesh."""
    from tests.test_bvh_update_gpu import _spheres, _moves, CFG_SPH
    L, ctx = one._L, one._ctx
    s = engine.Scene(); _spheres(s); one.commit(s)
    ids_l, xfs = _moves(len(s.arrays()["instances"]), "translate")
    xf = np.array([[getattr(a, "m%d%d" % (i, j)) for i in range(3) for j in range(4)] for a in xfs], np.float32)
    ids, xfg = _guarded_copy(np.array(ids_l, np.int32)), _guarded_copy(xf)
    _ok(one, L.hrt_scene_update_instances(ctx, ids.ctypes.data, len(ids), xfg.ctypes.data, T.REBUILD_FORCE_REFIT, None))
    inst = one.download_array("instances")
    o2w = np.stack([inst["objectToWorld"]["m%d%d" % (i, j)] for i in range(3) for j in range(4)], 1)
    assert H.bits_equal(o2w[ids_l], xf).all()
    _frame_matches_oracle_on_device_scene(orc, one, CFG_SPH, "update_instances")
    assert ids.tobytes() == np.array(ids_l, np.int32).tobytes() and xfg.tobytes() == xf.tobytes()
    G.check(ids, "instance ids"); G.check(xfg, "transforms")

    sp = np.array(one.download_array("spheres"), copy=True)[3:40]
    sp["center"]["Y"] += f32(0.25)
    sp["radius"] *= f32(0.9)
    spg = _guarded_copy(sp)
    _ok(one, L.hrt_scene_update_spheres(ctx, 3, len(spg), spg.ctypes.data, T.REBUILD_AUTO, None))
    assert one.download_array("spheres")[3:40].tobytes() == sp.tobytes()
    _frame_matches_oracle_on_device_scene(orc, one, CFG_SPH, "update_spheres")
    assert spg.tobytes() == sp.tobytes()
    G.check(spg, "spheres")

    _commit(one, "textured")
    pos = np.array(one.download_array("meshPositions"), copy=True)
    pos = np.stack([pos[a] for a in "XYZ"], 1).astype(np.float32)[1:]
    pos[:, 1] += f32(0.03)
    pg = _guarded_copy(pos)
    _ok(one, L.hrt_scene_update_positions(ctx, 1, len(pg), pg.ctypes.data, T.REBUILD_AUTO, None))
    now = one.download_array("meshPositions")
    assert np.stack([now[a] for a in "XYZ"], 1)[1:].tobytes() == pos.tobytes()
    _frame_matches_oracle_on_device_scene(orc, one, TEXTURED, "update_positions")
    assert pg.tobytes() == pos.tobytes()
    G.check(pg, "positions")


# ====================================================================== the library's own planes on the device
_PLANES = [("color", np.int32, 1), ("radiance", np.float32, 3), ("gb_worldPos", np.float32, 3), ("gb_normalWS", np.float32, 3),
           ("gb_baseColor", np.float32, 3), ("gb_matId", np.int32, 1), ("gb_objId", np.int32, 1), ("gb_hitMask", np.int32, 1)]


def _plane_tensors(views):
    """{output name: uint8 torch tensor [H, W * bytes per pixel]} over the planes of hrt_device_views a launch writes: colour, radiance,
    the six G-buffer planes and resCur of frame 0 (set A).  The exchanged ones come from tiling.device_tensors."""
    h, w = views.height, views.width
    out = {}
    for (name, _, _), t in zip(tiling.GBUFFER_EXCHANGE, tiling.device_tensors(views, "gbuffer")):
        out[name] = t
    for (name, _, _), t in zip(tiling.RESERVOIR_FIELDS, tiling.device_tensors(views, "reservoir", 0)):
        out["res_" + name] = t
    for name, dt, k in _PLANES:
        if name not in out:
            out[name] = torch.as_tensor(tiling._DeviceArray(getattr(views, name), (h, w * k), dt), device="cuda")
    return {name: t.view(torch.uint8) for name, t in out.items()}


def test_a_tile_leaves_the_other_rows_of_the_device_planes_alone(orc, one):
    """The exchange protocol of tests/test_exchange_gpu.py rests on a rank's launches leaving alone the rows other ranks all-gathered
    into its planes.  200x125, strips (3, 1): every plane is filled with 0xA5, the tile is rendered, every row outside the owned strips
    is unchanged and every row inside equals the full frame.
    resCur is written only where a path reaches a diffuse vertex (RTRay.cs:417 onwards; tests/test_parity_gpu.py): a pixel inside the
    tile that the full frame leaves at its initial zero may still hold the fill here."""
    w, h = 200, 125
    ref = _oracle(orc, "textured", w, h)
    _commit(one, "textured")
    p = _params("textured", w, h)
    _render(one, p, None)                                   # allocates the planes at this size
    one.reset_history()
    planes = _plane_tensors(one.device_views(0))
    for t in planes.values():
        t.fill_(G.FILL)
    torch.cuda.synchronize()
    _render(one, p, None, 0, None, (3, 1))
    torch.cuda.synchronize()
    inside = tiling.strip_rows(h, 3, 1)
    outside = np.setdiff1d(np.arange(h), inside)
    assert set(planes) == {n for n, _, _ in T.OUTPUT_ARRAYS} - {"depth", "objectId", "cameraId"}
    for name, t in planes.items():
        got = t.cpu().numpy()
        assert (got[outside] == G.FILL).all(), "%s: rows outside the tile changed" % name
        want = np.ascontiguousarray(ref[name]).view(np.uint8).reshape(h, -1)
        g4, w4 = np.ascontiguousarray(got[inside]).view(np.uint32), np.ascontiguousarray(want[inside]).view(np.uint32)
        ok = g4 == w4
        if name.startswith("res_"):
            ok |= (g4 == G.FILL_WORD) & (w4 == 0)
        elif ref[name].dtype == np.float32:
            f = lambda a: a.view(np.float32)
            ok |= np.isnan(f(g4)) & np.isnan(f(w4))
        assert ok.all(), "%s: %d words inside the tile differ from the full frame" % (name, int((~ok).sum()))
