"""Multi-hit ray queries (hrt_trace_hits) on the GPU: bit for bit over all eight fields, counts and totals against the CPU
restatement tests/hits_ref.py (packed walker, TracerRef, the non-finite fix-up), against CLOSEST / OCCLUDED at full size, across
devices, chunk edges, frame state and errors."""
import ctypes as C

import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, engine, scenes
from tests import helpers as H
from tests import hits_ref as HR
from tests.test_ray_query_gpu import (_oracle_scene, _commit, _params, _camera_rays, _ray_sets, _tmax_mix, _big_leaf_scene,
                                      _device_arrays, _aff, _unpack)

pytestmark = pytest.mark.gpu
f32 = np.float32


def _check_against_ref(orc, renderer, arrs, desc, p, n, seed, what, ks=(1, 3, 16)):
    V = HR.views(orc, arrs)
    rng = np.random.default_rng(seed)
    for rs, o, d in _ray_sets(orc, arrs, desc, p, n, seed=seed):
        tm = _tmax_mix(rng, len(o))
        tm[: len(o) // 4] = np.inf                           # a quarter without a limit, as picking casts
        ref, rcnt, rtot = HR.trace_hits(V, o, d, 16, tm)
        for k in ks:
            want = {f: a[:, :k] for f, a in HR.unpack(ref).items()}
            h0, c0, t0 = renderer.trace_hits(o, d, k, tm)
            h1, c1, t1 = renderer.trace_hits(o, d, k, tm, totals=True)
            assert t0 is None and t1.dtype == np.int32
            tag = "%s/%s/k=%d" % (what, rs, k)
            HR.assert_same(HR.unpack(h0), want, tag + "/no-totals")
            HR.assert_same(HR.unpack(h1), want, tag + "/totals")
            assert (c0 == np.minimum(rtot, k)).all() and (c1 == c0).all(), tag
            assert (t1 == rtot).all(), tag


SCENES = [
    ("default", lambda b: b.build_default_scene(), scenes.Config("d", 0, 0, 0, (0.0, 1.4, 4.5), (0.0, 0.5, 0.0)), 160),
    ("config1", scenes.build_config1, scenes.CONFIGS[1], 160),
    ("config2", scenes.build_config2, scenes.CONFIGS[2], 160),
    ("textured", scenes.build_textured_test_scene, scenes.Config("t", 0, 0, 0, (0.0, 1.2, 4.0), (0.0, 0.6, 0.0)), 160),
    ("rotated", scenes.build_rotated_instances_scene, scenes.Config("r", 0, 0, 0, (0.0, 1.5, 5.0), (0.0, 0.8, 0.0)), 160),
    ("config4_small", lambda b: scenes.build_config4(b, nu=48, nv=48), scenes.CONFIGS[4], 100),
    ("config5_small", lambda b: scenes.build_config5(b, n=96), scenes.CONFIGS[5], 100),
]


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("name,builder,cfg,n", SCENES, ids=[s[0] for s in SCENES])
def test_matches_restatement(orc, renderer, name, builder, cfg, n):
    arrs = _oracle_scene(orc, builder)
    desc, keep = _commit(renderer, arrs)
    _check_against_ref(orc, renderer, arrs, desc, _params(cfg, 160, 90), n, len(name), name)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("leaf_size", [15, 20])
def test_reference_layout_scenes(orc, renderer, leaf_size):
    arrs = _big_leaf_scene(orc, leaf_size)
    desc, keep = _commit(renderer, arrs)
    p = _params(scenes.Config("big", 0, 0, 0, (0.0, 2.5, 8.0), (0.0, 0.7, 0.0)), 160, 90)
    _check_against_ref(orc, renderer, arrs, desc, p, 160, 5, "big%d" % leaf_size)


# ------------------------------------------------------------------ after scene updates: the arrays now on the device
def _update_check(orc, renderer, arrs, cfg, what):
    a = _device_arrays(renderer, arrs)
    desc, keep = T.scene_desc_from_arrays(a)
    _check_against_ref(orc, renderer, a, desc, _params(cfg, 160, 90), 80, 9, what, ks=(3, 16))


@pytest.mark.timeout(900)
@pytest.mark.parametrize("policy", [T.REBUILD_FORCE_REFIT, T.REBUILD_FORCE_REBUILD])
def test_after_instance_updates(orc, renderer, policy):
    arrs = _oracle_scene(orc, scenes.build_rotated_instances_scene)
    _commit(renderer, arrs)
    n = len(arrs["instances"])
    ids = np.arange(0, n, 2, dtype=np.int32)
    xf = np.array([_aff(arrs["instances"][i]["objectToWorld"]) for i in ids], np.float32)
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
    arrs = _oracle_scene(orc, lambda b: scenes.build_config4(b, nu=48, nv=48))
    _commit(renderer, arrs)
    pos = np.stack([arrs["meshPositions"][a] for a in "XYZ"], 1).astype(np.float32)
    pos[:, 1] += np.float32(0.05) * np.sin(np.float32(3.0) * pos[:, 0]).astype(np.float32)
    renderer.update_positions(0, pos, policy)
    _update_check(orc, renderer, arrs, scenes.CONFIGS[4], "positions%d" % policy)


# ------------------------------------------------------------------ full size: GPU against GPU
def _plain_instances(arrs):
    """No rotated, scaled or alpha-mapped instance: the identities with CLOSEST and OCCLUDED below rest on that."""
    for r in arrs["instances"]:
        m = _aff(r["objectToWorld"])
        if m[0] != 1 or m[5] != 1 or m[10] != 1 or m[1] != 0 or m[2] != 0 or m[4] != 0 or m[6] != 0 or m[8] != 0 or m[9] != 0:
            return False
        if not (r["uniformScale"] <= 0 or r["uniformScale"] == 1):
            return False
    return not (len(arrs["materials"]) and (arrs["materials"]["HasAlphaMap"] != 0).any())


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("cfg_id", [2, 3, 4, 5])
def test_full_size_against_closest_and_occluded(orc, renderer, cfg_id):
    arrs = _oracle_scene(orc, lambda b: scenes.build(cfg_id, b))
    assert _plain_instances(arrs)
    desc, keep = _commit(renderer, arrs)
    w, h = 1920, 1080
    p = _params(scenes.CONFIGS[cfg_id], w, h)
    o, d = _camera_rays(p, np.arange(w * h))
    hits, cnt, tot = renderer.trace_hits(o, d, 2, totals=True)
    g = HR.unpack(hits)
    cl = _unpack(renderer.trace_rays(o, d))
    sel = (g["t"][:, 1] != g["t"][:, 0]) & (g["t"][:, 0] < f32(1e29))
    first = {f: a[:, 0] for f, a in g.items()}
    same = np.ones(w * h, bool)
    for f in HR.FIELDS:
        eq = HR.bits(first[f]) == HR.bits(cl[f])
        same &= eq.all(axis=-1) if eq.ndim > 1 else eq
    # CLOSEST prunes its box tests at the closest t so far, and a primitive's computed t can lie a rounding error below its box's
    # computed slab entry: then CLOSEST skips a nearer accepted test the unpruned walk records.  Such rays must be
    # rare, the restatement must confirm the GPU's records, and its first t must be below CLOSEST's.
    odd = np.flatnonzero(sel & ~same)
    assert len(odd) <= max(2, (w * h) // 100000), "config %d: hits[0] differs from CLOSEST at %d rays" % (cfg_id, len(odd))
    if len(odd):
        ref, rc, rt = HR.trace_hits(HR.views(orc, arrs), o[odd], d[odd], 2, np.float32(np.inf))
        HR.assert_same({f: a[odd] for f, a in g.items()}, HR.unpack(ref), "config %d: rays where CLOSEST differs" % cfg_id)
        assert (g["t"][odd, 0] < cl["t"][odd]).all()
    assert ((g["t"][:, 0] < f32(1e29)) == (cl["t"] < f32(1e29))).all()
    occ = renderer.trace_rays(o, d, np.float32(np.inf), query="occluded")
    assert ((tot > 0).astype(np.int32) == occ).all()
    assert (cnt == np.minimum(tot, 2)).all()
    h2, c2, _ = renderer.trace_hits(o, d, 2)
    HR.assert_same(HR.unpack(h2), g, "config %d totals off" % cfg_id)
    assert (c2 == cnt).all()
    if cfg_id == 4:
        rng = np.random.default_rng(4)
        sub = rng.choice(w * h, 300, replace=False)
        ref, rc, rt = HR.trace_hits(HR.views(orc, arrs), o[sub], d[sub], 2, np.float32(np.inf))
        HR.assert_same({f: a[sub] for f, a in g.items()}, HR.unpack(ref), "config 4 vs restatement")
        assert (rt == tot[sub]).all() and (rc == cnt[sub]).all()


# ------------------------------------------------------------------ devices and chunking
DEVICE_WORKER = r'''
import sys
sys.path.insert(0, %(root)r)
import torch
import numpy as np
from ilgpu_raytracing_amd import _types as T, engine, scenes
from oracle import orc
from tests import hits_ref as HR
from tests.test_ray_query_gpu import _oracle_scene, _commit, _params, _ray_sets, _tmax_mix

orc.build()
torch.cuda.set_device(0)
r = engine.RTRenderer([0])
arrs = _oracle_scene(orc, lambda b: scenes.build_config4(b, nu=48, nv=48))
desc, keep = _commit(r, arrs)
p = _params(scenes.CONFIGS[4], 320, 180)
rng = np.random.default_rng(3)
for what, o, d in _ray_sets(orc, arrs, desc, p, 5000, seed=1):
    tm = _tmax_mix(rng, len(o))
    for k in (1, 5, 16):
        hh, hc, ht = r.trace_hits(o, d, k, tm, totals=True)
        dh = r.trace_hits(torch.from_numpy(o).cuda(0), torch.from_numpy(d).cuda(0), k, torch.from_numpy(tm).cuda(0), totals=True)
        assert dh["t"].device.type == "cuda" and dh["t"].shape == (len(o), k) and dh["normal"].shape == (len(o), k, 3)
        got = {f: dh[f].cpu().numpy() for f in HR.FIELDS}
        HR.assert_same(got, HR.unpack(hh), "%%s k=%%d" %% (what, k))
        assert (dh["counts"].cpu().numpy() == hc).all() and (dh["totals"].cpu().numpy() == ht).all()
        d0 = r.trace_hits(torch.from_numpy(o).cuda(0), torch.from_numpy(d).cuda(0), k, torch.from_numpy(tm).cuda(0))
        assert d0["totals"] is None and (d0["counts"].cpu().numpy() == hc).all()
L, ctx = r._L, r._ctx
rays = torch.zeros((4, 8), dtype=torch.float32, device="cuda:0")
hits = torch.zeros((4 * 2, 12), dtype=torch.float32, device="cuda:0")
cnt = torch.zeros(4, dtype=torch.int32, device="cuda:0")
assert L.hrt_trace_hits(ctx, rays.data_ptr(), 4, 2, hits.data_ptr(), cnt.data_ptr(), None, 0, None) == 0
assert L.hrt_trace_hits(ctx, rays.data_ptr() + 4, 3, 2, hits.data_ptr(), cnt.data_ptr(), None, 0, None) == -1     # misaligned rays
assert L.hrt_trace_hits(ctx, rays.data_ptr(), 4, 2, hits.data_ptr() + 8, cnt.data_ptr(), None, 0, None) == -1     # misaligned hits
assert L.hrt_trace_hits(ctx, rays.data_ptr(), 4, 2, hits.data_ptr(), cnt.data_ptr(), None, -1, None) == -1        # device memory, host path
r.close()
print("DEVICE_PATH_OK")
'''


@pytest.mark.timeout(600)
def test_device_pointers_equal_host_pointers(tmp_path):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "hits_device_worker.py"
    script.write_text(DEVICE_WORKER % {"root": root})
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=540, cwd=root)
    assert out.returncode == 0 and "DEVICE_PATH_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def _same(a, b, what):
    HR.assert_same(HR.unpack(a[0]), HR.unpack(b[0]), what)
    assert (a[1] == b[1]).all(), what
    assert (a[2] is None and b[2] is None) or (a[2] == b[2]).all(), what


@pytest.mark.timeout(900)
def test_two_slots_equal_one_and_chunk_edges(orc, renderer):
    arrs = _oracle_scene(orc, scenes.build_config2)
    desc, keep = _commit(renderer, arrs)
    two = engine.RTRenderer([0, 0])
    try:
        two.commit(desc)
        p = _params(scenes.CONFIGS[2], 1920, 1200)
        rng = np.random.default_rng(5)
        per = T.QUERY_CHUNK // 16                       # rays per chunk at k = 16
        for n in (1, 65, per - 1, per, per + 1, 2 * per + 3):
            idx = rng.integers(0, p.width * p.height, n)
            o, d = _camera_rays(p, idx)
            d[::3] = rng.standard_normal((len(d[::3]), 3)).astype(np.float32)
            tm = _tmax_mix(rng, n)
            a = renderer.trace_hits(o, d, 16, tm, totals=True)
            _same(a, two.trace_hits(o, d, 16, tm, totals=True), "two slots n=%d" % n)
            sub = np.unique(np.concatenate([rng.choice(n, min(n, 200), replace=False), [0, n - 1], [x for x in (per - 1, per) if x < n]]).astype(np.int64))
            _same(tuple(x[sub] for x in a), renderer.trace_hits(o[sub], d[sub], 16, tm[sub], totals=True), "chunk edges n=%d" % n)
            if n <= 65:
                ref, rc, rt = HR.trace_hits(HR.views(orc, arrs), o, d, 16, tm)
                HR.assert_same(HR.unpack(a[0]), HR.unpack(ref), "n=%d vs restatement" % n)
                assert (a[1] == rc).all() and (a[2] == rt).all()
        e = two.trace_hits(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 4)
        assert e[0].shape == (0, 4) and e[1].shape == (0,)
    finally:
        two.close()


# ------------------------------------------------------------------ frame state untouched
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
            renderer.trace_hits(o, d, 4, tm, totals=True)
            renderer.trace_hits(o, d, 16)
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

    alone = renderer.trace_hits(o, d, 4, tm, totals=True)
    renderer.reset_history()
    p = scenes.frame_params(cfg, *H.host_funcs("hrt"), width=w, height=h, spp=2)
    for _ in range(3):
        renderer.render_params(p, None, flags=T.FLAG_NO_SYNC)
    q = renderer.trace_hits(o, d, 4, tm, totals=True)
    st = renderer.synchronize()
    assert st.frames == 3 and len(renderer.frame_times(1)) == 3
    _same(q, alone, "no-sync")


@pytest.mark.timeout(600)
def test_progressive_continuation_unaffected(orc, renderer):
    arrs = _oracle_scene(orc, scenes.build_config2)
    _commit(renderer, arrs)
    w, h = 96, 64
    p2, p4 = (scenes.frame_params(scenes.CONFIGS[2], *H.host_funcs("hrt"), width=w, height=h, spp=s) for s in (2, 4))
    o, d = _camera_rays(p4, np.arange(0, w * h, 7))

    def run(with_query):
        renderer.reset_history()
        a, og = T.alloc_outputs(w, h)
        renderer.render_progressive(p2, 0, og)
        if with_query:
            renderer.trace_hits(o, d, 3, totals=True)
        b, og2 = T.alloc_outputs(w, h)
        renderer.render_progressive(p4, 2, og2)
        return b

    ref, got = run(False), run(True)
    for k in ref:
        assert H.bits_equal(ref[k], got[k]).all(), k


# ------------------------------------------------------------------ error codes
def test_error_codes(renderer, hrt_lib):
    L = hrt_lib
    ray = (T.Ray * 4)()
    hits = (T.RayHit * 64)()
    cnt = (C.c_int32 * 4)()
    tot = (C.c_int32 * 4)()
    ms = C.c_float(-1.0)
    assert L.hrt_trace_hits(None, ray, 4, 2, hits, cnt, tot, -1, None) == -1
    fresh = engine.RTRenderer([0])
    try:
        ctx = fresh._ctx
        assert L.hrt_trace_hits(ctx, ray, 4, 2, hits, cnt, tot, -1, None) == -2          # no scene uploaded
        assert L.hrt_trace_hits(ctx, ray, 0, 2, hits, cnt, tot, -1, C.byref(ms)) == 0 and ms.value == 0.0
    finally:
        fresh.close()
    s = engine.Scene()
    s.build_default_scene()
    renderer.commit(s)
    ctx = renderer._ctx
    for k in (0, -1, T.HITS_MAX + 1, 1 << 30):
        assert L.hrt_trace_hits(ctx, ray, 4, k, hits, cnt, tot, -1, None) == -1, k
    assert L.hrt_trace_hits(ctx, ray, -1, 2, hits, cnt, tot, -1, None) == -1            # n < 0
    assert L.hrt_trace_hits(ctx, None, 4, 2, hits, cnt, tot, -1, None) == -1            # NULL rays
    assert L.hrt_trace_hits(ctx, ray, 4, 2, None, cnt, tot, -1, None) == -1             # NULL hits
    assert L.hrt_trace_hits(ctx, ray, 4, 2, hits, None, tot, -1, None) == -1            # NULL counts
    assert L.hrt_trace_hits(ctx, ray, 4, 2, hits, cnt, tot, 1, None) == -1              # slot out of range
    assert L.hrt_trace_hits(ctx, ray, 4, 2, hits, cnt, tot, 0, None) == -1              # dev >= 0 with host memory
    assert L.hrt_trace_hits(ctx, None, 0, 2, None, None, None, -1, None) == 0           # n == 0: nothing to do
    assert L.hrt_trace_hits(ctx, ray, 4, 16, hits, cnt, None, -1, C.byref(ms)) == 0 and ms.value >= 0.0
    assert L.hrt_trace_hits(ctx, ray, 4, 16, hits, cnt, tot, -1, None) == 0
