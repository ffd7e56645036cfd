"""Progressive frames (hrt_render_progressive) on the GPU: a frame rendered as samples [0, k1), [k1, k2), ... is after every call,
in every output array bit for bit, the frame hrt_render_frame gives at the running spp -- rendered here on a second context (or
taken from the CPU oracle / the committed full-size strips).  Every kernel organisation the library picks is covered (fused kernel,
fused kernel in sample groups, streamed pipeline over one and over many sample batches, reference layout, treelet walker), reuse
frames at the operating point on one and on two device slots, enqueued (NO_SYNC) chains, and the state rules of a continuation."""
import ctypes as C
import os

import numpy as np
import pytest
import torch          # before libhip_raytrace.so is loaded: torch brings its own HIP runtime of the same soname

from ilgpu_raytracing_amd import _types as T, engine, scenes, tiling
from tests import helpers as H
from tests.golden import make_golden as G

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
INVALID_STATE = -2


def _default_scene(b):
    b.build_default_scene()


DEFAULT = scenes.Config("default", 0, 0, 0, (0.0, 1.4, 4.5), (0.0, 0.5, 0.0))
TEXTURED = scenes.Config("textured", 0, 0, 0, (0.3, 1.3, 4.2), (0.0, 0.7, 0.0))
BUILDERS = {
    "default": (_default_scene, DEFAULT),
    "config1": (scenes.build_config1, scenes.CONFIGS[1]),
    "config2": (scenes.build_config2, scenes.CONFIGS[2]),
    "config3": (scenes.build_config3, scenes.CONFIGS[3]),                        # 10 001 sphere instances
    "config4": (scenes.build_config4, scenes.CONFIGS[4]),
    "config5": (scenes.build_config5, scenes.CONFIGS[5]),
    "textured": (scenes.build_textured_test_scene, TEXTURED),                    # alpha cut-outs
    "rotated": (scenes.build_rotated_instances_scene, scenes.CONFIGS[2]),         # general sphere instances
    "blob_64": (lambda b: scenes.build_config4(b, 64, 64), scenes.CONFIGS[4]),     # a triangle mesh
}
_SCENES = {}


def _commit(rs, name):
    if name not in _SCENES:
        s = engine.Scene()
        BUILDERS[name][0](s)
        _SCENES[name] = s
    for r in rs:
        r.commit(_SCENES[name])
        r.reset_history()


def _params(name, w, h, spp, frame=0, reuse=False, lock=0, prev_cam=None, cam_shift=0.0):
    cfg = BUILDERS[name][1]
    o = cfg.cam_origin
    c2 = scenes.Config(cfg.name, w, h, spp, (o[0] + cam_shift, o[1], o[2]), cfg.cam_lookat, extra=cfg.extra)
    return scenes.frame_params(c2, *H.host_funcs("hrt"), frame=frame, reuse=reuse, rng_lock_noise=lock, prev_cam=prev_cam)


def _with_spp(p, spp):
    q = T.FrameParams.from_buffer_copy(p)
    q.spp = spp
    return q


def _assert_same(ref, got, what):
    try:
        H.assert_outputs_equal(ref, got)
    except AssertionError as e:
        raise AssertionError("%s: %s" % (what, e)) from None


@pytest.fixture(scope="module")
def pair(hrt_lib):
    """(progressive ctx, one-shot ctx), one device slot each."""
    a, b = engine.RTRenderer([0]), engine.RTRenderer([0])
    yield a, b
    a.close()
    b.close()


def _check_schedule(prog, ref, p, schedule, flags=0, strips=None, what=""):
    """Progressive frame of p over `schedule` on prog; after each call every array equals the one-shot frame at that spp on ref
    (reservoir history zeroed on both first: a pixel without a winner keeps resCur as it was)."""
    prog.reset_history()
    begin = 0
    for spp in schedule:
        q = _with_spp(p, spp)
        got, o = T.alloc_outputs(p.width, p.height)
        st = prog.render_progressive(q, begin, o, flags=flags, strips=strips)
        assert st.counters_valid == 0
        ref.reset_history()
        want, o2 = T.alloc_outputs(p.width, p.height)
        ref.render_params(q, o2, flags=flags, strips=strips)
        _assert_same(want, got, "%s: samples [%d, %d)" % (what, begin, spp))
        begin = spp


# ------------------------------------------------------------------ 1. organisations x scenes
ORGS = {"auto": 0, "megakernel": T.FLAG_MEGAKERNEL, "streamed": T.FLAG_STREAMED,
        "megakernel_reflayout": T.FLAG_MEGAKERNEL | T.FLAG_REFERENCE_LAYOUT, "streamed_reflayout": T.FLAG_STREAMED | T.FLAG_REFERENCE_LAYOUT}


@pytest.mark.parametrize("org", list(ORGS))
@pytest.mark.parametrize("name", ["default", "config1", "config2", "textured", "rotated", "blob_64", "config3"])
def test_organisations(pair, name, org):
    w, h = 160, 96
    _commit(pair, name)
    _check_schedule(*pair, _params(name, w, h, 16, lock=7), (1, 2, 5, 16), ORGS[org], what="%s %s" % (name, org))


@pytest.mark.parametrize("name", ["config2", "blob_64"])
def test_streamed_many_batches(pair, name):
    """The path workspace capped at one sample of the frame: every call runs as one batch per sample (calls of 1, 3 and 11)."""
    w, h = 160, 96
    _commit(pair, name)
    n_ord = ((w + 7) // 8) * ((h + 7) // 8) * 64
    for r in pair:
        r.set_workspace_limit(n_ord + 5)
    try:
        _check_schedule(*pair, _params(name, w, h, 16), (1, 4, 15), T.FLAG_STREAMED, what="%s one-sample batches" % name)
        _check_schedule(*pair, _params(name, w, h, 16), (2, 9), T.FLAG_STREAMED | T.FLAG_REFERENCE_LAYOUT, what="%s one-sample batches, reference layout" % name)
    finally:
        for r in pair:
            r.set_workspace_limit(0)


def test_split_form(pair):
    """Config 2 at 1920 x 1080 as 8 interleaved strip tiles: a tile is small enough for the fused kernel in sample groups."""
    _commit(pair, "config2")
    p = _params("config2", 1920, 1080, 12)
    for i in (0, 5):
        _check_schedule(*pair, p, (1, 2, 7, 12), 0, strips=(8, i), what="config2 strips (8, %d)" % i)
    _check_schedule(*pair, p, (3, 12), T.FLAG_REFERENCE_LAYOUT, strips=(8, 3), what="config2 strips (8, 3) reference layout")


def test_treelets(pair):
    _commit(pair, "config4")
    _check_schedule(*pair, _params("config4", 640, 360, 6), (1, 2, 6), T.FLAG_STREAMED | T.FLAG_TREELETS, what="config4 treelets")


# ------------------------------------------------------------------ 2. against the CPU oracle
def test_against_the_oracle(orc, pair):
    w, h = 96, 54
    _commit(pair[:1], "config2")
    r = pair[0]
    r.reset_history()
    begin = 0
    for spp in (1, 3, 4):
        want, _, p = H.oracle_frame(orc, scenes.build_config2, scenes.CONFIGS[2], w, h, spp)
        got, o = T.alloc_outputs(w, h)
        r.render_progressive(p, begin, o)
        _assert_same(want, got, "config2 %dx%d vs the oracle at %d spp" % (w, h, spp))
        begin = spp


# ------------------------------------------------------------------ 3. full size, pinned by committed strips
def _golden_strip(name, full, w):
    want = np.load(os.path.join(GOLDEN, name + ".npz"))
    y0 = G.FULL_STRIPS[name][1]
    bad = {}
    for k in G.FULL_NAMES:
        a = full[k].reshape(-1, w, *full[k].shape[1:])[y0:y0 + 8]
        n = int(np.count_nonzero(~H.bits_equal(want[k], a)))
        if n:
            bad[k] = n
    assert not bad, "%s: the progressive frame's strip differs from the committed oracle strip: %s" % (name, bad)


def test_full_size_config5(pair):
    """Config 5 at 3840 x 2160 as 8, 24, 96, 256 samples: the 8-spp step equals a one-shot 8-spp frame, the last one the oracle's
    256-spp strip."""
    name = "full_config5_4k_256spp_rows800"
    cfg = scenes.CONFIGS[5]
    w, h = cfg.width, cfg.height
    _commit(pair, "config5")
    prog, ref = pair
    p = scenes.frame_params(cfg, *H.host_funcs("hrt"), width=w, height=h, spp=cfg.spp)
    got, o = T.alloc_outputs(w, h)
    prog.render_progressive(_with_spp(p, 8), 0, o)
    want, o2 = T.alloc_outputs(w, h)
    ref.render_params(_with_spp(p, 8), o2)
    _assert_same(want, got, "config5 4K at 8 spp")
    del want, o2
    begin = 8
    for spp in (24, 96, 256):
        prog.render_progressive(_with_spp(p, spp), begin, o if spp == 256 else None)
        begin = spp
    _golden_strip(name, got, w)


def test_full_size_config3(pair):
    name = "full_config3_1080p_16spp_rows304"
    cfg = scenes.CONFIGS[3]
    w, h = cfg.width, cfg.height
    _commit(pair[:1], "config3")
    p = scenes.frame_params(cfg, *H.host_funcs("hrt"), width=w, height=h, spp=cfg.spp)
    got, o = T.alloc_outputs(w, h, G.FULL_NAMES)
    steps = list(pair[0].refine(p, (1, 16), outputs=o))
    assert [s for s, _ in steps] == [1, 16]
    _golden_strip(name, got, w)


# ------------------------------------------------------------------ 4. reuse at the operating point
def _reuse_frames(name, w, h, n, seed=3):
    rng = np.random.default_rng(seed)
    out, prev_cam = [], None
    for f in range(n):
        p = _params(name, w, h, 2, frame=f, reuse=True, lock=int(rng.integers(1, 2 ** 31 - 1)) | 1, prev_cam=prev_cam, cam_shift=0.1 * f)
        out.append(p)
        prev_cam = engine.copy_camera(p.cam)
    return out


@pytest.mark.parametrize("slots", [[0], [0, 0]])
@pytest.mark.parametrize("name", ["config2", "config4"])
def test_reuse_operating_point(hrt_lib, name, slots):
    """1920 x 1080 at render scale 0.67 (1286 x 724), spp 2 rendered as 1, 2, temporal and spatial reuse, a moving camera, frames
    0..3.  After each call every array (reservoirs included) equals the one-shot frame at that spp; the TAAU image of each frame equals
    the one-shot sequence's.  slots [0, 0]: the progressive frames run on a context of two device slots (reservoir exchange)."""
    w, h = 1286, 724
    prog, ref = engine.RTRenderer(slots), engine.RTRenderer([0])
    try:
        _commit([prog, ref], name)
        for p in _reuse_frames(name, w, h, 4):
            begin = 0
            for spp in (1, 2):
                q = _with_spp(p, spp)
                got, o = T.alloc_outputs(w, h)
                prog.render_progressive(q, begin, o)
                want, o2 = T.alloc_outputs(w, h)
                ref.render_params(q, o2)          # the spp-1 frame's resCur is overwritten by the spp-2 frame exactly as in one shot
                _assert_same(want, got, "%s slots %s frame %d samples [%d, %d)" % (name, slots, p.frame, begin, spp))
                begin = spp
            shown_p = prog.present(1920, 1080, taau=True)
            shown_r = ref.present(1920, 1080, taau=True)
            assert np.array_equal(shown_p, shown_r), "%s slots %s frame %d: TAAU images differ" % (name, slots, p.frame)
    finally:
        prog.close()
        ref.close()


# ------------------------------------------------------------------ 5. NO_SYNC chains
_VIEW_ARRAYS = [("color", np.int32, 1), ("depth", np.float32, 1), ("objectId", np.int32, 1), ("radiance", np.float32, 3),
                ("gb_worldPos", np.float32, 3), ("gb_normalWS", np.float32, 3), ("gb_baseColor", np.float32, 3),
                ("gb_matId", np.int32, 1), ("gb_objId", np.int32, 1), ("gb_hitMask", np.int32, 1)]


def _views_to_host(r, frame):
    v = r.device_views(0)
    h, w = v.height, v.width
    out = {}
    for name, dt, k in _VIEW_ARRAYS:
        out[name] = torch.as_tensor(tiling._DeviceArray(getattr(v, name), (h, w * k), dt), device="cuda").cpu().numpy().reshape(-1)
    for name, t in zip(H.RES_NAMES, tiling.device_tensors(v, "reservoir", frame)):
        out[name] = t.cpu().numpy().reshape(-1)
    return out


@pytest.mark.parametrize("flags", [T.FLAG_MEGAKERNEL, T.FLAG_STREAMED])
def test_no_sync_chain(pair, flags):
    w, h = 160, 96
    _commit(pair, "config2")
    prog, ref = pair
    p = _params("config2", w, h, 24, frame=1)
    begin = 0
    for spp in (1, 3, 8, 24):
        prog.render_progressive(_with_spp(p, spp), begin, None, flags=flags | T.FLAG_NO_SYNC)
        begin = spp
    st = prog.synchronize()
    assert st.frames == 4
    got = _views_to_host(prog, p.frame)
    want, o = T.alloc_outputs(w, h)
    ref.render_params(p, o, flags=flags)
    for k in got:
        n = int(np.count_nonzero(~H.bits_equal(want[k].reshape(-1), got[k])))
        assert n == 0, "device view %s differs from the one-shot frame in %d elements" % (k, n)


# ------------------------------------------------------------------ 6. state rules
def _refused(fn):
    with pytest.raises(engine.HrtError) as e:
        fn()
    assert e.value.code == INVALID_STATE, str(e.value)
    return str(e.value)


def test_state_rules(pair):
    w, h = 96, 64
    prog, ref = pair
    _commit(pair, "blob_64")
    p = _params("blob_64", w, h, 8, frame=2)

    def fresh_frame_matches():
        _check_schedule(prog, ref, p, (2, 8), what="fresh frame after a refusal")

    def started():
        prog.reset_history()
        prog.render_progressive(_with_spp(p, 2), 0, None)

    # calls that end the frame
    started(); prog.render_params(p, None)
    assert "no progressive frame" in _refused(lambda: prog.render_progressive(_with_spp(p, 4), 2, None))
    fresh_frame_matches()
    started(); prog.reset_history()
    _refused(lambda: prog.render_progressive(_with_spp(p, 4), 2, None))
    for update in (lambda r: r.update_instances([], []), lambda r: r.update_positions(0, np.zeros((0, 3), np.float32))):
        started()
        for r in pair:
            update(r)
        _refused(lambda: prog.render_progressive(_with_spp(p, 4), 2, None))
        fresh_frame_matches()
    _commit(pair, "config2")
    p = _params("config2", w, h, 8, frame=2)
    started()
    for r in pair:
        r.update_spheres(0, [])
    _refused(lambda: prog.render_progressive(_with_spp(p, 4), 2, None))
    fresh_frame_matches()

    # continuations that do not continue: refused, and the frame they would have continued is intact
    started()
    q = _with_spp(p, 4)
    other_cam = _params("config2", w, h, 4, frame=2, cam_shift=0.5)
    assert "cam" in _refused(lambda: prog.render_progressive(other_cam, 2, None))
    other_frame = _with_spp(p, 4); other_frame.frame = 3
    assert "frame" in _refused(lambda: prog.render_progressive(other_frame, 2, None))
    other_size = _params("config2", w, h + 8, 4, frame=2)
    assert "height" in _refused(lambda: prog.render_progressive(other_size, 2, None))
    assert "sample_begin" in _refused(lambda: prog.render_progressive(q, 1, None))
    assert "strip" in _refused(lambda: prog.render_progressive(q, 2, None, strips=(2, 1)))
    assert "flags" in _refused(lambda: prog.render_progressive(q, 2, None, flags=T.FLAG_STREAMED))
    with pytest.raises(engine.HrtError) as e:                            # spp <= sample_begin: an argument error of the library too
        prog._check(prog._L.hrt_render_progressive(prog._ctx, C.byref(q), None, 4, None, None))
    assert e.value.code == -1
    # present, ray queries, device views and frame times between calls keep the chain
    prog.present(w, h, taau=False)
    prog.trace_rays(np.zeros((4, 3), np.float32), np.tile(np.float32([0, 0, -1]), (4, 1)))
    prog.device_views(0)
    prog.frame_times()
    got, o = T.alloc_outputs(w, h)
    prog.render_progressive(q, 2, o)
    ref.reset_history()
    want, o2 = T.alloc_outputs(w, h)
    ref.render_params(q, o2)
    _assert_same(want, got, "continuation after refusals, present and trace_rays")
    got, o = T.alloc_outputs(w, h)
    prog.render_progressive(_with_spp(p, 8), 4, o)
    ref.reset_history()
    want, o2 = T.alloc_outputs(w, h)
    ref.render_params(_with_spp(p, 8), o2)
    _assert_same(want, got, "second continuation")
