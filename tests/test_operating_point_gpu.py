"""ReSTIR reuse frames at the settings the reference renders every frame with (RTRenderer.cs:43-49, 104-236): both reuse switches,
render scale 0.67 (1920 x 1080 -> 1286 x 724), TAAU, spp 2, maxDepth 3, a dt-animated sun and a fresh temporal seed per frame --
and the neighbours of that point the rest of the suite does not reach: each reuse switch on its own, both forms of the fused reuse
kernel (one launch; sample groups and their resolve), reuse over sample batches and over the treelet walker.

Every case compares the whole internal image with the CPU oracle: every output array, the reservoirs included, literal bit for bit.
The oracle gets the product's own FrameParams (random seed included) and ping-pongs its reservoirs A / B by frame parity as the
product does (Framebuffer.GetReservoirPair)."""
import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, engine, scenes
from tests import helpers as H

pytestmark = pytest.mark.gpu

TEXTURED = scenes.Config("t", 0, 0, 0, (0.3, 1.3, 4.2), (0.0, 0.7, 0.0))
BUILDERS = {
    "config2": (scenes.build_config2, scenes.CONFIGS[2]),
    "config3": (scenes.build_config3, scenes.CONFIGS[3]),
    "config4": (scenes.build_config4, scenes.CONFIGS[4]),
    "config5": (scenes.build_config5, scenes.CONFIGS[5]),
    "textured": (scenes.build_textured_test_scene, TEXTURED),
    "blob_64": (lambda b: scenes.build_config4(b, 64, 64), scenes.CONFIGS[4]),
}
_ORC_SCENES = {}
_HRT_SCENES = {}


def _orc_scene(orc, name):
    if name not in _ORC_SCENES:
        so = orc.OrcScene()
        BUILDERS[name][0](so)
        _ORC_SCENES[name] = so
    return _ORC_SCENES[name]


def _commit(r, name):
    if name not in _HRT_SCENES:
        s = engine.Scene()
        BUILDERS[name][0](s)
        _HRT_SCENES[name] = s
    r.commit(_HRT_SCENES[name])
    r.reset_history()


def _frames(name, w, h, spp, n, temporal=1, spatial=1, seed=0):
    """n FrameParams of a camera that moves every frame (prevCam = the last frame's camera), a fresh non-zero temporal seed each."""
    cfg = BUILDERS[name][1]
    rng = np.random.default_rng(seed + 1000 * w + h)
    out, prev_cam = [], None
    for f in range(n):
        o = cfg.cam_origin
        c2 = scenes.Config("mv", w, h, spp, (o[0] + 0.12 * f, o[1] + 0.04 * f, o[2] - 0.08 * f), cfg.cam_lookat, extra=cfg.extra)
        p = scenes.frame_params(c2, *H.host_funcs("hrt"), frame=f, rng_lock_noise=int(rng.integers(-2 ** 31, 2 ** 31 - 1)) | 1,
                                prev_cam=prev_cam)
        p.enableTemporalReuse, p.enableSpatialReuse = temporal, spatial
        out.append(p)
        prev_cam = engine.copy_camera(p.cam)
    return out


class OracleRun:
    """The oracle over consecutive frames of one image size with the A / B reservoir ping-pong."""

    def __init__(self, orc, name, w, h):
        self.orc, self.so, self.w, self.h = orc, _orc_scene(orc, name), w, h
        self.A, self.B = H.new_reservoirs(w, h), H.new_reservoirs(w, h)

    def frame(self, p):
        assert (p.width, p.height) == (self.w, self.h)
        prev, cur = (self.B, self.A) if p.frame % 2 == 0 else (self.A, self.B)
        ref, oo = T.alloc_outputs(self.w, self.h)
        for k, a in cur.items():
            ref[k] = a
            setattr(oo, k, a.ctypes.data)
        po = T.Outputs()
        for k, a in prev.items():
            setattr(po, k, a.ctypes.data)
        st = self.orc.render_frame(self.so.desc(), p, oo, po)
        return {k: (v.copy() if k in H.RES_NAMES else v) for k, v in ref.items()}, st


def _oracle_seq(orc, name, params):
    run = OracleRun(orc, name, params[0].width, params[0].height)
    return [run.frame(p) for p in params]


def _check_seq(r, params, refs, flags, what):
    """Renders params on r from zeroed reservoirs and compares every frame (and the work counters when counting) with refs."""
    r.reset_history()
    w, h = params[0].width, params[0].height
    for p, (ref, ost) in zip(params, refs):
        got, o = T.alloc_outputs(w, h)
        st = r.render_params(p, o, flags=flags)
        try:
            H.assert_outputs_equal(ref, got)
        except AssertionError as e:
            raise AssertionError("%s, frame %d: %s" % (what, p.frame, e)) from None
        if flags & T.FLAG_COUNTERS:
            for i in range(2):
                assert st.k[i].as_dict() == ost.k[i].as_dict(), "%s, frame %d: work counters of launch %d" % (what, p.frame, i)
        else:
            assert st.counters_valid == 0


# ------------------------------------------------------------------ (a) RenderDirectToPbo end to end at the operating point
DT_SCHEDULE = [1.0 / 60.0, 0.033, 0.0, 0.25, -0.01, 1.0 / 60.0]


@pytest.mark.parametrize("name", ["config2", "config3", "config4", "config5"])
def test_operating_point_end_to_end(orc, hrt_lib, name):
    """A fresh RTRenderer with the reference's defaults (reuse on, spp 2, maxDepth 3, TAAU, render scale 0.67f, animated noise) and a
    moving sun renders six 1920 x 1080 frames through render_direct with production flags while the camera moves: the internal
    1286 x 724 arrays and the display-size TAAU image of every frame equal the oracle's."""
    builder, cfg = BUILDERS[name]
    r = engine.RTRenderer([0], 1920, 1080)
    try:
        assert (r.enable_temporal_reuse, r.enable_spatial_reuse, r.spp, r.max_depth, r.rng_lock_noise, r.enable_taau) == (1, 1, 2, 3, 1, True)
        s = engine.Scene()
        builder(s)
        r.commit(s)
        # the host placed its camera on the scene (what FlyCameraController does to _camera); the sun animates from the scene's angle
        r.camera = engine.camera_look_at(cfg.cam_origin, cfg.cam_lookat, (0.0, 1.0, 0.0), 60.0, float(np.float32(1920) / np.float32(1080)))
        r.prev_camera = engine.copy_camera(r.camera)
        r.sun_azimuth = np.float32(cfg.extra.get("sun_azimuth", 0.0))
        r.set_sun_params(0.7, cfg.extra.get("sun_elevation", 0.9))
        in_w, in_h = r.internal_size(1920, 1080)
        assert (in_w, in_h) == (1286, 724)
        run = OracleRun(orc, name, in_w, in_h)
        hist = (np.zeros(1920 * 1080, np.int32), np.zeros(1920 * 1080, np.int32))
        azimuths = set()
        for f, dt in enumerate(DT_SCHEDULE):
            if f:
                engine.camera_translate(r.camera, (0.05 * f, 0.02, -0.07))
            got, o = T.alloc_outputs(in_w, in_h)
            shown, st = r.render_direct(1920, 1080, f, dt, outputs=o)
            p = r.last_params
            assert (p.width, p.height, p.spp, p.maxDepth, p.enableTemporalReuse, p.enableSpatialReuse) == (in_w, in_h, 2, 3, 1, 1)
            assert st.counters_valid == 0
            azimuths.add(float(r.sun_azimuth))
            ref, ost = run.frame(p)
            H.assert_outputs_equal(ref, got)
            assert ost.k[1].reuse_imports > in_w * in_h, "frame %d: reuse did not run" % f
            want = orc.present(1, ref["color"], ref["objectId"], in_w, in_h, 1920, 1080, history=hist, first_frame=(f == 0))
            n_bad = int(np.count_nonzero(shown != want))
            assert n_bad == 0, "frame %d: %d TAAU pixels differ from the oracle" % (f, n_bad)
        assert len(azimuths) >= 4                       # the sun moved (dt 0 and a negative dt hold it)
    finally:
        r.close()


# ------------------------------------------------------------------ (b) both forms of the fused reuse kernel
# Production frames of a small scene run the fused path-trace kernel: sample groups (split kernel + resolve) when the tile gives the
# machine fewer than 5 rounds of waves, one launch otherwise or at spp 1 (hrt_runtime.hip run_path_stage).  On 256 CUs:
#   1920 x 1080 spp 2 -> 32 400+ waves: one launch;   320 x 180 spp 1: one launch;
#   1286 x 724 spp 2 -> ~15 000 waves: 2 groups;      96 x 64 spp 11 -> 8 groups of ceil(11 / 8) = 2 -> 6 groups of 2,2,2,2,2,1.
FORMS = {"1920x1080_spp2_single": (1920, 1080, 2), "320x180_spp1_single": (320, 180, 1),
         "1286x724_spp2_groups2": (1286, 724, 2), "96x64_spp11_groups6": (96, 64, 11)}
FORM_SCENES = {"config2": [0], "config3": [0, T.FLAG_MEGAKERNEL]}          # config 3's production frames are streamed: force the fused one too


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(FORM_SCENES))
def test_fused_reuse_forms(orc, renderer, name, form):
    """Two reuse frames per form on scenes with mirror and glass spheres (paths whose last sample groups end without writing a
    reservoir: the resolve must pick the last group that wrote one)."""
    w, h, spp = FORMS[form]
    params = _frames(name, w, h, spp, 2)
    refs = _oracle_seq(orc, name, params)
    assert sum(st.k[1].reuse_imports for _, st in refs) > w * h
    _commit(renderer, name)
    for fl in FORM_SCENES[name]:
        _check_seq(renderer, params, refs, fl, "%s %s flags %#x" % (name, form, fl))


# ------------------------------------------------------------------ (c) one reuse switch at a time
SWITCHES = {"temporal_only": (1, 0), "spatial_only": (0, 1)}
ORGS = {
    "auto_counters": T.FLAG_COUNTERS,
    "production": 0,
    "megakernel": T.FLAG_MEGAKERNEL,
    "streamed": T.FLAG_STREAMED,
    "streamed_reflayout": T.FLAG_STREAMED | T.FLAG_REFERENCE_LAYOUT,
    "counters_megakernel": T.FLAG_COUNTERS | T.FLAG_MEGAKERNEL,
    "counters_streamed": T.FLAG_COUNTERS | T.FLAG_STREAMED,
}


@pytest.fixture(scope="module")
def two_slots(hrt_lib):
    r = engine.RTRenderer([0, 0])
    yield r
    r.close()


@pytest.mark.parametrize("switch", list(SWITCHES))
@pytest.mark.parametrize("name", ["config2", "textured", "blob_64"])
def test_one_reuse_switch(orc, renderer, two_slots, name, switch):
    """Temporal-only and spatial-only frames (the kernel tests each switch on its own; the runtime keys the tile exchange and the
    partial-tile refusal on either): three frames with a moving camera in every kernel organisation, on one device slot and on
    two (exchange), counters included where counted; a partial tile of such a frame is refused."""
    w, h, spp = 160, 96, 2
    params = _frames(name, w, h, spp, 3, *SWITCHES[switch])
    refs = _oracle_seq(orc, name, params)
    assert sum(st.k[1].reuse_imports for _, st in refs) > 0
    _commit(renderer, name)
    for org, fl in ORGS.items():
        _check_seq(renderer, params, refs, fl, "%s %s %s" % (name, switch, org))
    _commit(two_slots, name)
    for fl in (0, T.FLAG_COUNTERS):
        _check_seq(two_slots, params, refs, fl, "%s %s two slots flags %#x" % (name, switch, fl))
    for r in (renderer, two_slots):
        for kw in ({"rows": (0, h // 2)}, {"rows": (8, h)}, {"strips": (2, 1)}):
            with pytest.raises(engine.HrtError) as e:
                r.render_params(params[1], None, **kw)
            assert e.value.code == -2, kw                    # HRT_ERR_INVALID_STATE
        p0 = _frames(name, w, h, spp, 1, 0, 0)[0]           # the same tile without reuse is rendered
        r.render_params(p0, None, rows=(0, h // 2))


# ------------------------------------------------------------------ (d) reuse over sample batches and over the treelet walker
def test_reuse_over_sample_batches(orc, renderer):
    """Config 4 at the internal size of the operating point, spp 3, with the path workspace capped at one sample of the frame:
    three sample batches per frame, three reuse frames (resCur keeps the last batch's writer)."""
    w, h, spp = 1286, 724, 3
    params = _frames("config4", w, h, spp, 3)
    refs = _oracle_seq(orc, "config4", params)
    _commit(renderer, "config4")
    n_ord = ((w + 7) // 8) * ((h + 7) // 8) * 64            # lanes of one sample of the frame (WfGeom.nOrd on one slot)
    renderer.set_workspace_limit(n_ord + 5)
    try:
        _check_seq(renderer, params, refs, T.FLAG_STREAMED, "config4 one-sample batches")
    finally:
        renderer.set_workspace_limit(0)


@pytest.mark.parametrize("name", ["config4", "config5"])
def test_reuse_through_treelets(orc, renderer, name):
    """STREAMED | TREELETS on the shipped library at its shipped treelet limits, three reuse frames at 1286 x 724."""
    w, h = 1286, 724
    params = _frames(name, w, h, 2, 3)
    refs = _oracle_seq(orc, name, params)
    _commit(renderer, name)
    _check_seq(renderer, params, refs, T.FLAG_STREAMED | T.FLAG_TREELETS, "%s treelets" % name)
