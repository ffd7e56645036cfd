"""hrt_denoise_temporal on the device against the restatement in tests/denoise_temporal_ref.py: every word of the denoised radiance and
colour and of the four history planes (colour, moments, length, variance), after every call, compared as 32-bit patterns; no pixel is
excluded.  The restatement is fed the frame's own arrays as the device produced them.  Also: the interplay with hrt_denoise and
hrt_present, device slots, the error contract, and that frame state stays as it was."""
import ctypes as C

import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, engine, scenes
from tests import denoise_ref as R
from tests import denoise_temporal_ref as DT
from tests import helpers as H
from tests.test_hostile_gpu import CASES as HOSTILE, _frame as hostile_frame

pytestmark = pytest.mark.gpu

TEXTURED = scenes.Config("t", 0, 0, 0, (0.3, 1.3, 4.2), (0.0, 0.7, 0.0))
ROTATED = scenes.Config("r", 0, 0, 0, (0.4, 1.8, 5.0), (0.0, 0.8, 0.0))
SCENES = {"textured": (scenes.build_textured_test_scene, TEXTURED), "config1": (scenes.build_config1, scenes.CONFIGS[1]),
          "config2": (scenes.build_config2, scenes.CONFIGS[2]), "rotated": (scenes.build_rotated_instances_scene, ROTATED)}
GUIDES = ["radiance", "color", "depth", "objectId", "gb_worldPos", "gb_normalWS", "gb_baseColor", "gb_hitMask"]
NAN = float("nan")
PLANES = ("color", "moments", "length", "variance")


def _commit(r, builder):
    s = engine.Scene(); builder(s); r.commit(s); r.reset_history()


def _render(r, cfg0, w, h, frame=0, shift=0.0, spp=2, names=GUIDES, jump=False):
    """Frame `frame` (its own random stream) from cfg0's camera moved sideways by `shift`; jump: from the far side of the look-at point."""
    o, l = cfg0.cam_origin, cfg0.cam_lookat
    if jump:
        o = (2 * l[0] - o[0], o[1] + 0.7, 2 * l[2] - o[2])
    cfg = scenes.Config("dt", w, h, spp, (o[0] + shift, o[1], o[2]), (l[0] + shift, l[1], l[2]), max_depth=cfg0.max_depth, extra=cfg0.extra)
    p = scenes.frame_params(cfg, *H.host_funcs("hrt"), frame=frame)
    low, o_ = T.alloc_outputs(w, h, names)
    r.render_params(p, o_)
    return p, low


def _same(got, want):
    return H.bits_equal(np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1))


def _check_history(r, ref, what):
    got, want = r.denoise_history(), ref.history()
    assert (got is None) == (want is None), what
    if got is not None:
        for k in PLANES:
            bad = ~_same(got[k], want[k])
            assert not bad.any(), "%s: %d words of the history %s differ" % (what, int(bad.sum()), k)
    return got


def _check(orc, r, ref, low, cam, w, h, what, **kw):
    got_rad, got_col = r.denoise_temporal(**kw)
    assert r.last_query_ms > 0.0
    want_rad, want_col = ref.step(low, w, h, cam, **kw)
    bad = ~H.bits_equal(got_rad.reshape(-1, 3), want_rad)
    assert not bad.any(), "%s: %d radiance words differ (%d only in the sign of a zero)" % (
        what, int(bad.sum()), int(H.zero_sign_only(got_rad.reshape(-1, 3), want_rad).sum()))
    assert np.array_equal(got_col.reshape(-1), want_col), "%s: %d colour words differ" % (what, int((got_col.reshape(-1) != want_col).sum()))
    _check_history(r, ref, what)
    return got_rad, got_col


@pytest.mark.timeout(900)
@pytest.mark.parametrize("seq", ["static", "pan", "jump", "resize", "reset_history", "t_reset"])
@pytest.mark.parametrize("name", list(SCENES))
def test_sequences_match_restatement(orc, renderer, name, seq):
    """Six frames.  static: one camera.  pan: about a pixel per frame.  jump: frame 3 looks from the far side, which invalidates every
    tap.  resize: frames 3.. at another size.  reset_history / t_reset: the history is emptied before frame 3."""
    builder, cfg = SCENES[name]
    _commit(renderer, builder)
    ref = DT.Temporal(DT.make_fns(orc))
    for f in range(6):
        w, h = (64, 40) if seq == "resize" and f >= 3 else (97, 61)     # 97x61: not a multiple of any tile
        shift = 0.0 if seq == "static" else 0.05 * f
        p, low = _render(renderer, cfg, w, h, frame=f, shift=shift, jump=seq == "jump" and f >= 3)
        kw = {}
        if f == 3 and seq == "reset_history":
            renderer.reset_history(); ref.reset()
        if f == 3 and seq == "t_reset":
            kw = dict(reset=True)
        _check(orc, renderer, ref, low, p.cam, w, h, "%s %s frame %d" % (name, seq, f), **kw)
        hit = low["gb_hitMask"] != 0
        n = ref.length.reshape(-1)[hit]
        if seq == "static":
            assert (n == f + 1).all()
        if f == 3 and seq in ("resize", "reset_history", "t_reset"):
            assert (n == 1).all()
        if f == 3 and seq == "jump":
            print("%s jump: %.3f of the hit pixels restarted" % (name, float((n == 1).mean()) if n.size else 1.0))


@pytest.mark.parametrize("size", [(200, 125), (20, 12), (1, 1), (33, 9)])
def test_sizes_match_restatement(orc, renderer, size):
    """(20, 12): the steps 8 and 16 of iterations 3 and 4 exceed the image, only the centre tap is inside."""
    _commit(renderer, scenes.build_textured_test_scene)
    ref = DT.Temporal(DT.make_fns(orc))
    for f in range(3):
        p, low = _render(renderer, TEXTURED, *size, frame=f, shift=0.04 * f)
        _check(orc, renderer, ref, low, p.cam, *size, "%dx%d frame %d" % (size + (f,)))


@pytest.mark.parametrize("kw", [dict(iterations=1), dict(iterations=2), dict(iterations=5), dict(iterations=8),
                                dict(demodulate=False), dict(spatial=False), dict(spatial=False, demodulate=False),
                                dict(alpha_color=0.05, alpha_moments=0.5, max_history=3), dict(max_history=1)], ids=str)
def test_parameters_match_restatement(orc, renderer, kw):
    _commit(renderer, scenes.build_config2)
    w, h = 97, 61
    ref = DT.Temporal(DT.make_fns(orc))
    for f in range(5):                                  # past N = 4, where the variance switches from the window to the moments
        p, low = _render(renderer, scenes.CONFIGS[2], w, h, frame=f, shift=0.03 * f)
        _check(orc, renderer, ref, low, p.cam, w, h, "%s frame %d" % (kw, f), **kw)


FLOATS = ["alpha_color", "alpha_moments", "sigma_lum", "sigma_normal", "sigma_plane", "normal_cos_min", "plane_tol"]


@pytest.mark.parametrize("value", [NAN, 1e30, 1e-30, -1.0], ids=str)
@pytest.mark.parametrize("field", FLOATS)
def test_hostile_parameters(orc, renderer, field, value):
    _commit(renderer, scenes.build_textured_test_scene)
    w, h = 70, 45
    ref = DT.Temporal(DT.make_fns(orc))
    for f in range(3):
        p, low = _render(renderer, TEXTURED, w, h, frame=f, shift=0.03 * f)
        _check(orc, renderer, ref, low, p.cam, w, h, "%s = %r frame %d" % (field, value, f), iterations=2, **{field: value})


@pytest.mark.parametrize("name", ["degenerate_spheres", "nonfinite_spheres", "degenerate_mesh", "odd_transforms", "odd_textures", "nonfinite_lights"])
def test_hostile_gbuffers(orc, renderer, name):
    """G-buffers of the hostile scenes of tests/test_hostile_gpu.py (NaN / infinite normals and positions among them), three frames."""
    builder, cfg, over = HOSTILE[name]
    w, h = 96, 64
    _commit(renderer, builder)
    ref = DT.Temporal(DT.make_fns(orc))
    for f in range(3):
        low, o_ = T.alloc_outputs(w, h, GUIDES)
        p = hostile_frame(cfg, w, h, 2, over)("hrt")
        p.frame = f
        renderer.render_params(p, o_)
        _check(orc, renderer, ref, low, p.cam, w, h, "%s frame %d" % (name, f), **(dict(demodulate=False, iterations=3) if f == 2 else {}))


@pytest.mark.parametrize("n", [2, 3])
def test_device_slots(orc, hrt_lib, n):
    """One GPU listed n times (independent slots, as tests/test_multidevice_gpu.py): slot 0 receives the other slots' strips first."""
    r = engine.RTRenderer([0] * n)
    try:
        w, h = 80, 52                                   # 7 strips, a ragged last one
        _commit(r, scenes.build_textured_test_scene)
        ref = DT.Temporal(DT.make_fns(orc))
        for f in range(3):
            p, low = _render(r, TEXTURED, w, h, frame=f, shift=0.04 * f)
            rad, col = _check(orc, r, ref, low, p.cam, w, h, "%d slots frame %d" % (n, f))
            assert np.array_equal(r.present(w, h, taau=False, denoised=True), col.reshape(-1))
            again, oa = T.alloc_outputs(w, h, GUIDES)
            r.render_params(p, oa)                      # the strips brought to slot 0 did not disturb the other slots' frame state
            H.assert_outputs_equal(low, again)
            low = again
    finally:
        r.close()


def test_interplay_with_hrt_denoise(orc, renderer):
    """hrt_denoise and hrt_denoise_temporal alternate on successive frames: each matches its own restatement (the temporal history
    simply skips the frames it was not called on), and HRT_PRESENT_DENOISED shows whichever ran last.  Both on one frame: the last
    one owns the planes.  A second temporal call on one frame is refused and leaves the history bit-equal."""
    _commit(renderer, scenes.build_textured_test_scene)
    w, h = 72, 44
    ref = DT.Temporal(DT.make_fns(orc))
    sfns = R.make_fns(orc)
    for f in range(6):
        p, low = _render(renderer, TEXTURED, w, h, frame=f, shift=0.04 * f)
        if f % 2 == 0:
            _, col = _check(orc, renderer, ref, low, p.cam, w, h, "temporal frame %d" % f)
        else:
            before = renderer.denoise_history()
            rad, col = renderer.denoise()
            want_rad, want_col = R.denoise(low, w, h, sfns)
            assert H.bits_equal(rad.reshape(-1, 3), want_rad).all() and np.array_equal(col.reshape(-1), want_col)
            after = _check_history(renderer, ref, "after hrt_denoise on frame %d" % f)        # the history is not hrt_denoise's business
            assert all(_same(before[k], after[k]).all() for k in PLANES)
        assert np.array_equal(renderer.present(w, h, taau=False, denoised=True), col.reshape(-1))
    # both on one frame, either order
    p, low = _render(renderer, TEXTURED, w, h, frame=6, shift=0.24)
    _, tcol = _check(orc, renderer, ref, low, p.cam, w, h, "temporal frame 6")
    _, scol = renderer.denoise()
    assert np.array_equal(renderer.present(w, h, taau=False, denoised=True), scol.reshape(-1))
    before = renderer.denoise_history()
    tp = T.DenoiseTemporalParams()
    ms = C.c_float(-1.0)
    assert renderer._L.hrt_denoise_temporal(renderer._ctx, C.byref(tp), None, None, C.byref(ms)) == -2 and ms.value == 0.0
    assert b"hrt_denoise_temporal" in renderer._L.hrt_last_error(renderer._ctx)
    with pytest.raises(engine.HrtError):
        renderer.denoise_temporal(reset=True)                                    # a reset does not buy a second call either
    after = _check_history(renderer, ref, "after the refused calls")
    assert all(_same(before[k], after[k]).all() for k in PLANES)
    assert np.array_equal(renderer.present(w, h, taau=False, denoised=True), scol.reshape(-1))     # the planes are still hrt_denoise's
    p, low = _render(renderer, TEXTURED, w, h, frame=7, shift=0.28)
    with pytest.raises(engine.HrtError):
        renderer.present(w, h, taau=False, denoised=True)                        # a newer frame
    renderer.denoise()
    _, tcol = _check(orc, renderer, ref, low, p.cam, w, h, "temporal after hrt_denoise on frame 7")
    assert np.array_equal(renderer.present(w, h, taau=False, denoised=True), tcol.reshape(-1))


def test_scene_changes(orc, renderer):
    """hrt_scene_upload empties the history; hrt_scene_update_instances does not."""
    _commit(renderer, scenes.build_rotated_instances_scene)
    w, h = 60, 38
    ref = DT.Temporal(DT.make_fns(orc))
    for f in range(2):
        p, low = _render(renderer, ROTATED, w, h, frame=f)
        _check(orc, renderer, ref, low, p.cam, w, h, "frame %d" % f)
    renderer.update_instances([], [], T.REBUILD_FORCE_REBUILD)
    p, low = _render(renderer, ROTATED, w, h, frame=2)
    _check(orc, renderer, ref, low, p.cam, w, h, "after an instance update")
    assert ref.length.max() == 3
    s = engine.Scene(); scenes.build_rotated_instances_scene(s); renderer.commit(s)          # no reset_history here
    assert renderer.denoise_history() is None
    ref.reset()
    p, low = _render(renderer, ROTATED, w, h, frame=3)
    _check(orc, renderer, ref, low, p.cam, w, h, "after an upload")
    assert ref.length.max() == 1


def test_frame_state_is_untouched(orc, renderer):
    """Two contexts render the same frames with ReSTIR reuse on and present them through the TAAU; one of them runs the temporal
    denoiser after every frame.  Frame outputs (what the next frame reads of this one: G-buffer and reservoirs), the present and
    hrt_frame_times' shape are equal, and a progressive frame continues across a temporal call."""
    other = engine.RTRenderer([0])
    try:
        for r in (renderer, other):
            _commit(r, scenes.build_textured_test_scene)
        w, h = 80, 52
        prev_cam = None
        for f in range(4):
            cfg = scenes.Config("fs", w, h, 3, (TEXTURED.cam_origin[0] + 0.03 * f,) + TEXTURED.cam_origin[1:], TEXTURED.cam_lookat)
            p = scenes.frame_params(cfg, *H.host_funcs("hrt"), frame=f, reuse=True, **({} if prev_cam is None else dict(prev_cam=prev_cam)))
            prev_cam = p.cam
            outs = []
            for r in (renderer, other):
                a, o_ = T.alloc_outputs(w, h)
                r.render_params(p, o_)
                views = r.device_views(0)
                if r is renderer:
                    times = [r.frame_times(launch=k).copy() for k in (0, 1)]
                    r.denoise_temporal()
                    after = r.device_views(0)
                    for name in ("color", "radiance", "gb_worldPos", "gb_hitMask", "present_color"):
                        assert getattr(views, name) == getattr(after, name)
                    for k in (0, 1):
                        assert np.array_equal(times[k], r.frame_times(launch=k))
                outs.append((a, r.present(120, 78, taau=True, reproject=f % 2 == 1)))
            H.assert_outputs_equal(outs[1][0], outs[0][0])
            assert np.array_equal(outs[0][1], outs[1][1]), "present of frame %d" % f
        # a pending progressive frame continues across a temporal call
        cfg = scenes.Config("pg", w, h, 8, TEXTURED.cam_origin, TEXTURED.cam_lookat)
        p = scenes.frame_params(cfg, *H.host_funcs("hrt"), frame=9)
        one, oo = T.alloc_outputs(w, h)
        other.reset_history(); other.render_params(p, oo)
        renderer.reset_history()
        q = T.FrameParams.from_buffer_copy(p)
        q.spp = 3
        renderer.render_progressive(q, 0)
        renderer.denoise_temporal()
        got, og = T.alloc_outputs(w, h)
        renderer.render_progressive(p, 3, og)
        H.assert_outputs_equal(one, got)
        renderer.denoise_temporal()                                              # the continuation is a newer frame
    finally:
        other.close()


def test_error_contract(renderer):
    L, ctx = renderer._L, renderer._ctx
    _commit(renderer, scenes.build_config1)
    _render(renderer, scenes.CONFIGS[1], 40, 24, names=["color"])
    ok = T.DenoiseTemporalParams()
    assert L.hrt_denoise_temporal(ctx, None, None, None, None) == -1
    for bad in (dict(iterations=9), dict(iterations=-1), dict(flags=8), dict(flags=0x80000001)):
        ms = C.c_float(-1.0)
        assert L.hrt_denoise_temporal(ctx, C.byref(T.DenoiseTemporalParams(**bad)), None, None, C.byref(ms)) == -1 and ms.value == 0.0
        assert b"hrt_denoise_temporal" in L.hrt_last_error(ctx)
    assert renderer.denoise_history() is None                               # refused calls accumulated nothing
    assert L.hrt_denoise_temporal(ctx, C.byref(ok), None, None, None) == 0
    assert L.hrt_denoise_temporal(ctx, C.byref(ok), None, None, None) == -2   # the same frame
    assert L.hrt_denoise_history(ctx, None) == -1
    assert L.hrt_denoise_history_read(ctx, None, None) == 0
    p = scenes.frame_params(scenes.Config("e", 40, 24, 1, (0.0, 1.0, 3.0), (0.0, 0.5, 0.0)), *H.host_funcs("hrt"))
    renderer.render_params(p, rows=(0, 16))
    assert L.hrt_denoise_temporal(ctx, C.byref(ok), None, None, None) == -2   # partial tile
    fresh = engine.RTRenderer([0])
    try:
        assert fresh.denoise_history() is None
        assert fresh._L.hrt_denoise_temporal(fresh._ctx, C.byref(ok), None, None, None) == -2      # no frame yet
    finally:
        fresh.close()
