"""hrt_denoise on the device against the restatement in tests/denoise_ref.py: every word of the denoised radiance and colour, compared
as 32-bit patterns (zero signs included).  The restatement is fed the frame's own arrays as the device produced them; frames are
checked elsewhere.  Also: the frame stays as it was, hrt_present with HRT_PRESENT_DENOISED, two device slots, the error contract."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, engine, scenes
from tests import denoise_ref as R
from tests import helpers as H
from tests.test_hostile_gpu import CASES as HOSTILE, _frame as hostile_frame
from tests.test_present_reproject import make_taa
from tests.test_present_reproject_gpu import RefHistory

pytestmark = pytest.mark.gpu

TEXTURED = scenes.Config("t", 0, 0, 0, (0.3, 1.3, 4.2), (0.0, 0.7, 0.0))
ROTATED = scenes.Config("r", 0, 0, 0, (0.4, 1.8, 5.0), (0.0, 0.8, 0.0))
SCENES = {"textured": (scenes.build_textured_test_scene, TEXTURED), "config1": (scenes.build_config1, scenes.CONFIGS[1]),
          "config2": (scenes.build_config2, scenes.CONFIGS[2]), "rotated": (scenes.build_rotated_instances_scene, ROTATED)}
GUIDES = ["radiance", "color", "depth", "objectId", "gb_worldPos", "gb_normalWS", "gb_baseColor", "gb_hitMask"]
NAN = float("nan")


def _commit(r, builder):
    s = engine.Scene(); builder(s); r.commit(s); r.reset_history()


def _render(r, cfg0, w, h, spp=2, frame=0, pan=0.0, names=GUIDES):
    o, l = cfg0.cam_origin, cfg0.cam_lookat
    cfg = scenes.Config("dn", w, h, spp, (o[0] + pan * frame, o[1] + 0.01 * frame, o[2] - 0.02 * frame), (l[0] + pan * frame, l[1], l[2]),
                        max_depth=cfg0.max_depth, extra=cfg0.extra)
    p = scenes.frame_params(cfg, *H.host_funcs("hrt"), frame=frame)
    low, o_ = T.alloc_outputs(w, h, names)
    r.render_params(p, o_)
    return p, low


def _check(orc, r, low, w, h, what, **kw):
    got_rad, got_col = r.denoise(**kw)
    assert r.last_query_ms > 0.0
    want_rad, want_col = R.denoise(low, w, h, R.make_fns(orc), **kw)
    bad = ~H.bits_equal(got_rad.reshape(-1, 3), want_rad)
    assert not bad.any(), "%s: %d radiance words differ (%d only in the sign of a zero)" % (
        what, int(bad.sum()), int(H.zero_sign_only(got_rad.reshape(-1, 3), want_rad).sum()))
    assert np.array_equal(got_col.reshape(-1), want_col), "%s: %d colour words differ" % (what, int((got_col.reshape(-1) != want_col).sum()))
    return got_rad, got_col


@pytest.mark.parametrize("name", list(SCENES))
def test_scenes_match_restatement(orc, renderer, name):
    builder, cfg = SCENES[name]
    _commit(renderer, builder)
    w, h = 97, 61                                      # not a multiple of any tile
    _, low = _render(renderer, cfg, w, h)
    _check(orc, renderer, low, w, h, name)
    _check(orc, renderer, low, w, h, name + " no demodulation", demodulate=False)


@pytest.mark.parametrize("size", [(200, 125), (20, 12), (1, 1), (33, 9)])
def test_sizes_match_restatement(orc, renderer, size):
    """(20, 12): the steps 8 and 16 of iterations 3 and 4 exceed the image, only the centre tap is inside."""
    _commit(renderer, scenes.build_textured_test_scene)
    _, low = _render(renderer, TEXTURED, *size)
    _check(orc, renderer, low, *size, "%dx%d" % size)


@pytest.mark.parametrize("iterations", [1, 2, 5, 8])
def test_iterations_match_restatement(orc, renderer, iterations):
    _commit(renderer, scenes.build_config2)
    w, h = 97, 61
    _, low = _render(renderer, scenes.CONFIGS[2], w, h)
    _check(orc, renderer, low, w, h, "iterations %d" % iterations, iterations=iterations)


@pytest.mark.parametrize("sig", [dict(sigma_color=0.7, sigma_normal=0.1, sigma_plane=0.5), dict(sigma_color=1e30), dict(sigma_color=NAN),
                                 dict(sigma_normal=NAN, iterations=2), dict(sigma_plane=NAN, demodulate=False), dict(sigma_plane=1e-30),
                                 dict(sigma_color=-1.0, sigma_normal=-2.0, sigma_plane=-0.0)])
def test_sigmas_match_restatement(orc, renderer, sig):
    _commit(renderer, scenes.build_textured_test_scene)
    w, h = 70, 45
    _, low = _render(renderer, TEXTURED, w, h)
    _check(orc, renderer, low, w, h, str(sig), **sig)


@pytest.mark.parametrize("name", ["degenerate_spheres", "nonfinite_spheres", "degenerate_mesh", "odd_transforms", "odd_textures", "nonfinite_lights"])
def test_hostile_gbuffers(orc, renderer, name):
    """G-buffers of the hostile scenes of tests/test_hostile_gpu.py (NaN / infinite normals and positions among them): inputs only."""
    builder, cfg, over = HOSTILE[name]
    w, h = 96, 64
    _commit(renderer, builder)
    low, o_ = T.alloc_outputs(w, h, GUIDES)
    renderer.render_params(hostile_frame(cfg, w, h, 2, over)("hrt"), o_)
    _check(orc, renderer, low, w, h, name)
    _check(orc, renderer, low, w, h, name + " no demodulation", demodulate=False, iterations=3)


def test_frame_state_is_untouched(orc, renderer):
    _commit(renderer, scenes.build_textured_test_scene)
    w, h = 80, 52
    cfg = scenes.Config("fs", w, h, 4, TEXTURED.cam_origin, TEXTURED.cam_lookat)
    p = scenes.frame_params(cfg, *H.host_funcs("hrt"), frame=3, reuse=True)
    before, ob = T.alloc_outputs(w, h)
    renderer.render_params(p, ob)
    times = [renderer.frame_times(launch=k).copy() for k in (0, 1)]
    views = renderer.device_views(0)
    renderer.denoise()
    renderer.denoise(iterations=2, demodulate=False)
    after_views = renderer.device_views(0)
    for f in ("color", "radiance", "gb_worldPos", "gb_hitMask", "present_color"):
        assert getattr(views, f) == getattr(after_views, f)
    for k in (0, 1):
        assert np.array_equal(times[k], renderer.frame_times(launch=k))
    # what the next frame reads of this one (G-buffer, reservoirs, through ReSTIR reuse) is what a context that never denoised
    # reads; the arrays themselves are read back in test_device_path_equals_host_path
    other = engine.RTRenderer([0])
    try:
        _commit(other, scenes.build_textured_test_scene)
        other.render_params(p)
        p2 = scenes.frame_params(cfg, *H.host_funcs("hrt"), frame=4, reuse=True, prev_cam=p.cam)
        nxt, on = T.alloc_outputs(w, h)
        ref, orf = T.alloc_outputs(w, h)
        renderer.render_params(p2, on)
        other.render_params(p2, orf)
        H.assert_outputs_equal(ref, nxt)
    finally:
        other.close()


def test_progressive_frame_continues_after_a_denoise(orc, renderer):
    _commit(renderer, scenes.build_config2)
    w, h = 64, 40
    cfg = scenes.Config("pg", w, h, 8, scenes.CONFIGS[2].cam_origin, scenes.CONFIGS[2].cam_lookat, extra=scenes.CONFIGS[2].extra)
    p = scenes.frame_params(cfg, *H.host_funcs("hrt"), frame=1)
    one, oo = T.alloc_outputs(w, h)
    renderer.reset_history()
    renderer.render_params(p, oo)
    want_full = renderer.denoise()
    renderer.reset_history()
    q = T.FrameParams.from_buffer_copy(p)
    q.spp = 3
    part, op = T.alloc_outputs(w, h, GUIDES)
    renderer.render_progressive(q, 0, op)
    _check(orc, renderer, part, w, h, "preview at 3 spp")                  # a preview may be denoised between refinements
    renderer.present(w, h, taau=False, denoised=True)
    got, og = T.alloc_outputs(w, h)
    renderer.render_progressive(p, 3, og)
    H.assert_outputs_equal(one, got)
    with pytest.raises(engine.HrtError) as e:                               # the continuation is a newer frame
        renderer.present(w, h, taau=False, denoised=True)
    assert e.value.code == -2 and "hrt_denoise" in str(e.value)
    full = renderer.denoise()
    assert H.bits_equal(full[0], want_full[0]).all() and np.array_equal(full[1], want_full[1])


@pytest.mark.timeout(900)
def test_present_denoised(orc, renderer):
    """mode | HRT_PRESENT_DENOISED for modes 0, 1, 2 over a 4-frame moving-camera sequence equals the reference present fed the
    restatement's denoised colour (objectId and gb_worldPos stay the frame's); flagged and unflagged presents alternate on one history."""
    in_w, in_h, ow, oh = 48, 30, 72, 45
    fns = R.make_fns(orc)
    for mode in (T.PRESENT_RESAMPLE, T.PRESENT_TAAU, T.PRESENT_TAAU_REPROJECT):
        _commit(renderer, scenes.build_textured_test_scene)
        ref = RefHistory(orc, make_taa(orc))
        for f in range(4):
            p, low = _render(renderer, TEXTURED, in_w, in_h, frame=f, pan=0.06)
            renderer.denoise()
            dn = dict(low); dn["color"] = R.denoise(low, in_w, in_h, fns)[1]
            flagged = (f != 2) or mode == T.PRESENT_RESAMPLE          # frame 2 of the TAAU modes is presented without the flag
            got = renderer.present(ow, oh, taau=mode != T.PRESENT_RESAMPLE, reproject=mode == T.PRESENT_TAAU_REPROJECT, denoised=flagged)
            want = ref.present(mode, dn if flagged else low, p.cam, in_w, in_h, ow, oh)
            assert np.array_equal(got, want), "mode %d frame %d: %d words differ" % (mode, f, int((got != want).sum()))
            if mode == T.PRESENT_RESAMPLE:
                same = renderer.present(in_w, in_h, taau=False, denoised=True)      # equal sizes: the blit of the denoised colour
                assert np.array_equal(same, dn["color"])
    # a newer frame: the planes are stale until the next hrt_denoise
    _render(renderer, TEXTURED, in_w, in_h, frame=9)
    for mode in (0, 1, 2):
        pp = T.PresentParams(ow, oh, mode | T.PRESENT_DENOISED, 0.0, 0.0, 0.0)
        assert renderer._L.hrt_present(renderer._ctx, C.byref(pp), None) == -2
        assert b"hrt_denoise" in renderer._L.hrt_last_error(renderer._ctx)
    renderer.denoise()
    renderer.present(ow, oh, denoised=True)
    _commit(renderer, scenes.build_textured_test_scene)                          # an upload too
    with pytest.raises(engine.HrtError):
        renderer.present(ow, oh, denoised=True)


def test_unflagged_present_is_what_it_was(hrt_lib):
    """Two contexts, the same frames; one denoises every frame, neither sets the flag: equal presents in every mode."""
    a, b = engine.RTRenderer([0]), engine.RTRenderer([0])
    try:
        for r in (a, b):
            _commit(r, scenes.build_textured_test_scene)
        for f in range(3):
            for mode in (0, 1, 2):
                outs = []
                for r in (a, b):
                    _render(r, TEXTURED, 56, 34, frame=f, pan=0.05, names=["color"])
                    if r is a:
                        r.denoise()
                    outs.append(r.present(84, 51, taau=mode != 0, reproject=mode == 2))
                assert np.array_equal(outs[0], outs[1]), (f, mode)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("n", [2, 3])
def test_device_slots(orc, hrt_lib, n):
    """One GPU listed n times (independent slots, as tests/test_multidevice_gpu.py): slot 0 receives the other slots' strips first."""
    r = engine.RTRenderer([0] * n)
    try:
        w, h = 80, 52                                   # 7 strips, a ragged last one
        _commit(r, scenes.build_textured_test_scene)
        p, low = _render(r, TEXTURED, w, h)
        rad, col = _check(orc, r, low, w, h, "%d slots" % n)
        again, oa = T.alloc_outputs(w, h, GUIDES)
        r.render_params(p, oa)                          # the strips brought to slot 0 did not disturb the other slots' frame state
        H.assert_outputs_equal(low, again)
        got = r.present(w, h, taau=False, denoised=False)
        assert np.array_equal(got, low["color"])
        r.denoise()
        assert np.array_equal(r.present(w, h, taau=False, denoised=True), col.reshape(-1))
    finally:
        r.close()


def test_error_contract(renderer):
    L, ctx = renderer._L, renderer._ctx
    _commit(renderer, scenes.build_config1)
    _render(renderer, scenes.CONFIGS[1], 40, 24, names=["color"])
    ok = T.DenoiseParams(0, 0, 0.0, 0.0, 0.0)
    assert L.hrt_denoise(ctx, C.byref(ok), None, None, None) == 0
    assert L.hrt_denoise(ctx, None, None, None, None) == -1
    for bad in (T.DenoiseParams(9, 0, 0, 0, 0), T.DenoiseParams(-1, 0, 0, 0, 0), T.DenoiseParams(0, 2, 0, 0, 0), T.DenoiseParams(0, 0x80000001, 0, 0, 0)):
        ms = C.c_float(-1.0)
        assert L.hrt_denoise(ctx, C.byref(bad), None, None, C.byref(ms)) == -1 and ms.value == 0.0
        assert b"hrt_denoise" in L.hrt_last_error(ctx)
    assert L.hrt_denoise(ctx, C.byref(ok), None, None, None) == 0           # a refused call changes nothing
    p = scenes.frame_params(scenes.Config("e", 40, 24, 1, (0.0, 1.0, 3.0), (0.0, 0.5, 0.0)), *H.host_funcs("hrt"))
    renderer.render_params(p, rows=(0, 16))
    assert L.hrt_denoise(ctx, C.byref(ok), None, None, None) == -2          # partial tile
    fresh = engine.RTRenderer([0])
    try:
        pr, pc = C.c_void_p(1), C.c_void_p(1)
        assert fresh._L.hrt_denoised_buffers(fresh._ctx, C.byref(pr), C.byref(pc)) == 0 and pr.value is None and pc.value is None
        assert fresh._L.hrt_denoise(fresh._ctx, C.byref(ok), None, None, None) == -2      # no frame yet
        with pytest.raises(engine.HrtError):
            fresh.present(8, 8, denoised=True)
    finally:
        fresh.close()


DEVICE_WORKER = r'''
import sys
sys.path.insert(0, %(root)r)
import ctypes as C
import torch
import numpy as np
from ilgpu_raytracing_amd import _types as T, engine, scenes
from tests import helpers as H
from tests.test_denoise_gpu import TEXTURED, _commit, _render

torch.cuda.set_device(0)
for slots in ([0], [0, 0]):
    r = engine.RTRenderer(slots)
    _commit(r, scenes.build_textured_test_scene)
    w, h = 97, 61
    cfg = scenes.Config("fs", w, h, 3, TEXTURED.cam_origin, TEXTURED.cam_lookat)
    p = scenes.frame_params(cfg, *H.host_funcs("hrt"), frame=2, reuse=True)
    before, ob = T.alloc_outputs(w, h)
    r.render_params(p, ob)
    host_rad, host_col = r.denoise()
    if len(slots) == 1:
        # frame state: every hrt_outputs array, read back through the device pointers after the denoise, is what the frame returned
        v = r.device_views(0)
        ptrs = {n: getattr(v, n) for n, _, _ in T.OUTPUT_ARRAYS if hasattr(v, n) and n != "cameraId"}
        ptrs.update({n: v.res_a[i] for i, n in enumerate(H.RES_NAMES)})            # frame 2 is even: resCur = A
        assert len(ptrs) == 17
        for n, ptr in ptrs.items():
            a = before[n]
            back = engine._device_plane(torch, ptr, a.shape, a.dtype.str, "cuda:0", r).cpu().numpy()
            assert H.bits_equal(a, back).all(), n
    dev_rad, dev_col = r.denoise(slot=0)
    assert dev_rad.device.type == "cuda" and tuple(dev_rad.shape) == (h, w, 3) and dev_rad.dtype == torch.float32
    assert tuple(dev_col.shape) == (h, w) and dev_col.dtype == torch.int32
    pr, pc = C.c_void_p(), C.c_void_p()
    assert r._L.hrt_denoised_buffers(r._ctx, C.byref(pr), C.byref(pc)) == 0
    assert dev_rad.data_ptr() == pr.value and dev_col.data_ptr() == pc.value          # views of the library's planes, no copy
    assert H.bits_equal(dev_rad.cpu().numpy(), host_rad).all(), slots
    assert np.array_equal(dev_col.cpu().numpy(), host_col), slots
    r.denoise(iterations=1, demodulate=False, slot=0)                                 # the same planes, overwritten
    assert r._L.hrt_denoised_buffers(r._ctx, C.byref(pr), C.byref(pc)) == 0 and dev_rad.data_ptr() == pr.value
    assert not np.array_equal(dev_col.cpu().numpy(), host_col)
    r.close()
print("DEVICE_PATH_OK")
'''


@pytest.mark.timeout(600)
def test_device_path_equals_host_path(tmp_path):
    """hrt_denoised_buffers through torch tensors against out_*_host, on one and on two device slots.  In a process of its own:
    torch's HIP runtime has to be loaded first."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "denoise_device_worker.py"
    script.write_text(DEVICE_WORKER % {"root": root})
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=540, cwd=root)
    assert out.returncode == 0 and "DEVICE_PATH_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
