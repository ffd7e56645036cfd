"""Reprojecting TAAU (hrt_present mode HRT_PRESENT_TAAU_REPROJECT) and hrt_motion_vectors on the device, against the restatement in
tests/taa_reproject_ref.py: every output word, over histories that mix the three present modes.  The reference side takes the
frame's own internal arrays (colour, objectId, gb_worldPos) as the device produced them; frames are checked elsewhere."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, engine, scenes
from tests import helpers as H
from tests.test_present_reproject import make_taa

pytestmark = pytest.mark.gpu

TEXTURED = scenes.Config("t", 0, 0, 0, (0.3, 1.3, 4.2), (0.0, 0.7, 0.0))
KNOBS = (0.075, 0.10, 1.25)


class RefHistory:
    """The history as the contract defines it: colour / objId per display size, a valid flag, and the camera of the frame a TAAU
    present last resolved into it."""

    def __init__(self, orc, taa):
        self.orc, self.taa = orc, taa
        self.size, self.hist, self.valid, self.cam = None, None, False, None

    def reset(self):
        self.valid = False

    def present(self, mode, low, cam, in_w, in_h, ow, oh):
        if self.size != (ow, oh):                     # RTTaa.Ensure: a new display size is a new, invalid history (any mode)
            self.size, self.hist, self.valid = (ow, oh), (np.zeros(ow * oh, np.int32), np.zeros(ow * oh, np.int32)), False
        if mode == T.PRESENT_RESAMPLE:
            return self.orc.present(0, low["color"], low["objectId"], in_w, in_h, ow, oh)
        first = not self.valid
        if mode == T.PRESENT_TAAU:
            out = self.orc.present(1, low["color"], low["objectId"], in_w, in_h, ow, oh, history=self.hist, first_frame=first)
        else:
            out = self.taa.resolve_reproject(low["color"], low["objectId"], low["gb_worldPos"], in_w, in_h, ow, oh, self.hist[0], self.hist[1],
                                             cam if first else self.cam, cam, first, *KNOBS)
        self.valid, self.cam = True, engine.copy_camera(cam)
        return out


def _present(r, mode, ow, oh):
    return r.present(ow, oh, taau=(mode != T.PRESENT_RESAMPLE), reproject=(mode == T.PRESENT_TAAU_REPROJECT))


def _frame(r, builder_cfg, in_w, in_h, f, reuse=False, prev_cam=None, pan=0.06, spp=1):
    o, l = builder_cfg.cam_origin, builder_cfg.cam_lookat
    cfg = scenes.Config("mv", in_w, in_h, spp, (o[0] + pan * f, o[1] + 0.01 * f, o[2] - 0.02 * f), (l[0] + pan * f, l[1], l[2]),
                        extra={"sun_azimuth": 1.5707963 + 0.02 * f, "sun_elevation": 0.6})
    p = scenes.frame_params(cfg, *H.host_funcs("hrt"), frame=f, reuse=reuse, prev_cam=prev_cam)
    low, o_ = T.alloc_outputs(in_w, in_h, ["color", "objectId", "gb_worldPos"])
    r.render_params(p, o_)
    return p, low


def _internal(ow, oh, scale):
    return max(1, int(np.rint(np.float32(ow) * np.float32(scale)))), max(1, int(np.rint(np.float32(oh) * np.float32(scale))))


@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("out_size,scale", [((192, 108), 0.67), ((160, 90), 1.0), ((131, 77), 0.5),
                                            ((1, 1), 1.0), ((3, 2), 0.5), ((257, 3), 0.67), ((2, 199), 0.3), ((64, 48), 0.01)])
def test_reproject_matches_restatement(orc, renderer, out_size, scale, reuse):
    """Six frames with a moving camera and sun, presented with mode 2, at the display / scale pairs of test_present_matches_oracle."""
    ow, oh = out_size
    in_w, in_h = _internal(ow, oh, scale)
    s = engine.Scene(); scenes.build_textured_test_scene(s); renderer.commit(s); renderer.reset_history()
    ref = RefHistory(orc, make_taa(orc))
    prev_cam = None
    for f in range(6):
        p, low = _frame(renderer, TEXTURED, in_w, in_h, f, reuse=reuse, prev_cam=prev_cam)
        got = _present(renderer, T.PRESENT_TAAU_REPROJECT, ow, oh)
        want = ref.present(T.PRESENT_TAAU_REPROJECT, low, p.cam, in_w, in_h, ow, oh)
        assert np.array_equal(got, want), "frame %d: %d words differ" % (f, int((got != want).sum()))
        prev_cam = engine.copy_camera(p.cam)


def test_modes_interleaved_on_one_history(orc, renderer):
    """Modes 0 / 1 / 2 from frame to frame on one history, a double present, hrt_reset_history and a display resize in the middle."""
    in_w, in_h = 56, 34
    s = engine.Scene(); scenes.build_textured_test_scene(s); renderer.commit(s); renderer.reset_history()
    ref = RefHistory(orc, make_taa(orc))
    size = (84, 51)
    plan = [(2,), (1,), (2, 2), (0,), (2,), (1, 2), ("reset", 2), (2,), ("resize", 2), (1,), (2,), (0, 2)]
    for f, steps in enumerate(plan):
        p, low = _frame(renderer, TEXTURED, in_w, in_h, f)
        for st in steps:
            if st == "reset":
                renderer.reset_history(); ref.reset()
                p, low = _frame(renderer, TEXTURED, in_w, in_h, f)        # the reset also ends reservoirs; the frame is rendered again
                continue
            if st == "resize":
                size = (70, 40)
                continue
            got = _present(renderer, st, *size)
            want = ref.present(st, low, p.cam, in_w, in_h, *size)
            assert np.array_equal(got, want), "frame %d mode %d: %d words differ" % (f, st, int((got != want).sum()))
            assert renderer.present_ms() > 0.0                        # hrt_present_time: the kernel of this present, HIP events


def test_static_camera_mode_2_equals_mode_1(hrt_lib):
    """Two contexts, the same static-camera frames (moving sun), one presenting with mode 1 and one with mode 2: equal words.  With
    an equal camera qx == px exactly, so columns 0 and outW - 1 (rows 0 and outH - 1) sit exactly on the borders of step 5 and stay valid."""
    a, b = engine.RTRenderer([0]), engine.RTRenderer([0])
    try:
        in_w, in_h, ow, oh = 129, 72, 192, 108
        for r in (a, b):
            s = engine.Scene(); scenes.build_textured_test_scene(s); r.commit(s)
        for f in range(5):
            outs = []
            for r, mode in ((a, T.PRESENT_TAAU), (b, T.PRESENT_TAAU_REPROJECT)):
                cfg = scenes.Config("st", in_w, in_h, 2, TEXTURED.cam_origin, TEXTURED.cam_lookat, extra={"sun_azimuth": 1.5707963 + 0.02 * f, "sun_elevation": 0.6})
                r.render_params(scenes.frame_params(cfg, *H.host_funcs("hrt"), frame=f))
                outs.append(_present(r, mode, ow, oh))
            assert np.array_equal(outs[0], outs[1]), "frame %d: %d words differ" % (f, int((outs[0] != outs[1]).sum()))
    finally:
        a.close(); b.close()


def test_history_camera_is_the_contexts_own(orc, renderer):
    """params.prevCam plays no part: frames whose prevCam is garbage present as frames whose prevCam is right.  A skipped present is
    followed: the history camera stays that of the last frame that was resolved."""
    in_w, in_h, ow, oh = 48, 30, 72, 45
    s = engine.Scene(); scenes.build_textured_test_scene(s); renderer.commit(s); renderer.reset_history()
    ref = RefHistory(orc, make_taa(orc))
    garbage = engine.copy_camera(scenes.frame_params(scenes.Config("g", in_w, in_h, 1, (9.0, -3.0, 1.0), (0.0, 40.0, 2.0)), *H.host_funcs("hrt")).cam)
    garbage.fovYRadians = 2.9
    for f in range(6):
        p, low = _frame(renderer, TEXTURED, in_w, in_h, f, prev_cam=garbage if f % 2 else None)
        if f in (2, 3):
            continue                                   # rendered, never presented
        got = _present(renderer, T.PRESENT_TAAU_REPROJECT, ow, oh)
        want = ref.present(T.PRESENT_TAAU_REPROJECT, low, p.cam, in_w, in_h, ow, oh)
        assert np.array_equal(got, want), "frame %d: %d words differ" % (f, int((got != want).sum()))


def _hostile(cam, what, point):
    c = engine.copy_camera(cam)
    nan, inf = float("nan"), float("inf")
    if what == "nan_origin": c.origin.Y = nan
    elif what == "inf_origin": c.origin.X = inf
    elif what == "zero_fov": c.fovYRadians = 0.0
    elif what == "nan_fov": c.fovYRadians = nan
    elif what == "zero_basis":
        for v in (c.right, c.up, c.forward): v.X = v.Y = v.Z = 0.0
    elif what == "zero_aspect": c.aspect = 0.0
    elif what == "on_camera_plane":                     # a surface point of the next frame exactly at the origin: z == 0
        c.origin.X, c.origin.Y, c.origin.Z = [float(v) for v in point]
    return c


@pytest.mark.parametrize("what", ["nan_origin", "inf_origin", "zero_fov", "nan_fov", "zero_basis", "zero_aspect", "on_camera_plane"])
def test_hostile_cameras(orc, renderer, what):
    """Cameras nobody would set, as the current camera of one resolve and as the history camera of the next: the calls return and
    match the restatement (NaN and infinite projections fail the comparisons of step 5).  Inputs only; nothing here is meant to fault."""
    in_w, in_h, ow, oh = 40, 26, 60, 39
    s = engine.Scene(); scenes.build_textured_test_scene(s); renderer.commit(s); renderer.reset_history()
    ref = RefHistory(orc, make_taa(orc))
    p0, low0 = _frame(renderer, TEXTURED, in_w, in_h, 0)
    point = low0["gb_worldPos"].reshape(-1, 3)[(in_h // 2) * in_w + in_w // 2]
    for f in range(3):
        o, l = TEXTURED.cam_origin, TEXTURED.cam_lookat
        cfg = scenes.Config("h", in_w, in_h, 1, o, l, extra={"sun_azimuth": 1.5707963 + 0.02 * f, "sun_elevation": 0.6})
        p = scenes.frame_params(cfg, *H.host_funcs("hrt"), frame=f)
        if f == 1:
            p.cam = _hostile(p.cam, what, point)
        low, o_ = T.alloc_outputs(in_w, in_h, ["color", "objectId", "gb_worldPos"])
        renderer.render_params(p, o_)
        got = _present(renderer, T.PRESENT_TAAU_REPROJECT, ow, oh)
        want = ref.present(T.PRESENT_TAAU_REPROJECT, low, p.cam, in_w, in_h, ow, oh)
        assert np.array_equal(got, want), "%s, frame %d: %d words differ" % (what, f, int((got != want).sum()))
        mv = renderer.motion_vectors(from_cam=_hostile(p0.cam, what, point)).reshape(-1, 2)
        want_mv = ref.taa.motion_vectors(low["gb_worldPos"], in_w, in_h, _hostile(p0.cam, what, point), p.cam)
        assert H.bits_equal(mv, want_mv).all(), "%s, frame %d: motion vectors" % (what, f)


def test_motion_vectors_host_path_and_error_contract(orc, renderer):
    in_w, in_h = 75, 43                                 # 43 rows: a ragged last strip
    s = engine.Scene(); scenes.build_textured_test_scene(s); renderer.commit(s); renderer.reset_history()
    taa = make_taa(orc)
    p0, _ = _frame(renderer, TEXTURED, in_w, in_h, 0)
    cam0 = engine.copy_camera(p0.cam)
    p, low = _frame(renderer, TEXTURED, in_w, in_h, 3, prev_cam=cam0)
    before = renderer.device_views(0)
    got = renderer.motion_vectors()                     # from_cam NULL: the frame's prevCam
    assert got.shape == (in_h, in_w, 2) and renderer.last_query_ms >= 0.0
    want = taa.motion_vectors(low["gb_worldPos"], in_w, in_h, cam0, p.cam)
    assert H.bits_equal(got.reshape(-1, 2), want).all()
    assert np.isfinite(want).all() and np.abs(want[:, 0]).max() > 1.0       # the camera did move
    other = engine.copy_camera(scenes.frame_params(scenes.Config("o", in_w, in_h, 1, (1.5, 0.9, 3.0), (0.0, 0.5, 0.0)), *H.host_funcs("hrt")).cam)
    got = renderer.motion_vectors(from_cam=other)
    assert H.bits_equal(got.reshape(-1, 2), taa.motion_vectors(low["gb_worldPos"], in_w, in_h, other, p.cam)).all()
    assert np.array_equal(renderer.motion_vectors(from_cam=p.cam).reshape(-1, 2), np.zeros((in_w * in_h, 2), np.float32))   # the same camera: exactly zero
    after = renderer.device_views(0)
    for f in ("color", "gb_worldPos", "present_color"):
        assert getattr(before, f) == getattr(after, f)
    # error contract: the status codes of hrt_present
    L, ctx = renderer._L, renderer._ctx
    buf = np.zeros((in_h, in_w, 2), np.float32)
    assert L.hrt_motion_vectors(ctx, None, None, -1, None) == -1                 # NULL mv
    assert L.hrt_motion_vectors(ctx, None, buf.ctypes.data, 1, None) == -1       # only slot 0 keeps vectors on the device
    assert L.hrt_motion_vectors(ctx, None, buf.ctypes.data, 0, None) == -1       # host memory on the device path
    renderer.render_params(p, rows=(0, 16))
    with pytest.raises(engine.HrtError) as e:
        renderer.motion_vectors()
    assert e.value.code == -2                                                    # partial tile
    fresh = engine.RTRenderer([0])
    try:
        assert fresh._L.hrt_motion_vectors(fresh._ctx, None, buf.ctypes.data, -1, None) == -2      # no frame yet
        with pytest.raises(engine.HrtError):
            fresh.present(8, 8, reproject=True)                                  # same contract as the other modes
    finally:
        fresh.close()


DEVICE_WORKER = r'''
import sys
sys.path.insert(0, %(root)r)
import ctypes as C
import torch
import numpy as np
from ilgpu_raytracing_amd import _types as T, engine, scenes
from oracle import orc
from tests import helpers as H
from tests.test_present_reproject import make_taa
from tests.test_present_reproject_gpu import TEXTURED, _frame, _present

orc.build()
torch.cuda.set_device(0)
taa = make_taa(orc)
for slots in ([0], [0, 0]):
    r = engine.RTRenderer(slots)
    s = engine.Scene(); scenes.build_textured_test_scene(s); r.commit(s)
    in_w, in_h, ow, oh = 64, 43, 96, 64
    p0, _ = _frame(r, TEXTURED, in_w, in_h, 0)
    cam0 = engine.copy_camera(p0.cam)
    _present(r, T.PRESENT_TAAU_REPROJECT, ow, oh)
    p, low = _frame(r, TEXTURED, in_w, in_h, 2, prev_cam=cam0)
    host = r.motion_vectors()
    dev = r.motion_vectors(slot=0)
    assert dev.device.type == "cuda" and tuple(dev.shape) == (in_h, in_w, 2)
    want = taa.motion_vectors(low["gb_worldPos"], in_w, in_h, cam0, p.cam)
    assert H.bits_equal(host.reshape(-1, 2), want).all(), slots
    assert H.bits_equal(dev.cpu().numpy().reshape(-1, 2), want).all(), slots
    assert r._L.hrt_motion_vectors(r._ctx, None, dev.data_ptr(), -1, None) == -1       # device memory on the host path
    assert r._L.hrt_motion_vectors(r._ctx, None, dev.data_ptr() + 4, 0, None) == -1    # misaligned (and too small)
    # the device copy of the presented image (hrt_device_views.present_color) holds what the host copy received
    shown = _present(r, T.PRESENT_TAAU_REPROJECT, ow, oh)
    v = r.device_views(0)
    assert v.present_width == ow and v.present_height == oh
    back = torch.zeros(ow * oh, dtype=torch.int32, device="cuda:0")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(back.data_ptr(), v.present_color, ow * oh * 4, 3) == 0        # device to device
    torch.cuda.synchronize()
    assert np.array_equal(back.cpu().numpy(), shown), slots
    r.close()
print("DEVICE_PATH_OK")
'''


@pytest.mark.timeout(600)
def test_motion_vectors_device_path_and_present_color(tmp_path):
    """Slot-0 device path of hrt_motion_vectors (a torch tensor) against the host path and the restatement, on one and on two device
    slots, and the device copy of a mode-2 present.  In a process of its own: torch's HIP runtime has to be loaded first."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "reproject_device_worker.py"
    script.write_text(DEVICE_WORKER % {"root": root})
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=540, cwd=root)
    assert out.returncode == 0 and "DEVICE_PATH_OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.parametrize("n", [2, 3])
def test_two_slots(orc, hrt_lib, n):
    """A context over several device slots: slot 0 receives the other slots' gb_worldPos strips before the resolve, and every slot
    computes the motion vectors of its own strips."""
    r = engine.RTRenderer([0] * n)                      # one GPU listed n times: independent slots, as tests/test_multidevice_gpu.py
    try:
        in_w, in_h, ow, oh = 80, 52, 120, 78            # 52 rows: 7 strips, ragged last one
        s = engine.Scene(); scenes.build_textured_test_scene(s); r.commit(s)
        ref = RefHistory(orc, make_taa(orc))
        cam0 = None
        for f in range(3):
            p, low = _frame(r, TEXTURED, in_w, in_h, f, prev_cam=cam0)
            got = _present(r, T.PRESENT_TAAU_REPROJECT, ow, oh)
            want = ref.present(T.PRESENT_TAAU_REPROJECT, low, p.cam, in_w, in_h, ow, oh)
            assert np.array_equal(got, want), "frame %d: %d words differ" % (f, int((got != want).sum()))
            if cam0 is not None:
                mv = r.motion_vectors().reshape(-1, 2)
                assert H.bits_equal(mv, ref.taa.motion_vectors(low["gb_worldPos"], in_w, in_h, cam0, p.cam)).all()
            cam0 = engine.copy_camera(p.cam)
    finally:
        r.close()
