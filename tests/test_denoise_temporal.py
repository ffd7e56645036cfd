"""The temporal denoiser (hrt_denoise_temporal) without a GPU: properties of the filter as include/hip_raytrace.h defines it, checked on
the restatement in tests/denoise_temporal_ref.py with frames from the CPU oracle, and the ABI of the new entry points."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, engine, scenes
from tests import denoise_ref as R
from tests import denoise_temporal_ref as DT
from tests import helpers as H
from tests.taa_reproject_ref import cam_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
TEXTURED = scenes.Config("t", 0, 0, 0, (0.3, 1.3, 4.2), (0.0, 0.7, 0.0))
U = 2.0 ** -24
f32 = np.float32


def _oracle(orc, builder, cfg0, w, h, spp, frame=0, shift=0.0):
    o, l = cfg0.cam_origin, cfg0.cam_lookat
    cfg = scenes.Config("d", w, h, spp, (o[0] + shift, o[1], o[2]), (l[0] + shift, l[1], l[2]), max_depth=cfg0.max_depth, extra=cfg0.extra)
    arrs, _, p = H.oracle_frame(orc, builder, cfg, w, h, spp, frame=frame)
    return arrs, T.Camera.from_buffer_copy(p.cam)


def _plane(orc, W, Hh, d, origin_shift=0.0, normal=(0.0, 0.0, 1.0), push=0.0, rad=None):
    """The set-up of test_closed_form_translation_parallax: a plane facing the camera at distance d (+ push), seen through a camera
    translated along `right` by origin_shift; pixel (x, y)'s point lies under its centre.  Returns (frame, camera dict)."""
    cam0 = orc.camera_lookat((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 40.0, float(f32(W) / f32(Hh)))
    orc.camera_bake(cam0, W, Hh)
    c0 = cam_of(cam0)
    t = DT.make_fns(orc)["tan"](f32(0.5) * c0["fovY"])
    c1 = dict(c0, origin=tuple(f32(c0["origin"][i] + f32(origin_shift) * c0["right"][i]) for i in range(3)))
    dd = f32(d + push)
    wp = np.zeros((W * Hh, 3), np.float32)
    for y in range(Hh):
        for x in range(W):
            nx = (f32(x) + f32(0.5)) / f32(W) * f32(2) - f32(1)
            ny = (f32(y) + f32(0.5)) / f32(Hh) * f32(2) - f32(1)
            wp[y * W + x] = [c1["origin"][i] + dd * c1["forward"][i] + nx * dd * t * c1["aspect"] * c1["right"][i] + ny * dd * t * c1["up"][i] for i in range(3)]
    n = W * Hh
    frame = dict(radiance=np.zeros((n, 3), np.float32) if rad is None else np.asarray(rad, np.float32).reshape(n, 3),
                 gb_normalWS=np.tile(np.array(normal, np.float32), (n, 1)), gb_worldPos=wp,
                 gb_baseColor=np.full((n, 3), 0.5, np.float32), depth=np.full(n, dd, np.float32), gb_hitMask=np.ones(n, np.int32))
    return frame, c1, float(t) * float(c0["aspect"])


def test_first_call_equals_no_history(orc):
    """A fresh history with NO_SPATIAL: hn = 0 on every pixel, so C = c as it is and the output is (radiance / a) * a bit for bit on
    hits; a miss has a = 1 and stays the frame's radiance on every call, with and without the spatial passes."""
    w, h = 64, 64
    fns = DT.make_fns(orc)
    t = DT.Temporal(fns)
    low, cam = _oracle(orc, scenes.build_config1, scenes.CONFIGS[1], w, h, 2)
    hit = low["gb_hitMask"] != 0
    assert hit.any() and (~hit).any()
    out, col = t.step(low, w, h, cam, spatial=False)
    a = fns["fmax"](low["gb_baseColor"][hit], 0.01)
    assert H.bits_equal(out[hit], (low["radiance"][hit] / a) * a).all()
    assert H.bits_equal(out[~hit], low["radiance"][~hit]).all()
    assert np.array_equal(col[~hit], low["color"][~hit])
    assert (t.length.reshape(-1)[hit] == 1).all() and (t.length.reshape(-1)[~hit] == 0).all()
    assert (t.moments.reshape(-1, 2)[~hit] == 0).all()
    for f in (1, 2):
        low, cam = _oracle(orc, scenes.build_config1, scenes.CONFIGS[1], w, h, 2, frame=f)
        out, _ = t.step(low, w, h, cam, spatial=(f == 2), pack=False)
        assert H.bits_equal(out[~hit], low["radiance"][~hit]).all()
        assert not H.bits_equal(out[hit], low["radiance"][hit]).all()            # the history did something
    assert (t.length.reshape(-1)[hit] == 3).all()


def test_static_camera_is_a_running_mean(orc):
    """N = 8 frames, fixed camera, a fresh seed each, NO_SPATIAL, alpha = 1e-30, max_history = 64: the blend factor is 1 / N', so C_k =
    C_{k-1} + (c_k - C_{k-1}) / k, the running mean.  The static camera reads its own pixel with weight 1 (x * 1 / 1 is exact), so the
    only error is the rounding of the N - 1 lerps.
    Bound (derived, not measured), m = the largest |c| of the pixel over the frames, u = 2^-24: every C_k is a convex combination of
    values within [-m, m] up to rounding.  A lerp is 1 / k (one rounding), a subtract of values <= m (result <= 2 m, error <= 2 m u), a
    multiply by ~1 / k (error <= 2 m u for the product and 2 m u for the rounded factor, both at most) and an add of a result <= m
    (<= m u): below 8 m u per lerp, generously, and an earlier error is multiplied by (1 - 1/k) <= 1,
    so after N lerps |C_N - mean| <= 8 N m u, which is asserted ("a few N u times the largest |c|")."""
    N, w, h = 8, 48, 30
    t = DT.Temporal(DT.make_fns(orc))
    cs = []
    for f in range(N):
        low, cam = _oracle(orc, scenes.build_textured_test_scene, TEXTURED, w, h, 1, frame=f)
        t.step(low, w, h, cam, spatial=False, pack=False, alpha_color=1e-30, alpha_moments=1e-30, max_history=64)
        hit = low["gb_hitMask"] != 0
        a = np.where(hit[:, None], DT.make_fns(orc)["fmax"](low["gb_baseColor"], 0.01), f32(1)).astype(np.float32)
        cs.append((low["radiance"] / a).astype(np.float64))
        if f == 0:
            hit0 = hit
        assert np.array_equal(hit, hit0)
        assert (t.length.reshape(-1)[hit] == f + 1).all(), "a pixel reset on frame %d" % f
    mean = np.mean(cs, axis=0)
    m = np.max(np.abs(cs), axis=(0, 2))
    err = np.abs(t.color.reshape(-1, 3).astype(np.float64) - mean).max(axis=1)
    print("running mean: max error / (N u m) = %.3g (bound 8)" % (err[hit0] / (N * U * m[hit0] + 1e-300)).max())
    assert (err[hit0] <= 8 * N * U * m[hit0]).all()
    assert (t.length.reshape(-1)[hit0] == N).all()


@pytest.mark.parametrize("k", [1, 3])
def test_translation_closed_form(orc, k):
    """The plane-and-parallax set-up of test_closed_form_translation_parallax: the camera moves k pixels along `right`, the history
    colour is the ramp c(x) = x.  A pixel whose reprojected position qx = px + k (to within that test's derived 40 W u) lies inside
    the image reads the bilinear history ramp at qx, which for a linear ramp IS qx; with NO_SPATIAL, alpha = 1 the output is the new
    colour, so alpha = 1e-30 and a new colour of 0 give C = hc + (0 - hc) * 0.5 = hc / 2, exactly (halving is exact): 2 C is the
    history value hc the pixel read.  Asserted: |2 C - (px + k)| <= 40 W u, that test's bound.  Columns beyond the border restart
    (length 1).  A history with perpendicular normals, or whose plane is displaced by more than plane_tol * depth, is rejected on
    every pixel."""
    W, Hh, d = 48, 20, 5.0
    fns = DT.make_fns(orc)
    ramp = np.tile(np.arange(W, dtype=np.float32), Hh)
    f0, c0, ta = _plane(orc, W, Hh, d, rad=np.stack([ramp] * 3, -1))
    s = float(f32(k) * f32(2.0) * f32(d) * f32(ta) / f32(W))
    f1, c1, _ = _plane(orc, W, Hh, d, origin_shift=s)
    kw = dict(spatial=False, pack=False, demodulate=False, alpha_color=1e-30, alpha_moments=1e-30)
    t = DT.Temporal(fns)
    t.step(f0, W, Hh, c0, **kw)
    t.step(f1, W, Hh, c1, **kw)
    px = np.arange(W)
    inside, beyond = px + k <= W - 2, px + k >= W
    C, N = t.color.reshape(Hh, W, 3), t.length.reshape(Hh, W)
    tol = 40.0 * W * U
    assert (N[:, inside] == 2).all() and (N[:, beyond] == 1).all()
    err = np.abs(2.0 * C[:, inside, 0].astype(np.float64) - (px[inside] + k))
    print("k=%d: max |2 C - (px + k)| = %.3g, tolerance %.3g" % (k, err.max(), tol))
    assert err.max() <= tol
    assert (C[:, beyond] == 0).all()                          # restarted: the frame's own colour
    # perpendicular normals in the history: dot = 0 < normal_cos_min everywhere
    t = DT.Temporal(fns)
    fp, _, _ = _plane(orc, W, Hh, d, normal=(1.0, 0.0, 0.0), rad=np.stack([ramp] * 3, -1))
    t.step(fp, W, Hh, c0, **kw)
    t.step(f1, W, Hh, c1, **kw)
    assert (t.length == 1).all()
    # a plane displaced along the view axis by 3 % of the depth > plane_tol = 2 %; by 0.5 % it is accepted
    for push, want in ((0.03 * d, 1), (0.005 * d, 2)):
        t = DT.Temporal(fns)
        fq, _, _ = _plane(orc, W, Hh, d, push=-push, rad=np.stack([ramp] * 3, -1))
        t.step(fq, W, Hh, c0, **kw)
        t.step(f0, W, Hh, c0, **kw)                           # static camera, the surface moved
        assert (t.length == want).all(), push


def test_variance(orc):
    """A plane whose radiance is i.i.d. uniform noise on [0, 1) in all channels (lum = 0.2126 + 0.7152 + 0.0722 = 1 times it, variance
    sigma^2 = 1/12), 16 static frames, seeded, alpha = 1e-30 so both moments are running means: step 3's v = M2 - M1^2 is the biased sample
    variance of n = 16 draws, expectation sigma^2 (n - 1) / n.  Its standard deviation is about sigma^2 sqrt((kurt - 1) / n) =
    sigma^2 sqrt(0.8 / 16) = 0.224 sigma^2 for the uniform law (kurtosis 1.8).  Bound: the mean of v over the 48 x 20 = 960 independent
    pixels lies within 5 standard errors (5 * 0.224 / sqrt(960) = 3.7 %) of sigma^2 * 15 / 16, and every pixel within [0, 0.25] (the
    largest variance of values in [0, 1]).  Both are asserted on step 3's v as the restatement computes it (Temporal.step3_variance,
    float32, before any a-trous pass), which also equals max(M2 - M1^2, 0) of the final moments to within 4 u (M <= 1).  With N < 4 (the first three frames) the 7x7 estimate is used: finite, >= 0, and on frame 0,
    where every pixel's M2 - M1^2 is exactly 0, not all zero."""
    W, Hh = 48, 20
    rng = np.random.default_rng(11)
    t = DT.Temporal(DT.make_fns(orc))
    sig2 = 1.0 / 12.0
    for f in range(16):
        x = rng.random(W * Hh).astype(np.float32)
        fr, cam, _ = _plane(orc, W, Hh, 5.0, rad=np.stack([x] * 3, -1))
        t.step(fr, W, Hh, cam, iterations=1, pack=False, demodulate=False, alpha_color=1e-30, alpha_moments=1e-30)
        M1, M2 = t.moments[..., 0].astype(np.float64), t.moments[..., 1].astype(np.float64)
        if f < 3:
            assert (t.length == f + 1).all()
            assert np.isfinite(t.variance).all() and (t.variance >= 0).all()
            assert np.isfinite(t.step3_variance).all() and (t.step3_variance >= 0).all()
            if f == 0:
                assert np.abs(M2 - M1 * M1).max() <= 4 * U and t.step3_variance.max() > 0 and t.variance.max() > 0
    assert (t.length == 16).all()
    v = t.step3_variance.astype(np.float64)                   # step 3's v (the history's variance is iteration 0's v')
    assert np.abs(v - np.maximum(M2 - M1 * M1, 0.0)).max() <= 4 * U          # N = 16 >= 4: the moment branch
    print("variance: mean v = %.5f, expected %.5f (ratio %.4f)" % (v.mean(), sig2 * 15 / 16, v.mean() / (sig2 * 15 / 16)))
    assert abs(v.mean() / (sig2 * 15 / 16) - 1.0) <= 0.037
    assert (v <= 0.25 + 1e-6).all()
    assert np.isfinite(t.variance).all() and (t.variance >= 0).all() and (t.variance <= t.step3_variance.max()).all()      # a weighted mean / ws


CASES = [("textured", scenes.build_textured_test_scene, TEXTURED, True),
         ("config2", scenes.build_config2, scenes.CONFIGS[2], True),
         ("config1", scenes.build_config1, scenes.CONFIGS[1], False)]


def helps(orc, name, builder, cfg0, pan, frames=8, w=120, h=68, truth_spp=128, **kw):
    """Per frame: mean squared error of the clamped radiance of (raw frame, denoise_ref.denoise, the temporal denoiser) against the
    oracle at truth_spp, 2 spp, defaults (or kw)."""
    fns, sfns = DT.make_fns(orc), R.make_fns(orc)
    clamp = lambda x: np.clip(np.asarray(x, np.float64), 0.0, 1.0)
    dist = float(np.linalg.norm(np.subtract(cfg0.cam_origin, cfg0.cam_lookat)))
    step = 2.0 * dist * np.tan(np.radians(cfg0.vfov) / 2) * (w / h) / w if pan else 0.0      # one pixel per frame at the look-at distance
    t = DT.Temporal(fns)
    out, truth = [], None
    for f in range(frames):
        low, cam = _oracle(orc, builder, cfg0, w, h, 2, frame=f, shift=step * f)
        if truth is None or pan:
            truth = clamp(_oracle(orc, builder, cfg0, w, h, truth_spp, frame=1000 + f, shift=step * f)[0]["radiance"])
        mse = lambda x: float(np.mean((clamp(x) - truth) ** 2))
        out.append((mse(low["radiance"]), mse(R.denoise(low, w, h, sfns, pack=False)[0]), mse(t.step(low, w, h, cam, pack=False, **kw)[0])))
    return out


@pytest.mark.timeout(3000)
@pytest.mark.parametrize("pan", [False, True], ids=["static", "pan"])
def test_it_helps(orc, pan):
    """8 frames at 2 spp, 120x68, defaults, against the oracle at 128 spp per frame: from the third frame on, on every frame, the mean
    squared error of the clamped radiance is below the single-frame filter's (tests/denoise_ref.denoise on the same frame) and below
    the raw frame's, on the textured test scene and config 2, under a static camera and under a pan of one pixel per frame.  A
    condition, not a tuned threshold.  Config 1 and alpha = 0.05 are printed.  Measured ratios: DESIGN.md 5.11."""
    failed = []
    for name, builder, cfg0, asserted in CASES:
        for label, kw in (("defaults", {}), ("alpha 0.05", dict(alpha_color=0.05, alpha_moments=0.05))):
            if not asserted and label != "defaults":
                continue
            errs = helps(orc, name, builder, cfg0, pan, **kw)
            for f, (raw, single, temporal) in enumerate(errs):
                print("it helps: %-8s %-6s %-10s frame %d: temporal / raw = %.3f, single / raw = %.3f, temporal / single = %.3f"
                      % (name, "pan" if pan else "static", label, f, temporal / raw, single / raw, temporal / single))
                if asserted and label == "defaults" and f >= 2 and not (temporal < single and temporal < raw):
                    failed.append((name, f, raw, single, temporal))
    assert not failed, failed


OUTSIDE = [("rotated", scenes.build_rotated_instances_scene, scenes.Config("r", 0, 0, 0, (0.4, 1.8, 5.0), (0.0, 0.8, 0.0))),
           ("config3", scenes.build_config3, scenes.CONFIGS[3]),
           ("config4 48x48", lambda b: scenes.build_config4(b, 48, 48), scenes.CONFIGS[4])]


@pytest.mark.timeout(3000)
def test_it_helps_outside_the_scenes_the_default_was_chosen_on(orc):
    """The default sigma_lum was chosen on the two asserted scenes of test_it_helps.  Three scenes that took no part
    in that choice, same protocol: the comparison with the single-frame filter is printed, not asserted (config 3, ten thousand
    spheres of about a pixel at this size, loses to it under the pan: 0.79 - 0.87 against 0.71 - 0.76 of the raw error); asserted is
    only that the temporal denoiser is below the raw frame from the third frame on."""
    failed = []
    for name, builder, cfg0 in OUTSIDE:
        for pan in (False, True):
            for f, (raw, single, temporal) in enumerate(helps(orc, name, builder, cfg0, pan)):
                print("outside: %-13s %-6s frame %d: temporal / raw = %.3f, single / raw = %.3f, temporal / single = %.3f"
                      % (name, "pan" if pan else "static", f, temporal / raw, single / raw, temporal / single))
                if f >= 2 and not temporal < raw:
                    failed.append((name, pan, f, raw, temporal))
    assert not failed, failed


def test_temporal_params_layout_matches_header():
    fields = ["iterations", "flags", "alpha_color", "alpha_moments", "sigma_lum", "sigma_normal", "sigma_plane", "normal_cos_min",
              "plane_tol", "max_history"]
    views = ["color", "moments", "length", "variance", "width", "height", "stride", "reserved"]
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "hip_raytrace.h"
int main(void){
 printf("%%zu %%zu", sizeof(hrt_denoise_temporal_params), sizeof(hrt_denoise_history_views));
 %s
 %s
 printf(" %%d %%d %%d\n", (int)HRT_DENOISE_T_NO_DEMODULATE, (int)HRT_DENOISE_T_NO_SPATIAL, (int)HRT_DENOISE_T_RESET);
 return 0; }''' % ("\n ".join('printf(" %%zu", offsetof(hrt_denoise_temporal_params, %s));' % f for f in fields),
                   "\n ".join('printf(" %%zu", offsetof(hrt_denoise_history_views, %s));' % f for f in views))
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-std=c11", "-I", INC, c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    P, V = T.DenoiseTemporalParams, T.DenoiseHistoryViews
    want = [C.sizeof(P), C.sizeof(V)] + [getattr(P, f).offset for f in fields] + [getattr(V, f).offset for f in views] + \
           [T.DENOISE_T_NO_DEMODULATE, T.DENOISE_T_NO_SPATIAL, T.DENOISE_T_RESET]
    assert got == want


def test_shipped_library_exports_the_temporal_denoiser(hrt_lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert {"hrt_denoise_temporal", "hrt_denoise_history", "hrt_denoise_history_read", "hrt_denoise", "hrt_denoised_buffers"} <= exported
