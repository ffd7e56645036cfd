"""The a-trous denoiser (hrt_denoise) without a GPU: properties of the filter as include/hip_raytrace.h defines it, checked on the
restatement in tests/denoise_ref.py with frames from the CPU oracle, and the ABI of the new entry points."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, engine, scenes
from tests import denoise_ref as R
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
TEXTURED = scenes.Config("t", 0, 0, 0, (0.3, 1.3, 4.2), (0.0, 0.7, 0.0))
U = 2.0 ** -24
f32 = np.float32


def _oracle_low(orc, builder, cfg0, w, h, spp):
    cfg = scenes.Config("d", w, h, spp, cfg0.cam_origin, cfg0.cam_lookat, extra=cfg0.extra)
    arrs, _, _ = H.oracle_frame(orc, builder, cfg, w, h, spp)
    return arrs


def _plane_frame(w, h, rad, normal=(0.0, 0.0, 1.0)):
    """A plane facing the camera: one normal, every P with the same z, every pixel a hit."""
    yy, xx = np.mgrid[0:h, 0:w]
    P = np.stack([xx * 0.1, yy * 0.1, np.full((h, w), -5.0)], -1).astype(np.float32).reshape(-1, 3)
    n = np.tile(np.array(normal, np.float32), (w * h, 1))
    return dict(radiance=np.asarray(rad, np.float32).reshape(-1, 3), gb_normalWS=n, gb_worldPos=P,
                gb_baseColor=np.full((w * h, 3), 0.5, np.float32), depth=np.full(w * h, 5.0, np.float32),
                gb_hitMask=np.ones(w * h, np.int32))


def test_misses_and_hostile_pixels_keep_their_value(orc):
    """Config 1 is mostly sky: every miss of the output is bit-equal to the frame's radiance (a = 1: x / 1 * 1 is x).  A block of NaN
    normals: dn is NaN for every tap of such a pixel, its own included, so no w passes w > 0 and the pixel keeps its c; the output
    is c * a, which is the input radiance bit for bit without demodulation and (radiance / a) * a with it."""
    w, h = 64, 64
    low = _oracle_low(orc, scenes.build_config1, scenes.CONFIGS[1], w, h, 2)
    fns = R.make_fns(orc)
    hit = low["gb_hitMask"] != 0
    assert 0.5 < (~hit).mean() < 1.0 and hit.any()
    out, col = R.denoise(low, w, h, fns)
    assert H.bits_equal(out[~hit], low["radiance"][~hit]).all()
    assert np.array_equal(col[~hit], low["color"][~hit])                   # and packs to the frame's own colour
    assert not H.bits_equal(out[hit], low["radiance"][hit]).all()            # the filter did something
    hostile = {k: v.copy() for k, v in low.items()}
    block = np.zeros((h, w), bool)
    ys, xs = np.nonzero(hit.reshape(h, w))
    block[ys.min():ys.min() + 6, xs.min():xs.max() + 1] = True
    block = (block & hit.reshape(h, w)).reshape(-1)
    assert block.sum() >= 4
    hostile["gb_normalWS"][block] = np.nan
    raw, _ = R.denoise(hostile, w, h, fns, demodulate=False)
    assert H.bits_equal(raw[block], low["radiance"][block]).all()
    dem, _ = R.denoise(hostile, w, h, fns)
    a = orc.math_eval("fmax", low["gb_baseColor"][block], np.full_like(low["gb_baseColor"][block], 0.01)).reshape(-1, 3)
    assert H.bits_equal(dem[block], (low["radiance"][block] / a) * a).all()
    assert np.isfinite(dem).all() and np.isfinite(raw).all()


def test_closed_form_b3_spline(orc):
    """One iteration on a plane facing the camera with sigma_color = 1e30 is the 5x5 B3-spline convolution.
    n is constant, so dn = 0; every P has the same z and n = (0, 0, 1), so d = 0 * dx' + 0 * dy' + 0 * 1 = 0 exactly; sc * sc
    overflows to +inf, so kc = 0 and dc * kc = 0: e = 0 exactly and w = h[dx] h[dy] exp(-0) = h[dx] h[dy] (exact products), provided
    hrt_exp(-0.0f) is exactly 1, which is asserted first.
    Bound (derived, not measured): acc is 25 products and 24 adds of non-negative terms, ws 24 adds, then one divide: every
    operation has relative error <= u = 2^-24 and non-negative terms do not cancel, so the relative error of acc / ws against the exact
    convolution (whose weights sum to 1) is at most (1 + u)^(26 + 24 + 1) - 1 < 60 u."""
    fns = R.make_fns(orc)
    assert fns[0](np.array([-0.0], np.float32)).view(np.uint32)[0] == 0x3F800000
    w, h = 23, 17
    rng = np.random.default_rng(7)
    rad = rng.random((h, w, 3)).astype(np.float32)
    out, _ = R.denoise(_plane_frame(w, h, rad), w, h, fns, iterations=1, sigma_color=1e30, demodulate=False, pack=False)
    out = out.reshape(h, w, 3).astype(np.float64)
    k = np.outer(R.H5.astype(np.float64), R.H5.astype(np.float64))
    want = np.zeros((h, w, 3))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            want[2:h - 2, 2:w - 2] += k[dy + 2, dx + 2] * rad.astype(np.float64)[2 + dy:h - 2 + dy, 2 + dx:w - 2 + dx]
    inner = (slice(2, h - 2), slice(2, w - 2))
    rel = np.abs(out[inner] - want[inner]) / want[inner]
    print("closed form: max relative error %.3g u" % (rel.max() / U))
    assert rel.max() <= 60 * U


def test_edges_stop(orc):
    """Two half-planes with perpendicular normals and different constant colours, sigma_normal = 0.5 (kn = 4): a cross-edge tap has
    dn = |(0,0,1) - (1,0,0)|^2 = 2, so e >= 8 (the other two terms are >= 0) and its weight is <= h[dx] h[dy] exp(-8); the
    cross-edge weights sum to at most exp(-8) (h sums to 1) and the same-side weights to at least the centre's 9/64 (e = 0 there).
    After one iteration a pixel therefore moves toward the other side by at most exp(-8) / (9/64) = 0.0024 of the difference, plus
    the 60 u rounding of the closed-form case."""
    fns = R.make_fns(orc)
    w, h = 24, 12
    left = np.zeros((h, w), bool); left[:, :w // 2] = True
    cl, cr = np.array([0.8, 0.2, 0.4], np.float32), np.array([0.1, 0.9, 0.6], np.float32)
    rad = np.where(left[..., None], cl, cr).astype(np.float32)
    fr = _plane_frame(w, h, rad)
    n = np.where(left[..., None], np.array([0, 0, 1], np.float32), np.array([1, 0, 0], np.float32)).astype(np.float32)
    fr["gb_normalWS"] = n.reshape(-1, 3)
    yy, xx = np.mgrid[0:h, 0:w]
    Pr = np.stack([np.full((h, w), 0.1 * (w // 2)), yy * 0.1, -5.0 - 0.1 * (xx - w // 2)], -1)
    fr["gb_worldPos"] = np.where(left[..., None], fr["gb_worldPos"].reshape(h, w, 3), Pr).astype(np.float32).reshape(-1, 3)
    out, _ = R.denoise(fr, w, h, fns, iterations=1, sigma_normal=0.5, demodulate=False, pack=False)
    out = out.reshape(h, w, 3).astype(np.float64)
    own = rad.astype(np.float64)
    diff = np.abs(cr.astype(np.float64) - cl.astype(np.float64))
    frac = np.exp(-8.0) / (9.0 / 64.0)
    moved = np.abs(out - own)
    print("edges: max move %.3g of the difference (bound %.3g)" % ((moved / diff).max(), frac))
    assert (moved <= (frac + 60 * U) * diff + 60 * U * own).all()
    assert moved[:, w // 2 - 2:w // 2 + 2].max() > 0.0               # the edge columns do see the other side, a little


CASES = [("textured", scenes.build_textured_test_scene, TEXTURED, True),
         ("config2", scenes.build_config2, scenes.CONFIGS[2], True),
         ("config1", scenes.build_config1, scenes.CONFIGS[1], False)]


@pytest.mark.timeout(900)
def test_it_helps(orc):
    """120x68, 2 spp against the oracle at 256 spp, defaults: the mean squared error of radiance clamped to [0, 1] goes down on the
    textured test scene and on config 2 (asserted); config 1, a sphere on noise-free sky, and NO_DEMODULATE are printed."""
    fns = R.make_fns(orc)
    w, h = 120, 68
    clamp = lambda x: np.clip(x.astype(np.float64), 0.0, 1.0)
    for name, builder, cfg0, asserted in CASES:
        low = _oracle_low(orc, builder, cfg0, w, h, 2)
        truth = clamp(_oracle_low(orc, builder, cfg0, w, h, 256)["radiance"])
        raw = np.mean((clamp(low["radiance"]) - truth) ** 2)
        ratios = {}
        for demod in (True, False):
            out, _ = R.denoise(low, w, h, fns, demodulate=demod, pack=False)
            ratios[demod] = np.mean((clamp(out) - truth) ** 2) / raw
        print("it helps: %-9s denoised / raw = %.3f (NO_DEMODULATE %.3f)" % (name, ratios[True], ratios[False]))
        if asserted:
            assert ratios[True] < 1.0, name


def test_denoise_params_layout_matches_header():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "hip_raytrace.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu %d %d\n", sizeof(hrt_denoise_params), offsetof(hrt_denoise_params, iterations),
   offsetof(hrt_denoise_params, flags), offsetof(hrt_denoise_params, sigma_color), offsetof(hrt_denoise_params, sigma_normal),
   offsetof(hrt_denoise_params, sigma_plane), (int)HRT_DENOISE_NO_DEMODULATE, (int)HRT_PRESENT_DENOISED);
 return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "s.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "s")
        subprocess.check_call(["gcc", "-std=c11", "-I", INC, c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    P = T.DenoiseParams
    want = [C.sizeof(P), P.iterations.offset, P.flags.offset, P.sigma_color.offset, P.sigma_normal.offset, P.sigma_plane.offset,
            T.DENOISE_NO_DEMODULATE, T.PRESENT_DENOISED]
    assert got == want


def test_shipped_library_exports_the_denoiser(hrt_lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", engine.LIB_PATH]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert {"hrt_denoise", "hrt_denoised_buffers"} <= exported
