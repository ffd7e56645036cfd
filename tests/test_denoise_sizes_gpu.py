"""hrt_denoise and hrt_denoise_temporal at the sizes they ship at and across every tile seam of their iteration kernels, against the
restatements in tests/denoise_ref.py and tests/denoise_temporal_ref.py.  Every comparison is the one of tests/test_denoise_gpu.py and
tests/test_denoise_temporal_gpu.py: all words of radiance and colour (and of the four history planes) as 32-bit patterns, no pixel
excluded.

The iteration kernels give every 32x8 tile of one sub-lattice of tap step s to a workgroup that stages 36x12 records
(tests/denoise_tiles.py models the launch).  tests/test_denoise_tiles.py proves that CASES cross a seam and take the whole-workgroup
return with a non-empty sub-lattice along both axes at every step 1..128.  With the default sigmas a tap 16 or more pixels away
mostly gets a weight that underflows to 0 and is skipped, so a wrong halo record would change no bit: every case also runs "open",
with sigmas so wide that every hit-to-hit tap counts, and the restatement's SeamTaps diagnostic shows that the taps across the seams
did count (at least half of the hit pixels that have one inside the image; a condition on the inputs, computed in the restatement,
never from the device result).  The scene is config 2, whose walls fill the view at any aspect ratio.

Cost on the CPU side (numpy restatement, about 12 us per pixel and five passes): see the docstrings of the tests over a minute."""
import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, scenes
from tests import denoise_ref as R
from tests import denoise_temporal_ref as DT
from tests import denoise_tiles as DTL
from tests import test_denoise_gpu as SG
from tests import test_denoise_temporal_gpu as TG
from tests.test_present_reproject import make_taa
from tests.test_present_reproject_gpu import RefHistory

pytestmark = pytest.mark.gpu

CONFIG2 = (scenes.build_config2, scenes.CONFIGS[2])
OPEN = dict(sigma_color=1e3, sigma_normal=1e3, sigma_plane=1e3)            # 1e30 would overflow the squared sigma
OPEN_TEMPORAL = dict(sigma_lum=1e3, sigma_normal=1e3, sigma_plane=1e3)
SIGMAS = {"default": None, "open": True}


def _guard(taps, w, h, iterations, what):
    """The far taps across every seam the case claims did count."""
    seams = DTL.seam_steps(w, h, iterations)
    assert [p["step"] for p in taps.passes] == [1 << i for i in range(iterations)]
    for p in taps.passes:
        for axis in sorted(seams.get(p["step"], ())):
            took, could = p[axis]
            print("%s: step %d %s seam taps taken for %d of %d hit pixels" % (what, p["step"], axis, took, could))
            assert could > 0 and 2 * took >= could, (what, p["step"], axis, took, could)


class TapTemporal(DT.Temporal):
    """The restatement, filling self.taps (a fresh R.SeamTaps per step when wanted)."""
    taps = None

    def step(self, *a, **kw):
        return super().step(*a, seam_taps=self.taps, **kw)


# ---------------------------------------------------------------------------------------------------------------- (a, b) tile geometry
@pytest.mark.timeout(900)
@pytest.mark.parametrize("sigmas", list(SIGMAS))
@pytest.mark.parametrize("case", DTL.CASES, ids=lambda c: "%dx%d_it%d" % c)
def test_tile_geometry_spatial(orc, renderer, monkeypatch, case, sigmas):
    """4097 x 1025 with 8 passes: about 115 s of restatement per run on one core, the others a few seconds."""
    w, h, it = case
    SG._commit(renderer, CONFIG2[0])
    _, low = SG._render(renderer, CONFIG2[1], w, h)
    kw = dict(iterations=it, **(OPEN if SIGMAS[sigmas] else {}))
    taps = R.SeamTaps()
    plain = R.denoise
    monkeypatch.setattr(R, "denoise", lambda *a, **k: plain(*a, seam_taps=taps, **k))     # SG._check's own call, with the diagnostic
    what = "%dx%d %s" % (w, h, sigmas)
    SG._check(orc, renderer, low, w, h, what, **kw)
    if SIGMAS[sigmas]:
        _guard(taps, w, h, it, what)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("sigmas", list(SIGMAS))
@pytest.mark.parametrize("case", DTL.TEMPORAL_CASES, ids=lambda c: "%dx%d_it%d" % c)
def test_tile_geometry_temporal(orc, renderer, case, sigmas):
    """Three frames under a sideways shift: the history taps and the 7x7 variance window run as well."""
    w, h, it = case
    TG._commit(renderer, CONFIG2[0])
    ref = TapTemporal(DT.make_fns(orc))
    kw = dict(iterations=it, **(OPEN_TEMPORAL if SIGMAS[sigmas] else {}))
    for f in range(3):
        p, low = TG._render(renderer, CONFIG2[1], w, h, frame=f, shift=0.03 * f)
        ref.taps = R.SeamTaps()
        what = "%dx%d %s frame %d" % (w, h, sigmas, f)
        TG._check(orc, renderer, ref, low, p.cam, w, h, what, **kw)
        if SIGMAS[sigmas]:
            _guard(ref.taps, w, h, it, what)
    assert ref.length.max() == 3


# ---------------------------------------------------------------------------------------------------------------- (c) shipping sizes
@pytest.mark.timeout(900)
@pytest.mark.parametrize("size", [(1286, 724), (1920, 1080), (3840, 2160)], ids=lambda s: "%dx%d" % s)
def test_shipping_sizes_spatial(orc, renderer, size):
    """One frame, default parameters: the operating point's internal size, the bench and README size, the size of configs 4 and 5."""
    w, h = size
    SG._commit(renderer, CONFIG2[0])
    _, low = SG._render(renderer, CONFIG2[1], w, h)
    SG._check(orc, renderer, low, w, h, "%dx%d" % size)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("size", [(1286, 724), (1920, 1080)], ids=lambda s: "%dx%d" % s)
def test_shipping_sizes_temporal(orc, renderer, size):
    """Four frames under a pan of about a pixel per frame: past N = 4, where the variance switches from the 7x7 window to the pixel's
    own moments and workgroups along the disoccluded strip mix both paths."""
    w, h = size
    TG._commit(renderer, scenes.build_textured_test_scene)
    ref = DT.Temporal(DT.make_fns(orc))
    for f in range(4):
        p, low = TG._render(renderer, TG.TEXTURED, w, h, frame=f, shift=0.05 * 97 / w * f)      # the pan of the 97-wide sequences, in pixels
        TG._check(orc, renderer, ref, low, p.cam, w, h, "%dx%d frame %d" % (w, h, f))
    n = ref.length[np.asarray(low["gb_hitMask"]).reshape(h, w) != 0]
    assert (n >= 4).any() and (n < 4).any()                 # both variance paths ran on the last frame


# ---------------------------------------------------------------------------------------------------------------- (d) the documented pipeline
@pytest.mark.timeout(900)
def test_pipeline_at_the_operating_point(orc, renderer):
    """Render at the operating point's internal size (1286 x 724, 2 spp, a moving camera), hrt_denoise_temporal, then hrt_present with
    HRT_PRESENT_TAAU_REPROJECT | HRT_PRESENT_DENOISED, four frames on one history: equals the reference present
    (RefHistory of tests/test_present_reproject_gpu.py) fed the restatement's denoised colour, as test_present_denoised at 48 x 30.
    The display is 480 x 270, not the 1920 x 1080 of the operating point: the present restatement is scalar Python, 410 us per
    output pixel measured (3400 s for four 1920 x 1080 frames); at 480 x 270 it takes about 215 s, the four denoiser restatements
    about 120 s.  What reaches the present is the full 1286 x 724 denoised plane either way."""
    in_w, in_h, ow, oh = 1286, 724, 480, 270
    SG._commit(renderer, scenes.build_textured_test_scene)
    dref = DT.Temporal(DT.make_fns(orc))
    ref = RefHistory(orc, make_taa(orc))
    for f in range(4):
        p, low = SG._render(renderer, SG.TEXTURED, in_w, in_h, spp=2, frame=f, pan=0.004)
        _, col = TG._check(orc, renderer, dref, low, p.cam, in_w, in_h, "frame %d" % f)
        dn = dict(low); dn["color"] = col.reshape(-1)         # equal to the restatement's, word for word: _check has just said so
        got = renderer.present(ow, oh, taau=True, reproject=True, denoised=True)
        want = ref.present(T.PRESENT_TAAU_REPROJECT, dn, p.cam, in_w, in_h, ow, oh)
        assert np.array_equal(got, want), "frame %d: %d words differ" % (f, int((got != want).sum()))
