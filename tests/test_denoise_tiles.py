"""The tile geometry the denoisers' device tests cover, proved from the model in tests/denoise_tiles.py without a GPU: the sizes of
tests/test_denoise_sizes_gpu.py cross a tile seam and take the whole-workgroup return with a non-empty sub-lattice along both axes
at every tap step, and the sizes the suite used before did neither from step 8 up."""
import numpy as np

from tests import denoise_ref as R
from tests import denoise_tiles as DTL

STEPS = [1 << i for i in range(8)]


def test_model_against_a_brute_force_enumeration():
    """classes() against a direct walk over launch_iter's grid, workgroup by workgroup, at sizes small enough to enumerate."""
    for W, H, it in [(129, 33, 5), (97, 61, 8), (20, 12, 5), (1, 1, 5), (200, 125, 5), (517, 133, 5), (33, 9, 4)]:
        want = set()
        for i in range(it):
            s = 1 << i
            gx, gy, gz = DTL.grid(W, H, s)
            assert gz == s * s
            for z in range(gz):
                oy, ox = divmod(z, s)
                nx, ny = (W - ox + s - 1) // s, (H - oy + s - 1) // s               # the kernels' own expressions
                for axis, n, g, tile in (("x", nx, gx, 32), ("y", ny, gy, 8)):
                    live = [b for b in range(g) if b * tile < n]                    # workgroups that pass `b * tile >= n -> return`
                    if n <= 0:
                        want.add((s, axis, "empty_lattice"))
                        continue
                    if len(live) >= 2:
                        want.add((s, axis, "seam"))
                    if len(live) < g:
                        want.add((s, axis, "short_lattice"))
                    if n - live[-1] * tile < tile:
                        want.add((s, axis, "ragged_tile"))
        assert DTL.classes(W, H, it) == want, (W, H, it)


def test_cases_cover_every_seam_and_short_lattice():
    for cases in (DTL.CASES, DTL.TEMPORAL_CASES):
        got = DTL.union(cases)
        for s in STEPS:
            for axis in "xy":
                assert (s, axis, "seam") in got, (s, axis)
                if s >= 2:                                  # step 1 has one sub-lattice: nothing to be shorter than
                    assert (s, axis, "short_lattice") in got, (s, axis)
        kinds = {k for _, _, k in got}
        assert {"empty_lattice", "ragged_tile"} <= kinds
    assert not any(k == "short_lattice" for s, _, k in DTL.union(DTL.CASES) if s == 1)


def test_issue_sizes_are_what_they_claim():
    c = DTL.classes(129, 33, 5)
    assert {(s, a, "short_lattice") for s in (2, 4) for a in "xy"} <= c
    c = DTL.classes(517, 133, 5)
    assert {(s, a, k) for s in (8, 16) for a in "xy" for k in ("seam", "short_lattice")} <= c
    c = DTL.classes(4097, 1025, 8)
    assert {(s, a, k) for s in (32, 64, 128) for a in "xy" for k in ("seam", "short_lattice")} <= c
    assert {(s, "x", k) for s in (32, 64, 128) for k in ("seam", "short_lattice")} <= DTL.classes(4097, 24, 8)
    assert {(s, "y", k) for s in (32, 64, 128) for k in ("seam", "short_lattice")} <= DTL.classes(40, 1025, 8)


def test_the_sizes_used_before_left_the_gap():
    """The record of what tests/test_denoise_sizes_gpu.py closes: over every size the two device test modules ran, from step 8 up no
    sub-lattice took the whole-workgroup return with pixels in it and none spanned two tiles, but for the 16 rows per sub-lattice of
    200 x 125 at step 8.  Below step 8 the one short sub-lattice is 56 x 34 at step 4 (9 / 8 rows), a size at which no test compares
    the denoised image with anything."""
    old = DTL.union(DTL.OLD_SIZES)
    assert {(s, a, k) for s, a, k in old if s >= 8 and k in ("seam", "short_lattice")} == {(8, "y", "seam")}
    assert DTL.seam_steps(200, 125).get(8) == {"y"}
    assert {(s, a) for s, a, k in old if k == "short_lattice"} == {(4, "y")}
    assert [c[:2] for c in DTL.OLD_SIZES if (4, "y", "short_lattice") in DTL.classes(*c)] == [(56, 34)]


def test_seam_taps_diagnostic_counts_what_it_says():
    """tests/denoise_ref.SeamTaps on a plane of equal pixels (every tap inside the image is taken): at 70 x 20, step 1, the pixels
    with an outer-ring tap in another tile along x are the columns 30, 31 | 32, 33 and 62, 63 | 64, 65; along y the rows 6, 7 | 8, 9
    and 14, 15 | 16, 17.  At step 2 the lattice coordinate is x div 2: 35 columns per sub-lattice, one seam, columns 60..67."""
    from tests.test_denoise import _plane_frame

    ident = lambda x: np.ones_like(x)                        # exp: every weight positive
    fns = (ident, lambda a, b: np.maximum(a, np.float32(b)), None)
    w, h = 70, 20
    st = R.SeamTaps()
    R.denoise(_plane_frame(w, h, np.full((h, w, 3), 0.5, np.float32)), w, h, fns, iterations=2, pack=False, seam_taps=st)
    assert [p["step"] for p in st.passes] == [1, 2]
    assert st.passes[0]["x"] == (8 * h, 8 * h) and st.passes[0]["y"] == (8 * w, 8 * w)
    assert st.passes[1]["x"] == (8 * h, 8 * h)               # lattice columns 30..33 of both sub-lattices: x = 60..67
    assert st.passes[1]["y"] == (8 * w, 8 * w)               # 10 rows per sub-lattice, tiles of 8: rows 6..9 of each, y = 12..19
