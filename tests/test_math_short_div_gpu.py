"""The short divide forms of hrt_device.hpp (rcp_normal_range, recip_of + div_by) and the wave-uniform guards of their hot sites
(inv_dir, TracerFlat's sphere step with the sqrt of the discriminant) against the IEEE results hipcc compiles for / and sqrtf."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32


def test_short_forms_equal_ieee_over_their_domains(hooks_renderer):
    """2: 1 / x for every float of rcp_domain; 3: n / d for every float n and 1028 denominators of [1, 4), edges included;
    4: 2^34 hashed pairs.  Exhaustive on the device, compared with the device's own IEEE divide."""
    for which in (2, 3, 4):
        bad, first = hooks_renderer.math_exhaustive(which)
        assert bad == 0, "case %d: %d mismatches, first numerator bits 0x%08X" % (which, bad, first)


def test_short_forms_match_host_ieee_division(hooks_renderer):
    """The raw forms on a sample, against numpy's correctly rounded float32 division, so 'IEEE on the device' is pinned too."""
    rng = np.random.default_rng(41)
    x = (rng.choice([-1.0, 1.0], 1 << 20) * 2.0 ** rng.uniform(-94, 125, 1 << 20)).astype(f32)
    x = np.concatenate([x, np.array([2.0 ** -94, 2.0 ** 125, -(2.0 ** -94), -(2.0 ** 125), 1.0, 1.0 - 2.0 ** -24], f32)])
    assert np.array_equal((f32(1) / x).view(np.uint32), hooks_renderer.math_probe(28, x).view(np.uint32))
    n = (rng.choice([-1.0, 1.0], 1 << 20) * 2.0 ** rng.uniform(-100, 127.9, 1 << 20)).astype(f32)
    d = rng.uniform(1.0, 4.0, 1 << 20).astype(f32)
    d = np.minimum(d, np.nextafter(f32(4), f32(0)))
    assert np.array_equal((n / d).view(np.uint32), hooks_renderer.math_probe(29, n, d).view(np.uint32))


def _inv_dir_ref(a):
    a = np.where(a != 0, a, f32(1e-8)).astype(f32)
    with np.errstate(divide="ignore", over="ignore"):
        return f32(1) / a


def test_inv_dir_guard_falls_back_per_wave(hooks_renderer):
    """Waves wholly in rcp_domain take the short reciprocal; a wave with one lane outside it (denormal, tiny, huge, NaN, +-inf)
    takes 1.0f / x for every lane.  Both give the IEEE bits; every 64-lane wave below is one of the two kinds."""
    rng = np.random.default_rng(42)
    inside = rng.uniform(-1.0, 1.0, 64 * 64).astype(f32)
    inside[::97] = 0.0                                             # -> 1e-8, in the domain
    outside = rng.uniform(-1.0, 1.0, 64 * 64).astype(f32)
    odd = np.array([1e-40, -1e-45, 2.0 ** -95, 2.0 ** 126, 3e38, np.inf, -np.inf, np.nan], f32)
    outside[::64] = np.resize(odd, 64)                             # one per wave
    for a in (inside, outside):
        b = np.full_like(a, 0.5)
        got = hooks_renderer.math_probe(30, a, b)
        ref = _inv_dir_ref(a)
        fin = ~np.isnan(ref)
        assert np.array_equal(got[fin].view(np.uint32), ref[fin].view(np.uint32))
        assert np.isnan(got[~fin]).all()


def _sphere_ref(cz, dz):
    """hit_sphere_ta in float32, one rounding per operation: ray (0,0,0) + t (0,0,dz), sphere (0.25, 0, cz) of radius 1."""
    with np.errstate(all="ignore"):
        z = f32(0)
        ocx, ocy, ocz = f32(-0.25) * np.ones_like(cz), np.zeros_like(cz), z - cz
        a = (z * z + z * z) + dz * dz
        b = f32(2) * ((ocx * z + ocy * z) + ocz * dz)
        cc = ((ocx * ocx + ocy * ocy) + ocz * ocz) - f32(1) * f32(1)
        disc = b * b - (f32(4) * a) * cc
        sq = np.sqrt(np.maximum(disc, z))
        t1 = (-b - sq) / (f32(2) * a)
        t2 = (-b + sq) / (f32(2) * a)
        t = np.where(t1 < f32(0.001), t2, t1)
        return np.where((disc >= 0) & (t >= f32(0.001)) & ~((t1 < f32(0.001)) & (t2 < f32(0.001))), t, f32(-1)).astype(f32)


def test_sphere_step_guards_fall_back_per_wave(hooks_renderer):
    """TracerFlat's sphere step: waves of normalised-length rays take div_by and sqrt_normal_range; a wave with a ray of
    |d|^2 outside [0.5, 2) takes the IEEE divide, and one with 0 < disc < 2^-96 (|d| ~ 1e-20) takes hrt_sqrt too."""
    rng = np.random.default_rng(43)
    w = 64 * 256
    cz = rng.uniform(-4.0, 4.0, w).astype(f32)
    dz = rng.choice([-1.0, 1.0], w).astype(f32) * rng.uniform(0.71, 1.41, w).astype(f32)
    long_ = dz.copy()
    long_[::64] = f32(3.0)                                         # a = 9: Recip guard
    tiny = dz.copy()
    tiny[::64] = f32(1e-20)                                        # a and disc denormal: both guards
    cz[::128] = f32(0.5)                                           # some origins inside the sphere (second root)
    for d in (dz, long_, tiny):
        got = hooks_renderer.math_probe(31, cz, d)
        ref = _sphere_ref(cz, d)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert (_sphere_ref(cz, dz) > 0).any() and (_sphere_ref(cz, dz) < 0).any()
