"""Multi-hit ray queries (hrt_trace_hits) without a GPU: the CPU restatement (tests/hits_ref.py) against CLOSEST and OCCLUDED, the
entry point in the header, both libraries and the C# binding, and the Python wrapper's argument checks."""
import os
import re
import subprocess

import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, engine, scenes
from oracle import orc_indep as OI
from tests import hits_ref as HR
from tests.test_ray_query import _decl, _renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
f32 = np.float32


def _scene(orc, builder):
    so = orc.OrcScene()
    builder(so)
    return so, so.arrays()


def _rays(arrs, n, seed):
    """Rays from a camera-like point into the scene, rays from inside its bounds, and hostile ones (non-finite, zero, huge)."""
    rng = np.random.default_rng(seed)
    r = arrs["tlasNodes"][0]
    lo = np.array([r["boundsMin"][a] for a in "XYZ"], np.float32)
    hi = np.array([r["boundsMax"][a] for a in "XYZ"], np.float32)
    o = (lo + (hi - lo) * rng.random((n, 3), dtype=np.float32)).astype(np.float32)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    o[: n // 3] = np.array([0.0, 1.4, 4.5], np.float32)
    d[: n // 3, 2] = -np.abs(d[: n // 3, 2]) - f32(1.0)
    return o, d


SCENES = [
    ("default", lambda b: b.build_default_scene()),
    ("config1", scenes.build_config1),
    ("config2", scenes.build_config2),
    ("textured", scenes.build_textured_test_scene),
]


@pytest.mark.parametrize("name,builder", SCENES, ids=[s[0] for s in SCENES])
def test_first_record_is_closest_and_totals_are_occlusion(orc, name, builder):
    so, arrs = _scene(orc, builder)
    V = HR.views(orc, arrs)
    o, d = _rays(arrs, 90, len(name))
    hits, counts, totals = HR.trace_hits(V, o, d, 4, np.float32(np.inf))
    g = HR.unpack(hits)
    ref = orc.trace_rays(so.desc(), o, d)
    sel = (g["t"][:, 1] != g["t"][:, 0]) & (g["t"][:, 0] < f32(1e29))
    assert sel.sum() > 10
    for f in ("t", "normal", "albedo", "objId", "shade"):
        eq = HR.bits(g[f][sel, 0]) == HR.bits(ref[f][sel])
        eq = eq.all(axis=-1) if eq.ndim > 1 else eq
        assert eq.all(), (name, f, np.flatnonzero(~eq)[:5])
    assert ((counts > 0) == (ref["hit"] != 0)).all()
    assert (counts == np.minimum(totals, 4)).all()
    # sorted by (t bits, instance, prim); padding is CLOSEST's miss record
    for i in range(len(o)):
        keys = [(int(HR.bits(g["t"][i, j:j + 1])[0]), int(g["instance"][i, j]), int(g["prim"][i, j])) for j in range(counts[i])]
        assert keys == sorted(keys)
        for j in range(counts[i], 4):
            assert g["t"][i, j] == f32(1e30) and g["instance"][i, j] == -1 and g["prim"][i, j] == -1 and g["objId"][i, j] == -1
    # no alpha maps: an accepted test is exactly what ShadowOcclusion stops at, for any tMax
    alpha = len(arrs["materials"]) > 0 and bool((arrs["materials"]["HasAlphaMap"] != 0).any())
    if not alpha:
        rng = np.random.default_rng(3)
        tm = np.array([1e29, 0.0, -1.0, np.nan, np.inf, 2.0, 5.0, 0.5], np.float32)[rng.integers(0, 8, len(o))]
        _, _, tt = HR.trace_hits(V, o, d, 1, tm)
        for i in range(len(o)):
            w = (tuple(map(f32, o[i])), tuple(map(f32, d[i])), OI.inv_dir(tuple(map(f32, d[i]))))
            with np.errstate(all="ignore"):
                assert (tt[i] > 0) == V.shadow_occlusion(w, f32(tm[i])), (name, i, tm[i])


def test_restatement_on_hostile_rays(orc):
    """Non-finite, zero and huge rays and every kind of tMax: the walk does not fail and k only truncates."""
    so, arrs = _scene(orc, scenes.build_textured_test_scene)
    V = HR.views(orc, arrs)
    o, d = _rays(arrs, 40, 1)
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, 1e19], np.float32)
    o[::4, 0] = specials[np.arange(len(o[::4])) % len(specials)]
    d[1::4, 1] = specials[np.arange(len(d[1::4])) % len(specials)]
    d[2::9] = 0.0
    tm = np.array([1e29, 0.0, -1.0, np.nan, np.inf, -np.inf, 3.0], np.float32)[np.arange(len(o)) % 7]
    h16, c16, t16 = HR.trace_hits(V, o, d, 16, tm)
    h3, c3, t3 = HR.trace_hits(V, o, d, 3, tm)
    assert (t3 == t16).all() and (c3 == np.minimum(t16, 3)).all()
    HR.assert_same(HR.unpack(h3), {f: a[:, :3] for f, a in HR.unpack(h16).items()}, "k=3 vs k=16")
    assert (c16[tm <= 0] == 0).all() and (c16[np.isnan(tm)] == 0).all()


def test_header_declares_trace_hits():
    src = open(os.path.join(INC, "hip_raytrace.h")).read()
    args = [a.strip() for a in _decl(src, "hrt_trace_hits").split(",")]
    assert args == ["hrt_ctx* ctx", "const hrt_ray* rays", "int64_t n", "int32_t k", "hrt_ray_hit* hits", "int32_t* counts",
                    "int32_t* totals", "int32_t dev", "float* device_ms"]
    m = re.search(r"#define HRT_HITS_MAX (\d+)", src)
    assert m and int(m.group(1)) == 16 == T.HITS_MAX
    block = src[src.index("multi-hit queries"):src.index("int  hrt_trace_hits")]
    assert re.search(r"SceneDeviceViews\.cs:\d+", block)


def test_both_libraries_export_trace_hits(hrt_lib, hooks_lib):
    for path in (engine.LIB_PATH, engine.HOOKS_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert "hrt_trace_hits" in {l.split()[-1] for l in out.splitlines() if l.strip()}, path
    assert hasattr(hrt_lib, "hrt_trace_hits") and hasattr(hooks_lib, "hrt_trace_hits")


def test_csharp_binding_declares_trace_hits():
    src = open(os.path.join(ROOT, "bindings", "csharp", "HipRaytrace.cs")).read()
    m = re.search(r"\[DllImport\(Lib\)\] public static extern int hrt_trace_hits\(([^)]*)\);", src)
    assert m
    args = [a.strip().rsplit(" ", 1)[0] for a in m.group(1).split(",")]
    assert args == ["IntPtr", "HrtRay*", "long", "int", "HrtRayHit*", "int*", "int*", "int", "float*"]
    assert re.search(r"public const int HRT_HITS_MAX = 16;", src)
    fr = open(os.path.join(ROOT, "bindings", "csharp", "HipFrameRenderer.cs")).read()
    assert "public int TraceHits(" in fr and "public HrtRayHit[] PickAll(" in fr and "hrt_trace_hits" in fr


Z = np.zeros((4, 3), np.float32)


@pytest.mark.parametrize("origins,dirs,k,kw,exc", [
    (Z, Z, 0, {}, ValueError),
    (Z, Z, 17, {}, ValueError),
    (Z, Z, -1, {}, ValueError),
    (Z, Z, 2.0, {}, TypeError),
    (Z, Z, True, {}, TypeError),
    (Z, Z, None, {}, TypeError),
    (Z, np.zeros((5, 3), np.float32), 2, {}, ValueError),
    (Z, np.zeros((4, 2), np.float32), 2, {}, ValueError),
    (np.zeros(12, np.float32), np.zeros(12, np.float32), 2, {}, ValueError),
    (np.zeros((4, 3), np.float64), Z, 2, {}, ValueError),
    (Z, Z, 2, {"tmax": np.zeros(3, np.float32)}, ValueError),
    (Z, Z, 2, {"tmax": np.zeros(4, np.float64)}, ValueError),
    (Z, Z, 2, {"slot": 0}, ValueError),
    ([[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]], 2, {}, TypeError),
])
def test_python_checks_arguments_first(origins, dirs, k, kw, exc):
    with pytest.raises(exc):
        _renderer().trace_hits(origins, dirs, k, **kw)


def test_torch_inputs_checked_first():
    import torch
    r = _renderer()
    o = torch.zeros((4, 3), dtype=torch.float32)
    with pytest.raises(ValueError):                                  # host tensors: numpy arrays take the host path
        r.trace_hits(o, o, 2)
    with pytest.raises(ValueError):
        r.trace_hits(o.double(), o.double(), 2)
    with pytest.raises(TypeError):                                   # mixed numpy / torch
        r.trace_hits(o, np.zeros((4, 3), np.float32), 2)
    with pytest.raises(TypeError):
        r.trace_hits(np.zeros((4, 3), np.float32), o, 2)
    with pytest.raises(ValueError):
        r.trace_hits(o, o, 0)
