"""Ray queries (hrt_trace_rays) without a GPU: the entry point is declared and exported by both libraries, the wire structs agree
between C, ctypes and the C# binding, and the Python wrapper refuses bad arguments before it calls the library."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _decl(src, name):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
    assert m, name
    return m.group(1)


def test_header_declares_trace_rays():
    src = open(os.path.join(INC, "hip_raytrace.h")).read()
    args = [a.strip() for a in _decl(src, "hrt_trace_rays").split(",")]
    assert args == ["hrt_ctx* ctx", "int32_t query", "const hrt_ray* rays", "int64_t n", "void* results", "int32_t dev", "float* device_ms"]
    assert re.search(r"HRT_QUERY_CLOSEST\s*=\s*0", src) and re.search(r"HRT_QUERY_OCCLUDED\s*=\s*1", src)
    assert re.search(r"#define HRT_QUERY_CHUNK \(1 << 21\)", src) and T.QUERY_CHUNK == 1 << 21


def test_both_libraries_export_trace_rays(hrt_lib, hooks_lib):
    for path in (engine.LIB_PATH, engine.HOOKS_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert "hrt_trace_rays" in {l.split()[-1] for l in out.splitlines() if l.strip()}, path
    assert hasattr(hrt_lib, "hrt_trace_rays") and hasattr(hooks_lib, "hrt_trace_rays")


def test_ray_structs_match_c():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "hip_raytrace.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu\n", sizeof(hrt_ray), offsetof(hrt_ray, origin), offsetof(hrt_ray, tMax), offsetof(hrt_ray, dir),
        offsetof(hrt_ray, pad), sizeof(hrt_ray_hit));
 printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(hrt_ray_hit, t), offsetof(hrt_ray_hit, normal), offsetof(hrt_ray_hit, albedo),
        offsetof(hrt_ray_hit, ior), offsetof(hrt_ray_hit, objId), offsetof(hrt_ray_hit, shade), offsetof(hrt_ray_hit, instance),
        offsetof(hrt_ray_hit, prim));
 return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "q.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "q")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    want = [C.sizeof(T.Ray), T.Ray.origin.offset, T.Ray.tMax.offset, T.Ray.dir.offset, T.Ray.pad.offset, C.sizeof(T.RayHit)]
    want += [getattr(T.RayHit, f).offset for f in ("t", "normal", "albedo", "ior", "objId", "shade", "instance", "prim")]
    assert got == want
    assert got[0] == 32 and got[5] == 48
    assert np.dtype(T.RayHit).itemsize == 48 and np.dtype(T.Ray).itemsize == 32


def test_csharp_binding_declares_trace_rays():
    src = open(os.path.join(ROOT, "bindings", "csharp", "HipRaytrace.cs")).read()
    m = re.search(r"\[DllImport\(Lib\)\] public static extern int hrt_trace_rays\(([^)]*)\);", src)
    assert m
    args = [a.strip().rsplit(" ", 1)[0] for a in m.group(1).split(",")]
    assert args == ["IntPtr", "int", "HrtRay*", "long", "void*", "int", "float*"]
    for struct, fields in (("HrtRay", ["origin", "tMax", "dir", "pad"]),
                           ("HrtRayHit", ["t", "normal", "albedo", "ior", "objId", "shade", "instance", "prim"])):
        body = re.search(r"public struct %s\b[^{]*\{(.*?)\n    \}" % struct, src, flags=re.S).group(1)
        body = re.sub(r"//[^\n]*", "", body)
        names = re.findall(r"public\s+\w+\s+([\w\s,]+);", body)
        assert [n.strip() for grp in names for n in grp.split(",")] == fields, struct
    fr = open(os.path.join(ROOT, "bindings", "csharp", "HipFrameRenderer.cs")).read()
    assert "public HrtRayHit Pick(" in fr and "hrt_trace_rays" in fr


class _NoLib:
    """Stands in for the library: any call fails the test (argument checks must raise first)."""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) although the arguments are invalid" % name)


def _renderer():
    r = engine.RTRenderer.__new__(engine.RTRenderer)       # no hrt_create: the wrapper's checks only
    r._L = _NoLib()
    r._ctx = None
    r.device_ids = [0]
    r.last_made_params = None
    return r


@pytest.mark.parametrize("origins,dirs,kw,exc", [
    (np.zeros((4, 3), np.float32), np.zeros((5, 3), np.float32), {}, ValueError),                         # shapes differ
    (np.zeros((4, 3), np.float32), np.zeros((4, 2), np.float32), {}, ValueError),                         # not (n, 3)
    (np.zeros(12, np.float32), np.zeros(12, np.float32), {}, ValueError),
    (np.zeros((4, 3), np.float64), np.zeros((4, 3), np.float32), {}, ValueError),                         # not float32
    (np.zeros((4, 3), np.float32), np.zeros((4, 3), np.int32), {}, ValueError),
    (np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), {"query": "any"}, ValueError),           # unknown query
    (np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), {"query": 0}, ValueError),
    (np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), {"query": "occluded", "tmax": np.zeros(3, np.float32)}, ValueError),
    (np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), {"query": "occluded", "tmax": np.zeros(4, np.float64)}, ValueError),
    (np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32), {"slot": 0}, ValueError),                # host arrays take every slot
    ([[0.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]], {}, TypeError),                                                # not arrays
])
def test_python_checks_arguments_first(origins, dirs, kw, exc):
    with pytest.raises(exc):
        _renderer().trace_rays(origins, dirs, **kw)


def test_pick_needs_a_camera():
    with pytest.raises(RuntimeError):
        _renderer().pick(64, 48, 1, 1)


def test_torch_inputs_checked_first():
    import torch
    r = _renderer()
    o = torch.zeros((4, 3), dtype=torch.float32)
    with pytest.raises(ValueError):                                  # host tensors: numpy arrays take the host path
        r.trace_rays(o, o)
    with pytest.raises(ValueError):
        r.trace_rays(o.double(), o.double())
    with pytest.raises(TypeError):
        r.trace_rays(o, np.zeros((4, 3), np.float32))
