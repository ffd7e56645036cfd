"""Radiance queries (hrt_trace_paths) without a GPU: the entry point is declared and exported by both libraries, hrt_path_result
agrees between C, ctypes and the C# binding, the Python wrapper refuses bad arguments before it calls the library, and
RTRenderer.camera_rays is the frame's primary ray bit for bit."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, engine, scenes
from oracle import orc_indep as OI
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _decl(src, name):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
    assert m, name
    return m.group(1)


def test_header_declares_trace_paths():
    src = open(os.path.join(INC, "hip_raytrace.h")).read()
    args = [" ".join(a.split()) for a in _decl(src, "hrt_trace_paths").split(",")]
    assert args == ["hrt_ctx* ctx", "const hrt_frame_params* params", "uint32_t flags", "const hrt_ray* rays", "int64_t n",
                    "int64_t first_key", "hrt_path_result* results", "int32_t dev", "float* device_ms"]


def test_both_libraries_export_trace_paths(hrt_lib, hooks_lib):
    for path in (engine.LIB_PATH, engine.HOOKS_LIB_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
        assert "hrt_trace_paths" in {l.split()[-1] for l in out.splitlines() if l.strip()}, path
    assert hasattr(hrt_lib, "hrt_trace_paths") and hasattr(hooks_lib, "hrt_trace_paths")


def test_path_result_matches_c():
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "hip_raytrace.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu\n", sizeof(hrt_path_result), offsetof(hrt_path_result, radiance), offsetof(hrt_path_result, color),
        offsetof(hrt_path_result, depth), offsetof(hrt_path_result, objId), offsetof(hrt_path_result, reserved));
 return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "q.c")
        open(c, "w").write(prog)
        exe = os.path.join(d, "q")
        subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", INC, c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    want = [C.sizeof(T.PathResult)] + [getattr(T.PathResult, f).offset for f in ("radiance", "color", "depth", "objId", "reserved")]
    assert got == want == [32, 0, 12, 16, 20, 24]
    assert np.dtype(T.PathResult).itemsize == 32


def test_csharp_binding_declares_trace_paths():
    src = open(os.path.join(ROOT, "bindings", "csharp", "HipRaytrace.cs")).read()
    m = re.search(r"\[DllImport\(Lib\)\] public static extern int hrt_trace_paths\(([^)]*)\);", src)
    assert m
    args = [a.strip().rsplit(" ", 1)[0] for a in m.group(1).split(",")]
    assert args == ["IntPtr", "HrtFrameParams*", "uint", "HrtRay*", "long", "long", "HrtPathResult*", "int", "float*"]
    i = src.index("public struct HrtPathResult")
    assert "[StructLayout(LayoutKind.Sequential)]" in src[i - 60:i]
    body = re.search(r"public struct HrtPathResult\b[^{]*\{(.*?)\n    \}", src, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    fields = re.findall(r"public\s+(\w+)\s+([\w\s,]+);", body)
    size = {"Float3": 12, "int": 4, "float": 4}
    assert sum(size[t] * len(n.split(",")) for t, n in fields) == 32
    assert [n.strip() for _, grp in fields for n in grp.split(",")] == ["radiance", "color", "depth", "objId", "reserved0", "reserved1"]
    assert "public void TracePaths(" in open(os.path.join(ROOT, "bindings", "csharp", "HipFrameRenderer.cs")).read()


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


def _params(w=16, h=8, **kw):
    return scenes.frame_params(scenes.CONFIGS[2], *H.host_funcs("hrt"), width=w, height=h, spp=1, **kw)


def _reuse(which):
    p = _params()
    setattr(p, which, 1)
    return p


Z = np.zeros((4, 3), np.float32)


@pytest.mark.parametrize("case", ["temporal", "spatial", "flags", "flags_nosync", "key_overflow", "key_negative", "shape", "not_n3",
                                  "float64", "slot", "width", "depth", "params"])
def test_python_checks_arguments_first(case):
    r, p = _renderer(), _params()
    o, d, kw, exc = Z, Z, {}, ValueError
    if case == "temporal":
        p = _reuse("enableTemporalReuse")
    elif case == "spatial":
        p = _reuse("enableSpatialReuse")
    elif case == "flags":
        kw = {"flags": T.FLAG_COUNTERS}
    elif case == "flags_nosync":
        kw = {"flags": T.FLAG_NO_SYNC | T.FLAG_MEGAKERNEL}
    elif case == "key_overflow":
        kw = {"first_key": 0x7FFFFFFF - 3}
    elif case == "key_negative":
        kw = {"first_key": -1}
    elif case == "shape":
        d = np.zeros((5, 3), np.float32)
    elif case == "not_n3":
        d = np.zeros((4, 2), np.float32)
    elif case == "float64":
        o = np.zeros((4, 3), np.float64)
    elif case == "slot":
        kw = {"slot": 0}
    elif case == "width":
        p.width = 0
    elif case == "depth":
        p.maxDepth = -1
    elif case == "params":
        p, exc = None, TypeError
    with pytest.raises(exc):
        r.trace_paths(o, d, p, **kw)


def test_key_limit_is_inclusive_of_the_last_int():
    # first_key + n == 2^31 - 1 is legal: the refusal above is for one key more (reaches the library, which _NoLib refuses)
    with pytest.raises(AssertionError, match="library was called"):
        _renderer().trace_paths(Z, Z, _params(), first_key=0x7FFFFFFF - 4)


def test_mixed_numpy_and_torch_refused():
    import torch
    r = _renderer()
    with pytest.raises(TypeError):
        r.trace_paths(torch.zeros((4, 3), dtype=torch.float32), Z, _params())
    with pytest.raises(TypeError):
        r.trace_paths(Z, torch.zeros((4, 3), dtype=torch.float32), _params())
    with pytest.raises(ValueError):                                   # host tensors: numpy arrays take the host path
        r.trace_paths(torch.zeros((4, 3)), torch.zeros((4, 3)), _params())


@pytest.mark.parametrize("cfg,w,h", [(2, 64, 36), (4, 40, 30)])
def test_camera_rays_are_the_frames_primary_rays(cfg, w, h):
    p = scenes.frame_params(scenes.CONFIGS[cfg], *H.host_funcs("hrt"), width=w, height=h, spp=1)
    o, d = engine.RTRenderer.camera_rays(p)
    assert o.shape == d.shape == (w * h, 3) and o.dtype == d.dtype == np.float32
    K = OI.Frame(p)
    idx = np.unique(np.concatenate([np.arange(0, w * h, 5), [0, w - 1, w * h - 1, w * (h - 1)]]))
    assert len(idx) >= 200
    for i in idx:
        ro, rd, _ = K.primary_ray(int(i))
        assert H.bits_equal(np.array(ro, np.float32), o[i]).all() and H.bits_equal(np.array(rd, np.float32), d[i]).all(), int(i)
