"""Progressive frames (hrt_render_progressive) without a GPU: the C declaration and both libraries' exports, the C# binding, and
the Python wrapper's argument checks, which must refuse a call before the library sees it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = os.path.join(ROOT, "bindings", "csharp")


def _no_comments(src):
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_entry_point():
    src = _no_comments(open(os.path.join(ROOT, "include", "hip_raytrace.h")).read())
    decl = re.search(r"\bint\s+hrt_render_progressive\s*\(([^)]*)\)\s*;", src)
    assert decl, "include/hip_raytrace.h does not declare hrt_render_progressive"
    params = [re.sub(r"\s+", " ", p).strip() for p in decl.group(1).split(",")]
    assert params == ["hrt_ctx* ctx", "const hrt_frame_params* params", "const hrt_render_opts* opts",
                      "int32_t sample_begin", "const hrt_outputs* outputs", "hrt_stats* stats"]


@pytest.mark.parametrize("lib", ["libhip_raytrace.so", "libhip_raytrace_test.so"])
def test_both_libraries_export_it(hrt_lib, lib):
    path = os.path.join(os.path.dirname(engine.LIB_PATH), lib)
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    assert "hrt_render_progressive" in exported and "hrt_render_frame" in exported


def test_python_binding_types(hrt_lib):
    f = hrt_lib.hrt_render_progressive
    assert f.argtypes[3] is C.c_int32 and len(f.argtypes) == 6


def test_csharp_binding():
    src = open(os.path.join(CS, "HipRaytrace.cs")).read()
    m = re.search(r"\[DllImport\(Lib\)\]\s*public static extern int hrt_render_progressive\(([^)]*)\);", src)
    assert m, "HipRaytrace.cs has no [DllImport] of hrt_render_progressive"
    types = [p.strip().rsplit(" ", 1)[0] for p in m.group(1).split(",")]
    # hrt_ctx* -> IntPtr, int32_t -> int, the structs by pointer (as hrt_render_frame's binding has them)
    assert types == ["IntPtr", "HrtFrameParams*", "HrtRenderOpts*", "int", "HrtOutputs*", "HrtStats*"]
    r = open(os.path.join(CS, "HipFrameRenderer.cs")).read()
    assert re.search(r"public ReadOnlySpan<int> RenderProgressive\(in HrtFrameParams frame, int sampleBegin, int outW, int outH, bool taau\)", r)
    assert "hrt_render_progressive(_ctx" in r


class _NoLib:
    """Stands in for the library: any call fails the test (argument checks must raise first)."""

    def __getattr__(self, name):
        raise AssertionError("the library was called (%s) although the arguments are invalid" % name)


def _renderer():
    r = engine.RTRenderer.__new__(engine.RTRenderer)       # no hrt_create: the wrapper's checks only
    r._L = _NoLib()
    r._ctx = None
    r.device_ids = [0]
    return r


def _params(spp):
    p = T.FrameParams()
    p.width, p.height, p.spp, p.maxDepth = 64, 32, spp, 3
    return p


@pytest.mark.parametrize("spp,begin,flags,outputs,exc", [
    (4, -1, 0, None, ValueError),                          # negative sample_begin
    (4, 4, 0, None, ValueError),                           # spp == sample_begin
    (4, 5, 0, None, ValueError),                           # spp < sample_begin
    (0, 0, 0, None, ValueError),                           # spp < 1
    (-3, 0, 0, None, ValueError),
    (4, 0, T.FLAG_COUNTERS, None, ValueError),             # forbidden flags
    (4, 0, T.FLAG_PRIMARY_ONLY, None, ValueError),
    (4, 1, T.FLAG_SKIP_PRIMARY, None, ValueError),
    (4, 1, T.FLAG_EXCHANGED, None, ValueError),
    (4, 0, T.FLAG_MEGAKERNEL | T.FLAG_COUNTERS, None, ValueError),
    (4, 0, T.FLAG_NO_SYNC, T.Outputs(), ValueError),       # NO_SYNC cannot gather
    (4, 1.0, 0, None, TypeError),
    (4, True, 0, None, TypeError),
])
def test_render_progressive_refuses_before_the_library(spp, begin, flags, outputs, exc):
    with pytest.raises(exc):
        _renderer().render_progressive(_params(spp), begin, outputs, flags)


@pytest.mark.parametrize("schedule,flags", [
    ((8, 8, 16), 0),                                       # not strictly increasing
    ((8, 4), 0),
    ((0, 4), 0),                                           # < 1 sample
    ((), 0),
    ((1, 2), T.FLAG_COUNTERS),
    ((1, 2), T.FLAG_SKIP_PRIMARY),
])
def test_refine_refuses_before_the_library(schedule, flags):
    with pytest.raises(ValueError):
        _renderer().refine(_params(4), schedule, flags=flags)


def test_refine_walks_the_schedule():
    """refine calls render_progressive once per step with the running spp and the previous step's spp as sample_begin, on a copy
    of params, and yields after each call."""
    calls = []

    class _Rec(engine.RTRenderer):
        def __init__(self):
            pass

        def render_progressive(self, params, sample_begin, outputs=None, flags=0, rows=None, strips=None):
            calls.append((params.spp, sample_begin, flags, params.width))
            return "stats%d" % params.spp

    p = _params(99)
    got = list(_Rec().refine(p, np.array([1, 2, 5, 16]), flags=T.FLAG_STREAMED))
    assert got == [(1, "stats1"), (2, "stats2"), (5, "stats5"), (16, "stats16")]
    assert calls == [(1, 0, T.FLAG_STREAMED, 64), (2, 1, T.FLAG_STREAMED, 64), (5, 2, T.FLAG_STREAMED, 64), (16, 5, T.FLAG_STREAMED, 64)]
    assert p.spp == 99
