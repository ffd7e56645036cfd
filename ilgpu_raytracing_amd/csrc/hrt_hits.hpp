// hrt_hits.hpp -- launch interface of the multi-hit ray queries (hrt_trace_hits; kernels in hrt_hits.hip).
//
// The kernels live in a translation unit of their own, as the radiance queries' do (hrt_paths.hpp): new call sites of the walker's
// device functions in hrt_runtime.hip would move the compiler's inlining decisions, and the code, of the frame's kernels.  The
// runtime hands one chunk of rays to hits_launch with everything the kernels read.
#pragma once
#include "hrt_trace_packed.hpp"

// one chunk of a multi-hit query on one device.  Hit slot s = i * k + j (ray i, rank j) is three float4, the hrt_ray_hit of the
// result.  The walk keeps ray i's sorted candidates in its own k slots (raw: t, tObj, bits(a), bits(b) | bits(instance),
// bits(prim), 0, 0) and the finish overwrites each slot in place with its record or CLOSEST's miss record: no other workspace.
struct HitsK {
    const float4* rays;       // 2 per ray (hrt_ray)
    float4* hits;             // 3 per hit slot, n * k slots
    int32_t* counts;          // n: records stored for ray i
    int32_t* totals;          // n: accepted tests of ray i (saturating); may be null
    int* grab;                // 8 hand-out counters kQueryGrabStride ints apart (packed walk), zeroed by hits_launch
    int n, nSegs, k;
};

struct HitsLaunch {
    int variant;              // -1 TracerRef (scene beyond the packed layout), 0 / 1 / 3 TracerPackedT<variant>
    bool lt3;                 // packed: triangle records per leaf step (DPacked::leafTris == 3)
    unsigned gridW;           // packed: workgroups of the persistent walk
    hrt::DScene S;
    hrt::DPacked P;
    HitsK h;
};

// enqueues walk, finish and fix-up (packed) or the one-ray-per-lane TracerRef kernel on st
hipError_t hits_launch(const HitsLaunch& L, hipStream_t st);
