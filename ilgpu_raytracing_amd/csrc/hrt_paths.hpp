// hrt_paths.hpp -- launch interface of the radiance queries (hrt_trace_paths; kernels in hrt_paths.hip).
//
// The kernels live in a translation unit of their own: they instantiate the device functions the frame's kernels use, and in
// the same unit new call sites of those functions would move the compiler's inlining decisions -- and the code -- of the
// frame's kernels.  The runtime hands one chunk of keys to paths_launch with everything the kernels read.
#pragma once
#include "hrt_pixels.hpp"

// one chunk of a radiance query on one device: the frame's tracer for the scene (render_impl's choice for a fused path stage) and
// the chunk's layout (PathsK, TileMap), G-buffer and sample-group scratch
struct PathsLaunch {
    int variant;              // -1 TracerRef, 0 / 1 / 3 TracerPackedT<variant>
    bool flat;                // TracerFlat (variant 0, tiny fast-sphere scene)
    bool second;              // primary over the second tree (TracerSecond; variant 0, not flat)
    DScene S;
    DPacked P, PAny;          // uploaded packed tree, second tree
    const NodeQ* leaves;      // TracerFlat: TLAS leaves in walk order
    int nLeaves;
    FrameK k;                 // the frame's constants; rows [row_begin, row_end) of this chunk, one strip set
    TileMap tm;
    PathsK q;
    DGBuffer gb;              // the chunk's private G-buffer planes (slot = key - q.base)
    float* split;             // sample groups: per-sample radiance [spp][nLocal] then the staged reservoirs [nGroups][12][nLocal]
    int nGroups, perGroup;    // nGroups == 1: one fused kernel
};

// enqueues primary + path stage (+ resolve) on st
hipError_t paths_launch(const PathsLaunch& L, hipStream_t st);
