// hrt_query.hpp -- ray queries on the uploaded scene (hrt_trace_rays): TraceClosest and ShadowOcclusion
// (SceneDeviceViews.cs:30-121) over rays the caller supplies, result i for ray i.
//
// Packed scenes: the persistent-wave walker of the path tracer (walk_queue, hrt_walker.hpp) on the uploaded tree (ALT = false:
// exact by construction).  Its queue is the caller's ray array cut into segments, handed out through 8 per-XCD counters
// (as RangeGrab, hrt_wavefront.hpp), so the waves of one XCD walk neighbouring rays and keep their lanes full however uneven the
// rays' costs are.  A closest-hit walk stores the raw winner (t, tObj, leaf slot, primitive); the finish kernel shades it at
// full lane occupancy (TracerPackedT::finish_hit), as the streamed pipeline does.  An occlusion walk stores its bit directly.
// Scenes beyond the packed layout: one ray per lane on TracerRef, which walks the reference's own arrays.
// Rays with a non-finite origin or direction take TracerRef on packed scenes too: the walkers skip the ray transform of identity
// instances, exact for finite rays (TransformRay with the identity changes at most the sign of a zero), but the reference's
// 0 * inf and 0 * NaN turn every component of such a ray NaN, and the walk over the plain ray can then find occluders the reference
// cannot.  The packed walk leaves them out and a fix-up pass over the whole batch answers them (none in rays a renderer makes).
//
// A ray is two float4 (hrt_ray: origin.xyz, tMax | dir.xyz, pad); a hit is three (hrt_ray_hit: t, normal | albedo, ior |
// objId, shade, instance, prim).  The host side guarantees 16-byte alignment of both arrays.
#pragma once
#include "hrt_wavefront.hpp"
#include "../../include/hrt_types.h"

namespace hrt {

#ifndef HRT_QUERY_SEG
#define HRT_QUERY_SEG 256
#endif
#ifndef HRT_QUERY_GRAB_STRIDE
#define HRT_QUERY_GRAB_STRIDE 64
#endif
// rays per segment of the hand-out, and ints between two of its 8 counters.  Every segment costs one atomic on its XCD's counter, and
// device-scope atomics to one address serialise: 64-ray segments on 8 counters in one cache line put a floor of ~0.76 ms under every
// 1920x1080 batch, whatever the scene (tools/query_bench.py)
constexpr int kQuerySeg = HRT_QUERY_SEG;
constexpr int kQueryGrabStride = HRT_QUERY_GRAB_STRIDE;
static_assert(kQuerySeg % 64 == 0, "a segment is a whole number of wave refills");

struct QueryK {
    const float4* rays;       // 2 per ray
    float4* raw;              // closest-hit walk: raw winner per ray (t, tObj, bits(slot), bits(prim))
    float4* hits;             // 3 per ray (hrt_ray_hit)
    int32_t* occ;             // occlusion bit per ray
    int* grab;                // 8 hand-out counters kQueryGrabStride ints apart, zeroed before the walk
    int n, nSegs;
};

HRT_D Ray query_ray(const QueryK& q, int i, float& tMax)
{
    const float4 a = q.rays[2 * i], b = q.rays[2 * i + 1];
    Ray r; r.o = mk3(a.x, a.y, a.z); r.d = mk3(b.x, b.y, b.z); r.inv = inv_dir(r.d);     // InvDir, RTRay.cs:548-549
    tMax = a.w;
    return r;
}

HRT_D bool query_finite(const Ray& r)
{
    return hrt_isfinite(r.o.x) && hrt_isfinite(r.o.y) && hrt_isfinite(r.o.z) && hrt_isfinite(r.d.x) && hrt_isfinite(r.d.y) && hrt_isfinite(r.d.z);
}

HRT_D void query_store_hit(const QueryK& q, int i, const Hit& h, int instance, int prim)
{
    q.hits[3 * i + 0] = make_float4(h.t, h.n.x, h.n.y, h.n.z);
    q.hits[3 * i + 1] = make_float4(h.albedo.x, h.albedo.y, h.albedo.z, h.ior);
    q.hits[3 * i + 2] = make_float4(__int_as_float(h.objId), __int_as_float(h.shade), __int_as_float(instance), __int_as_float(prim));
}

// the queue of a walk: segment r = rays [kQuerySeg r, min(kQuerySeg (r + 1), n)).  As RangeGrab (hrt_wavefront.hpp): the segments are
// cut into 8 contiguous partitions, one per XCD (workgroup i runs on XCD i & 7), a wave whose partition is exhausted steals from the
// next ones; here each partition's counter has a cache line of its own
struct QuerySegs {
    int* ctr;
    int nSegs, n;
    int part, tried;     // wave-uniform
    HRT_D void init(const QueryK& q) { ctr = q.grab; nSegs = q.nSegs; n = q.n; part = blockIdx.x & 7; tried = 0; }
    HRT_D bool next(int& base, int& cnt)
    {
        int r = -1, t = tried;
        if ((threadIdx.x & 63) == 0)
        {
            while (t < 8)
            {
                const int p = (part + t) & 7;
                const int lo = (int)((long long)nSegs * p / 8), hi = (int)((long long)nSegs * (p + 1) / 8);
                const int i = (hi > lo) ? atomicAdd(&ctr[p * kQueryGrabStride], 1) : 0;
                if (i < hi - lo) { r = lo + i; break; }
                t++;
            }
        }
        tried = __builtin_amdgcn_readfirstlane(t);
        r = __builtin_amdgcn_readfirstlane(r);
        if (r < 0) return false;
        base = r * kQuerySeg;
        cnt = n - base < kQuerySeg ? n - base : kQuerySeg;
        return true;
    }
};

} // namespace hrt

#ifndef HRT_QUERY_WAVES
#define HRT_QUERY_WAVES 4
#endif

// closest hit: raw winners of the walk over the uploaded tree
template <int FEAT, int LT>
__global__ void __launch_bounds__(256, HRT_QUERY_WAVES)
hrt_query_closest_kernel(hrt::TracerPackedT<FEAT> tr, hrt::QueryK q)
{
    using namespace hrt;
    Cnt<false> C;
    QuerySegs segs; segs.init(q);
    walk_queue<FEAT, false, false, false, false, LT>(tr, tr,
        [&](int& base, int& cnt) { return segs.next(base, cnt); },
        [&](int i, Ray& r, float& tMax) { r = query_ray(q, i, tMax); return query_finite(r); },      // false: left to the fix-up pass
        [&](int i, const WalkResult& res) { q.raw[i] = make_float4(res.t, res.tObj, __int_as_float(res.slot), __int_as_float(res.prim)); },
        C);
}

// ShadowOcclusion(ray, ray.tMax)
template <int FEAT, int LT>
__global__ void __launch_bounds__(256, HRT_QUERY_WAVES)
hrt_query_occluded_kernel(hrt::TracerPackedT<FEAT> tr, hrt::QueryK q)
{
    using namespace hrt;
    Cnt<false> C;
    QuerySegs segs; segs.init(q);
    walk_queue<FEAT, true, false, false, false, LT>(tr, tr,
        [&](int& base, int& cnt) { return segs.next(base, cnt); },
        [&](int i, Ray& r, float& tMax) { r = query_ray(q, i, tMax); return query_finite(r); },      // false: left to the fix-up pass
        [&](int i, const WalkResult& res) { q.occ[i] = res.occluded ? 1 : 0; },
        C);
}

// TraceClosest's outputs of the raw winners (finish_hit) + the instance record (tlasInstanceIndices[leaf slot]) and the primitive:
// the sphere index of a sphere hit, the triangle index of a triangle hit (== objId)
template <int FEAT>
__global__ void __launch_bounds__(256)
hrt_query_finish_kernel(hrt::TracerPackedT<FEAT> tr, hrt::QueryK q)
{
    using namespace hrt;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= q.n) return;
    float tMax;
    const Ray r = query_ray(q, i, tMax);
    const float4 w = q.raw[i];
    const int slot = __float_as_int(w.z), prim = __float_as_int(w.w);
    Hit h;
    const bool hit = tr.finish_hit(r, w.x, w.y, slot, prim, h);
    query_store_hit(q, i, h, hit ? tr.S.tlasInst[slot] : -1, hit ? (h.objId >= 0 ? h.objId : prim) : -1);
}

// scenes beyond the packed layout: one ray per lane on the reference's own arrays.  NONFINITE: the fix-up pass after a packed walk,
// which answers only the rays with a non-finite origin or direction (overwriting what the walk and the finish stored for them)
template <bool ANY, bool NONFINITE>
__global__ void __launch_bounds__(256)
hrt_query_ref_kernel(hrt::TracerRef tr, hrt::QueryK q)
{
    using namespace hrt;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= q.n) return;
    Cnt<false> C;
    float tMax;
    const Ray r = query_ray(q, i, tMax);
    if (NONFINITE && query_finite(r)) return;
    if (ANY) { q.occ[i] = tr.occluded<false>(r, tMax, C) ? 1 : 0; return; }
    Hit h;
    int win[2] = {-1, -1};
    tr.closest<false>(r, h, C, win);
    query_store_hit(q, i, h, win[0], win[1]);
}
