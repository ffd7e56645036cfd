// hrt_hits.hip -- multi-hit ray queries (hrt_trace_hits): the k nearest accepted primitive tests along each caller ray.
//
// Definition (include/hip_raytrace.h): an unpruned walk of the uploaded tree with ShadowOcclusion's limits (SceneDeviceViews.cs:89-121:
// TLAS boxes against ray.tMax, BLAS boxes and primitive t against tMaxObj = tMax * scale) and TraceClosest's per-hit rules (:30-86,
// :124-237: the linear alpha rule of :206-221, the record CLOSEST would return for that hit).  Every accepted test is one record; the
// records are ordered by (t as unsigned bits, instance, prim) and the first k are kept.
//
// No box test is cut at the k-th distance.  That a primitive's computed t is never below its boxes' computed slab entry is not true
// in float arithmetic (grazing spheres, skimming triangles: hrt_trace_packed.hpp "Closest-hit walks over the SECOND tree"), and the
// `/ scale` of an instance rounds differently from its object-space bound, so no cut is provably exact: the walk with totals and the
// walk without are the same walk.
//
// Packed scenes: a persistent-wave walk (walk_hits below, the structure of walk_queue in hrt_walker.hpp with the any-hit limits and
// no early exit) pulls rays through the per-XCD segment hand-out of hrt_query.hpp (QuerySegs).  An accepted test looks up its
// instance (tlasInst[leaf slot]) and is inserted into the ray's sorted list, which lives in the ray's own k hit slots of the output;
// the lane keeps the list's length, the accepted count and the key of its last record.  A finish kernel shades every hit slot at full
// lane occupancy through TracerPackedT::finish_hit (called with t = 0 so that its `>= 1e29 is a miss` guard never fires: a hit at
// t >= 1e29 is a hit here) and writes the miss padding.  Rays with a non-finite origin or direction are left to a TracerRef fix-up
// pass, as in hrt_query.hpp.  Scenes beyond the packed layout: one ray per lane on the reference's arrays.
#include <hip/hip_runtime.h>
#include <climits>
#include "hrt_hits.hpp"
#include "hrt_query.hpp"

using namespace hrt;

namespace {

// (t, instance, prim) < (t', instance', prim'): t by its unsigned bit pattern (IEEE totalOrder for t >= +0 and NaN)
__device__ __forceinline__ bool key_less(unsigned t, int inst, int prim, unsigned t2, int inst2, int prim2)
{
    return t < t2 || (t == t2 && (inst < inst2 || (inst == inst2 && prim < prim2)));
}

// one ray's sorted list of at most k raw records in its own hit slots
struct HitList {
    float4* base;             // hits + 3 k i
    int cnt, tot;
    unsigned lastT; int lastI, lastP;       // key of record k - 1 once the list is full

    __device__ __forceinline__ void start(const HitsK& h, int i)
    {
        base = h.hits + (size_t)i * (size_t)h.k * 3;
        cnt = 0; tot = 0; lastT = 0u; lastI = 0; lastP = 0;
    }
    // an accepted test: world t, object t, what the finish needs (a, b), the ordering key's instance and prim
    __device__ __forceinline__ void add(int k, float t, float tObj, int a, int b, int inst, int prim)
    {
        tot += tot < INT_MAX ? 1 : 0;
        const unsigned tb = __float_as_uint(t);
        if (cnt == k && !key_less(tb, inst, prim, lastT, lastI, lastP)) return;
        int j = cnt < k ? cnt : k - 1;
        for (; j > 0; j--)
        {
            const float4 r0 = base[3 * (j - 1)], r1 = base[3 * (j - 1) + 1];
            if (!key_less(tb, inst, prim, __float_as_uint(r0.x), __float_as_int(r1.x), __float_as_int(r1.y))) break;
            base[3 * j] = r0; base[3 * j + 1] = r1;
        }
        base[3 * j] = make_float4(t, tObj, __int_as_float(a), __int_as_float(b));
        base[3 * j + 1] = make_float4(__int_as_float(inst), __int_as_float(prim), 0.f, 0.f);
        if (cnt < k) cnt++;
        if (cnt == k)
        {
            const float4 r0 = base[3 * (k - 1)], r1 = base[3 * (k - 1) + 1];
            lastT = __float_as_uint(r0.x); lastI = __float_as_int(r1.x); lastP = __float_as_int(r1.y);
        }
    }
};

__device__ __forceinline__ void hits_done(const HitsK& h, int i, const HitList& L)
{
    h.counts[i] = L.cnt;
    if (h.totals) h.totals[i] = L.tot;
}

__device__ __forceinline__ void store_miss(float4* s)
{
    s[0] = make_float4(1e30f, 0.f, 0.f, 0.f);
    s[1] = make_float4(1.f, 1.f, 1.f, 1.f);
    s[2] = make_float4(__int_as_float(-1), __int_as_float(0), __int_as_float(-1), __int_as_float(-1));
}

__device__ __forceinline__ void store_hit(float4* s, const Hit& h, int instance, int prim)
{
    s[0] = make_float4(h.t, h.n.x, h.n.y, h.n.z);
    s[1] = make_float4(h.albedo.x, h.albedo.y, h.albedo.z, h.ior);
    s[2] = make_float4(__int_as_float(h.objId), __int_as_float(h.shade), __int_as_float(instance), __int_as_float(prim));
}

__device__ __forceinline__ QueryK seg_k(const HitsK& h)
{
    QueryK q{};
    q.rays = h.rays; q.grab = h.grab; q.n = h.n; q.nSegs = h.nSegs;
    return q;
}

// The persistent-wave walk of walk_queue (hrt_walker.hpp: refill, node bursts with lookahead, one TLAS leaf entry and one BLAS leaf
// entry per iteration, LDS-parked world ray) with ShadowOcclusion's limits, no early exit, and every accepted test handed to the
// lane's HitList.  Node visits, box tests and primitive tests are those of the reference's ShadowOcclusion walk run to the end.
template <int FEAT, int LT>
__device__ __forceinline__ void walk_hits(const TracerPackedT<FEAT>& tr, const HitsK& h)
{
    constexpr bool kGeneral = (FEAT & 1) != 0;
    constexpr bool kAlpha = (FEAT & 2) != 0;
    const bool inl = !kGeneral && tr.P.tlasX != nullptr;
    __shared__ float park_mem[kGeneral ? 9 : 1][256];
    RayPark park; park.sh = park_mem;
    const DPacked& P = tr.P;
    const DScene& S = tr.S;
    Tex tex(S);
    const int lane = threadIdx.x & 63;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const QueryK q = seg_k(h);
    QuerySegs segs; segs.init(q);
    const int k = h.k;

    int segBase = 0, segN = 0, segCur = 0;
    bool more = true;
    int mode = M_IDLE, rayIdx = -1;
    Ray w;
    w.o = w.d = w.inv = mk3(0.f, 0.f, 0.f);
    float tMaxW = 0.f;
    HitList L; L.base = h.hits; L.cnt = 0; L.tot = 0; L.lastT = 0u; L.lastI = 0; L.lastP = 0;
    int cur = 0, li = 0, lend = 0, lskip = kEnd;
    const int xlast = P.nTlasX - 1;
    int bj = 0, bend = 0, bskip = kEnd;
    int blasEnd = 0, iflags = 0, islot = 0, iinst = 0; float iscale = 1.f;

    for (;;)
    {
        // ---------------- refill idle lanes from the chain
        {
            unsigned long long idle = __ballot(mode == M_IDLE);
            int nIdle = __popcll(idle);
            if (more && (nIdle >= kRefillMin || nIdle == 64))
            {
                while (nIdle > 0)
                {
                    if (segCur >= segN)
                    {
                        more = segs.next(segBase, segN);
                        segCur = 0;
                        if (!more) { segN = 0; break; }
                        continue;
                    }
                    const int avail = segN - segCur;
                    const int rank = __popcll(idle & lt);
                    if (mode == M_IDLE && rank < avail)
                    {
                        rayIdx = segBase + segCur + rank;
                        L.start(h, rayIdx);
                        w = query_ray(q, rayIdx, tMaxW);
                        // a non-finite ray is left to the fix-up pass (its count 0 is overwritten there)
                        if (query_finite(w)) { cur = 0; mode = M_TLAS; }
                        else mode = M_DONE;
                    }
                    segCur += nIdle < avail ? nIdle : avail;
                    idle = __ballot(mode == M_IDLE);
                    nIdle = __popcll(idle);
                }
            }
            if (!more && __popcll(__ballot(mode == M_IDLE)) == 64) break;
        }

        // ---------------- node steps: TLAS and BLAS nodes alike
        for (int burst = 0; burst < kNodeBurst; burst++)
        {
            const bool walking = (mode == M_TLAS) || (kGeneral && mode == M_BLAS);
            const int nWalk = __popcll(__ballot(walking));
            if (nWalk == 0 || (burst > 0 && nWalk < 24)) break;
            if (walking)
            {
                const bool top = !kGeneral || mode == M_TLAS;
                const NodeQ* nodes = top ? (inl ? P.tlasX : P.tlas) : P.blas;
                const int last = top ? (inl ? xlast : P.nTlas - 1) : blasEnd - 1;
                NodeQ nds[kLook];
#pragma unroll
                for (int kk = 0; kk < kLook; kk++) nds[kk] = nodes[cur + kk <= last ? cur + kk : last];
                __builtin_amdgcn_sched_barrier(0);
                const float lim = top ? tMaxW : tMaxW * iscale;
#pragma unroll
                for (int kk = 0; kk < kLook; kk++)
                {
                    const NodeQ nd = nds[kk];
                    int sk = wbits(nd.hi);
                    const int cnt = (int)((unsigned)sk >> 28);
                    sk &= kEnd;
                    const int here = cur;
                    bool stay = true;
                    const bool isInst = inl && cnt == 15;        // the one-node BLAS of a fast-sphere instance: limit tMax * 1
                    if (!hit_box(w, nd.lo, nd.hi, 0.001f, lim)) cur = sk;
                    else if (isInst) { stay = false; li = wbits(nd.lo); lskip = sk; mode = M_TLEAF; }
                    else if (cnt > 0)
                    {
                        if (inl) cur = here + 1;
                        else
                        {
                            stay = false;
                            if (top) { li = wbits(nd.lo); lend = li + cnt; lskip = sk; mode = M_TLEAF; }
                            else     { bj = wbits(nd.lo); bend = bj + cnt; bskip = sk; mode = M_BLEAF; }
                        }
                    }
                    else cur = wbits(nd.lo) & kEnd;
                    if (!(stay && cur == here + 1 && here < last)) break;
                }
            }
            if (kGeneral && mode == M_BLAS && !(cur < blasEnd)) { w = park.get(); mode = M_TLEAF; }
            if (!inl && mode == M_TLEAF && li == lend) { cur = lskip; mode = M_TLAS; }
            if (mode == M_TLAS && cur == kEnd) mode = M_DONE;
        }

        // ---------------- one TLAS leaf entry
        if (inl && mode == M_TLEAF)
        {   // the sphere of the instance record whose box was hit (scale 1)
            const float4 fb = P.finst[li].b, fc = P.finst[li].c;
            float t;
            if (hit_sphere_t(w, xyz(fc), fc.w, t) && t > 0.001f && t < tMaxW)
                L.add(k, t, t, li, wbits(fb), S.tlasInst[li], wbits(fb));
            cur = lskip; mode = (cur == kEnd) ? M_DONE : M_TLAS;
        }
        else if (mode == M_TLEAF)
        {
            FInst f = P.finst[li];
            const int flags = wbits(f.a);
            if (!kGeneral || (flags & FI_FAST_SPHERE))
            {
                if (hit_box(w, f.a, f.b, 0.001f, tMaxW))
                {
                    float t;
                    if (hit_sphere_t(w, xyz(f.c), f.c.w, t) && t > 0.001f && t < tMaxW)
                        L.add(k, t, t, li, wbits(f.b), S.tlasInst[li], wbits(f.b));
                }
                li++;
            }
            else
            {   // general instance: park the world ray, walk its BLAS with the object-space ray
                islot = li; iflags = flags; iscale = f.c.z; iinst = -1;
                cur = __float_as_int(f.c.x); blasEnd = __float_as_int(f.c.y);
                park.put(w);
                w = tr.object_ray(w, flags, wbits(f.b));
                li++;
                mode = M_BLAS;
                if (!(cur < blasEnd)) { w = park.get(); mode = M_TLEAF; }
            }
            if (mode == M_TLEAF && li == lend) { cur = lskip; mode = (cur == kEnd) ? M_DONE : M_TLAS; }
        }

        // ---------------- one BLAS leaf entry
        if (kGeneral && mode == M_BLEAF)
        {
            const float lim = tMaxW * iscale;
            if (iflags & FI_SPHERESET)
            {
                const int p = S.spherePrimIdx[bj];
                const hrt_sphere* sp = &S.spheres[p];
                float t;
                if (hit_sphere_t(w, cv3(sp->center), sp->radius, t) && t > 0.001f && t < lim)
                {
                    if (iinst < 0) iinst = S.tlasInst[islot];
                    L.add(k, t / iscale, t, islot, p, iinst, p);
                }
            }
            else
            {
                FTri trs[LT];
#pragma unroll
                for (int qq = 0; qq < LT; qq++) trs[qq] = P.ftri[bj + qq < bend ? bj + qq : bend - 1];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int qq = 0; qq < LT; qq++)
                {
                    if (qq > 0) { if (!(bj + 1 < bend)) break; bj++; }
                    const FTri trr = trs[qq];
                    float t, bu, bv;
                    if (hit_tri_t(w, xyz(trr.v0), xyz(trr.v1), xyz(trr.v2), t, bu, bv) && t > 0.001f && t < lim)
                    {   // TraceClosest's alpha rule (:206-221): the linear mask sample
                        bool accept = true;
                        if (kAlpha && (wbits(trr.v2) & FT_TEXTURED))
                        {
                            const hrt_material* mat = &S.materials[wbits(trr.v1)];
                            const int ati = mat->AlphaTexIndex;
                            float alpha = 1.f;
                            if (mat->HasAlphaMap != 0 && ati >= 0 && ati < S.n_texInfos)
                            {
                                float uu, vv;
                                tr.tri_uv(wbits(trr.v0), bu, bv, uu, vv);
                                alpha = tex.mask_linear(S.texInfos[ati], uu, vv);
                            }
                            accept = !(alpha < mat->AlphaCutoff);
                        }
                        if (accept)
                        {
                            if (iinst < 0) iinst = S.tlasInst[islot];
                            L.add(k, t / iscale, t, islot, bj, iinst, wbits(trr.v0));
                        }
                    }
                }
            }
            bj++;
            if (bj == bend)
            {
                cur = bskip; mode = M_BLAS;
                if (!(cur < blasEnd))
                {
                    w = park.get();
                    mode = M_TLEAF;
                    if (li == lend) { cur = lskip; mode = (cur == kEnd) ? M_DONE : M_TLAS; }
                }
            }
        }

        // ---------------- retire finished rays
        if (mode == M_DONE)
        {
            hits_done(h, rayIdx, L);
            mode = M_IDLE;
        }
    }
}

// record of a candidate on the reference's arrays (TraceClosest's shading of a winner, SceneDeviceViews.cs:65-86, 146-159, 196-227)
__device__ __forceinline__ void ref_shade(const DScene& S, const Ray& wray, float t, float tObj, int instIdx, int prim, Hit& best)
{
    Tex tex(S);
    const hrt_instance* inst = &S.instances[instIdx];
    Ray iray;
    iray.o = xform_point(inst->worldToObject, wray.o);
    iray.d = xform_vector(inst->worldToObject, wray.d);
    iray.inv = inv_dir(iray.d);
    F3 nObj, alb; int shade = 0; float ior = 1.f; int objId;
    if (inst->type == HRT_BLAS_SPHERESET)
    {
        const hrt_sphere* sp = &S.spheres[prim];
        nObj = sphere_normal(iray, cv3(sp->center), tObj);
        F3 kd = cv3(sp->material.Kd);
        alb = (kd.x == 0.f && kd.y == 0.f && kd.z == 0.f) ? cv3(sp->albedo) : kd;
        int dti = sp->material.DiffuseTexIndex;
        if (sp->material.HasDiffuseMap != 0 && dti >= 0 && dti < S.n_texInfos)
        {
            float u = 0.5f + hrt_atan2(nObj.z, nObj.x) / (2.f * kPI);
            float v = hrt_acos(hrt_fmin(1.f, hrt_fmax(-1.f, nObj.y))) / kPI;
            alb = tex.linear_rgb(S.texInfos[dti], u, v);
        }
        shade = sp->shading;
        float sior = sp->ior;
        ior = sior > 0.f ? sior : 1.f;
        objId = -1;
    }
    else
    {
        hrt_mesh_tri tri = S.meshTris[prim];
        F3 v0 = ld3(&S.meshPositions[tri.i0]), v1 = ld3(&S.meshPositions[tri.i1]), v2 = ld3(&S.meshPositions[tri.i2]);
        const hrt_material* mat = &S.materials[S.triMatIndex[prim]];
        F3 kd = cv3(mat->Kd);
        int dti = mat->DiffuseTexIndex;
        if (mat->HasDiffuseMap != 0 && dti >= 0 && dti < S.n_texInfos)
        {
            float th, bu, bv;
            hit_tri_t(iray, v0, v1, v2, th, bu, bv);          // same inputs -> same (bu, bv) as in the walk
            hrt_mesh_tri_uv tuv = S.meshTriUVs[prim];
            hrt_float2 t0 = S.meshTexcoords[tuv.t0], t1 = S.meshTexcoords[tuv.t1], t2 = S.meshTexcoords[tuv.t2];
            float ww = 1.f - bu - bv;
            float uu = t0.X * ww + t1.X * bu + t2.X * bv;
            float vv = t0.Y * ww + t1.Y * bu + t2.Y * bv;
            kd = tex.linear_rgb(S.texInfos[dti], uu, vv);
        }
        nObj = normalize(cross(v1 - v0, v2 - v0));
        if ((mat->TwoSided != 0) && (dot(nObj, iray.d) > 0.f)) nObj = nObj * -1.f;
        alb = kd;
        objId = prim;
    }
    best.t = t;
    best.n = normalize(xform_vector(inst->objectToWorld, nObj));
    best.albedo = alb; best.objId = objId; best.shade = shade; best.ior = ior;
}

} // namespace

#ifndef HRT_QUERY_WAVES
#define HRT_QUERY_WAVES 4
#endif

template <int FEAT, int LT>
__global__ void __launch_bounds__(256, HRT_QUERY_WAVES)
hrt_hits_walk_kernel(TracerPackedT<FEAT> tr, HitsK h)
{
    walk_hits<FEAT, LT>(tr, h);
}

// every hit slot: the record of its raw candidate (finish_hit with t = 0 passes its miss guard; t is the candidate's world t), or the
// miss padding
template <int FEAT>
__global__ void __launch_bounds__(256)
hrt_hits_finish_kernel(TracerPackedT<FEAT> tr, HitsK h)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= (long long)h.n * h.k) return;
    const int i = (int)(s / h.k), j = (int)(s - (long long)i * h.k);
    float4* slot = h.hits + 3 * s;
    if (j >= h.counts[i]) { store_miss(slot); return; }
    const float4 w = slot[0], w1 = slot[1];
    float tMax;
    const Ray r = query_ray(seg_k(h), i, tMax);
    const int lslot = __float_as_int(w.z), prim = __float_as_int(w.w);
    Hit hh;
    (void)tr.finish_hit(r, 0.f, w.y, lslot, prim, hh);
    hh.t = w.x;
    store_hit(slot, hh, __float_as_int(w1.x), __float_as_int(w1.y));
}

// the reference's arrays, one ray per lane: ShadowOcclusion's walk (SceneDeviceViews.cs:89-121, 240-327) run to the end with
// TraceClosest's acceptance (:124-237), then the ray's records shaded in place and the padding written.  NONFINITE: the fix-up pass of
// a packed walk, which answers only the rays with a non-finite origin or direction
template <bool NONFINITE>
__global__ void __launch_bounds__(256)
hrt_hits_ref_kernel(DScene S, HitsK h)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= h.n) return;
    float tMaxWorld;
    const Ray wray = query_ray(seg_k(h), i, tMaxWorld);
    if (NONFINITE && query_finite(wray)) return;
    Tex tex(S);
    const int k = h.k;
    HitList L; L.start(h, i);
    int cur = 0;
    while (cur != -1)
    {
        const hrt_bvh_node* n = &S.tlasNodes[cur];
        const int skip = n->skipIndex;
        if (!hit_aabb(wray, n, 0.001f, tMaxWorld)) { cur = skip; continue; }
        if (n->count <= 0) { cur = n->left; continue; }
        for (int e = n->first; e < n->first + n->count; e++)
        {
            const int instIdx = S.tlasInst[e];
            const hrt_instance* inst = &S.instances[instIdx];
            Ray iray;
            iray.o = xform_point(inst->worldToObject, wray.o);
            iray.d = xform_vector(inst->worldToObject, wray.d);
            iray.inv = inv_dir(iray.d);
            const float us = inst->uniformScale;
            const float scale = us > 0.f ? us : 1.f;
            const float tMaxObj = tMaxWorld * scale;
            const int blasStart = inst->blasRoot, blasEnd = blasStart + inst->blasNodeCount;
            const bool isSphere = inst->type == HRT_BLAS_SPHERESET;
            int bcur = blasStart;
            while (bcur != -1 && bcur < blasEnd)
            {
                const hrt_bvh_node* bn = &S.blasNodes[bcur];
                const int bskip = bn->skipIndex;
                if (!hit_aabb(iray, bn, 0.001f, tMaxObj)) { bcur = bskip; continue; }
                if (bn->count <= 0) { bcur = bn->left; continue; }
                for (int jj = bn->first; jj < bn->first + bn->count; jj++)
                {
                    if (isSphere)
                    {
                        const int p = S.spherePrimIdx[jj];
                        const hrt_sphere* sp = &S.spheres[p];
                        float t;
                        if (hit_sphere_t(iray, cv3(sp->center), sp->radius, t) && t > 0.001f && t < tMaxObj)
                            L.add(k, t / scale, t, instIdx, p, instIdx, p);
                    }
                    else
                    {
                        const int ti = S.triPrimIdx[jj];
                        const hrt_mesh_tri tri = S.meshTris[ti];
                        const F3 v0 = ld3(&S.meshPositions[tri.i0]), v1 = ld3(&S.meshPositions[tri.i1]), v2 = ld3(&S.meshPositions[tri.i2]);
                        float t, bu, bv;
                        if (hit_tri_t(iray, v0, v1, v2, t, bu, bv) && t > 0.001f && t < tMaxObj)
                        {
                            const hrt_material* mat = &S.materials[S.triMatIndex[ti]];
                            const int ati = mat->AlphaTexIndex;
                            float alpha = 1.f;
                            if (mat->HasAlphaMap != 0 && ati >= 0 && ati < S.n_texInfos)
                            {
                                const hrt_mesh_tri_uv tuv = S.meshTriUVs[ti];
                                const hrt_float2 t0 = S.meshTexcoords[tuv.t0], t1 = S.meshTexcoords[tuv.t1], t2 = S.meshTexcoords[tuv.t2];
                                const float ww = 1.f - bu - bv;
                                const float uu = t0.X * ww + t1.X * bu + t2.X * bv;
                                const float vv = t0.Y * ww + t1.Y * bu + t2.Y * bv;
                                alpha = tex.mask_linear(S.texInfos[ati], uu, vv);
                            }
                            if (!(alpha < mat->AlphaCutoff)) L.add(k, t / scale, t, instIdx, ti, instIdx, ti);
                        }
                    }
                }
                bcur = bskip;
            }
        }
        cur = skip;
    }
    hits_done(h, i, L);
    for (int j = 0; j < k; j++)
    {
        float4* slot = L.base + 3 * j;
        if (j >= L.cnt) { store_miss(slot); continue; }
        const float4 w = slot[0];
        Hit hh;
        ref_shade(S, wray, w.x, w.y, __float_as_int(w.z), __float_as_int(w.w), hh);
        store_hit(slot, hh, __float_as_int(w.z), __float_as_int(w.w));
    }
}

template <int F>
static void launch_packed(const HitsLaunch& L, hipStream_t st)
{
    TracerPackedT<F> tr; tr.P = L.P; tr.S = L.S;
    const dim3 block(256), gridS((unsigned)(((long long)L.h.n * L.h.k + 255) / 256));
    if (L.lt3) hipLaunchKernelGGL((hrt_hits_walk_kernel<F, (F != 0 ? 3 : 2)>), dim3(L.gridW), block, 0, st, tr, L.h);
    else       hipLaunchKernelGGL((hrt_hits_walk_kernel<F, 2>), dim3(L.gridW), block, 0, st, tr, L.h);
    hipLaunchKernelGGL((hrt_hits_finish_kernel<F>), gridS, block, 0, st, tr, L.h);
}

hipError_t hits_launch(const HitsLaunch& L, hipStream_t st)
{
    const dim3 block(256), gridR((unsigned)((L.h.n + 255) / 256));
    if (L.variant < 0)
    {
        hipLaunchKernelGGL((hrt_hits_ref_kernel<false>), gridR, block, 0, st, L.S, L.h);
        return hipGetLastError();
    }
    hipError_t e = hipMemsetAsync(L.h.grab, 0, 8 * kQueryGrabStride * sizeof(int), st);
    if (e != hipSuccess) return e;
    if (L.variant == 0)      launch_packed<0>(L, st);
    else if (L.variant == 1) launch_packed<1>(L, st);
    else                     launch_packed<3>(L, st);
    hipLaunchKernelGGL((hrt_hits_ref_kernel<true>), gridR, block, 0, st, L.S, L.h);
    return hipGetLastError();
}
