// hrt_scene.hip -- the scene entry points of include/hip_raytrace.h: hrt_scene_upload, hrt_scene_update_instances / _positions /
// _spheres, hrt_scene_download_array / _tlas, and what they share (the second tree, the LBVH scratch, the tail of the updates).
// Host code only: this unit defines no kernel.  What runs on a device goes through hrt_bvh.hpp (TLAS / BLAS maintenance) and plain
// copies; what is computed on the host before that comes from hrt_scene_pack.hpp.
// (Engine/Scene.cs:258-279, 370-377; BvhManager.cs)
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "hrt_ctx.hpp"
#include "hrt_scene_pack.hpp"
#include "hrt_bvh.hpp"
#include "hrt_treelets.hpp"

using namespace hrt;
using namespace hrt::detail;

namespace {

TreeletLimits g_treelet_limits;              // shipped values unless a test lowered them (hrt_debug_set_treelet_limits)

} // namespace

namespace hrt { namespace detail {

TreeletLimits& treelet_limits() { return g_treelet_limits; }

void free_scene(DeviceState& d)
{
    for (int i = 0; i < 15; i++) { if (d.scene[i]) (void)hipFree(d.scene[i]); d.scene[i] = nullptr; }
    for (int i = 0; i < 7; i++) { if (d.packed[i]) (void)hipFree(d.packed[i]); d.packed[i] = nullptr; }
    for (int i = 0; i < 10; i++) { if (d.tlaux[i]) (void)hipFree(d.tlaux[i]); d.tlaux[i] = nullptr; }
    for (int i = 0; i < 18; i++) { if (d.tl2mem[i]) (void)hipFree(d.tl2mem[i]); d.tl2mem[i] = nullptr; }
    d.tl2 = TlasDevice{}; d.any_ok = false; d.any_built = false; d.ordX = d.ordP = 0;
    if (d.tlscratch) (void)hipFree(d.tlscratch);
    d.tlscratch = nullptr; d.tl = TlasDevice{}; d.tlas_base_valid = false; d.tlas_lbvh = false;
    for (int i = 0; i < 12; i++) { if (d.blaux[i]) (void)hipFree(d.blaux[i]); d.blaux[i] = nullptr; }
    d.bl = BlasDevice{}; d.n_mesh_inst = 0; d.n_sphere_inst = 0; d.blas_base_valid = false;
    for (int i = 0; i < 3; i++) { if (d.tlmem[i]) (void)hipFree(d.tlmem[i]); d.tlmem[i] = nullptr; }
    d.dtl = DTreelets{}; d.tl_ok = false;
}

}} // namespace hrt::detail

namespace {

// Organisation of the path-trace launch when the caller does not force one: scenes whose whole BVH
// is a few cache lines (the reference's default scene, BASELINE config 2) spend their time in ReSTIR
// arithmetic, not in the walk -- streaming path state through HBM only adds traffic there (measured:
// 2.8 ms fused vs 5.3 ms streamed on config 2; 158 ms vs 33 ms on config 3).
constexpr long long kSmallSceneNodes = 256;

constexpr int64_t kAnyTreeMinInstances = 256;       // scenes of fewer instances keep the uploaded tree alone (second tree: see build_second_tree)
#ifndef HRT_SAH_MAX_LOG2            // A/B (300 001 instances: LBVH topology 12.3 ms per frame and 0.29 s per upload, SAH 11.5 ms and 0.38 s)
#define HRT_SAH_MAX_LOG2 21
#endif
constexpr int64_t kHostSahMaxInstances = (int64_t)1 << HRT_SAH_MAX_LOG2;
int build_second_tree(hrt_ctx* c, DeviceState& d, const int32_t* uploadedSlots, int64_t nSlots, bool instOnce, const SahTopology* pre = nullptr, const hrt_instance* hostInst = nullptr);       // defined with the scene-update code below

} // namespace

extern "C" {

int hrt_scene_upload(hrt_ctx* c, const hrt_scene_desc* s)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    c->prog.valid = false;                     // a progressive frame cannot be continued across this call
    c->frame_serial++;                         // ... and denoised planes no longer belong to what is on the device
    c->dev[0].dt_valid = false;                // ... nor does the temporal denoiser's history
    if (!s) return fail(c, HRT_ERR_INVALID_ARG, "hrt_scene_upload: scene is NULL");
    const void* src[15] = {s->tlasNodes, s->tlasInstanceIndices, s->instances, s->blasNodes, s->spherePrimIdx, s->spheres,
                           s->triPrimIdx, s->meshPositions, s->meshTris, s->meshTexcoords, s->meshTriUVs, s->triMatIndex,
                           s->materials, s->texels, s->texInfos};
    const int64_t cnt[15] = {s->n_tlasNodes, s->n_tlasInstanceIndices, s->n_instances, s->n_blasNodes, s->n_spherePrimIdx, s->n_spheres,
                             s->n_triPrimIdx, s->n_meshPositions, s->n_meshTris, s->n_meshTexcoords, s->n_meshTriUVs, s->n_triMatIndex,
                             s->n_materials, s->n_texels, s->n_texInfos};
    for (int i = 0; i < 15; i++)
        if (cnt[i] < 0 || (cnt[i] > 0 && !src[i])) return fail(c, HRT_ERR_INVALID_ARG, "hrt_scene_upload: array " + std::to_string(i) + " has a count but no pointer");
    PackedHost ph;
    {
        std::string verr = validate_and_pack(s, ph);
        if (!verr.empty()) return fail(c, HRT_ERR_INVALID_ARG, "hrt_scene_upload: " + verr);
    }
    int rc = hrt_synchronize(c, nullptr);
    if (rc != HRT_OK) return rc;
    c->scene_ready = false;
    c->packed_ok = ph.ok;
    c->packed_feat = (ph.feat & 2) ? 3 : (ph.feat & 1);
    c->small_scene = (s->n_tlasNodes + s->n_blasNodes) <= kSmallSceneNodes;
    c->flat_leaves = ph.n_flat;
    c->own_in_world = ph.own_in_world;
    c->refit_ok = ph.refit_ok && ph.ok;
    c->feat_alpha = (ph.feat & 2) != 0;
    c->n_inst = s->n_instances; c->n_tlas = s->n_tlasNodes; c->n_slots = s->n_tlasInstanceIndices; c->n_blas = s->n_blasNodes;
    c->tlas_leaves = ph.reach_leaves;
    c->tlas_on_device = false;
    c->blas_refit_ok = ph.blas_refit_ok && ph.ok;
    c->blas_rebuild_ok = c->blas_refit_ok && ph.blas_rebuild_ok;
    c->mesh_jobs = ph.meshJobs;
    c->max_mesh_items = 0;
    for (const MeshJob& J : ph.meshJobs) c->max_mesh_items = std::max(c->max_mesh_items, J.n);
    c->n_positions = s->n_meshPositions; c->n_spheres = s->n_spheres;
    for (int i = 0; i < 15; i++) c->scene_count[i] = cnt[i];
    // room for a TLAS rebuilt on the device over all instances (leaves of two: hrt_bvh.hpp)
    const int64_t capT = std::max<int64_t>(std::max<int64_t>(s->n_tlasNodes, 2 * s->n_instances - 1), 1);
    const int64_t capTI = std::max<int64_t>(std::max<int64_t>(s->n_tlasInstanceIndices, s->n_instances), 1);
    hrt_bvh_node emptyTlas; std::memset(&emptyTlas, 0, sizeof(emptyTlas));
    emptyTlas.left = emptyTlas.right = emptyTlas.first = emptyTlas.skipIndex = -1;   // an empty TLAS ends the walk at once
    // topology of the second tree (many-sphere scenes): a function of the instances alone, computed once for all devices
    SahTopology sahOnce; bool haveSah = false;
    if (ph.ok && ph.feat == 0 && s->n_instances >= kAnyTreeMinInstances && ph.n_tlasX > 0 && ph.inst_once && s->n_tlasInstanceIndices == s->n_instances &&
        ph.own_in_world && s->n_instances <= kHostSahMaxInstances && s->n_instances > 2)
    {
        const std::vector<hrt_instance> inst(s->instances, s->instances + s->n_instances);
        host_sah_topology(inst, sahOnce);
        haveSah = true;
    }
    TreeletsHost tlh;
    if (ph.ok && (ph.feat & 1) && ph.blas_refit_ok && !ph.meshRanges.empty()) build_treelets(ph.blas, ph.bsubend, ph.meshRanges, g_treelet_limits, tlh);
    for (DeviceState& d : c->dev)
    {
        HIPCHK(c, hipSetDevice(d.device_id));
        free_scene(d);                                  // UploadAll disposes + reallocates all 15 (Scene.cs:260-278)
        for (int i = 0; i < 15; i++)
        {
            int64_t n = cnt[i] > 0 ? cnt[i] : 1;       // AllocateOrEmpty: empty -> 1 zeroed element
            size_t bytes = (size_t)n * kSceneElem[i];
            const size_t room = i == 0 ? (size_t)capT * kSceneElem[0] : (i == 1 ? (size_t)capTI * kSceneElem[1] : bytes);
            HIPCHK(c, hipMalloc(&d.scene[i], std::max(bytes, room)));
            if (cnt[i] > 0) HIPCHK(c, hipMemcpyAsync(d.scene[i], src[i], bytes, hipMemcpyHostToDevice, d.stream));
            else if (i == 0) HIPCHK(c, hipMemcpyAsync(d.scene[i], &emptyTlas, bytes, hipMemcpyHostToDevice, d.stream));
            else HIPCHK(c, hipMemsetAsync(d.scene[i], 0, bytes, d.stream));
        }
        DScene& S = d.dscene;
        S.tlasNodes = (const hrt_bvh_node*)d.scene[0]; S.tlasInst = (const int32_t*)d.scene[1];
        S.instances = (const hrt_instance*)d.scene[2]; S.blasNodes = (const hrt_bvh_node*)d.scene[3];
        S.spherePrimIdx = (const int32_t*)d.scene[4]; S.spheres = (const hrt_sphere*)d.scene[5];
        S.triPrimIdx = (const int32_t*)d.scene[6]; S.meshPositions = (const hrt_float3*)d.scene[7];
        S.meshTris = (const hrt_mesh_tri*)d.scene[8]; S.meshTexcoords = (const hrt_float2*)d.scene[9];
        S.meshTriUVs = (const hrt_mesh_tri_uv*)d.scene[10]; S.triMatIndex = (const int32_t*)d.scene[11];
        S.materials = (const hrt_material*)d.scene[12]; S.texels = (const hrt_rgba32*)d.scene[13];
        S.texInfos = (const hrt_tex_info*)d.scene[14];
        S.n_texInfos = (int32_t)(cnt[14] > 0 ? cnt[14] : 1);
        // device-private repack (TracerPacked)
        const void* psrc[7] = {ph.tlas.data(), ph.finst.data(), ph.blas.data(), ph.ftri.data(), ph.flat.data(), nullptr, ph.tlasX.data()};       // slot 5 unused
        const size_t pbytes[7] = {ph.tlas.size() * sizeof(NodeQ), ph.finst.size() * sizeof(FInst), ph.blas.size() * sizeof(NodeQ), ph.ftri.size() * sizeof(FTri),
                                  ph.flat.size() * sizeof(NodeQ), 0, ph.tlasX.size() * sizeof(NodeQ)};
        const size_t proom[7] = {(size_t)capT * sizeof(NodeQ), (size_t)capTI * sizeof(FInst), 0, 0, (size_t)kFlatMaxLeaves * sizeof(NodeQ), 0,
                                 (size_t)(capT + capTI) * sizeof(NodeQ)};
        for (int i = 0; i < 7; i++)
        {
            if (!psrc[i]) continue;
            HIPCHK(c, hipMalloc(&d.packed[i], std::max(pbytes[i], proom[i])));
            HIPCHK(c, hipMemcpyAsync(d.packed[i], psrc[i], pbytes[i], hipMemcpyHostToDevice, d.stream));
        }
        {   // maintenance arrays of the device-side TLAS update
            const size_t scanTmp = (tlas_scan_temp_bytes((int)capT) + 255) & ~(size_t)255, nPart = (size_t)(capT + 255) / 256;
            const size_t ab[10] = {(size_t)capT * 4, (size_t)capT * 4, (size_t)capT * 4, (size_t)capT * 8, (size_t)capT * 8, (size_t)capT * 4, 16, 16, (size_t)capT * 4,
                                   scanTmp + 3 * nPart * 4};
            for (int i = 0; i < 10; i++) { HIPCHK(c, hipMalloc(&d.tlaux[i], ab[i])); HIPCHK(c, hipMemsetAsync(d.tlaux[i], 0, ab[i], d.stream)); }
            if (!ph.parent.empty())
            {
                HIPCHK(c, hipMemcpyAsync(d.tlaux[0], ph.parent.data(), std::min(ph.parent.size(), (size_t)capT) * 4, hipMemcpyHostToDevice, d.stream));
                HIPCHK(c, hipMemcpyAsync(d.tlaux[1], ph.nchild.data(), std::min(ph.nchild.size(), (size_t)capT) * 4, hipMemcpyHostToDevice, d.stream));
            }
            TlasDevice& T = d.tl;
            T = TlasDevice{};
            T.tlasNodes = (hrt_bvh_node*)d.scene[0]; T.tlasInst = (int32_t*)d.scene[1]; T.instances = (hrt_instance*)d.scene[2];
            T.blasNodes = (const hrt_bvh_node*)d.scene[3]; T.spherePrimIdx = (const int32_t*)d.scene[4]; T.spheres = (const hrt_sphere*)d.scene[5];
            T.tlas = (NodeQ*)d.packed[0]; T.finst = (FInst*)d.packed[1]; T.tlasX = (NodeQ*)d.packed[6]; T.flat = (NodeQ*)d.packed[4];
            T.parent = (int*)d.tlaux[0]; T.nchild = (int*)d.tlaux[1]; T.arrive = (int*)d.tlaux[2]; T.scanIn = (unsigned long long*)d.tlaux[3]; T.scanOut = (unsigned long long*)d.tlaux[4];
            T.scanTmp = d.tlaux[9]; T.scanTmpBytes = scanTmp; T.costPartial = (float*)((char*)d.tlaux[9] + scanTmp);
            T.directMax = 63;                                   // walk order; apply_update rebuilds a tree that fails refit_ok first
            T.sa = (float*)d.tlaux[5]; T.flags = (int*)d.tlaux[6]; T.cost = (float*)d.tlaux[7]; T.saBase = (float*)d.tlaux[8];
            T.nI = (int)s->n_instances; T.nT = (int)s->n_tlasNodes; T.nTI = (int)s->n_tlasInstanceIndices;
            if ((!ph.meshInst.empty() || !ph.sphereInst.empty()) && ph.blas_refit_ok)
            {
                const size_t nBq = ph.blas.size();
                static const int32_t none = 0;
                const void* bsrc[12] = {ph.bparent.data(), ph.bnchild.data(), ph.bsubend.data(), ph.borig.data(), nullptr,
                                        ph.meshInst.empty() ? &none : ph.meshInst.data(), ph.bkind.data(), ph.sphereInst.empty() ? &none : ph.sphereInst.data(),
                                        nullptr, nullptr, nullptr, nullptr};
                const size_t bb[12] = {nBq * 4, nBq * 4, nBq * 4, nBq * 4, nBq * 4, std::max<size_t>(ph.meshInst.size(), 1) * 4, nBq * 4, std::max<size_t>(ph.sphereInst.size(), 1) * 4,
                                       nBq * 4, nBq * 4, ((nBq + 255) / 256) * 8, 16};
                for (int i = 0; i < 12; i++)
                {
                    HIPCHK(c, hipMalloc(&d.blaux[i], bb[i]));
                    if (bsrc[i]) HIPCHK(c, hipMemcpyAsync(d.blaux[i], bsrc[i], bb[i], hipMemcpyHostToDevice, d.stream));
                    else HIPCHK(c, hipMemsetAsync(d.blaux[i], 0, bb[i], d.stream));
                }
                BlasDevice& B = d.bl;
                B.blasNodes = (hrt_bvh_node*)d.scene[3]; B.triPrimIdx = (const int32_t*)d.scene[6]; B.meshTris = (const hrt_mesh_tri*)d.scene[8];
                B.triPrimIdxW = (int32_t*)d.scene[6]; B.triMatIndex = (const int32_t*)d.scene[11]; B.materials = (const hrt_material*)d.scene[12];
                B.nMaterials = (int)s->n_materials; B.texLen = (int)(s->n_texInfos > 0 ? s->n_texInfos : 1);
                B.spherePrimIdx = (const int32_t*)d.scene[4]; B.spheres = (const hrt_sphere*)d.scene[5]; B.kind = (int*)d.blaux[6];
                B.sa = (float*)d.blaux[8]; B.saBase = (float*)d.blaux[9]; B.growPartial = (float*)d.blaux[10]; B.grow = (float*)d.blaux[11];
                B.positions = (hrt_float3*)d.scene[7]; B.blas = (NodeQ*)d.packed[2]; B.ftri = (FTri*)d.packed[3];
                B.parent = (int*)d.blaux[0]; B.nchild = (int*)d.blaux[1]; B.subend = (int*)d.blaux[2]; B.orig = (int*)d.blaux[3]; B.arrive = (int*)d.blaux[4];
                B.nB = (int)s->n_blasNodes; B.nSlots = (int)s->n_triPrimIdx; B.directMax = 7;   // leaves cost up to four triangle records each: 7 / 15 / 31 / 63 measured 0.47 / 0.50 / 0.52 / 0.56 ms for the refit of a 524 k-node BLAS
                B.maxRange[0] = 0; B.maxRange[1] = ph.max_range[1]; B.maxRange[2] = ph.max_range[2];
                d.n_sphere_inst = (int)ph.sphereInst.size();
                d.n_mesh_inst = (int)ph.meshInst.size();
            }
            T.capT = (int)capT; T.capTI = (int)capTI; T.flatMax = kFlatMaxLeaves;
        }
        d.dpacked.tlas = (const NodeQ*)d.packed[0]; d.dpacked.finst = (const FInst*)d.packed[1];
        d.dpacked.blas = (const NodeQ*)d.packed[2]; d.dpacked.ftri = (const FTri*)d.packed[3];
        d.dpacked.nTlas = (int)ph.tlas.size();
        d.dpacked.tlasX = ph.n_tlasX > 0 ? (const NodeQ*)d.packed[6] : nullptr; d.dpacked.nTlasX = ph.n_tlasX;
        {   // triangle records per leaf step of the walker: three where leaves of three outnumber the fuller ones, else two (hrt_walker.hpp)
            size_t n3 = 0, n4 = 0;
            for (const NodeQ& q : ph.blas)
            {
                const unsigned cnt = (unsigned)__builtin_bit_cast(int, q.hi.w) >> 28;
                if (cnt == 3) n3++; else if (cnt >= 4) n4++;
            }
            d.dpacked.leafTris = n3 > n4 ? 3 : 2;
        }
        // treelets of the big triangle-mesh BLASes: what the LDS-staged walker of production frames walks (hrt_walker_tl.hpp)
        if (ph.ok && (ph.feat & 1) && ph.blas_refit_ok && !ph.meshRanges.empty() && !tlh.tl.empty())
        {
            const void* tsrc[3] = {tlh.red.data(), tlh.tl.data(), tlh.redOfRoot.data()};
            const size_t tbytes[3] = {tlh.red.size() * sizeof(NodeQ), tlh.tl.size() * sizeof(Treelet), tlh.redOfRoot.size() * sizeof(int32_t)};
            for (int i = 0; i < 3; i++)
            {
                HIPCHK(c, hipMalloc(&d.tlmem[i], tbytes[i]));
                HIPCHK(c, hipMemcpyAsync(d.tlmem[i], tsrc[i], tbytes[i], hipMemcpyHostToDevice, d.stream));
            }
            d.dtl.red = (const NodeQ*)d.tlmem[0]; d.dtl.tl = (const Treelet*)d.tlmem[1]; d.dtl.redOfRoot = (const int*)d.tlmem[2];
            d.dtl.nTl = (int)tlh.tl.size(); d.dtl.nRed = (int)tlh.red.size();
            d.dtl.redLds = (int)std::min<size_t>(tlh.red.size(), (size_t)kTlRedLdsMax);
            d.dtl.tlBytesMax = (tlh.tlBytesMax + 15) & ~15;
            const int histBins = d.dtl.nTl <= kTlHistLds ? d.dtl.nTl : 0;
            d.tl_ok = tl_shared_bytes(d.dtl.tlBytesMax, d.dtl.redLds, histBins) <= (size_t)d.max_lds;
        }
        HIPCHK(c, hipStreamSynchronize(d.stream));      // host arrays are only borrowed for the duration of the call
        if (int rcB = build_second_tree(c, d, s->tlasInstanceIndices, s->n_tlasInstanceIndices, ph.inst_once, haveSah ? &sahOnce : nullptr, s->instances))
        {   // the second tree is an accelerator, not part of the scene: without memory for it the walks use the uploaded tree
            if (rcB != HRT_ERR_OUT_OF_MEMORY) return rcB;
            (void)hipGetLastError();
            for (int i = 0; i < 18; i++) { if (d.tl2mem[i]) (void)hipFree(d.tl2mem[i]); d.tl2mem[i] = nullptr; }
            d.tl2 = TlasDevice{}; d.any_ok = false; d.any_built = false; d.ordX = d.ordP = 0;
            c->err.clear();
        }
    }
    c->scene_ready = true;
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_scene_upload"); }

namespace {

constexpr float kAutoRebuildGrowth = 1.5f;     // HRT_REBUILD_AUTO: rebuild when the node boxes grew to this multiple of their built area (geometric mean)

int ensure_lbvh_scratch(hrt_ctx* c, DeviceState& d)
{
    if (d.tlscratch) return HRT_OK;
    TlasDevice& T = d.tl;
    const size_t n = (size_t)std::max(std::max(T.nI, c->max_mesh_items), 1);
    const size_t L = n + 1;                                                                                   // Karras' tree over the single items
    const size_t sortBytes = tlas_sort_temp_bytes((int)n), iscanBytes = tlas_iscan_temp_bytes((int)n + 1);
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t total = 3 * up(n * 4) + 5 * up(L * 4) + up(6 * 4) + up(sortBytes) + 2 * up((n + 1) * 4) + up(16 * 4) + up(iscanBytes);
    HIPCHK(c, hipMalloc(&d.tlscratch, total));
    char* p = (char*)d.tlscratch;
    auto take = [&](size_t b) { char* r = p; p += up(b); return (void*)r; };
    T.keys = (unsigned*)take(n * 4); T.keysSorted = (unsigned*)take(n * 4); T.vals = (int*)take(n * 4);
    T.rngA = (int*)take(L * 4); T.rngB = (int*)take(L * 4); T.split = (int*)take(L * 4); T.parInt = (int*)take(L * 4);
    T.parLeaf = (int*)take(L * 4);
    T.cboundsKey = (unsigned*)take(6 * 4);
    T.lstart = (int*)take((n + 1) * 4); T.lsum = (int*)take((n + 1) * 4); T.leafCounts = (int*)take(16 * 4);
    T.iscanTmp = take(iscanBytes); T.iscanTmpBytes = iscanBytes;
    T.sortTmp = take(sortBytes); T.sortTmpBytes = sortBytes;
    return HRT_OK;
}

// Scenes made of many fast-sphere instances (identity transform, one sphere): a second TLAS over the same instances (topology from
// host_sah_topology below, or the LBVH of the scene updates for very many instances; everything else by the device kernels of the
// scene updates), for the walks of the streamed pipeline (hrt_walker.hpp, ALT) and launch 1.  Any-hit walks and
// the last bounce's hit-or-miss walk do not depend on the tree at all; a closest-hit walk depends on it only through the order
// in which instances at exactly the same distance are met, which the walker detects and resolves on the uploaded tree.  The
// reference's median split cuts such a scene into slabs when one instance dominates the bounds (the ground sphere of BASELINE
// config 3: 103 node visits per ray against 50).  Needs the uploaded tree to list every instance exactly once (the
// second tree is built over "the instances").  Scene updates refit it (refit_second_tree).
int build_second_tree(hrt_ctx* c, DeviceState& d, const int32_t* uploadedSlots, int64_t nSlots, bool instOnce, const SahTopology* pre, const hrt_instance* hostInst)
{
    d.any_ok = false; d.any_built = false;
    // own_in_world: the second tree's leaf boxes are unions of the instances' worldBounds, and its exactness argument needs every instance's
    // own box inside them (an instance whose BLAS the position-indexed builder put over another sphere, Scene.cs:386-395, breaks that)
    if (!c->packed_ok || c->packed_feat != 0 || c->n_inst < kAnyTreeMinInstances || !d.dpacked.tlasX || !instOnce || nSlots != c->n_inst || !c->own_in_world) return HRT_OK;
    int rc = ensure_lbvh_scratch(c, d);
    if (rc != HRT_OK) return rc;
    TlasDevice T = d.tl;                                        // inputs, capacities, temporaries and LBVH scratch are shared; outputs are its own
    const size_t capT = (size_t)T.capT, capTI = (size_t)T.capTI;
    const size_t bytes[14] = {capT * sizeof(hrt_bvh_node), capTI * 4, capT * sizeof(NodeQ), capTI * sizeof(FInst), (capT + capTI) * sizeof(NodeQ),
                              (size_t)kFlatMaxLeaves * sizeof(NodeQ), capT * 4, capT * 4, capT * 4, capT * 8, capT * 8, capT * 4, capT * 4, 32};
    for (int i = 0; i < 14; i++)
    {
        if (d.tl2mem[i]) { (void)hipFree(d.tl2mem[i]); d.tl2mem[i] = nullptr; }
        HIPCHK(c, hipMalloc(&d.tl2mem[i], bytes[i]));
        HIPCHK(c, hipMemsetAsync(d.tl2mem[i], 0, bytes[i], d.stream));
    }
    T.tlasNodes = (hrt_bvh_node*)d.tl2mem[0]; T.tlasInst = (int32_t*)d.tl2mem[1]; T.tlas = (NodeQ*)d.tl2mem[2]; T.finst = (FInst*)d.tl2mem[3];
    T.tlasX = (NodeQ*)d.tl2mem[4]; T.flat = (NodeQ*)d.tl2mem[5]; T.parent = (int*)d.tl2mem[6]; T.nchild = (int*)d.tl2mem[7]; T.arrive = (int*)d.tl2mem[8];
    T.scanIn = (unsigned long long*)d.tl2mem[9]; T.scanOut = (unsigned long long*)d.tl2mem[10]; T.sa = (float*)d.tl2mem[11]; T.saBase = (float*)d.tl2mem[12];
    T.flags = (int*)d.tl2mem[13]; T.cost = (float*)((char*)d.tl2mem[13] + 16);
    int leaves = 0;
    // the instances as the host uploaded them (no copy back from the device when the caller still has them)
    std::vector<hrt_instance> inst;
    if (hostInst) inst.assign(hostInst, hostInst + c->n_inst);
    else
    {
        inst.resize((size_t)c->n_inst);
        HIPCHK(c, hipMemcpy(inst.data(), T.instances, inst.size() * sizeof(hrt_instance), hipMemcpyDeviceToHost));
    }
    if (c->n_inst <= kHostSahMaxInstances && c->n_inst > 2)
    {
        // the topology depends on the instances alone: the upload computes it once and hands it to every device
        SahTopology own;
        if (!pre) host_sah_topology(inst, own);
        const SahTopology& sah = pre ? *pre : own;
        T.nT = (int)sah.nodes.size(); T.nTI = (int)c->n_inst; leaves = sah.leaves;
        if (T.nT > T.capT || T.nTI > T.capTI || T.nT != 2 * leaves - 1) return fail(c, HRT_ERR_HIP, "second tree: host topology does not fit");
        HIPCHK(c, hipMemcpyAsync(T.tlas, sah.nodes.data(), sah.nodes.size() * sizeof(NodeQ), hipMemcpyHostToDevice, d.stream));
        HIPCHK(c, hipMemcpyAsync(T.tlasInst, sah.order.data(), sah.order.size() * 4, hipMemcpyHostToDevice, d.stream));
        HIPCHK(c, hipMemcpyAsync(T.parent, sah.parent.data(), sah.parent.size() * 4, hipMemcpyHostToDevice, d.stream));
        HIPCHK(c, hipMemcpyAsync(T.nchild, sah.nchild.data(), sah.nchild.size() * 4, hipMemcpyHostToDevice, d.stream));
        HIPCHK(c, hipStreamSynchronize(d.stream));              // the vectors go out of scope
    }
    else
        HIPCHK(c, tlas_rebuild_topology(T, d.stream, &leaves));
    T.directMax = 63;                                           // emitted in walk order
    HIPCHK(c, tlas_finish(T, d.stream));
    HIPCHK(c, tlas_inflate(T, d.stream));
    int flags[4] = {1, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(flags, T.flags, sizeof(flags), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    if (flags[0] != 0 || flags[1] != 0 || leaves <= 0 || (int64_t)T.nT + T.nTI >= kEnd) return HRT_OK;      // an instance that is not a fast sphere after all
    // leaf slot of the uploaded tree -> leaf slot of this one (both list every instance once)
    if (T.nTI != (int)nSlots) return HRT_OK;
    std::vector<int32_t> mine((size_t)nSlots), slotOfInst((size_t)c->n_inst, -1), map((size_t)nSlots);
    HIPCHK(c, hipMemcpyAsync(mine.data(), T.tlasInst, (size_t)nSlots * 4, hipMemcpyDeviceToHost, d.stream));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    for (int64_t a = 0; a < nSlots; a++)
    {
        if (mine[(size_t)a] < 0 || mine[(size_t)a] >= c->n_inst || slotOfInst[(size_t)mine[(size_t)a]] >= 0) return HRT_OK;
        slotOfInst[(size_t)mine[(size_t)a]] = (int32_t)a;
    }
    for (int64_t o = 0; o < nSlots; o++) map[(size_t)o] = slotOfInst[(size_t)uploadedSlots[o]];
    if (d.tl2mem[14]) { (void)hipFree(d.tl2mem[14]); d.tl2mem[14] = nullptr; }
    HIPCHK(c, hipMalloc(&d.tl2mem[14], (size_t)nSlots * 4));
    HIPCHK(c, hipMemcpy(d.tl2mem[14], map.data(), (size_t)nSlots * 4, hipMemcpyHostToDevice));
    d.tl2 = T;
    d.dpackedAny = d.dpacked;
    d.dpackedAny.tlas = T.tlas; d.dpackedAny.finst = T.finst; d.dpackedAny.nTlas = T.nT;
    d.dpackedAny.tlasX = T.tlasX; d.dpackedAny.nTlasX = T.nT + T.nTI;
    d.dpackedAny.slotMap = (const int*)d.tl2mem[14];
    d.dpackedAny.tlasXO = nullptr; d.dpackedAny.xStride = 0; d.dpackedAny.xAxes = 0; d.dpackedAny.tlasO = nullptr; d.dpackedAny.oStride = 0;
    d.ordX = d.ordP = 0;
    if (d.tl2mem[17]) { (void)hipFree(d.tl2mem[17]); d.tl2mem[17] = nullptr; }
    HIPCHK(c, hipMalloc(&d.tl2mem[17], (size_t)nSlots * 4));
    if (d.tl2mem[15]) { (void)hipFree(d.tl2mem[15]); d.tl2mem[15] = nullptr; }
    // Which signs select a numbering: the two axes along which the instances are spread most (extent of the box centres between their
    // 5th and 95th percentile: one huge ground sphere must not count) -- measured on config 3 (22 k records, 0.7 MB a copy), every walk
    // ordered: x and z 16.2 ms, z 16.8, x 16.7, all three 18.1, none 17.5, y alone 18.9 (along y the builder's order, ground first, is the
    // better one: one sphere test bounds every ray that goes down).  The copies need not fit the L2: with only the closest-hit walks
    // on them, frames of 30 001 / 100 001 instances at 4 spp go 10.65 -> 9.4 / 14.9 -> 10.7 ms with four copies of 2.1 / 7.4 MB; the
    // budget only bounds the memory a huge scene may take.
    const int nX = T.nT + T.nTI;
#ifndef HRT_ORDERED_BUDGET_MB       // A/B
#define HRT_ORDERED_BUDGET_MB 1024
#endif
    constexpr size_t kOrderedBudget = (size_t)HRT_ORDERED_BUDGET_MB << 20;
    int axes = 0;
    {
        float ext[3];
        std::vector<float> v(inst.size());
        for (int a = 0; a < 3; a++)
        {
            for (size_t i = 0; i < inst.size(); i++)
                v[i] = a == 0 ? inst[i].worldBoundsMin.X + inst[i].worldBoundsMax.X : (a == 1 ? inst[i].worldBoundsMin.Y + inst[i].worldBoundsMax.Y : inst[i].worldBoundsMin.Z + inst[i].worldBoundsMax.Z);
            for (float& x : v) if (!std::isfinite(x)) x = 0.f;       // (an ordering for std::sort; infinite boxes are legal here)
            std::sort(v.begin(), v.end());
            ext[a] = v[v.size() - 1 - v.size() / 20] - v[v.size() / 20];
        }
        int order[3] = {0, 1, 2};
        std::sort(order, order + 3, [&](int p, int q) { return ext[p] > ext[q] || (ext[p] == ext[q] && p < q); });
        for (int k = 0; k < 2; k++)
            if (ext[order[k]] > 0.f && ext[order[k]] >= 0.25f * ext[order[0]] && (size_t)nX * sizeof(NodeQ) * (size_t)ord_copies(axes | (1 << order[k])) <= kOrderedBudget)
                axes |= 1 << order[k];
    }
    const int copies = ord_copies(axes);
    if (axes != 0 && (int64_t)nX * copies < kEnd)
    {
        std::vector<NodeQ> X((size_t)nX), all((size_t)nX * (size_t)copies);
        std::vector<int> from((size_t)(nX + T.nT) * (size_t)copies);
        HIPCHK(c, hipMemcpy(X.data(), T.tlasX, (size_t)nX * sizeof(NodeQ), hipMemcpyDeviceToHost));
        bool ok = true;
        for (int o = 0; ok && o < copies; o++)
        {
            int sign[3] = {0, 0, 0};
            for (int a = 0; a < 3; a++)      // the copy bit of axis a = the index of a direction that is positive along a only
                if (axes & (1 << a)) sign[a] = (ord_copy(axes, a == 0 ? 1.f : -1.f, a == 1 ? 1.f : -1.f, a == 2 ? 1.f : -1.f) & o) ? 1 : -1;
            ok = reorder_second_tree(X, sign, o * nX, all.data() + (size_t)o * (size_t)nX, from.data() + (size_t)o * (size_t)nX, true);
        }
        // ... and of the plain node array, for launch 1 (both in one allocation: the inlined copies first)
        const int nP = T.nT;
        std::vector<NodeQ> Pn((size_t)nP), allP((size_t)nP * (size_t)copies);
        HIPCHK(c, hipMemcpy(Pn.data(), T.tlas, (size_t)nP * sizeof(NodeQ), hipMemcpyDeviceToHost));
        for (int o = 0; ok && o < copies; o++)
        {
            int sign[3] = {0, 0, 0};
            for (int a = 0; a < 3; a++)
                if (axes & (1 << a)) sign[a] = (ord_copy(axes, a == 0 ? 1.f : -1.f, a == 1 ? 1.f : -1.f, a == 2 ? 1.f : -1.f) & o) ? 1 : -1;
            ok = reorder_second_tree(Pn, sign, o * nP, allP.data() + (size_t)o * (size_t)nP, from.data() + all.size() + (size_t)o * (size_t)nP, false);
        }
        if (ok)
        {
            HIPCHK(c, hipMalloc(&d.tl2mem[15], (all.size() + allP.size()) * sizeof(NodeQ)));
            HIPCHK(c, hipMemcpy(d.tl2mem[15], all.data(), all.size() * sizeof(NodeQ), hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy((NodeQ*)d.tl2mem[15] + all.size(), allP.data(), allP.size() * sizeof(NodeQ), hipMemcpyHostToDevice));
            d.dpackedAny.tlasXO = (const NodeQ*)d.tl2mem[15]; d.dpackedAny.xStride = nX; d.dpackedAny.xAxes = axes;
            d.dpackedAny.tlasO = (const NodeQ*)d.tl2mem[15] + all.size(); d.dpackedAny.oStride = nP;
            if (d.tl2mem[16]) { (void)hipFree(d.tl2mem[16]); d.tl2mem[16] = nullptr; }
            HIPCHK(c, hipMalloc(&d.tl2mem[16], from.size() * sizeof(int)));
            HIPCHK(c, hipMemcpy(d.tl2mem[16], from.data(), from.size() * sizeof(int), hipMemcpyHostToDevice));
            d.ordX = all.size(); d.ordP = allP.size();
        }
    }
    d.any_ok = true; d.any_built = true;
    return HRT_OK;
}

// After a scene update: the second tree keeps its topology and takes the new boxes (instance records and spheres are shared with the
// tree in use and already updated), as long as the scene is still what the second tree is exact for -- every instance a fast sphere
// with a regular box (the flags of its own finish pass), the tree in use a device refit / rebuild (unions of regular boxes: nested,
// every instance once).  A new topology of the tree in use needs a new slot map.  Otherwise the walks go back to the tree in use.
int refit_second_tree(hrt_ctx* c, DeviceState& d, bool newTopologyInUse, bool sceneStillFits)
{
    d.any_ok = false;
    if (!d.any_built || !sceneStillFits || !c->own_in_world) return HRT_OK;
    const TlasDevice& T2 = d.tl2;
    if (d.tl.nTI != T2.nTI) return HRT_OK;
    HIPCHK(c, tlas_finish(T2, d.stream));
    HIPCHK(c, tlas_inflate(T2, d.stream));
    int flags[4] = {1, 1, 0, 0};
    HIPCHK(c, hipMemcpyAsync(flags, T2.flags, sizeof(flags), hipMemcpyDeviceToHost, d.stream));
    if (newTopologyInUse) HIPCHK(c, tlas_slot_map(d.tl.tlasInst, T2.tlasInst, (int*)d.tl2mem[17], (int*)d.tl2mem[14], T2.nTI, d.stream));
    if (d.dpackedAny.tlasXO)
    {
        HIPCHK(c, tlas_refresh_copies((NodeQ*)d.tl2mem[15], T2.tlasX, (const int*)d.tl2mem[16], (int)d.ordX, d.stream));
        HIPCHK(c, tlas_refresh_copies((NodeQ*)d.tl2mem[15] + d.ordX, T2.tlas, (const int*)d.tl2mem[16] + d.ordX, (int)d.ordP, d.stream));
    }
    HIPCHK(c, hipStreamSynchronize(d.stream));
    d.any_ok = flags[0] == 0 && flags[1] == 0;
    return HRT_OK;
}

} // namespace

namespace {

// Shared tail of the scene updates: `mutate` enqueues what changes the instance records on one device (staging buffers it
// allocates go into the vector and are freed here), then the TLAS is refitted / rebuilt per `policy` and the walkers' view of
// the tree is refreshed.
int apply_update(hrt_ctx* c, int policy, const char* who, const std::function<int(DeviceState&, std::vector<void*>&)>& mutate, hrt_bvh_update_stats* st)
{
    if (policy != HRT_REBUILD_AUTO && policy != HRT_REBUILD_FORCE_REFIT && policy != HRT_REBUILD_FORCE_REBUILD)
        return fail(c, HRT_ERR_INVALID_ARG, std::string(who) + ": unknown policy");
    if (!c->packed_ok) return fail(c, HRT_ERR_INVALID_STATE, std::string(who) + ": the scene exceeds the limits of the packed layout");
    if (c->n_inst <= 0) return fail(c, HRT_ERR_INVALID_STATE, std::string(who) + ": the scene has no instances");
    if (policy != HRT_REBUILD_FORCE_REBUILD && !c->refit_ok && !c->tlas_on_device)
    {
        if (policy == HRT_REBUILD_FORCE_REFIT)
            return fail(c, HRT_ERR_INVALID_STATE, std::string(who) + ": this TLAS cannot be refitted (a node has several parents or more than 64 children); use HRT_REBUILD_FORCE_REBUILD");
        policy = HRT_REBUILD_FORCE_REBUILD;
    }
    int rc = hrt_synchronize(c, nullptr);
    if (rc != HRT_OK) return rc;
    hrt_bvh_update_stats out; std::memset(&out, 0, sizeof(out));
    bool first = true;
    for (DeviceState& d : c->dev)
    {
        HIPCHK(c, hipSetDevice(d.device_id));
        TlasDevice& T = d.tl;
        hipEvent_t e0 = d.ev[0][0], e1 = d.ev[0][1];
        HIPCHK(c, hipEventRecord(e0, d.stream));
        int h_flags[4]; float h_cost[2] = {1.f, 0.f};
        auto finish_and_read = [&]() -> int {
            HIPCHK(c, tlas_finish(T, d.stream));
            HIPCHK(c, hipMemcpyAsync(h_flags, T.flags, sizeof(h_flags), hipMemcpyDeviceToHost, d.stream));
            HIPCHK(c, hipMemcpyAsync(h_cost, T.cost, sizeof(h_cost), hipMemcpyDeviceToHost, d.stream));
            HIPCHK(c, hipStreamSynchronize(d.stream));
            return HRT_OK;
        };
        auto keep_as_base = [&]() -> int {
            HIPCHK(c, hipMemcpyAsync(T.saBase, T.sa, (size_t)T.nT * 4, hipMemcpyDeviceToDevice, d.stream));
            d.tlas_base_valid = true;
            return HRT_OK;
        };
        if (!d.tlas_base_valid && policy != HRT_REBUILD_FORCE_REBUILD)
        {   // node areas of the tree as it was built: taken once, before anything moves
            HIPCHK(c, tlas_finish(T, d.stream));
            if ((rc = keep_as_base()) != HRT_OK) return rc;
        }
        d.any_ok = false;                      // the second tree describes the scene as it was: refit_second_tree brings it back below
        std::vector<void*> staged;
        struct StagedGuard {               // staging buffers of `mutate` are freed on every way out (their copies are ordered on d.stream)
            std::vector<void*>& v; hipStream_t st;
            ~StagedGuard() { if (!v.empty()) { (void)hipStreamSynchronize(st); for (void* p : v) (void)hipFree(p); } }
        } stagedGuard{staged, d.stream};
        if ((rc = mutate(d, staged)) != HRT_OK) return rc;
        int action = policy == HRT_REBUILD_FORCE_REBUILD ? HRT_REBUILD_FORCE_REBUILD : HRT_REBUILD_FORCE_REFIT;
        if (policy == HRT_REBUILD_AUTO && !d.tlas_lbvh) action = HRT_REBUILD_FORCE_REBUILD;   // an uploaded tree: the device-built one costs as much as a refit and walks faster
        float growthRefit = 0.f;
        int rebuiltLeaves = 0;
        if (action == HRT_REBUILD_FORCE_REFIT)
        {
            if ((rc = finish_and_read()) != HRT_OK) return rc;
            growthRefit = h_cost[0];
            if (policy == HRT_REBUILD_AUTO && growthRefit > kAutoRebuildGrowth) action = HRT_REBUILD_FORCE_REBUILD;
        }
        if (action == HRT_REBUILD_FORCE_REBUILD)
        {
            if ((rc = ensure_lbvh_scratch(c, d)) != HRT_OK) return rc;
            HIPCHK(c, tlas_rebuild_topology(T, d.stream, &rebuiltLeaves));
            T.directMax = 63;                                           // emitted in walk order
            if ((rc = finish_and_read()) != HRT_OK) return rc;
            if ((rc = keep_as_base()) != HRT_OK) return rc;
            h_cost[0] = 1.f;                                            // as built
            d.tlas_lbvh = true;
        }
        HIPCHK(c, hipEventRecord(e1, d.stream));
        HIPCHK(c, hipEventSynchronize(e1));
        for (void* p : staged) (void)hipFree(p);
        staged.clear();
        // the walkers' view of the tree
        const bool general = h_flags[0] != 0;
        d.dpacked.nTlas = T.nT;
        const bool inl = !general && !c->feat_alpha && (int64_t)T.nT + T.nTI < kEnd;
        d.dpacked.tlasX = inl ? (const NodeQ*)d.packed[6] : nullptr;
        d.dpacked.nTlasX = inl ? T.nT + T.nTI : 0;
        // the second tree follows the scene (same topology, new boxes) or stands down
        if ((rc = refit_second_tree(c, d, action == HRT_REBUILD_FORCE_REBUILD, !general && !c->feat_alpha && h_flags[1] == 0)) != HRT_OK) return rc;
        if (first)
        {
            float ms = 0.f;
            HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
            out.action = action; out.tlas_nodes = T.nT; out.tlas_slots = T.nTI; out.general_instances = general ? 1 : 0;
            out.growth_refit = growthRefit; out.growth_final = h_cost[0]; out.sah_cost = h_cost[1]; out.device_ms = ms;
            if (action == HRT_REBUILD_FORCE_REBUILD) { c->tlas_leaves = rebuiltLeaves; c->refit_ok = true; }
            c->packed_feat = c->feat_alpha ? 3 : (general ? 1 : 0);
            // the leaf sweep skips box tests the reference makes, which is only sound over nested boxes: the device's trees are unions of
            // the instances' worldBounds, so it takes every fast-sphere instance's own box to lie inside its worldBounds
            // ... and every worldBounds to be a regular box (no NaN bound, min <= max: h_flags[1]), or the unions are not nested
            c->flat_leaves = (!general && !c->feat_alpha && c->own_in_world && h_flags[1] == 0 && c->tlas_leaves > 0 && c->tlas_leaves <= kFlatMaxLeaves) ? c->tlas_leaves : 0;
            c->n_tlas = T.nT; c->n_slots = T.nTI;
            c->small_scene = (c->n_tlas + c->n_blas) <= kSmallSceneNodes;
            c->tlas_on_device = true;
            first = false;
        }
    }
    if (st) *st = out;
    return HRT_OK;
}

} // namespace

int hrt_scene_update_instances(hrt_ctx* c, const int32_t* ids, int32_t n, const hrt_affine3x4* xf, int32_t policy, hrt_bvh_update_stats* st)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    c->prog.valid = false;                     // a progressive frame cannot be continued across this call
    if (!c->scene_ready) return fail(c, HRT_ERR_INVALID_STATE, "hrt_scene_update_instances: no scene uploaded");
    if (n < 0 || (n > 0 && (!ids || !xf))) return fail(c, HRT_ERR_INVALID_ARG, "hrt_scene_update_instances: n instances need ids and transforms");
    {
        std::vector<uint8_t> seen((size_t)std::max<int64_t>(c->n_inst, 0), 0);
        for (int i = 0; i < n; i++)
        {
            if (ids[i] < 0 || ids[i] >= c->n_inst) return fail(c, HRT_ERR_INVALID_ARG, "hrt_scene_update_instances: instance id out of range");
            if (seen[(size_t)ids[i]]++) return fail(c, HRT_ERR_INVALID_ARG, "hrt_scene_update_instances: instance id listed twice");
        }
    }
    return apply_update(c, policy, "hrt_scene_update_instances", [&](DeviceState& d, std::vector<void*>& staged) -> int {
        if (n <= 0) return HRT_OK;
        const size_t idb = ((size_t)n * 4 + 63) & ~(size_t)63;
        void* buf = nullptr;
        HIPCHK(c, hipMalloc(&buf, idb + (size_t)n * sizeof(hrt_affine3x4)));
        staged.push_back(buf);
        HIPCHK(c, hipMemcpyAsync(buf, ids, (size_t)n * 4, hipMemcpyHostToDevice, d.stream));
        HIPCHK(c, hipMemcpyAsync((char*)buf + idb, xf, (size_t)n * sizeof(hrt_affine3x4), hipMemcpyHostToDevice, d.stream));
        HIPCHK(c, tlas_set_transforms(d.tl, (const int32_t*)buf, (const hrt_affine3x4*)((char*)buf + idb), n, d.stream));
        return HRT_OK;
    }, st);
}
catch (...) { return on_exception(c, "hrt_scene_update_instances"); }

int hrt_scene_update_positions(hrt_ctx* c, int64_t first, int64_t n, const hrt_float3* positions, int32_t policy, hrt_bvh_update_stats* st)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    c->prog.valid = false;                     // a progressive frame cannot be continued across this call
    if (!c->scene_ready) return fail(c, HRT_ERR_INVALID_STATE, "hrt_scene_update_positions: no scene uploaded");
    if (first < 0 || n < 0 || first + n > c->n_positions || (n > 0 && !positions))
        return fail(c, HRT_ERR_INVALID_ARG, "hrt_scene_update_positions: vertex range outside meshPositions");
    if (!c->blas_refit_ok)
        return fail(c, HRT_ERR_INVALID_STATE, "hrt_scene_update_positions: a triangle-mesh BLAS of this scene cannot be refitted (shared or overlapping node ranges, unreachable nodes)");
    const bool rebuildBlas = policy >= 0 && (policy & HRT_REBUILD_BLAS) != 0;
    if (policy >= 0) policy &= ~HRT_REBUILD_BLAS;
    if (rebuildBlas && !c->blas_rebuild_ok)
        return fail(c, HRT_ERR_INVALID_STATE, "hrt_scene_update_positions: a triangle-mesh BLAS of this scene cannot be rebuilt on the device (its leaves do not list their triangles in one region of triPrimIdx)");
    int blasAction = 0; float blasGrowth = 0.f;
    const int rc = apply_update(c, policy, "hrt_scene_update_positions", [&](DeviceState& d, std::vector<void*>&) -> int {
        const bool meshes = d.n_mesh_inst > 0;
        d.tl_ok = false;                                // the reduced trees hold copies of the boxes as uploaded: walks go back to the plain walker
        auto keep_base = [&]() -> int {
            HIPCHK(c, hipMemcpyAsync(d.bl.saBase, d.bl.sa, (size_t)d.bl.nB * 4, hipMemcpyDeviceToDevice, d.stream));
            d.blas_base_valid = true;
            return HRT_OK;
        };
        int rebuiltMeshes = 0;
        auto rebuild_all = [&]() -> int {
            int rc2 = ensure_lbvh_scratch(c, d);
            if (rc2 != HRT_OK) return rc2;
            rebuiltMeshes = 0;
            for (const MeshJob& J : c->mesh_jobs)
            {
                int limit = 0;
                HIPCHK(c, blas_rebuild_mesh(d.tl, d.bl, J, d.stream, &limit));
                if (limit > 0) rebuiltMeshes++;           // 0: no leaf size fits the node range of this mesh; it keeps its topology
            }
            return HRT_OK;
        };
        int rc2;
        if (meshes && !d.blas_base_valid && !rebuildBlas)
        {   // node areas of the BLASes as they were built: taken once, before the first vertex moves
            HIPCHK(c, blas_refit(d.bl, 1, d.stream));
            if ((rc2 = keep_base()) != HRT_OK) return rc2;
        }
        if (n > 0) HIPCHK(c, hipMemcpyAsync((hrt_float3*)d.scene[7] + first, positions, (size_t)n * sizeof(hrt_float3), hipMemcpyHostToDevice, d.stream));
        bool rebuilt = false;
        if (rebuildBlas && !c->mesh_jobs.empty()) { if ((rc2 = rebuild_all()) != HRT_OK) return rc2; rebuilt = true; }
        if (meshes) HIPCHK(c, blas_refit(d.bl, 1, d.stream));
        float growth = 0.f;
        if (meshes && !rebuilt)
        {
            HIPCHK(c, blas_growth(d.bl, 1, d.stream));
            HIPCHK(c, hipMemcpyAsync(&growth, d.bl.grow, 4, hipMemcpyDeviceToHost, d.stream));
            HIPCHK(c, hipStreamSynchronize(d.stream));
            if (policy == HRT_REBUILD_AUTO && growth > kAutoRebuildGrowth && c->blas_rebuild_ok && !c->mesh_jobs.empty())
            {
                if ((rc2 = rebuild_all()) != HRT_OK) return rc2;
                HIPCHK(c, blas_refit(d.bl, 1, d.stream));
                rebuilt = true;
            }
        }
        if (rebuilt && (rc2 = keep_base()) != HRT_OK) return rc2;
        if (&d == &c->dev[0]) { blasAction = meshes ? (rebuilt && rebuiltMeshes > 0 ? HRT_REBUILD_FORCE_REBUILD : HRT_REBUILD_FORCE_REFIT) : 0; blasGrowth = growth; }
        HIPCHK(c, tlas_rebound_instances(d.tl, (const int32_t*)d.blaux[5], d.n_mesh_inst, d.stream));
        return HRT_OK;
    }, st);
    if (rc == HRT_OK && st) { st->blas_action = blasAction; st->blas_growth = blasGrowth; }
    return rc;
}
catch (...) { return on_exception(c, "hrt_scene_update_positions"); }

int hrt_scene_update_spheres(hrt_ctx* c, int64_t first, int64_t n, const hrt_sphere* spheres, int32_t policy, hrt_bvh_update_stats* st)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    c->prog.valid = false;                     // a progressive frame cannot be continued across this call
    if (!c->scene_ready) return fail(c, HRT_ERR_INVALID_STATE, "hrt_scene_update_spheres: no scene uploaded");
    if (first < 0 || n < 0 || first + n > c->n_spheres || (n > 0 && !spheres))
        return fail(c, HRT_ERR_INVALID_ARG, "hrt_scene_update_spheres: range outside spheres");
    if (!c->blas_refit_ok)
        return fail(c, HRT_ERR_INVALID_STATE, "hrt_scene_update_spheres: a BLAS of this scene cannot be refitted (shared or overlapping node ranges, unreachable nodes)");
    return apply_update(c, policy, "hrt_scene_update_spheres", [&](DeviceState& d, std::vector<void*>&) -> int {
        if (n > 0) HIPCHK(c, hipMemcpyAsync((hrt_sphere*)d.scene[5] + first, spheres, (size_t)n * sizeof(hrt_sphere), hipMemcpyHostToDevice, d.stream));
        if (d.n_sphere_inst > 0) HIPCHK(c, blas_refit(d.bl, 2, d.stream));
        HIPCHK(c, tlas_rebound_instances(d.tl, (const int32_t*)d.blaux[7], d.n_sphere_inst, d.stream));
        return HRT_OK;
    }, st);
}
catch (...) { return on_exception(c, "hrt_scene_update_spheres"); }

int hrt_scene_download_array(hrt_ctx* c, int dev, int array, void* dst, int64_t cap, int64_t* count)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (!c->scene_ready) return fail(c, HRT_ERR_INVALID_STATE, "hrt_scene_download_array: no scene uploaded");
    if (dev < 0 || dev >= (int)c->dev.size() || array < 0 || array >= 15) return fail(c, HRT_ERR_INVALID_ARG, "hrt_scene_download_array: device slot or array index out of range");
    int rc = hrt_synchronize(c, nullptr);
    if (rc != HRT_OK) return rc;
    const int64_t have = array == 0 ? c->n_tlas : (array == 1 ? c->n_slots : c->scene_count[array]);
    if (count) *count = have;
    if (!dst) return HRT_OK;
    if (cap < have) return fail(c, HRT_ERR_INVALID_ARG, "hrt_scene_download_array: destination too small");
    DeviceState& d = c->dev[(size_t)dev];
    HIPCHK(c, hipSetDevice(d.device_id));
    if (have > 0) HIPCHK(c, hipMemcpyAsync(dst, d.scene[array], (size_t)have * kSceneElem[array], hipMemcpyDeviceToHost, d.stream));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_scene_download_array"); }

int hrt_scene_download_tlas(hrt_ctx* c, int dev, hrt_bvh_node* nodes, int64_t capN, int32_t* idx, int64_t capI, hrt_instance* inst, int64_t capInst, int64_t* counts)
try {
    if (!c) return HRT_ERR_INVALID_ARG;
    if (!c->scene_ready) return fail(c, HRT_ERR_INVALID_STATE, "hrt_scene_download_tlas: no scene uploaded");
    if (dev < 0 || dev >= (int)c->dev.size()) return fail(c, HRT_ERR_INVALID_ARG, "hrt_scene_download_tlas: device slot out of range");
    int rc = hrt_synchronize(c, nullptr);
    if (rc != HRT_OK) return rc;
    DeviceState& d = c->dev[(size_t)dev];
    const int64_t have[3] = {c->n_tlas, c->n_slots, c->n_inst};
    if (counts) { counts[0] = have[0]; counts[1] = have[1]; counts[2] = have[2]; }
    if ((nodes && capN < have[0]) || (idx && capI < have[1]) || (inst && capInst < have[2]))
        return fail(c, HRT_ERR_INVALID_ARG, "hrt_scene_download_tlas: destination too small");
    HIPCHK(c, hipSetDevice(d.device_id));
    if (nodes && have[0] > 0) HIPCHK(c, hipMemcpyAsync(nodes, d.scene[0], (size_t)have[0] * sizeof(hrt_bvh_node), hipMemcpyDeviceToHost, d.stream));
    if (idx && have[1] > 0) HIPCHK(c, hipMemcpyAsync(idx, d.scene[1], (size_t)have[1] * 4, hipMemcpyDeviceToHost, d.stream));
    if (inst && have[2] > 0) HIPCHK(c, hipMemcpyAsync(inst, d.scene[2], (size_t)have[2] * sizeof(hrt_instance), hipMemcpyDeviceToHost, d.stream));
    HIPCHK(c, hipStreamSynchronize(d.stream));
    return HRT_OK;
}
catch (...) { return on_exception(c, "hrt_scene_download_tlas"); }

} // extern "C"
