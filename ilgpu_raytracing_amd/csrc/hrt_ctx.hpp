// hrt_ctx.hpp -- the context behind the C ABI's opaque hrt_ctx and what every host unit of the library needs to work on it:
// the per-device state, error reporting across the ABI, the HIP error check and the per-slot dispatch.  Internal: the host
// halves of hrt_runtime.hip (create / destroy / synchronise, frames, presentation, queries, denoisers) and hrt_scene.hip (scene
// upload, updates, downloads) share it; nothing above include/hip_raytrace.h sees it.
// One definition of each struct, here; the functions are defined in hrt_runtime.hip unless a comment says otherwise.
#pragma once
#include <hip/hip_runtime.h>
#include <functional>
#include <string>
#include <utility>
#include <vector>
#include "hrt_device.hpp"
#include "hrt_trace_packed.hpp"
#include "hrt_bvh.hpp"
#include "hrt_treelets.hpp"
#include "../../include/hip_raytrace.h"

namespace hrt { namespace detail {


#ifndef HRT_BATCH_LANES
#define HRT_BATCH_LANES 2
#endif
constexpr int kMaxLanes = 4, kBatchLanes = HRT_BATCH_LANES;      // sample batches in flight: 1 / 2 / 3 / 4 measured on configs 4 / 5 at 64 / 256 spp: 362 / 328 / 334 / 325 ms and 1412 / 1323 / 1376 / 1330 ms
static_assert(kBatchLanes >= 1 && kBatchLanes <= kMaxLanes, "");

// Grow-only device (or pinned host) memory of one DeviceState.  It never shrinks and is reallocated only when it is too small.
struct Scratch {
    void* p = nullptr; size_t bytes = 0;
    enum Drain { kStream, kDevice };           // what grow() waits for before it frees the old block (work enqueued earlier may use it)
    int grow(hrt_ctx* c, size_t need, hipStream_t st, Drain drain = kStream, bool pinned = false);     // no-op when need <= bytes
    void release(bool pinned = false);
};

struct DeviceState {
    int device_id = -1;
    int n_cu = 256;                            // compute units (MI355X: 256)
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;             // shadow walks run beside the closest-hit walks of the same bounce
    static constexpr int kRing = 128;          // frames that may be in flight between two syncs
    hipEvent_t ev[kRing][4] = {};
    int ring_head = 0;                         // frames enqueued since the last synchronize
    bool ring_counts = false;
    std::vector<float> frame_ms[2];            // per-frame HIP-event times (launch 1, path-trace stage) of the frames the last hrt_synchronize collected
    // scene (15 arrays)
    void* scene[15] = {};
    DScene dscene{};
    void* packed[7] = {};                      // NodeQ tlas, FInst, NodeQ blas, FTri, NodeQ TLAS leaves in walk order (device-private repack)
    DPacked dpacked{};
    TlasDevice tl{};                           // device-side TLAS maintenance (hrt_bvh.hpp); aux arrays below
    void* tlaux[10] = {};                      // parent, nchild, arrive, scanIn, scanOut, sa, flags, cost, saBase, scanTmp + costPartial
    void* tlscratch = nullptr;                 // LBVH scratch, allocated on the first rebuild
    // a second tree over the same instances, built on the device at upload: what boolean queries of fast-sphere scenes walk
    TlasDevice tl2{};
    void* tl2mem[18] = {};          // [14] slot map, [15] renumbered copies, [16] what they permute, [17] scratch of the slot map
    bool any_built = false;                    // a second tree exists for this scene (any_ok: and it describes the scene as it is now)
    size_t ordX = 0, ordP = 0;                 // records in the renumbered copies of tlasX / of tlas
    DPacked dpackedAny{};
    bool any_ok = false;
    bool tlas_base_valid = false;              // saBase holds the node areas of the TLAS as it was last built
    bool tlas_lbvh = false;                    // the TLAS in use was BUILT on the device (Auto rebuilds an uploaded tree once: the LBVH walks faster)
    BlasDevice bl{};                           // triangle-mesh BLAS maintenance after vertex updates
    void* blaux[12] = {};                      // parent, nchild, subend, orig, arrive, ids of the TriMesh instances, kind, ids of the SphereSet instances, sa, saBase, growPartial, grow
    int n_mesh_inst = 0, n_sphere_inst = 0;
    // treelets of the big triangle-mesh BLASes (hrt_treelets.hpp) and the queues of the treelet walker, per batch lane and walk kind (0 shadow, 1 closest)
    void* tlmem[3] = {};                       // reduced trees, treelet table, BLAS root -> reduced root
    DTreelets dtl{};
    bool tl_ok = false;                        // the treelets describe the BLASes as they are now (a vertex update or BLAS rebuild drops them)
    Scratch tlq_mem[kMaxLanes];
    int max_lds = 65536;                       // LDS a workgroup may ask for
    bool blas_base_valid = false;              // saBase holds the node areas of the mesh BLASes as they were last built
    // presentation (TAAU history + display-size colour), device slot 0 only
    int32_t *present_color = nullptr, *taa_hist_color = nullptr, *taa_hist_obj = nullptr;
    int present_w = 0, present_h = 0; bool taa_history_valid = false;
    // HRT_PRESENT_TAAU_REPROJECT: the pair a reprojecting resolve writes while it reads the current one (swapped after the launch;
    // allocated by the first such present), and the camera of the frame last resolved into the history (valid with the history)
    int32_t *taa_spare_color = nullptr, *taa_spare_obj = nullptr;
    hrt_camera taa_hist_cam{};
    float present_ms = 0.f;                    // HIP-event time of the last hrt_present's kernel (hrt_present_time)
    // streamed path-trace workspace
    // two sample batches are in flight at a time (lane 0 on stream / stream2, lane 1 on stream3 / stream4): each has its own workspace
    Scratch wf_mem[kMaxLanes], wf_cnt[kMaxLanes];   // path state (float planes) and counters (ints) of a lane
    Scratch wf_accum;                          // Lframe carried across the batches of a frame (one plane set of floats, shared)
    hipStream_t laneStream[kMaxLanes][2] = {};  // lanes >= 1: main and side stream (lane 0 uses stream / stream2)
    hipEvent_t evLane[kMaxLanes][3] = {};      // per lane: fork, join, resolve done
    hipEvent_t evStage = nullptr;
    Scratch split_mem;                         // fused kernel in sample groups: per-sample radiance + staged reservoirs (floats)
    // per-pixel buffers, full image size on every device (rows outside the tile stay untouched)
    int64_t nPix = 0;
    DGBuffer gb{};
    DFramebuffer fb{};
    DReservoir resA{}, resB{};
    hrt_float3* prog_carry = nullptr;          // hrt_render_progressive: raw sample sum (Lframe before 1/spp) per global pixel index, 12 B/px;
                                               // allocated by the first progressive call, at the size of the per-pixel buffers
    unsigned long long* counters = nullptr;   // 2 x 10
    int row_begin = 0, row_end = 0;            // rows [row_begin,row_end) ...
    int strip_n = 1, strip_i = 0;              // ... of which this device owns 8-row strips s with s % strip_n == strip_i
    int n_strips = 0;
    // caller-ray queries (hrt_trace_rays / hrt_trace_hits / hrt_trace_paths): one chunk in flight, shared by the three and carved per
    // chunk by ChunkStager; grown on demand and separate from the frame's buffers, so hrt_device_views pointers never move because of a
    // query and a radiance chunk's G-buffer and sample-group scratch never live in the frame's
    Scratch q_dev;                             // the chunk's device workspace, then (host path) its staged caller arrays
    Scratch q_pin;                             // pinned staging of the host path: the chunk's caller arrays
    hipEvent_t q_ev[2] = {};                   // bracket the kernels of a chunk; hrt_present and hrt_motion_vectors time theirs with them too
    // hrt_motion_vectors, host path: the slot's vectors before they are gathered (8 B per pixel, global pixel index)
    Scratch mv_mem;
    // hrt_denoise, device slot 0 only: guide records (32 B per pixel), two colour planes (16 B each), then the two result planes
    // (denoised radiance 12 B, packed colour 4 B); dn_pix = the frame size they were allocated for
    Scratch dn_mem;
    int64_t dn_pix = 0;
    hrt_float3* dn_radiance = nullptr;
    int32_t* dn_color = nullptr;
    // hrt_denoise_temporal, device slot 0 only: two guide sets (32 B per pixel each), two history colour and two history moment planes
    // (16 B each); set dt_cur holds what the last call wrote.  dt_valid: the history is not empty; dt_cam: the camera of the frame it
    // was last accumulated from (what the next call reprojects from)
    Scratch dt_mem;
    int dt_w = 0, dt_h = 0, dt_cur = 0;
    bool dt_valid = false;
    hrt_camera dt_cam{};
};

}} // namespace hrt::detail

struct hrt_ctx {
    std::vector<hrt::detail::DeviceState> dev;
    std::string err;
    bool scene_ready = false;
    bool packed_ok = false;                    // false: scene exceeds the packed layout's limits -> TracerRef
    int packed_feat = 3;                       // TracerPackedT<FEAT> variant of the committed scene
    int flat_leaves = 0;                       // > 0: TLAS leaves of a fast-sphere-only scene that fits TracerFlat
    bool own_in_world = false;                 // PackedHost::own_in_world of the uploaded scene
    bool small_scene = false;                  // <= kSmallSceneNodes BVH nodes: the walk is ALU-bound and L1-resident -> megakernel
    // state of hrt_scene_update_instances
    bool refit_ok = false;                     // every reachable TLAS node has one parent and <= 64 children
    bool feat_alpha = false;                   // the triangle half of packed_feat (does not change with the TLAS)
    int64_t n_inst = 0, n_tlas = 0, n_slots = 0, n_blas = 0;
    int tlas_leaves = 0;                       // reachable leaves of the TLAS in use
    bool tlas_on_device = false;               // the TLAS in use was refitted / rebuilt on the device (walk-order numbering)
    bool blas_refit_ok = false;                // hrt_scene_update_positions can refit every triangle-mesh BLAS
    bool blas_rebuild_ok = false;              // ... and rebuild it (HRT_REBUILD_BLAS)
    std::vector<hrt::MeshJob> mesh_jobs;
    int max_mesh_items = 0;
    int64_t n_positions = 0, n_spheres = 0;
    int64_t scene_count[15] = {};
    int width = 0, height = 0;
    hrt_camera frame_cam{}, frame_prev_cam{};  // cam / prevCam of the last frame call (what gb_worldPos was rendered from)
    uint64_t frame_serial = 0;                 // counts frame calls and scene uploads: what the denoised planes are checked against
    uint64_t dn_serial = 0;                    // frame_serial of the frame hrt_denoise or hrt_denoise_temporal last ran on (0: never)
    uint64_t dt_serial = 0;                    // frame_serial of the frame hrt_denoise_temporal last accumulated (0: never)
    long long max_resident_paths = 0;          // hrt_set_workspace_limit: 0 = kWfMaxPaths
    std::vector<std::pair<char*, size_t>> pinned;   // hrt_host_register: page-locked ranges of the caller (gather targets)
    // the progressive frame a continuation (hrt_render_progressive with sample_begin > 0) may extend: what its last call rendered.
    // Cleared by every call that changes what the next samples would see (frames, scene changes, history reset).
    struct {
        bool valid = false;
        hrt_frame_params p{};                  // params of the last call; p.spp = samples rendered so far
        int rb = 0, re = 0, sn = 1, si = 0;    // row range and strips, normalised as the render call normalises them
        uint32_t pathFlags = 0;                // HRT_FLAG_REFERENCE_LAYOUT | MEGAKERNEL | STREAMED | TREELETS of the calls
    } prog;
};

namespace hrt { namespace detail {

inline constexpr size_t kSceneElem[15] = {sizeof(hrt_bvh_node), 4, sizeof(hrt_instance), sizeof(hrt_bvh_node), 4, sizeof(hrt_sphere), 4,
                               sizeof(hrt_float3), sizeof(hrt_mesh_tri), sizeof(hrt_float2), sizeof(hrt_mesh_tri_uv), 4,
                               sizeof(hrt_material), sizeof(hrt_rgba32), sizeof(hrt_tex_info)};

// the error text of a failed call: the context's, or without a context the calling thread's (what hrt_last_error(NULL) returns)
int fail(hrt_ctx* c, int code, const std::string& msg);

// no exception crosses the C ABI: std::bad_alloc of the host-side vectors / strings -> HRT_ERR_OUT_OF_MEMORY, anything else -> HRT_ERR_HIP
int on_exception(hrt_ctx* c, const char* who) noexcept;

#define HIPCHK(ctx, expr)                                                                          \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess)                                                                     \
            return fail(ctx, e__ == hipErrorOutOfMemory ? HRT_ERR_OUT_OF_MEMORY : HRT_ERR_HIP,     \
                        std::string(#expr) + ": " + hipGetErrorString(e__));                       \
    } while (0)

// Runs fn(slot, ec) once per device slot: inline with ec = c, or, with `threads`, on one host thread per slot with ec = nullptr, so
// that fn's error text lands in the worker thread's own error text.  A call that blocks its issuing thread (a copy into pageable memory,
// a synchronise) would otherwise serialise the slots.  Reports the first failing slot as "<who>: <what>device slot <i>: <text>".
int for_each_slot(hrt_ctx* c, bool threads, const char* who, const char* what, const std::function<int(int, hrt_ctx*)>& fn);

// frees everything a scene upload allocated on one device (hrt_scene.hip); the caller has made the device current
void free_scene(DeviceState& d);

// limits of the treelet cut of the scenes committed from now on, process-wide (hrt_scene.hip): the shipped values unless a test
// lowered them (hrt_debug_set_treelet_limits)
TreeletLimits& treelet_limits();

}} // namespace hrt::detail
