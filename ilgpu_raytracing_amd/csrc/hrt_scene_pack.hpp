// hrt_scene_pack.hpp -- what a scene upload computes on the HOST before anything reaches a device: validation of the caller's
// 15 arrays, the device-private repack (walk-order nodes, instance and triangle records, refit bookkeeping) and the topology
// and renumberings of the second tree of many-sphere scenes.  Pure host code (hrt_scene_pack.hip): no kernel, no HIP runtime
// call, no context -- hipcc compiles it only because NodeQ, FInst, FTri and float4 live in device headers.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>
#include "hrt_trace_packed.hpp"
#include "hrt_bvh.hpp"
#include "../../include/hip_raytrace.h"

namespace hrt { namespace detail {


struct PackedHost {
    std::vector<NodeQ> tlas, blas, flat;     // flat: the TLAS leaves in walk order (TracerFlat)
    std::vector<FInst> finst;
    std::vector<FTri> ftri;
    std::vector<NodeQ> tlasX; // FEAT 0: TLAS with instance records inlined after their leaf (walker)
    int n_tlasX = 0;          // records in tlasX (0: not built)
    int n_flat = 0;           // leaves in `flat` (0: scene does not qualify)
    std::vector<int32_t> parent, nchild;     // TLAS, packed numbering: parent of a node (-1: none), children of an inner node
    std::vector<int32_t> bparent, bnchild, bsubend, borig;   // BLAS nodes of triangle meshes, packed numbering: parent (-1 root, -2 not maintained),
                                                             // children, end of the subtree's index range, index in the uploaded numbering
    std::vector<int32_t> bkind;                              // 0: node of no maintained BLAS, 1: triangle mesh, 2: sphere set
    int max_range[3] = {0, 0, 0};                            // largest node range of a maintained BLAS, per kind
    std::vector<int32_t> sphereInst;                         // ids of the SphereSet instances whose BLAS is maintained
    std::vector<int32_t> meshInst;                           // ids of the TriMesh instances whose BLAS is maintained
    std::vector<MeshJob> meshJobs;                           // the same, with what a device-side rebuild of the BLAS needs
    std::vector<std::pair<int64_t, int64_t>> meshRanges;     // node ranges of the maintained triangle-mesh BLASes (walk order): candidates for treelets
    bool blas_rebuild_ok = true;                             // every mesh's leaves list their triangles in one region of triPrimIdx
    bool blas_refit_ok = true;                               // every TriMesh BLAS can be refitted on the device
    bool refit_ok = true;     // the TLAS can be refitted bottom-up on the device (hrt_bvh.hpp)
    int reach_leaves = 0;     // reachable TLAS leaves
    bool nested = true;       // every reachable TLAS node's box lies inside its parent's, every fast-sphere instance's own box inside its leaf's:
                              // what "the boxes above only accelerate" (TracerFlat, the second tree) needs; the builders guarantee it, an uploaded tree may not
    bool own_in_world = true; // every fast-sphere instance's own box (its one-node BLAS) lies inside its worldBounds: a TLAS refitted or rebuilt on the
                              // device (leaf boxes = unions of worldBounds) is then nested like the builder's; false e.g. for an instance whose BLAS
                              // the position-indexed builder put over another sphere (Scene.cs:386-395)
    bool inst_once = false;   // the reachable TLAS leaves list every instance exactly once (a second tree over "the instances" answers the same queries)
    bool ok = true;           // false -> limits of the packed encoding exceeded (not an error)
    int feat = 0;             // TracerPackedT<FEAT> bits the committed scene needs
};

// nodes[lo,hi): every link in {-1} U [lo,hi) (TLAS: lo = 0), walk graph (left edge of inner nodes, skip edge of
// all nodes) acyclic from `root`.  Returns "" or an error text.
std::string check_nodes(const hrt_bvh_node* nodes, int64_t lo, int64_t hi, int64_t root, int64_t leafLimit, const char* what);

// Validates the scene ("" or an error text: every index a kernel will dereference is in range, the node graphs are acyclic) and
// fills `out`.  Reads the arrays only after their counts passed the 32-bit check; counts >= 0 and non-NULL pointers of
// non-empty arrays are the caller's to check (hrt_scene_upload does).
std::string validate_and_pack(const hrt_scene_desc* s, PackedHost& out);

struct SahTopology { std::vector<int32_t> order; std::vector<NodeQ> nodes; std::vector<int> parent, nchild; int leaves = 0; };
// binned-SAH topology of the second tree over the instances' world bounds, in walk order (hrt_scene_pack.hip)
void host_sah_topology(const std::vector<hrt_instance>& inst, SahTopology& out);
// renumbering of a second tree for rays of one direction class; false: not the binary tree in walk order it should be (hrt_scene_pack.hip)
bool reorder_second_tree(const std::vector<NodeQ>& X, const int sign[3], int base, NodeQ* out, int* from, bool inlined);

}} // namespace hrt::detail
