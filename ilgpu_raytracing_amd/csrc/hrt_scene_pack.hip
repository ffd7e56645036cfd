// hrt_scene_pack.hip -- host half of a scene upload that never touches a device (hrt_scene_pack.hpp): scene validation, the
// walk-order repack with its refit bookkeeping, and the second tree's host topology and renumberings.
// No __global__ function and no hip* call in this unit; hrt_scene.hip does the device work with what is computed here.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include "hrt_scene_pack.hpp"

namespace hrt { namespace detail {


// ---------------------------------------------------------------------------------------
// Scene validation + repack (host, once per commit).
// Validation: every index a kernel will dereference is range-checked and the node graphs are
// checked to be acyclic, so a malformed scene is an HRT_ERR_INVALID_ARG here instead of a GPU
// fault or a walk that never ends.  (The reference trusts its own builder and checks nothing.)
// ---------------------------------------------------------------------------------------
namespace {

inline float bits_f(int v) { float f; std::memcpy(&f, &v, 4); return f; }
inline float4 mkf4(float x, float y, float z, float w) { float4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }

bool is_identity(const hrt_affine3x4& m)
{
    return m.m00 == 1.f && m.m01 == 0.f && m.m02 == 0.f && m.m03 == 0.f && m.m10 == 0.f && m.m11 == 1.f && m.m12 == 0.f && m.m13 == 0.f &&
           m.m20 == 0.f && m.m21 == 0.f && m.m22 == 1.f && m.m23 == 0.f;
}

} // namespace

// nodes[lo,hi): every link in {-1} U [lo,hi) (TLAS: lo = 0), walk graph (left edge of inner nodes, skip edge of
// all nodes) acyclic from `root`.  Returns "" or an error text.
std::string check_nodes(const hrt_bvh_node* nodes, int64_t lo, int64_t hi, int64_t root, int64_t leafLimit, const char* what)
{
    if (hi <= lo) return "";
    for (int64_t i = lo; i < hi; i++)
    {
        const hrt_bvh_node& n = nodes[i];
        if (n.skipIndex < -1 || n.skipIndex >= hi) return std::string(what) + ": skipIndex out of range";   // skip may leave a BLAS range upward? no: reference skips are -1 or inside
        if (n.skipIndex != -1 && n.skipIndex < lo) return std::string(what) + ": skipIndex below its BLAS";
        if (n.count > 0) { if (n.first < 0 || (int64_t)n.first + n.count > leafLimit) return std::string(what) + ": leaf range outside the index list"; }
        else if (n.left < -1 || n.left >= hi || (n.left != -1 && n.left < lo)) return std::string(what) + ": left child out of range";
    }
    // iterative DFS, colours: 0 new, 1 on stack, 2 done
    std::vector<uint8_t> col((size_t)(hi - lo), 0);
    std::vector<std::pair<int64_t, int>> st;
    st.emplace_back(root, 0);
    col[(size_t)(root - lo)] = 1;
    while (!st.empty())
    {
        auto& top = st.back();
        const hrt_bvh_node& n = nodes[top.first];
        int64_t next = -2;
        if (top.second == 0) { top.second = 1; next = n.count > 0 ? -1 : n.left; }
        else if (top.second == 1) { top.second = 2; next = n.skipIndex; }
        else { col[(size_t)(top.first - lo)] = 2; st.pop_back(); continue; }
        if (next < 0) continue;
        uint8_t& c = col[(size_t)(next - lo)];
        if (c == 1) return std::string(what) + ": node links form a cycle";
        if (c == 0) { c = 1; st.emplace_back(next, 0); }
    }
    return "";
}

std::string validate_and_pack(const hrt_scene_desc* s, PackedHost& out)
{
    const int64_t nT = s->n_tlasNodes, nTI = s->n_tlasInstanceIndices, nI = s->n_instances, nB = s->n_blasNodes;
    const int64_t nSP = s->n_spherePrimIdx, nS = s->n_spheres, nTP = s->n_triPrimIdx, nPos = s->n_meshPositions, nTri = s->n_meshTris;
    const int64_t nTC = s->n_meshTexcoords, nTU = s->n_meshTriUVs, nTM = s->n_triMatIndex, nM = s->n_materials, nTx = s->n_texels, nTxI = s->n_texInfos;
    for (int64_t v : {nT, nTI, nI, nB, nSP, nS, nTP, nPos, nTri, nTC, nTU, nTM, nM, nTx, nTxI})
        if (v > 0x7FFFFFF0LL) return "array too long for 32-bit indices";
    for (int64_t i = 0; i < nTI; i++) if (s->tlasInstanceIndices[i] < 0 || s->tlasInstanceIndices[i] >= nI) return "tlasInstanceIndices entry out of range";
    for (int64_t i = 0; i < nSP; i++) if (s->spherePrimIdx[i] < 0 || s->spherePrimIdx[i] >= nS) return "spherePrimIdx entry out of range";
    for (int64_t i = 0; i < nTP; i++) if (s->triPrimIdx[i] < 0 || s->triPrimIdx[i] >= nTri) return "triPrimIdx entry out of range";
    if (nTri > 0 && (nTM < nTri || nTU < nTri)) return "triMatIndex / meshTriUVs shorter than meshTris";
    const int64_t limTC = nTC > 0 ? nTC : 1, limM = nM > 0 ? nM : 1;      // an empty list is one zeroed element (Scene.cs:370-377)
    for (int64_t i = 0; i < nTri; i++)
    {
        const hrt_mesh_tri& t = s->meshTris[i];
        if (t.i0 < 0 || t.i1 < 0 || t.i2 < 0 || t.i0 >= nPos || t.i1 >= nPos || t.i2 >= nPos) return "meshTris vertex index out of range";
        const hrt_mesh_tri_uv& u = s->meshTriUVs[i];
        if (u.t0 < 0 || u.t1 < 0 || u.t2 < 0 || u.t0 >= limTC || u.t1 >= limTC || u.t2 >= limTC) return "meshTriUVs index out of range";
        if (s->triMatIndex[i] < 0 || s->triMatIndex[i] >= limM) return "triMatIndex entry out of range";
    }
    for (int64_t i = 0; i < nTxI; i++)
    {
        const hrt_tex_info& ti = s->texInfos[i];
        if (ti.Width > 0 && ti.Height > 0 && (ti.Offset < 0 || (int64_t)ti.Offset + (int64_t)ti.Width * ti.Height > nTx)) return "texInfos entry outside texels";
    }
    if (nT > 0) { std::string e = check_nodes(s->tlasNodes, 0, nT, 0, nTI, "tlasNodes"); if (!e.empty()) return e; }
    for (int64_t i = 0; i < nI; i++)
    {
        const hrt_instance& in = s->instances[i];
        if (in.blasNodeCount < 0 || in.blasRoot < 0 || (int64_t)in.blasRoot + in.blasNodeCount > nB) return "instance BLAS range outside blasNodes";
        if (in.blasNodeCount == 0) continue;
        std::string e = check_nodes(s->blasNodes, in.blasRoot, (int64_t)in.blasRoot + in.blasNodeCount, in.blasRoot,
                                    in.type == HRT_BLAS_SPHERESET ? nSP : nTP, "blasNodes");
        if (!e.empty()) return e;
    }

    // ---- repack
    // Nodes are renumbered into walk order (depth-first, hit edge before skip edge): the child a ray enters after
    // a hit is the next node in memory, so a descent reads consecutive 32-byte records (4 per 128-byte line)
    // instead of jumping between the two halves of the builder's right-first numbering.  Pure permutation: every
    // walk visits the same nodes in the same order.  perm[old - lo] = new - lo.
    auto walk_order = [&](const hrt_bvh_node* src, int64_t lo, int64_t hi, int64_t root, std::vector<int32_t>& perm) -> int32_t {   // returns the number of reachable nodes
        const size_t n = (size_t)(hi - lo);
        perm.assign(n, -1);
        int32_t next = 0;
        std::vector<int64_t> st;
        st.push_back(root);
        while (!st.empty())
        {
            const int64_t i = st.back(); st.pop_back();
            if (i < lo || i >= hi || perm[(size_t)(i - lo)] >= 0) continue;
            perm[(size_t)(i - lo)] = next++;
            const hrt_bvh_node& b = src[i];
            st.push_back(b.skipIndex);
            if (b.count <= 0) st.push_back(b.left);
        }
        const int32_t reachable = next;
        for (size_t i = 0; i < n; i++) if (perm[i] < 0) perm[i] = next++;        // unreachable nodes keep a slot
        return reachable;
    };
    auto pack_range = [&](const hrt_bvh_node* src, int64_t lo, int64_t hi, const std::vector<int32_t>& perm, std::vector<NodeQ>& dst) {
        auto remap = [&](int32_t link) -> int { return (link < lo || link >= hi) ? kEnd : (int)(lo + perm[(size_t)(link - lo)]); };
        for (int64_t i = lo; i < hi; i++)
        {
            const hrt_bvh_node& b = src[i];
            int cnt = b.count > 0 ? b.count : 0;
            if (cnt > 15) out.ok = false;
            int link = cnt > 0 ? b.first : remap(b.left);
            int hiw = remap(b.skipIndex) | (int)((unsigned)(cnt & 15) << 28);
            NodeQ& q = dst[(size_t)(lo + perm[(size_t)(i - lo)])];
            q.lo = mkf4(b.boundsMin.X, b.boundsMin.Y, b.boundsMin.Z, bits_f(link));
            q.hi = mkf4(b.boundsMax.X, b.boundsMax.Y, b.boundsMax.Z, bits_f(hiw));
        }
    };
    auto alloc_nodes = [&](int64_t n, std::vector<NodeQ>& dst) {
        dst.resize((size_t)std::max<int64_t>(n, 1));
        std::memset(dst.data(), 0, dst.size() * sizeof(NodeQ));
        if (n == 0) { dst[0].lo.w = bits_f(kEnd); dst[0].hi.w = bits_f(kEnd); }    // the 1-element zero buffer: count 0, left 0 -> treat as end
        if (n >= kEnd) out.ok = false;
    };
    std::vector<int32_t> perm;
    alloc_nodes(nT, out.tlas);
    int32_t reachableT = -1;
    if (nT > 0) { reachableT = walk_order(s->tlasNodes, 0, nT, 0, perm); pack_range(s->tlasNodes, 0, nT, perm, out.tlas); }
    {   // parents and child counts for the device refit: the children of an inner node are the chain left, left.skip, ...
        // up to the node's own skip link (two nodes for both builders)
        const size_t n = out.tlas.size();
        out.parent.assign(n, -1); out.nchild.assign(n, 0);
        auto cntq = [&](size_t i) { return (int)((unsigned)__builtin_bit_cast(int, out.tlas[i].hi.w) >> 28); };
        auto skipq = [&](size_t i) { return __builtin_bit_cast(int, out.tlas[i].hi.w) & kEnd; };
        for (size_t i = 0; i < (size_t)nT; i++)
        {
            if (cntq(i) > 0) { if ((int32_t)i < reachableT) out.reach_leaves++; continue; }
            int c = __builtin_bit_cast(int, out.tlas[i].lo.w) & kEnd;
            const int end = skipq(i);
            int steps = 0;
            while (c != kEnd && c != end)
            {
                if (c == 0 || out.parent[(size_t)c] != -1 || ++steps > 64) { out.refit_ok = false; break; }
                out.parent[(size_t)c] = (int32_t)i; out.nchild[i]++;
                c = skipq((size_t)c);
            }
        }
        if (nT == 0) out.refit_ok = false;
        // does the walk meet every instance exactly once?
        std::vector<uint8_t> seen((size_t)std::max<int64_t>(nI, 1), 0);
        bool once = nT > 0 && out.refit_ok;
        for (size_t i = 0; once && i < (size_t)nT; i++)
        {
            if (cntq(i) == 0 || (int32_t)i >= reachableT) continue;
            const int first = __builtin_bit_cast(int, out.tlas[i].lo.w);
            for (int j = 0; j < cntq(i); j++)
            {
                const int64_t slot = (int64_t)first + j;
                if (slot < 0 || slot >= nTI) { once = false; break; }
                const int64_t ii = s->tlasInstanceIndices[slot];
                if (ii < 0 || ii >= nI || seen[(size_t)ii]++) { once = false; break; }
            }
        }
        for (int64_t ii = 0; once && ii < nI; ii++) if (!seen[(size_t)ii]) once = false;
        out.inst_once = once;
        auto inside = [](const NodeQ& c, const NodeQ& p) {
            // false with a NaN.  The child has to be a regular box (min <= max) too: the slab test reads an inverted box as its
            // mirror image, which these comparisons say nothing about
            return c.lo.x <= c.hi.x && c.lo.y <= c.hi.y && c.lo.z <= c.hi.z &&
                   c.lo.x >= p.lo.x && c.lo.y >= p.lo.y && c.lo.z >= p.lo.z && c.hi.x <= p.hi.x && c.hi.y <= p.hi.y && c.hi.z <= p.hi.z;
        };
        for (size_t i = 1; i < (size_t)nT; i++)
            if ((int32_t)i < reachableT && out.parent[i] >= 0 && !inside(out.tlas[i], out.tlas[(size_t)out.parent[i]])) out.nested = false;
    }
    alloc_nodes(nB, out.blas);
    {
        // every instance owns the node range [blasRoot, blasRoot + blasNodeCount); each distinct range is renumbered
        // on its own (root stays first).  Ranges that overlap without being equal cannot all be in walk order:
        // the whole array then keeps the builder's numbering.
        std::vector<std::pair<int64_t, int64_t>> ranges;
        for (int64_t i = 0; i < nI; i++)
            if (s->instances[i].blasNodeCount > 0) ranges.emplace_back((int64_t)s->instances[i].blasRoot, (int64_t)s->instances[i].blasRoot + s->instances[i].blasNodeCount);
        std::sort(ranges.begin(), ranges.end());
        ranges.erase(std::unique(ranges.begin(), ranges.end()), ranges.end());
        bool disjoint = true;
        for (size_t i = 1; i < ranges.size(); i++) if (ranges[i].first < ranges[i - 1].second) disjoint = false;
        const size_t nBq = out.blas.size();
        out.bparent.assign(nBq, -2); out.bnchild.assign(nBq, 0); out.bsubend.assign(nBq, 0); out.borig.assign(nBq, 0); out.bkind.assign(nBq, 0);
        for (size_t j = 0; j < nBq; j++) out.borig[j] = (int32_t)j;
        if (!disjoint)
        {
            perm.resize((size_t)nB);
            for (size_t j = 0; j < perm.size(); j++) perm[j] = (int32_t)j;
            pack_range(s->blasNodes, 0, nB, perm, out.blas);
            out.blas_refit_ok = false;
        }
        else
        {
            // who owns each range: bit 0 a triangle mesh, bit 1 anything else
            std::vector<uint8_t> rangeKind(ranges.size(), 0);
            for (int64_t i = 0; i < nI; i++)
            {
                const hrt_instance& in = s->instances[i];
                if (in.blasNodeCount <= 0) continue;
                const auto it = std::lower_bound(ranges.begin(), ranges.end(), std::make_pair((int64_t)in.blasRoot, (int64_t)in.blasRoot + in.blasNodeCount));
                rangeKind[(size_t)(it - ranges.begin())] |= in.type == HRT_BLAS_TRIMESH ? 1 : (in.type == HRT_BLAS_SPHERESET ? 2 : 4);
            }
            int64_t at = 0;
            for (const auto& r : ranges)
            {
                for (; at < r.first; at++) { perm.assign(1, 0); pack_range(s->blasNodes, at, at + 1, perm, out.blas); }   // owned by no instance: never walked
                const int32_t reach = walk_order(s->blasNodes, r.first, r.second, r.first, perm);
                pack_range(s->blasNodes, r.first, r.second, perm, out.blas);
                at = r.second;
                // maintenance arrays for the BLAS of a triangle mesh (device refit after a vertex update, hrt_bvh.hpp)
                const uint8_t kind = rangeKind[(size_t)(&r - ranges.data())];
                if (kind != 1 && kind != 2) { if (kind != 0) out.blas_refit_ok = false; continue; }               // shared between a mesh and a sphere set, or of an unknown type
                if (reach != (int32_t)(r.second - r.first)) { out.blas_refit_ok = false; continue; }              // unreachable nodes
                for (int64_t k = r.first; k < r.second; k++) out.bkind[(size_t)k] = kind;
                if (kind == 1) out.meshRanges.push_back(r);
                out.max_range[kind] = std::max(out.max_range[kind], (int)(r.second - r.first));
                auto cntq = [&](int64_t i) { return (int)((unsigned)__builtin_bit_cast(int, out.blas[(size_t)i].hi.w) >> 28); };
                auto skipq = [&](int64_t i) { return __builtin_bit_cast(int, out.blas[(size_t)i].hi.w) & kEnd; };
                for (int64_t k = r.first; k < r.second; k++) out.borig[(size_t)(r.first + perm[(size_t)(k - r.first)])] = (int32_t)k;
                out.bparent[(size_t)r.first] = -1;
                for (int64_t i = r.first; i < r.second; i++)
                {
                    const int sk = skipq(i);
                    out.bsubend[(size_t)i] = (int32_t)(sk == kEnd ? r.second : sk);
                    if (cntq(i) > 0) continue;
                    int c = __builtin_bit_cast(int, out.blas[(size_t)i].lo.w) & kEnd;
                    int steps = 0;
                    while (c != kEnd && c != sk)
                    {
                        if (c <= i || c >= r.second || out.bparent[(size_t)c] != -2 || ++steps > 64) { out.blas_refit_ok = false; break; }
                        out.bparent[(size_t)c] = (int32_t)i; out.bnchild[(size_t)i]++;
                        c = skipq(c);
                    }
                }
            }
            for (; at < nB; at++) { perm.assign(1, 0); pack_range(s->blasNodes, at, at + 1, perm, out.blas); }
        }
        for (int64_t i = 0; i < nI; i++)
        {
            const hrt_instance& in = s->instances[i];
            if (in.type == HRT_BLAS_SPHERESET && in.blasNodeCount > 0) out.sphereInst.push_back((int32_t)i);
            if (in.type != HRT_BLAS_TRIMESH || in.blasNodeCount <= 0) continue;
            out.meshInst.push_back((int32_t)i);
            // region of triPrimIdx the leaves of this BLAS point into (the builder appends it behind the item list, Scene.cs:439-440)
            int64_t lo = INT64_MAX, hi = -1, sum = 0;
            for (int64_t k = in.blasRoot; k < (int64_t)in.blasRoot + in.blasNodeCount; k++)
            {
                const hrt_bvh_node& b = s->blasNodes[k];
                if (b.count <= 0) continue;
                lo = std::min<int64_t>(lo, b.first); hi = std::max<int64_t>(hi, (int64_t)b.first + b.count); sum += b.count;
            }
            const int64_t n = in.primIndexCount;
            MeshJob J; J.inst = (int)i; J.root = in.blasRoot; J.nodeCap = in.blasNodeCount; J.leafBase = (int)lo; J.n = (int)n; J.itemFirst = in.primIndexFirst;
            const bool items_ok = n > 0 && in.primIndexFirst >= 0 && (int64_t)in.primIndexFirst + n <= nTP;
            const bool region_ok = hi - lo == n && sum == n && (lo >= (int64_t)in.primIndexFirst + n || hi <= in.primIndexFirst);
            if (!items_ok || !region_ok || 2 * ((n + 13) / 14) - 1 > in.blasNodeCount) out.blas_rebuild_ok = false;
            out.meshJobs.push_back(J);
        }
        {   // two meshes must not share a node range or a leaf region
            std::vector<std::pair<int, int>> byRoot, byLeaf;
            for (const MeshJob& J : out.meshJobs) { byRoot.emplace_back(J.root, J.nodeCap); byLeaf.emplace_back(J.leafBase, J.n); }
            std::sort(byRoot.begin(), byRoot.end()); std::sort(byLeaf.begin(), byLeaf.end());
            for (size_t k = 1; k < byRoot.size(); k++)
                if (byRoot[k].first < byRoot[k - 1].first + byRoot[k - 1].second || byLeaf[k].first < byLeaf[k - 1].first + byLeaf[k - 1].second) out.blas_rebuild_ok = false;
        }
    }
    if (nT == 0)
    {   // reference semantics of the zeroed 1-element TLAS: node 0 has count 0, left 0 -> loops forever on a hit;
        // its bounds are all zero so only rays through the origin would.  We end the walk instead.
    }
    out.finst.resize((size_t)std::max<int64_t>(nTI, 1));
    std::memset(out.finst.data(), 0, out.finst.size() * sizeof(FInst));
    for (int64_t i = 0; i < nTI; i++)
    {
        int ii = s->tlasInstanceIndices[i];
        const hrt_instance& in = s->instances[ii];
        const bool ident = is_identity(in.objectToWorld) && is_identity(in.worldToObject) && in.uniformScale == 1.0f;
        const bool sph = in.type == HRT_BLAS_SPHERESET;
        FInst f;
        bool fast = false;
        if (sph && ident && in.blasNodeCount >= 1)
        {
            const hrt_bvh_node& root = s->blasNodes[in.blasRoot];
            int64_t end = (int64_t)in.blasRoot + in.blasNodeCount;
            if (root.count == 1 && (root.skipIndex == -1 || root.skipIndex >= end))
            {
                int sid = s->spherePrimIdx[root.first];
                const hrt_sphere& sp = s->spheres[sid];
                f.a = mkf4(root.boundsMin.X, root.boundsMin.Y, root.boundsMin.Z, bits_f(FI_FAST_SPHERE | FI_IDENTITY | FI_SPHERESET));
                f.b = mkf4(root.boundsMax.X, root.boundsMax.Y, root.boundsMax.Z, bits_f(sid));
                f.c = mkf4(sp.center.X, sp.center.Y, sp.center.Z, sp.radius);
                fast = true;
            }
        }
        if (!fast)
        {
            out.feat |= 1;
            float scale = in.uniformScale > 0.f ? in.uniformScale : 1.f;
            f.a = mkf4(0.f, 0.f, 0.f, bits_f((ident ? FI_IDENTITY : 0) | (sph ? FI_SPHERESET : 0)));
            f.b = mkf4(0.f, 0.f, 0.f, bits_f(ii));
            f.c = mkf4(bits_f(in.blasRoot), bits_f(in.blasRoot + in.blasNodeCount), scale, 0.f);
        }
        out.finst[(size_t)i] = f;
        // BOTH corners of the own box: a negative radius inverts it (max < min), and the slab test reads that as the mirror image
        auto within = [](float v, float lo, float hi) { return v >= lo && v <= hi; };      // false with a NaN
        if (fast && !(within(f.a.x, in.worldBoundsMin.X, in.worldBoundsMax.X) && within(f.b.x, in.worldBoundsMin.X, in.worldBoundsMax.X) &&
                      within(f.a.y, in.worldBoundsMin.Y, in.worldBoundsMax.Y) && within(f.b.y, in.worldBoundsMin.Y, in.worldBoundsMax.Y) &&
                      within(f.a.z, in.worldBoundsMin.Z, in.worldBoundsMax.Z) && within(f.b.z, in.worldBoundsMin.Z, in.worldBoundsMax.Z))) out.own_in_world = false;
    }
    out.ftri.resize((size_t)std::max<int64_t>(nTP, 1));
    std::memset(out.ftri.data(), 0, out.ftri.size() * sizeof(FTri));
    const int64_t texLen = nTxI > 0 ? nTxI : 1;
    for (int64_t j = 0; j < nTP; j++)
    {
        int ti = s->triPrimIdx[j];
        const hrt_mesh_tri& t = s->meshTris[ti];
        const hrt_float3 &a = s->meshPositions[t.i0], &b = s->meshPositions[t.i1], &c = s->meshPositions[t.i2];
        int mi = s->triMatIndex[ti];
        static const hrt_material kZeroMaterial = {};
        const hrt_material& m = nM > 0 ? s->materials[mi] : kZeroMaterial;
        bool dmap = m.HasDiffuseMap != 0 && m.DiffuseTexIndex >= 0 && m.DiffuseTexIndex < texLen;
        bool amap = m.HasAlphaMap != 0 && m.AlphaTexIndex >= 0 && m.AlphaTexIndex < texLen;
        bool rejects_opaque = 1.0f < m.AlphaCutoff;
        int fl = ((dmap || amap || rejects_opaque) ? FT_TEXTURED : 0) | (m.TwoSided != 0 ? FT_TWOSIDED : 0);
        if (amap || rejects_opaque) out.feat |= 2;          // the walk itself must evaluate alpha (diffuse-only maps are resolved after it)
        FTri& o = out.ftri[(size_t)j];
        o.v0 = mkf4(a.X, a.Y, a.Z, bits_f(ti));
        o.v1 = mkf4(b.X, b.Y, b.Z, bits_f(mi));
        o.v2 = mkf4(c.X, c.Y, c.Z, bits_f(fl));
    }
    // ---- sphere-instance scenes: instance records inlined into the TLAS node stream (hrt_walker.hpp).  A leaf is followed by
    // one record per instance holding the box of its one-node BLAS; the walker treats them as nodes (count field 15), so the
    // instance box tests ride the node steps and their lookahead instead of costing a leaf step each.
    out.tlasX.assign(1, NodeQ{});
    bool leavesFit = true;                   // count code 15 marks an instance record in this stream: a leaf of 15 instances cannot be told from one
    for (int64_t i = 0; i < nT; i++) if (((unsigned)__builtin_bit_cast(int, out.tlas[(size_t)i].hi.w) >> 28) > 14u) leavesFit = false;
    if (out.ok && out.feat == 0 && reachableT > 0 && nT + nTI < kEnd && leavesFit)
    {
        std::vector<int32_t> nidx((size_t)nT);
        int32_t at = 0;
        auto cnt_of = [&](int64_t i) { return (int)((unsigned)__builtin_bit_cast(int, out.tlas[(size_t)i].hi.w) >> 28); };
        for (int64_t i = 0; i < nT; i++) { nidx[(size_t)i] = at; at += 1 + cnt_of(i); }
        auto remap = [&](int v) { return v == kEnd ? kEnd : (int)nidx[(size_t)v]; };
        out.tlasX.assign((size_t)at, NodeQ{});
        for (int64_t i = 0; i < nT; i++)
        {
            const NodeQ& q = out.tlas[(size_t)i];
            const int c = cnt_of(i), link = __builtin_bit_cast(int, q.lo.w), sk = remap(__builtin_bit_cast(int, q.hi.w) & kEnd);
            NodeQ& o = out.tlasX[(size_t)nidx[(size_t)i]];
            o = q;
            o.hi.w = bits_f(sk | (int)((unsigned)c << 28));
            if (c == 0) { o.lo.w = bits_f(remap(link & kEnd)); continue; }
            for (int j = 0; j < c; j++)
            {
                const FInst& f = out.finst[(size_t)(link + j)];
                NodeQ& r = out.tlasX[(size_t)(nidx[(size_t)i] + 1 + j)];
                r.lo = mkf4(f.a.x, f.a.y, f.a.z, bits_f(link + j));
                const int next = (j + 1 < c) ? nidx[(size_t)i] + 2 + j : sk;
                r.hi = mkf4(f.b.x, f.b.y, f.b.z, bits_f(next | (int)(15u << 28)));
            }
        }
        out.n_tlasX = at;
    }

    // fast-sphere instances: own box inside the box of the leaf that lists them
    for (int64_t i = 0; out.nested && i < nT; i++)
    {
        const NodeQ& q = out.tlas[(size_t)i];
        const int cnt = (int)((unsigned)__builtin_bit_cast(int, q.hi.w) >> 28), first = __builtin_bit_cast(int, q.lo.w);
        if (cnt == 0 || (int32_t)i >= reachableT) continue;
        for (int j = 0; j < cnt; j++)
        {
            if ((int64_t)first + j < 0 || (int64_t)first + j >= nTI) { out.nested = false; break; }
            const FInst& f = out.finst[(size_t)(first + j)];
            if (!(__builtin_bit_cast(int, f.a.w) & FI_FAST_SPHERE)) continue;
            // both corners of the own box (a negative radius inverts it, and the slab test reads that as the mirror image)
            auto within = [](float v, float lo, float hi) { return v >= lo && v <= hi; };
            if (!(within(f.a.x, q.lo.x, q.hi.x) && within(f.b.x, q.lo.x, q.hi.x) && within(f.a.y, q.lo.y, q.hi.y) && within(f.b.y, q.lo.y, q.hi.y) &&
                  within(f.a.z, q.lo.z, q.hi.z) && within(f.b.z, q.lo.z, q.hi.z))) { out.nested = false; break; }
        }
    }
    if (!out.nested) out.inst_once = false;
    // TracerFlat: the reachable TLAS leaves in walk order, for scenes made of fast-sphere instances only
    out.flat.assign(1, NodeQ{});
    if (out.ok && out.feat == 0 && reachableT > 0 && out.nested)
    {
        std::vector<NodeQ> leaves;
        for (int32_t i = 0; i < reachableT; i++)
            if (((unsigned)__builtin_bit_cast(int, out.tlas[(size_t)i].hi.w) >> 28) != 0) leaves.push_back(out.tlas[(size_t)i]);
        if (!leaves.empty() && (int)leaves.size() <= kFlatMaxLeaves) out.flat = leaves;
        else out.flat.clear(), out.flat.assign(1, NodeQ{});
        out.n_flat = (!leaves.empty() && (int)leaves.size() <= kFlatMaxLeaves) ? (int)leaves.size() : 0;
    }
    return "";
}

// Topology of the second tree built on the HOST with a binned surface-area heuristic (16 bins on each axis over the box centres of
// the range, the split of least area(left) * n(left) + area(right) * n(right); leaves of at most four instances; a range the bins cannot
// split is halved), in the numbering the walkers want (walk order: a node's first child follows it).
// Only WHICH instances share a subtree is decided here -- boxes, leaf-slot records, the inlined layout and the slack are the
// device's (tlas_finish, tlas_inflate), exactly as for the LBVH the scene updates build.  Against that LBVH: 6-10 % fewer node
// visits per ray on config 3 (tools/tree_order_model.py); the scene updates keep the LBVH, which is built in 0.3 ms, and so do
// scenes of more than two million instances.
constexpr int kSahLeaf = 4;       // instances per leaf at most (config 3, path stage + launch 1: 15.66 / 15.37 / 15.39 / 15.41 ms for 2 / 3 / 4 / 6)
void host_sah_topology(const std::vector<hrt_instance>& inst, SahTopology& out)
{
    const int n = (int)inst.size();
    constexpr int kBins = 16;
    std::vector<float> cx((size_t)n), cy((size_t)n), cz((size_t)n);
    for (int i = 0; i < n; i++)
    {
        cx[(size_t)i] = 0.5f * (inst[(size_t)i].worldBoundsMin.X + inst[(size_t)i].worldBoundsMax.X);
        cy[(size_t)i] = 0.5f * (inst[(size_t)i].worldBoundsMin.Y + inst[(size_t)i].worldBoundsMax.Y);
        cz[(size_t)i] = 0.5f * (inst[(size_t)i].worldBoundsMin.Z + inst[(size_t)i].worldBoundsMax.Z);
        // (an infinite box is legal here; its centre only has to be a number the binning can convert to an integer)
        if (!std::isfinite(cx[(size_t)i])) cx[(size_t)i] = 0.f;
        if (!std::isfinite(cy[(size_t)i])) cy[(size_t)i] = 0.f;
        if (!std::isfinite(cz[(size_t)i])) cz[(size_t)i] = 0.f;
    }
    const float* cen[3] = {cx.data(), cy.data(), cz.data()};
    struct Box { float lo[3], hi[3]; };
    auto grow = [&](Box& b, int i) {
        const hrt_instance& r = inst[(size_t)i];
        const float l[3] = {r.worldBoundsMin.X, r.worldBoundsMin.Y, r.worldBoundsMin.Z}, h[3] = {r.worldBoundsMax.X, r.worldBoundsMax.Y, r.worldBoundsMax.Z};
        for (int a = 0; a < 3; a++) { b.lo[a] = std::min(b.lo[a], l[a]); b.hi[a] = std::max(b.hi[a], h[a]); }
    };
    auto unite = [](Box& b, const Box& o) { for (int a = 0; a < 3; a++) { b.lo[a] = std::min(b.lo[a], o.lo[a]); b.hi[a] = std::max(b.hi[a], o.hi[a]); } };
    auto area = [](const Box& b) { const float x = b.hi[0] - b.lo[0], y = b.hi[1] - b.lo[1], z = b.hi[2] - b.lo[2]; return x * y + y * z + z * x; };
    const Box empty = {{FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}};
    out.order.resize((size_t)n);
    for (int i = 0; i < n; i++) out.order[(size_t)i] = i;
    out.nodes.clear(); out.parent.clear(); out.nchild.clear(); out.leaves = 0;
    struct Job { int a, b, parent; };
    std::vector<Job> todo;
    todo.push_back({0, n, -1});
    while (!todo.empty())
    {
        const Job j = todo.back();
        todo.pop_back();
        const int idx = (int)out.nodes.size();
        NodeQ q{};
        out.parent.push_back(j.parent);
        const int m = j.b - j.a;
        if (m <= kSahLeaf)
        {
            q.lo.w = bits_f(j.a);
            q.hi.w = bits_f((int)((unsigned)m << 28));           // the skip link comes with the subtree sizes, below
            out.nodes.push_back(q); out.nchild.push_back(0); out.leaves++;
            continue;
        }
        int32_t* it = out.order.data() + j.a;
        int bestAxis = -1, bestK = 0; float bestCost = 0.f, bestLo = 0.f, bestScale = 0.f;
        for (int a = 0; a < 3; a++)
        {
            float lo = FLT_MAX, hi = -FLT_MAX;
            for (int i = 0; i < m; i++) { lo = std::min(lo, cen[a][it[i]]); hi = std::max(hi, cen[a][it[i]]); }
            if (!(hi > lo) || !std::isfinite(hi - lo)) continue;
            const float scale = (float)kBins / (hi - lo);
            Box bb[kBins]; int cnt[kBins];
            for (int k = 0; k < kBins; k++) { bb[k] = empty; cnt[k] = 0; }
            for (int i = 0; i < m; i++)
            {
                const int k = std::min(kBins - 1, std::max(0, (int)((cen[a][it[i]] - lo) * scale)));
                grow(bb[k], it[i]); cnt[k]++;
            }
            Box right[kBins]; int rcnt[kBins];
            Box acc = empty; int c = 0;
            for (int k = kBins - 1; k >= 1; k--) { unite(acc, bb[k]); c += cnt[k]; right[k] = acc; rcnt[k] = c; }
            acc = empty; c = 0;
            for (int k = 1; k < kBins; k++)
            {
                unite(acc, bb[k - 1]); c += cnt[k - 1];
                if (c == 0 || rcnt[k] == 0) continue;
                const float cost = area(acc) * (float)c + area(right[k]) * (float)rcnt[k];
                if (std::isfinite(cost) && (bestAxis < 0 || cost < bestCost)) { bestAxis = a; bestK = k; bestCost = cost; bestLo = lo; bestScale = scale; }
            }
        }
        int mid = m / 2;
        if (bestAxis >= 0)
        {
            const float* ca = cen[bestAxis];
            int32_t* p2 = std::partition(it, it + m, [&](int32_t i) { return std::min(kBins - 1, std::max(0, (int)((ca[i] - bestLo) * bestScale))) < bestK; });
            const int left = (int)(p2 - it);
            if (left > 0 && left < m) mid = left;
        }
        q.lo.w = bits_f(idx + 1);
        out.nodes.push_back(q); out.nchild.push_back(2);
        todo.push_back({j.a + mid, j.b, idx});       // popped second: the first child is the next node
        todo.push_back({j.a, j.a + mid, idx});
    }
    // skip link = index + size of the subtree (walk order: children have larger indices than their parent)
    const int nT = (int)out.nodes.size();
    std::vector<int> size((size_t)nT, 1);
    for (int i = nT - 1; i > 0; i--) size[(size_t)out.parent[(size_t)i]] += size[(size_t)i];
    for (int i = 0; i < nT; i++)
    {
        const int end = i + size[(size_t)i];
        const int w = __builtin_bit_cast(int, out.nodes[(size_t)i].hi.w);
        out.nodes[(size_t)i].hi.w = bits_f((w & ~kEnd) | (end >= nT ? kEnd : end));
    }
}

// The inlined second tree (TlasDevice::tlasX: nodes in walk order, every leaf followed by one record per instance) renumbered for the
// rays whose direction has the signs `sign` (+1 / -1 per axis, 0: not known): at every inner node the child whose box centre comes first along such a ray,
// on the axis that separates the two centres most, is walked first.  Same records, same subtree sizes; only the order of the two
// subtrees under a node, and with it every link, changes.  Links are written as indices into the array of all eight copies
// (`base` = where this copy starts); from[i] = the record of X that position i of the copy holds (a refit refreshes the boxes through it).
// false: the array is not the binary tree in walk order it should be (nothing is used then).
bool reorder_second_tree(const std::vector<NodeQ>& X, const int sign[3], int base, NodeQ* out, int* from, bool inlined)
{
    const int nX = (int)X.size();
    auto w_ = [](float f) { return __builtin_bit_cast(int, f); };
    auto f_ = [](int v) { return __builtin_bit_cast(float, v); };
    auto cnt = [&](int i) { return (int)((unsigned)w_(X[(size_t)i].hi.w) >> 28); };
    auto end = [&](int i) { const int sk = w_(X[(size_t)i].hi.w) & kEnd; return sk == kEnd ? nX : sk; };
    std::vector<std::pair<int, int>> todo;                  // (record in X, its index in this numbering)
    todo.emplace_back(0, 0);
    int placed = 0;
    while (!todo.empty())
    {
        const int src = todo.back().first, at = todo.back().second;
        todo.pop_back();
        if (src < 0 || src >= nX || at < 0 || at >= nX) return false;
        const int size = end(src) - src;
        if (size < 1 || at + size > nX) return false;
        const int skip = at + size == nX ? kEnd : base + at + size;
        const int c = cnt(src);
        NodeQ q = X[(size_t)src];
        if (c == 15) return false;                          // an instance record where a node should be
        if (c > 0)
        {
            if (size != (inlined ? 1 + c : 1)) return false;
            q.hi.w = f_(skip | (int)((unsigned)c << 28));
            out[at] = q; from[at] = src;
            placed += size;
            if (!inlined) continue;                         // the plain node array: a leaf names its slots, no records follow
            for (int j = 0; j < c; j++)
            {
                NodeQ r = X[(size_t)(src + 1 + j)];
                if (cnt(src + 1 + j) != 15) return false;
                r.hi.w = f_((j + 1 < c ? base + at + 2 + j : skip) | (int)(15u << 28));
                out[at + 1 + j] = r; from[at + 1 + j] = src + 1 + j;
            }
            continue;
        }
        const int l = w_(q.lo.w) & kEnd;
        if (l != src + 1 || l >= nX) return false;
        const int r = end(l);
        if (r >= nX || end(r) != end(src)) return false;    // exactly two children
        const NodeQ &L = X[(size_t)l], &R = X[(size_t)r];
        const float cl[3] = {0.5f * (L.lo.x + L.hi.x), 0.5f * (L.lo.y + L.hi.y), 0.5f * (L.lo.z + L.hi.z)};
        const float cr[3] = {0.5f * (R.lo.x + R.hi.x), 0.5f * (R.lo.y + R.hi.y), 0.5f * (R.lo.z + R.hi.z)};
        int ax = 0;
        for (int a = 1; a < 3; a++) if (std::fabs(cl[a] - cr[a]) > std::fabs(cl[ax] - cr[ax])) ax = a;
        // +1 / -1: the rays of this copy go that way along ax; 0: either way -- the builder's order stays (lower Morton code first)
        const bool leftFirst = sign[ax] > 0 ? cl[ax] <= cr[ax] : (sign[ax] < 0 ? cl[ax] >= cr[ax] : true);
        const int a = leftFirst ? l : r, b = leftFirst ? r : l;
        q.lo.w = f_(base + at + 1);
        q.hi.w = f_(skip);
        out[at] = q; from[at] = src;
        placed += 1;
        todo.emplace_back(b, at + 1 + (end(a) - a));
        todo.emplace_back(a, at + 1);
    }
    return placed == nX;
}

}} // namespace hrt::detail
