// hrt_scene_pack_check.cpp -- stand-alone check of the host-only scene code (hrt_scene_pack.hip, hrt_treelets.hpp) for a build
// with AddressSanitizer and UndefinedBehaviorSanitizer: `make hostcheck`.  Its own main, no GPU, no Python, no test framework.
//
// Feeds validate_and_pack, host_sah_topology, reorder_second_tree and build_treelets
//   * a small valid scene (two one-sphere instances and one textured mesh of 8 triangles; the scene of tests/scene_mutations.py),
//   * a scene of 300 one-sphere instances (what the second tree is built for),
//   * one minimal mutation of the small scene per rejection path of the validator (the 15 messages; 1-5 for tlasNodes and blasNodes),
// and expects the verdicts the test suite expects: accepted, or rejected with that path's text.  Exit status 0: every verdict as
// expected and no sanitizer report (the build makes undefined behaviour fatal).
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "hrt_scene_pack.hpp"
#include "hrt_treelets.hpp"
#include "../../include/hrt_host.h"

using namespace hrt;
using namespace hrt::detail;

namespace {

// the 15 arrays of a scene, owned: what a mutation edits
struct SceneCopy {
    std::vector<hrt_bvh_node> tlasNodes, blasNodes;
    std::vector<int32_t> tlasInstanceIndices, spherePrimIdx, triPrimIdx, triMatIndex;
    std::vector<hrt_instance> instances;
    std::vector<hrt_sphere> spheres;
    std::vector<hrt_float3> meshPositions;
    std::vector<hrt_mesh_tri> meshTris;
    std::vector<hrt_float2> meshTexcoords;
    std::vector<hrt_mesh_tri_uv> meshTriUVs;
    std::vector<hrt_material> materials;
    std::vector<hrt_rgba32> texels;
    std::vector<hrt_tex_info> texInfos;

    explicit SceneCopy(const hrt_scene_desc& d)
    {
#define HRT_TAKE(f) if (d.n_##f > 0) f.assign(d.f, d.f + d.n_##f)
        HRT_TAKE(tlasNodes); HRT_TAKE(tlasInstanceIndices); HRT_TAKE(instances); HRT_TAKE(blasNodes); HRT_TAKE(spherePrimIdx);
        HRT_TAKE(spheres); HRT_TAKE(triPrimIdx); HRT_TAKE(meshPositions); HRT_TAKE(meshTris); HRT_TAKE(meshTexcoords);
        HRT_TAKE(meshTriUVs); HRT_TAKE(triMatIndex); HRT_TAKE(materials); HRT_TAKE(texels); HRT_TAKE(texInfos);
#undef HRT_TAKE
    }
    hrt_scene_desc desc() const
    {
        hrt_scene_desc d;
        std::memset(&d, 0, sizeof(d));
#define HRT_GIVE(f) d.f = f.empty() ? nullptr : f.data(); d.n_##f = (int64_t)f.size()
        HRT_GIVE(tlasNodes); HRT_GIVE(tlasInstanceIndices); HRT_GIVE(instances); HRT_GIVE(blasNodes); HRT_GIVE(spherePrimIdx);
        HRT_GIVE(spheres); HRT_GIVE(triPrimIdx); HRT_GIVE(meshPositions); HRT_GIVE(meshTris); HRT_GIVE(meshTexcoords);
        HRT_GIVE(meshTriUVs); HRT_GIVE(triMatIndex); HRT_GIVE(materials); HRT_GIVE(texels); HRT_GIVE(texInfos);
#undef HRT_GIVE
        return d;
    }
};

hrt_affine3x4 identity()
{
    hrt_affine3x4 m;
    std::memset(&m, 0, sizeof(m));
    m.m00 = m.m11 = m.m22 = 1.f;
    return m;
}

hrt_sphere make_sphere(float x, float y, float z, float r)
{
    hrt_sphere s;
    std::memset(&s, 0, sizeof(s));
    s.center.X = x; s.center.Y = y; s.center.Z = z; s.radius = r;
    s.albedo.X = s.albedo.Y = s.albedo.Z = 0.7f;
    s.material.Kd = s.albedo; s.material.DiffuseTexIndex = -1; s.material.AlphaTexIndex = -1; s.material.AlphaCutoff = 0.5f; s.material.IOR = 1.f;
    s.ior = 1.f;
    return s;
}

int add_sphere_instance(void* scene, float x, float y, float z, float r)
{
    const hrt_sphere s = make_sphere(x, y, z, r);
    const int id = hrth_scene_add_sphere(scene, &s);
    const hrt_affine3x4 m = identity();
    return hrth_scene_build_sphere_instance(scene, &id, 1, &m);
}

// two one-sphere instances and a 2 x 2 grid of quads (8 triangles) with one 4 x 4 diffuse texture
SceneCopy small_scene()
{
    void* sc = hrth_scene_new();
    add_sphere_instance(sc, -1.f, 0.5f, 0.f, 0.5f);
    add_sphere_instance(sc, 1.f, 0.5f, 0.f, 0.5f);
    std::vector<hrt_float3> pos; std::vector<hrt_float2> uv; std::vector<hrt_mesh_tri> tris; std::vector<hrt_mesh_tri_uv> tuv;
    for (int j = 0; j < 3; j++)
        for (int i = 0; i < 3; i++)
        {
            hrt_float3 p; p.X = -1.f + (float)i; p.Y = 0.5f + 0.5f * (float)j; p.Z = -1.f; pos.push_back(p);
            hrt_float2 t; t.X = 0.5f * (float)i; t.Y = 0.5f * (float)j; uv.push_back(t);
        }
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < 2; i++)
        {
            const int a = j * 3 + i, b = a + 1, c = a + 3, d = c + 1;
            hrt_mesh_tri t0 = {a, c, b}, t1 = {b, c, d};
            tris.push_back(t0); tris.push_back(t1);
            hrt_mesh_tri_uv u0 = {a, c, b}, u1 = {b, c, d};
            tuv.push_back(u0); tuv.push_back(u1);
        }
    hrt_material m;
    std::memset(&m, 0, sizeof(m));
    m.Kd.X = m.Kd.Y = m.Kd.Z = 0.9f; m.HasDiffuseMap = 1; m.DiffuseTexIndex = 0; m.AlphaTexIndex = -1; m.AlphaCutoff = 0.5f; m.IOR = 1.f;
    const int tw = 4, th = 4;
    std::vector<uint8_t> bgra((size_t)tw * th * 4, 255);
    const hrt_affine3x4 xf = identity();
    hrth_scene_load_mesh_instance(sc, pos.data(), (int)pos.size(), tris.data(), (int)tris.size(), uv.data(), (int)uv.size(), tuv.data(),
                                  nullptr, 0, &m, 1, &tw, &th, bgra.data(), 1, &xf);
    hrth_scene_rebuild_tlas(sc);
    hrt_scene_desc d;
    hrth_scene_get_desc(sc, &d);
    SceneCopy out(d);
    hrth_scene_free(sc);
    return out;
}

// a ground sphere and 299 small ones on a jittered grid, one instance each
SceneCopy many_spheres_scene()
{
    void* sc = hrth_scene_new();
    add_sphere_instance(sc, 0.f, -500.f, 0.f, 500.f);
    unsigned x = 0x5EEDu;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return (float)(x & 0xFFFFu) * (1.f / 65536.f); };
    for (int i = 0; i < 299; i++)
        add_sphere_instance(sc, -5.f + 0.6f * (float)(i % 17) + 0.3f * rnd(), 0.2f + 0.1f * rnd(), -5.f + 0.6f * (float)(i / 17) + 0.3f * rnd(), 0.1f + 0.1f * rnd());
    hrth_scene_rebuild_tlas(sc);
    hrt_scene_desc d;
    hrth_scene_get_desc(sc, &d);
    SceneCopy out(d);
    hrth_scene_free(sc);
    return out;
}

int g_failed = 0;

void expect(bool ok, const char* name, const std::string& detail)
{
    std::printf("%-4s %-32s %s\n", ok ? "ok" : "FAIL", name, detail.c_str());
    if (!ok) g_failed++;
}

// everything the upload computes on the host for an accepted scene
void run_host_pipeline(const char* name, const hrt_scene_desc& d, const PackedHost& ph)
{
    char what[160];
    if (d.n_instances > 2)
    {
        const std::vector<hrt_instance> inst(d.instances, d.instances + d.n_instances);
        SahTopology t;
        host_sah_topology(inst, t);
        const bool tree = (int)t.nodes.size() == 2 * t.leaves - 1 && t.order.size() == inst.size() && t.parent.size() == t.nodes.size();
        std::snprintf(what, sizeof(what), "second tree: %zu nodes, %d leaves over %zu instances", t.nodes.size(), t.leaves, inst.size());
        expect(tree, name, what);
        // its renumberings for the eight direction classes (the device inflates the tree before the library does this; the topology is the same)
        std::vector<NodeQ> out(t.nodes.size());
        std::vector<int> from(t.nodes.size());
        int good = 0;
        for (int o = 0; o < 8; o++)
        {
            const int sign[3] = {o & 1 ? 1 : -1, o & 2 ? 1 : -1, o & 4 ? 1 : 0};
            good += reorder_second_tree(t.nodes, sign, o * (int)t.nodes.size(), out.data(), from.data(), false) ? 1 : 0;
        }
        std::snprintf(what, sizeof(what), "renumbered for %d of 8 direction classes", good);
        expect(good == 8, name, what);
    }
    TreeletLimits lim;
    lim.bytes = 256; lim.minNodes = 1; lim.minBlasNodes = 1;        // the lowest limits: the 3-node BLAS of the small mesh is analysed, and has nothing to cut
                                                                    // (a cut needs two inner subtrees; tests/test_treelets.py has the meshes that are cut)
    TreeletsHost th;
    if (ph.ok && (ph.feat & 1) && ph.blas_refit_ok && !ph.meshRanges.empty()) build_treelets(ph.blas, ph.bsubend, ph.meshRanges, lim, th);
    std::snprintf(what, sizeof(what), "treelets: %zu over %zu reduced records", th.tl.size(), th.red.size());
    expect(true, name, what);
}

void check_accepted(const char* name, const SceneCopy& s)
{
    const hrt_scene_desc d = s.desc();
    PackedHost ph;
    const std::string e = validate_and_pack(&d, ph);
    expect(e.empty(), name, e.empty() ? "accepted" : "rejected: " + e);
    if (e.empty()) run_host_pipeline(name, d, ph);
}

void check_rejected(const char* name, const SceneCopy& valid, const std::function<void(SceneCopy&)>& mutate, const char* message)
{
    SceneCopy s = valid;
    mutate(s);
    const hrt_scene_desc d = s.desc();
    PackedHost ph;
    const std::string e = validate_and_pack(&d, ph);
    expect(e == message, name, e.empty() ? "accepted" : "rejected: " + e);
}

} // namespace

int main()
{
    const SceneCopy small = small_scene();
    // the layout the mutations index by position (tests/scene_mutations.py states it)
    const bool layout = small.tlasNodes.size() == 3 && small.blasNodes.size() == 5 && small.tlasInstanceIndices.size() == 3 && small.triPrimIdx.size() == 16 &&
                        small.meshTris.size() == 8 && small.meshPositions.size() == 9 && small.instances.size() == 3 && small.instances[2].blasRoot == 2 &&
                        small.instances[2].blasNodeCount == 3 && small.tlasNodes[0].count == 0 && small.tlasNodes[1].count == 2 && small.blasNodes[2].count == 0 &&
                        small.blasNodes[3].count == 4 && small.blasNodes[4].skipIndex == 3;
    expect(layout, "small scene", "layout as the mutations assume");
    if (!layout) return 1;
    check_accepted("small scene", small);
    check_accepted("300 one-sphere instances", many_spheres_scene());

    // messages 1-5 (check_nodes), TLAS and mesh BLAS
    check_rejected("tlas skip past the end", small, [](SceneCopy& s) { s.tlasNodes[2].skipIndex = 3; }, "tlasNodes: skipIndex out of range");
    check_rejected("tlas skip below -1", small, [](SceneCopy& s) { s.tlasNodes[2].skipIndex = -2; }, "tlasNodes: skipIndex out of range");
    check_rejected("tlas leaf range", small, [](SceneCopy& s) { s.tlasNodes[1].first = 2; }, "tlasNodes: leaf range outside the index list");
    check_rejected("tlas left child", small, [](SceneCopy& s) { s.tlasNodes[0].left = 3; }, "tlasNodes: left child out of range");
    check_rejected("tlas cycle", small, [](SceneCopy& s) { s.tlasNodes[1].skipIndex = 0; }, "tlasNodes: node links form a cycle");
    check_rejected("blas skip past the end", small, [](SceneCopy& s) { s.blasNodes[4].skipIndex = 5; }, "blasNodes: skipIndex out of range");
    check_rejected("blas skip below its BLAS", small, [](SceneCopy& s) { s.blasNodes[4].skipIndex = 1; }, "blasNodes: skipIndex below its BLAS");
    check_rejected("blas leaf range", small, [](SceneCopy& s) { s.blasNodes[3].first = 13; }, "blasNodes: leaf range outside the index list");
    check_rejected("blas left child past the end", small, [](SceneCopy& s) { s.blasNodes[2].left = 5; }, "blasNodes: left child out of range");
    check_rejected("blas left child below its BLAS", small, [](SceneCopy& s) { s.blasNodes[2].left = 1; }, "blasNodes: left child out of range");
    check_rejected("blas cycle", small, [](SceneCopy& s) { s.blasNodes[3].skipIndex = 2; }, "blasNodes: node links form a cycle");
    // message 6: a count alone -- the check runs before any element is read, so the short array behind it is never dereferenced
    {
        hrt_scene_desc d = small.desc();
        d.n_texels = 0x7FFFFFF1LL;
        PackedHost ph;
        const std::string e = validate_and_pack(&d, ph);
        expect(e == "array too long for 32-bit indices", "count above 0x7FFFFFF0", e.empty() ? "accepted" : "rejected: " + e);
    }
    // messages 7-15 (validate_and_pack)
    check_rejected("tlasInstanceIndices entry", small, [](SceneCopy& s) { s.tlasInstanceIndices[0] = 3; }, "tlasInstanceIndices entry out of range");
    check_rejected("tlasInstanceIndices negative", small, [](SceneCopy& s) { s.tlasInstanceIndices[2] = -1; }, "tlasInstanceIndices entry out of range");
    check_rejected("spherePrimIdx entry", small, [](SceneCopy& s) { s.spherePrimIdx[0] = 2; }, "spherePrimIdx entry out of range");
    check_rejected("triPrimIdx entry", small, [](SceneCopy& s) { s.triPrimIdx[5] = 8; }, "triPrimIdx entry out of range");
    check_rejected("triMatIndex short", small, [](SceneCopy& s) { s.triMatIndex.pop_back(); }, "triMatIndex / meshTriUVs shorter than meshTris");
    check_rejected("meshTriUVs short", small, [](SceneCopy& s) { s.meshTriUVs.pop_back(); }, "triMatIndex / meshTriUVs shorter than meshTris");
    check_rejected("meshTris vertex index", small, [](SceneCopy& s) { s.meshTris[0].i0 = 9; }, "meshTris vertex index out of range");
    check_rejected("meshTriUVs index", small, [](SceneCopy& s) { s.meshTriUVs[7].t2 = 9; }, "meshTriUVs index out of range");
    check_rejected("triMatIndex entry", small, [](SceneCopy& s) { s.triMatIndex[0] = 1; }, "triMatIndex entry out of range");
    check_rejected("texInfos entry", small, [](SceneCopy& s) { s.texInfos[0].Offset = 1; }, "texInfos entry outside texels");
    check_rejected("instance BLAS range", small, [](SceneCopy& s) { s.instances[2].blasNodeCount = 4; }, "instance BLAS range outside blasNodes");

    std::printf("%s\n", g_failed ? "hrt_scene_pack_check: FAILED" : "hrt_scene_pack_check: all verdicts as expected");
    return g_failed ? 1 : 0;
}
