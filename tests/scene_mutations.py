"""A small valid scene and one minimal mutation of it per rejection path of the scene validator (csrc/hrt_scene_pack.hip:
check_nodes, validate_and_pack).  Shared by tests/test_scene_validation.py (host only, every path) and tests/test_api_gpu.py
(hrt_scene_upload surfaces the same texts and leaves the committed scene alone).

The scene: two one-sphere instances and one textured mesh of 8 triangles, built by engine.Scene.  Its arrays, which the mutations
below index by position:
  tlasNodes   [0] inner, left 2      [1] leaf, slots 1..2, skip -1    [2] leaf, slot 0, skip 1          (3 instance slots)
  blasNodes   [0] [1] the spheres' one-node BLASes;  the mesh BLAS is [2, 5): [2] inner, left 4   [3] leaf, skip -1
              [4] leaf, skip 3                                                                      (16 triPrimIdx entries)
  2 spheres, 9 positions, 9 texcoords, 8 triangles, 1 material, one 4x4 texture (16 texels)."""
import numpy as np

from ilgpu_raytracing_amd import _types as T, engine, scenes

TOO_LONG = 0x7FFFFFF1          # the first count the validator's 32-bit check refuses


def build_scene():
    s = engine.Scene()
    tex = np.zeros((4, 4, 4), np.uint8)
    tex[..., 3] = 255
    tex[::2, ::2, 0] = 200
    a = s.add_sphere(scenes.sphere((-1.0, 0.5, 0.0), 0.5, (0.8, 0.3, 0.3)))
    b = s.add_sphere(scenes.sphere((1.0, 0.5, 0.0), 0.5, (0.3, 0.8, 0.3)))
    s.build_sphere_instance([a])
    s.build_sphere_instance([b])
    g = np.linspace(-1.0, 1.0, 3)
    yq, xq = np.meshgrid(g * 0.5 + 1.0, g, indexing="ij")
    q = scenes.grid_mesh(xq, yq, -1.0 + 0.0 * xq, (xq + 1.0) / 2.0, yq - 0.5)
    m = scenes.material(kd=(0.9, 0.9, 0.9), diffuse_tex=0)
    s.load_mesh_instance(engine.MeshData(q.positions, q.triangles, q.texcoords, q.tri_uvs, [m], None, [tex]))
    s.rebuild_tlas()
    return s


def valid_arrays():
    """The scene's 15 arrays as fresh numpy copies, after checking that they are laid out as the mutations assume."""
    A = build_scene().arrays()
    tn, bn, inst = A["tlasNodes"], A["blasNodes"], A["instances"]
    assert {k: len(v) for k, v in A.items()} == dict(
        tlasNodes=3, tlasInstanceIndices=3, instances=3, blasNodes=5, spherePrimIdx=4, spheres=2, triPrimIdx=16, meshPositions=9,
        meshTris=8, meshTexcoords=9, meshTriUVs=8, triMatIndex=8, materials=1, texels=16, texInfos=1)
    assert tn["count"].tolist() == [0, 2, 1] and tn["left"][0] == 2 and tn["skipIndex"].tolist() == [-1, -1, 1] and tn["first"][1] == 1
    assert bn["count"].tolist() == [1, 1, 0, 4, 4] and bn["left"][2] == 4 and bn["skipIndex"].tolist()[2:] == [-1, -1, 3] and bn["first"][3] == 8
    assert inst["type"].tolist() == [T.BLAS_SPHERESET, T.BLAS_SPHERESET, T.BLAS_TRIMESH]
    assert (inst["blasRoot"][2], inst["blasNodeCount"][2]) == (2, 3)
    return A


def _set(array, index, field, value):
    def mutate(A):
        if field is None: A[array][index] = value
        else: A[array][field][index] = value
    return mutate


def _truncate(array):
    def mutate(A):
        A[array] = A[array][:-1].copy()
    return mutate


# id -> (mutation of the arrays in place, the validator's text).  Messages 1-5 come from check_nodes, once for tlasNodes and once for
# the mesh BLAS in blasNodes (message 2 has no TLAS form: the TLAS range starts at node 0); 7-15 from validate_and_pack.
MUTATIONS = {
    "tlas_skip_past_the_end":     (_set("tlasNodes", 2, "skipIndex", 3), "tlasNodes: skipIndex out of range"),
    "tlas_skip_below_minus_one":  (_set("tlasNodes", 2, "skipIndex", -2), "tlasNodes: skipIndex out of range"),
    "tlas_leaf_range":            (_set("tlasNodes", 1, "first", 2), "tlasNodes: leaf range outside the index list"),
    "tlas_left_child":            (_set("tlasNodes", 0, "left", 3), "tlasNodes: left child out of range"),
    "tlas_cycle":                 (_set("tlasNodes", 1, "skipIndex", 0), "tlasNodes: node links form a cycle"),
    "blas_skip_past_the_end":     (_set("blasNodes", 4, "skipIndex", 5), "blasNodes: skipIndex out of range"),
    "blas_skip_below_its_blas":   (_set("blasNodes", 4, "skipIndex", 1), "blasNodes: skipIndex below its BLAS"),
    "blas_leaf_range":            (_set("blasNodes", 3, "first", 13), "blasNodes: leaf range outside the index list"),
    "blas_left_child_past_end":   (_set("blasNodes", 2, "left", 5), "blasNodes: left child out of range"),
    "blas_left_child_below_blas": (_set("blasNodes", 2, "left", 1), "blasNodes: left child out of range"),
    "blas_cycle":                 (_set("blasNodes", 3, "skipIndex", 2), "blasNodes: node links form a cycle"),
    "tlas_instance_index":        (_set("tlasInstanceIndices", 0, None, 3), "tlasInstanceIndices entry out of range"),
    "tlas_instance_index_neg":    (_set("tlasInstanceIndices", 2, None, -1), "tlasInstanceIndices entry out of range"),
    "sphere_prim_idx":            (_set("spherePrimIdx", 0, None, 2), "spherePrimIdx entry out of range"),
    "tri_prim_idx":               (_set("triPrimIdx", 5, None, 8), "triPrimIdx entry out of range"),
    "tri_mat_index_short":        (_truncate("triMatIndex"), "triMatIndex / meshTriUVs shorter than meshTris"),
    "tri_uvs_short":              (_truncate("meshTriUVs"), "triMatIndex / meshTriUVs shorter than meshTris"),
    "tri_vertex_index":           (_set("meshTris", 0, "i0", 9), "meshTris vertex index out of range"),
    "tri_uv_index":               (_set("meshTriUVs", 7, "t2", 9), "meshTriUVs index out of range"),
    "tri_mat_index":              (_set("triMatIndex", 0, None, 1), "triMatIndex entry out of range"),
    "tex_info_outside_texels":    (_set("texInfos", 0, "Offset", 1), "texInfos entry outside texels"),
    "instance_blas_range":        (_set("instances", 2, "blasNodeCount", 4), "instance BLAS range outside blasNodes"),
}


def mutated_desc(valid, name):
    """(SceneDesc, keepalive, message) of mutation `name` applied to a copy of the arrays `valid` (which stay as they are)."""
    A = {k: v.copy() for k, v in valid.items()}
    mutate, message = MUTATIONS[name]
    mutate(A)
    desc, keep = T.scene_desc_from_arrays(A)
    return desc, keep, message
