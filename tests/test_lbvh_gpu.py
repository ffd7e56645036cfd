"""The trees the device builds (hrt_bvh.hip: TLAS rebuild of hrt_scene_update_instances, mesh-BLAS rebuild of
hrt_scene_update_positions) against tests/lbvh_ref.py, bit for bit through the downloads: links, index lists and node counts
against the restatement, boxes against the refit restatements of tests/test_bvh_update_gpu.py, sah_cost against its bits,
the growth figures against their float64 value, and one small frame against the oracle over the downloaded arrays.

A wrong Morton key, wrong centroid bounds, an unstable sort, a wrong split or tie-break, a leaf limit that is too large or a
collapse at the wrong level all still give a valid, deterministic tree whose frames match the oracle over that same tree;
only the comparison with the restatement sees them."""
import numpy as np
import pytest

from ilgpu_raytracing_amd import _types as T, engine, scenes
from tests import helpers as H, lbvh_cases as K, lbvh_ref as R
from tests.test_bvh_update_gpu import (_desc_with_tlas, _download, _gpu_render, _moves, _oracle_render, _refit_blas_numpy, _refit_numpy,
                                       SCENES)

pytestmark = pytest.mark.gpu

W, HGT, SPP = 64, 40, 1
FRAME_MODES = {"auto": T.FLAG_COUNTERS, "stream_production": T.FLAG_STREAMED}
CFG = scenes.Config("lbvh", 0, 0, 0, (2.0, 2.5, 11.0), (2.0, 1.8, 2.0))
CFG_MESH = scenes.Config("lbvh_mesh", 0, 0, 0, (0.4, 1.6, 4.6), (0.0, 0.8, 0.0))
NAN, INF = float("nan"), float("inf")

# growth_refit / blas_growth against the float64 value: the device sums __logf terms in float32 and takes __expf of the mean.
# Largest |device / reference - 1| measured over the cases of test_growth_* and test_blas_growth_* on an MI355X: 1.9e-7
# (third_doubled under AUTO: device 2.59075713, float64 2.59075762; the device's result is itself rounded to float32, 6e-8).
# The tolerance is 8 x that (never above 1e-3); one dropped or doubled node of these trees changes the value by 6e-4 .. 1.5e-2.
GROWTH_MEASURED = 1.9e-7
GROWTH_TOL = min(8 * GROWTH_MEASURED, 1e-3)


def _frames(orc, r, desc, cfg):
    ref, ost = _oracle_render(orc, desc, cfg, W, HGT, SPP)
    for mode, flags in FRAME_MODES.items():
        got, gst = _gpu_render(r, cfg, W, HGT, SPP, flags)
        H.assert_outputs_equal(ref, got)
        if flags & T.FLAG_COUNTERS:
            for i in range(2):
                assert gst.k[i].as_dict() == ost.k[i].as_dict(), (mode, i)


def _bits(x):
    x = np.float32(x)
    return 0x7FC00000 if np.isnan(x) else int(x.view(np.uint32))


def _assert_links(got, want, what):
    for f in R.LINK_FIELDS:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.tolist() == b.tolist(), "%s: %s differs from the restatement, first at node %s" % (
            what, f, int(np.nonzero(a != b)[0][0]) if len(a) == len(b) else "(lengths %d / %d)" % (len(a), len(b)))


def _check_tlas(r, st, want_inst, slot=0):
    """The downloaded TLAS of `slot` against the restatement over the downloaded instance records (themselves compared with
    want_inst when given).  Returns (nodes, idx, inst)."""
    nodes, idx, inst, cnt = r.download_tlas(slot)
    nodes = np.frombuffer(nodes, dtype=T.np_dtype(T.BvhNode), count=cnt[0]).copy()
    idx = np.frombuffer(idx, dtype=np.int32, count=cnt[1]).copy()
    inst = np.frombuffer(inst, dtype=T.np_dtype(T.InstanceRecord), count=cnt[2]).copy()
    if want_inst is not None:
        assert H.canon(inst).tobytes() == H.canon(want_inst).tobytes(), "instance records"
    links, order = R.tlas(inst)
    assert len(nodes) == len(links["count"]), "node count %d, restatement %d" % (len(nodes), len(links["count"]))
    assert idx.tolist() == order.tolist(), "tlasInstanceIndices: the stable sort by Morton key"
    _assert_links(R.links_of(nodes), links, "TLAS")
    R.check_tree(links, len(inst), 2)
    with np.errstate(all="ignore"):
        assert H.canon(nodes).tobytes() == H.canon(_refit_numpy(nodes, idx, inst)).tobytes(), "every box is the union of what it holds"
        if st is not None:
            assert st.tlas_nodes == len(nodes) and st.tlas_slots == len(idx)
            assert _bits(st.sah_cost) == _bits(R.sah_cost(nodes)), (st.sah_cost, R.sah_cost(nodes))
    return nodes, idx, inst


# ------------------------------------------------------------------ TLAS
def _centres(layout, n):
    rng = np.random.default_rng(100 * n + len(layout))
    q = lambda a: (np.round(np.asarray(a) * 256.0) / 256.0).astype(np.float32)       # centre -+ 0.25 and their mean are exact
    if layout == "uniform":
        return q(rng.uniform(0.0, 4.0, (n, 3)))
    if layout == "lattice":                                                           # 3 x 3 x 3 points: many equal keys
        p = np.array([[x, y, z] for x in (0.0, 2.0, 4.0) for y in (0.0, 1.5, 3.0) for z in (0.0, 2.0, 4.0)], np.float32)
        return p[rng.integers(0, 27, n)]
    if layout == "equal":                                                             # no extent at all
        return np.tile(np.array([[1.5, 1.0, 2.0]], np.float32), (n, 1))
    if layout == "collinear":                                                         # two extents zero
        c = np.zeros((n, 3), np.float32); c[:, 1] = 1.0; c[:, 2] = 2.0; c[:, 0] = q(rng.uniform(0.0, 4.0, n)); return c
    if layout == "coplanar":                                                          # one extent zero, and y shorter than x
        c = q(rng.uniform(0.0, 4.0, (n, 3))); c[:, 2] = 2.0; c[:, 1] = q(c[:, 1] * 0.5); return c
    if layout == "clamp":           # x spans exactly [0, 4]: 4 and 4 * 1023 / 1024 land on the clamp, 4 * 1022.5 / 1024 just below it
        c = q(rng.uniform(0.0, 4.0, (n, 3)))
        special = [0.0, 4.0, 4.0 * 1023.0 / 1024.0, 4.0 * 1022.5 / 1024.0, 4.0 / 1024.0]
        c[:min(n, 5), 0] = special[:min(n, 5)]
        c[:, 1:] = q(c[:, 1:] * 0.5)
        return c
    raise KeyError(layout)


def _sphere_builder(centres, radius=0.25):
    def build(b):
        for k, c in enumerate(centres):
            i = b.add_sphere(scenes.sphere(tuple(float(v) for v in c), radius, (0.3 + 0.6 * ((k * 37) % 11) / 10.0, 0.5, 0.9 - 0.6 * ((k * 13) % 7) / 6.0)))
            b.build_sphere_instance([i])
        b.rebuild_tlas()
    return build


@pytest.mark.parametrize("layout", ["uniform", "lattice", "equal", "collinear", "coplanar", "clamp"])
@pytest.mark.parametrize("n", [3, 4, 5, 128, 129, 256, 257])
def test_tlas_rebuild_equals_the_restatement(orc, renderer, n, layout):
    build = _sphere_builder(_centres(layout, n))
    s = engine.Scene(); build(s); renderer.commit(s)
    so = orc.OrcScene(); build(so)
    st = renderer.update_instances([], [], T.REBUILD_FORCE_REBUILD)
    assert st.action == T.REBUILD_FORCE_REBUILD and st.growth_final == 1.0 and st.growth_refit == 0.0
    nodes, idx, inst = _check_tlas(renderer, st, so.arrays()["instances"])
    if layout == "clamp" and n >= 5:
        keys = R.morton_keys(R.instance_centroids(inst))
        x = [sum(((int(k) >> (3 * b + 2)) & 1) << b for b in range(10)) for k in keys[:5]]
        assert x == [0, 1023, 1023, 1022, 1], "the restatement's own cells at the clamp"
    _frames(orc, renderer, _desc_with_tlas(so.desc(), nodes, idx, inst), CFG)
    # a refit of the rebuilt tree keeps it, and reports the same cost
    st2 = renderer.update_instances([], [], T.REBUILD_FORCE_REFIT)
    nodes2, idx2, _ = _check_tlas(renderer, st2, None)
    assert nodes2.tobytes() == nodes.tobytes() and idx2.tolist() == idx.tolist()


@pytest.mark.parametrize("kind", ["rigid", "hostile"])
def test_tlas_rebuild_with_moves(orc, renderer, kind):
    """Moves and the rebuild in one call; 'hostile': zero / negative / huge scales, NaN and infinite entries, so the rebuild runs
    over non-finite world bounds."""
    builder, cfg, _, _, _ = SCENES["sphere_instances"]
    s = engine.Scene(); builder(s); renderer.commit(s)
    so = orc.OrcScene(); builder(so)
    ids, xfs = _moves(len(so.arrays()["instances"]), kind)
    st = renderer.update_instances(ids, xfs, T.REBUILD_FORCE_REBUILD)
    for i, m in zip(ids, xfs):
        so.set_instance_transform(i, m)
    nodes, idx, inst = _check_tlas(renderer, st, so.arrays()["instances"])
    _frames(orc, renderer, _desc_with_tlas(so.desc(), nodes, idx, inst), cfg)


@pytest.mark.parametrize("value", ["nan", "inf"])
@pytest.mark.parametrize("n,lo,hi", [(192, 64, 128), (513, 256, 512)], ids=["a_wave_of_64", "a_workgroup_of_256"])
def test_rebuild_over_a_run_of_non_finite_centroids(orc, renderer, n, lo, hi, value):
    """ids lo..hi-1 all get a NaN (or infinite) x translation: a whole wave, or a whole workgroup, of the centroid-bounds kernel
    holds nothing but such centroids.  The bounds, and with them every key of the scene, must not depend on that alignment."""
    build = _sphere_builder(_centres("uniform", n))
    s = engine.Scene(); build(s); renderer.commit(s)
    so = orc.OrcScene(); build(so)
    ids = list(range(lo, hi))
    xfs = []
    for i in ids:
        m = T.identity_affine(); m.m03 = NAN if value == "nan" else INF
        xfs.append(m)
        so.set_instance_transform(i, m)
    st = renderer.update_instances(ids, xfs, T.REBUILD_FORCE_REBUILD)
    nodes, idx, inst = _check_tlas(renderer, st, so.arrays()["instances"])
    keys = R.morton_keys(R.instance_centroids(inst))
    if value == "nan":
        assert len(set(keys[:lo].tolist())) > lo // 2, "the finite instances keep real keys"
        assert all((int(k) & 0x24924924) == 0 for k in keys[lo:hi]), "a NaN x lands in cell 0"
    else:
        assert set(keys.tolist()) == {0}, "one infinite extent: every cell is cell 0, the tie-break builds the tree"
    _frames(orc, renderer, _desc_with_tlas(so.desc(), nodes, idx, inst), CFG)


def test_every_slot_builds_the_same_tree(orc):
    build = _sphere_builder(_centres("lattice", 129))
    r = engine.RTRenderer([0, 0, 0])
    try:
        s = engine.Scene(); build(s); r.commit(s)
        so = orc.OrcScene(); build(so)
        st = r.update_instances([], [], T.REBUILD_FORCE_REBUILD)
        got = [_check_tlas(r, st, so.arrays()["instances"], slot) for slot in range(3)]
        for nodes, idx, inst in got[1:]:
            assert nodes.tobytes() == got[0][0].tobytes() and idx.tolist() == got[0][1].tolist() and inst.tobytes() == got[0][2].tobytes()
        _frames(orc, r, _desc_with_tlas(so.desc(), *got[0]), CFG)
    finally:
        r.close()


# ------------------------------------------------------------------ mesh BLASes
def _mesh_data(mesh, kd=(0.8, 0.5, 0.3)):
    pos, tris = mesh
    return scenes.MeshData(pos, tris, np.zeros((len(pos), 2), np.float32), tris.copy(), [scenes.material(kd=kd, two_sided=1)], None, [])


def _mesh_builder(meshes):
    def build(b):
        g = b.add_sphere(scenes.sphere((0.0, -1000.0, 0.0), 1000.0, (0.6, 0.6, 0.6)))
        b.build_sphere_instance([g])
        for k, m in enumerate(meshes):
            b.load_mesh_instance(_mesh_data(m), scenes.rotation_affine("y", 0.0, 1.0, (1.5 * k, 0.0, -0.5 * k)) if k else None)
    return build


def _xyz(a):
    return np.stack([a[f] for f in "XYZ"], axis=1).astype(np.float32)


def _set_positions(arrs, pos):
    arrs["meshPositions"] = arrs["meshPositions"].copy()
    for k, f in enumerate("XYZ"):
        arrs["meshPositions"][f] = pos[:, k]


def _leaf_region(arrs, ii):
    b = arrs["instances"][ii]
    rng = arrs["blasNodes"][int(b["blasRoot"]):int(b["blasRoot"] + b["blasNodeCount"])]
    return int(rng["first"][rng["count"] > 0].min())


def _check_blas_rebuild(orc, r, arrs, st, cfg=CFG_MESH, frames=True):
    """arrs: the scene as uploaded, with meshPositions as they are on the device now.  Every mesh BLAS of the device against the
    restatement (or, where that says "does not fit", against the uploaded topology), boxes against the refit restatement.
    Returns {instance: limit}."""
    got = {k: r.download_array(k) for k in ("meshPositions", "blasNodes", "triPrimIdx")}
    nodes, idx, inst = _download(r)
    assert got["meshPositions"].tobytes() == arrs["meshPositions"].tobytes()
    pos = _xyz(arrs["meshPositions"])
    tris = np.stack([arrs["meshTris"][f] for f in ("i0", "i1", "i2")], axis=1)
    # Meshes are rebuilt in instance order, each reading its item list as it is at its turn.  That matters for scenes of the
    # reference's own builder: it gives a later mesh primIndexFirst = its first triangle id, a window of triPrimIdx that lies in
    # an earlier mesh's leaf region (hrt_host.cpp, Scene.cs:398-403), so that mesh's items are what the earlier rebuild left there.
    limits, want_prim, want_count = {}, arrs["triPrimIdx"].copy(), arrs["instances"]["blasNodeCount"].copy()
    for ii, b in enumerate(arrs["instances"]):
        root, cap = int(b["blasRoot"]), int(b["blasNodeCount"])
        if b["type"] != 2:
            assert got["blasNodes"][root:root + cap].tobytes() == arrs["blasNodes"][root:root + cap].tobytes(), "sphere BLASes are untouched"
            continue
        n, first = int(b["primIndexCount"]), int(b["primIndexFirst"])
        leaf_base = _leaf_region(arrs, ii)
        limit, links, region, count = R.blas(pos, tris, want_prim[first:first + n].copy(), cap, node_base=root, leaf_base=leaf_base)
        limits[ii] = limit
        dev = got["blasNodes"][root:root + cap]
        if limit is R.DOES_NOT_FIT:
            _assert_links(R.links_of(dev), R.links_of(arrs["blasNodes"][root:root + cap]), "mesh %d keeps its uploaded topology" % ii)
            continue
        _assert_links(R.links_of(dev), links, "BLAS of mesh %d (limit %d)" % (ii, limit))
        sizes = R.check_tree(links, n, limit, node_base=root, leaf_base=leaf_base, n_nodes=count)
        assert limit == 4 or max(sizes) > 4
        want_prim[leaf_base:leaf_base + n] = region
        want_count[ii] = count
        tail = dev[count:]
        assert not tail["boundsMin"].tobytes().strip(b"\0") and not tail["boundsMax"].tobytes().strip(b"\0"), "nodes behind the tree are zeroed"
    assert got["triPrimIdx"].tolist() == want_prim.tolist(), "leaf regions in sorted order; item lists and regions of kept meshes untouched"
    assert inst["blasNodeCount"].tolist() == want_count.tolist()
    now = dict(arrs)
    now["blasNodes"], now["triPrimIdx"], now["instances"] = got["blasNodes"], got["triPrimIdx"], inst
    want_blas, want_inst = _refit_blas_numpy(now)
    assert want_blas.tobytes() == got["blasNodes"].tobytes() and want_inst.tobytes() == inst.tobytes(), "boxes and world bounds"
    assert nodes.tobytes() == _refit_numpy(nodes, idx, inst).tobytes()
    assert _bits(st.sah_cost) == _bits(R.sah_cost(nodes))
    if frames:
        now["tlasNodes"], now["tlasInstanceIndices"] = nodes, idx
        desc, keep = T.scene_desc_from_arrays(now)
        _frames(orc, r, desc, cfg)
    return limits


def _wobble(pos):
    return (pos * (1.0 + 0.1 * np.sin(6.0 * pos[:, [2, 0, 1]] + 0.5))).astype(np.float32)


def _blob(b):
    scenes.build_config4(b, 24, 24)


BLAS_CASES = {("tris_%d" % n): _mesh_builder([K.random_mesh(n, 40 + n)]) for n in (1, 2, 4, 5, 14, 15, 16, 255, 256, 257)}
BLAS_CASES.update({
    "blob_24x24": _blob,
    "doubled_triangles": _mesh_builder([K.doubled_mesh(130, 7)]),
    "one_centroid": _mesh_builder([K.one_centroid_mesh(37)]),
    "two_meshes": _mesh_builder([K.random_mesh(77, 8), K.doubled_mesh(50, 9)]),
})


@pytest.mark.parametrize("name", list(BLAS_CASES))
def test_blas_rebuild_equals_the_restatement(orc, renderer, name):
    build = BLAS_CASES[name]
    s = engine.Scene(); build(s)
    arrs = s.arrays()
    renderer.commit(s)
    new = _wobble(_xyz(arrs["meshPositions"]))
    try:
        st = renderer.update_positions(0, new, T.REBUILD_FORCE_REFIT | T.REBUILD_BLAS)
    except engine.HrtError as e:
        rebuildable = all(2 * ((int(b["primIndexCount"]) + 13) // 14) - 1 <= int(b["blasNodeCount"]) for b in arrs["instances"] if b["type"] == 2)
        assert not rebuildable and "cannot be rebuilt on the device" in str(e)
        return
    _set_positions(arrs, new)
    limits = _check_blas_rebuild(orc, renderer, arrs, st, scenes.CONFIGS[4] if name == "blob_24x24" else CFG_MESH)
    assert st.action == T.REBUILD_FORCE_REFIT and st.blas_action == (T.REBUILD_FORCE_REBUILD if any(limits.values()) else T.REBUILD_FORCE_REFIT)
    # a second rebuild reads the items from the item list again, not from the (now sorted) leaf region: the same tree
    before = {k: renderer.download_array(k).tobytes() for k in ("blasNodes", "triPrimIdx")}
    renderer.update_positions(0, new[:0], T.REBUILD_FORCE_REFIT | T.REBUILD_BLAS)
    assert {k: renderer.download_array(k).tobytes() for k in before} == before


def _tight_scene(mesh, leaf):
    """ground + one mesh whose uploaded BLAS is the walk-ordered median-split tree with leaves of `leaf`: the scene arrays."""
    s = engine.Scene(); _mesh_builder([mesh])(s)
    arrs = dict(s.arrays())
    ii = int(np.nonzero(arrs["instances"]["type"] == 2)[0][0])
    b = arrs["instances"][ii]
    root, n, first = int(b["blasRoot"]), int(b["primIndexCount"]), int(b["primIndexFirst"])
    assert root + int(b["blasNodeCount"]) == len(arrs["blasNodes"]), "the mesh's node range is the last one"
    leaf_base = _leaf_region(arrs, ii)
    tris = np.stack([arrs["meshTris"][f] for f in ("i0", "i1", "i2")], axis=1)
    items = arrs["triPrimIdx"][first:first + n]
    links, order = K.median_tree(_xyz(arrs["meshPositions"]), tris[items], leaf, node_base=root, leaf_base=leaf_base)
    mine = np.zeros(len(links["count"]), arrs["blasNodes"].dtype)
    for f in R.LINK_FIELDS:
        mine[f] = links[f]
    arrs["blasNodes"] = np.concatenate([arrs["blasNodes"][:root], mine])
    arrs["triPrimIdx"] = arrs["triPrimIdx"].copy()
    arrs["triPrimIdx"][leaf_base:leaf_base + n] = items[order]
    arrs["instances"] = arrs["instances"].copy()
    arrs["instances"]["blasNodeCount"][ii] = len(mine)
    arrs["blasNodes"], arrs["instances"] = _refit_blas_numpy(arrs)
    arrs["tlasNodes"] = _refit_numpy(arrs["tlasNodes"], arrs["tlasInstanceIndices"], arrs["instances"])
    return arrs, ii


@pytest.mark.parametrize("case", K.tight_cases(), ids=[c[0] for c in K.tight_cases()])
def test_leaf_limit_is_the_smallest_that_fits(orc, renderer, case):
    """Node ranges made tight by hand: the device takes the restatement's limit (4, 7, 9, 14 here, tests/test_lbvh_ref.py), and a
    mesh that does not fit even at 14 keeps its uploaded topology and is refitted."""
    name, mesh, leaf = case
    arrs, ii = _tight_scene(mesh, leaf)
    desc, keep = T.scene_desc_from_arrays(arrs)
    renderer.commit(desc)
    st = renderer.update_positions(0, np.zeros((0, 3), np.float32), T.REBUILD_FORCE_REFIT | T.REBUILD_BLAS)   # the positions of the CPU test
    limits = _check_blas_rebuild(orc, renderer, arrs, st)
    want = {"roomy_leaf2": 4, "leaf6": 7, "leaf10": 9, "leaf10_flat": 14, "leaf14_full": None, "leaf14_doubled": None}[name]
    assert limits[ii] == want
    assert st.blas_action == (T.REBUILD_FORCE_REBUILD if want else T.REBUILD_FORCE_REFIT)


def test_auto_refits_a_mesh_whose_rebuild_does_not_fit(orc, renderer):
    """AUTO wants to rebuild (the boxes grew) but no leaf size fits the node range: the call succeeds, the mesh keeps its
    topology and its triPrimIdx and is refitted; a second mesh of the same scene that does fit is rebuilt."""
    name, mesh, leaf = [c for c in K.tight_cases() if c[0] == "leaf14_full"][0]
    arrs, ii = _tight_scene(mesh, leaf)
    desc, keep = T.scene_desc_from_arrays(arrs)
    renderer.commit(desc)
    pos = _xyz(arrs["meshPositions"])
    st = renderer.update_positions(0, pos, T.REBUILD_AUTO)
    assert st.blas_action == T.REBUILD_FORCE_REFIT and abs(st.blas_growth - 1.0) <= GROWTH_TOL
    new = pos[np.random.default_rng(3).permutation(len(pos))].astype(np.float32)   # neighbours in the tree end up far apart
    st = renderer.update_positions(0, new, T.REBUILD_AUTO)
    assert st.blas_growth > 1.6 and st.blas_action == T.REBUILD_FORCE_REFIT
    _set_positions(arrs, new)
    limits = _check_blas_rebuild(orc, renderer, arrs, st)
    assert limits[ii] is R.DOES_NOT_FIT
    assert renderer.download_array("triPrimIdx").tobytes() == arrs["triPrimIdx"].tobytes()


def test_a_mesh_that_does_not_fit_leaves_the_others_their_rebuild(orc, renderer):
    """two meshes, the first with a full-leaf range: the second is rebuilt all the same"""
    arrs, ii = _tight_scene(K.random_mesh(224, 25), 14)
    s2 = engine.Scene(); _mesh_builder([K.random_mesh(224, 25), K.random_mesh(61, 31)])(s2)
    two = dict(s2.arrays())
    # graft the tight tree of the one-mesh scene over the first mesh of the two-mesh scene if the layouts allow it
    a, b = two["instances"][ii], arrs["instances"][ii]
    if not (a["blasRoot"] == b["blasRoot"] and a["primIndexFirst"] == b["primIndexFirst"] and _leaf_region(two, ii) == _leaf_region(arrs, ii)):
        pytest.fail("the host builder lays a second mesh out differently than this test assumes")
    cap_old, cap_new = int(a["blasNodeCount"]), int(b["blasNodeCount"])
    root = int(a["blasRoot"])
    two["blasNodes"] = two["blasNodes"].copy()
    two["blasNodes"][root:root + cap_new] = arrs["blasNodes"][root:root + cap_new]
    two["blasNodes"][root + cap_new:root + cap_old] = np.zeros(1, two["blasNodes"].dtype)
    for f in ("left", "right", "first", "skipIndex"):
        two["blasNodes"][f][root + cap_new:root + cap_old] = -1
    n = int(a["primIndexCount"])
    lb = _leaf_region(arrs, ii)
    two["triPrimIdx"] = two["triPrimIdx"].copy()
    two["triPrimIdx"][lb:lb + n] = arrs["triPrimIdx"][lb:lb + n]
    two["instances"] = two["instances"].copy()
    two["instances"]["blasNodeCount"][ii] = cap_new
    two["blasNodes"], two["instances"] = _refit_blas_numpy(two)
    two["tlasNodes"] = _refit_numpy(two["tlasNodes"], two["tlasInstanceIndices"], two["instances"])
    desc, keep = T.scene_desc_from_arrays(two)
    renderer.commit(desc)
    new = _wobble(_xyz(two["meshPositions"]))
    st = renderer.update_positions(0, new, T.REBUILD_FORCE_REFIT | T.REBUILD_BLAS)
    _set_positions(two, new)
    limits = _check_blas_rebuild(orc, renderer, two, st)
    others = [v for k, v in limits.items() if k != ii]
    assert limits[ii] is R.DOES_NOT_FIT and len(others) == 1 and others[0] is not R.DOES_NOT_FIT
    assert st.blas_action == T.REBUILD_FORCE_REBUILD


# ------------------------------------------------------------------ the numbers AUTO decides by
def _check_refit(r, st, base):
    """after a refit: the topology of `base`, every box recomputed, the cost of the new boxes"""
    nodes, idx, inst = _download(r)
    _assert_links(R.links_of(nodes), R.links_of(base), "a refit keeps the topology")
    assert nodes.tobytes() == _refit_numpy(nodes, idx, inst).tobytes()
    assert st.tlas_nodes == len(nodes) and _bits(st.sah_cost) == _bits(R.sah_cost(nodes))
    return nodes


def _scale_moves(ids, centres, scale):
    """instance i scaled by `scale` about its own centre: its box grows, its centroid stays"""
    return [scenes.rotation_affine("y", 0.0, scale, tuple(float(v) for v in (centres[i] * (1.0 - scale)))) for i in ids]


GROWTH_CASES = {            # (instances, ids that move, scale, reference value of growth_refit)
    "few_doubled": (33, [1, 5], 2.0),
    "third_doubled": (33, list(range(0, 33, 3)), 2.0),
    "all_doubled": (30, list(range(30)), 2.0),
    "some_shrunk": (17, [2, 3, 11], 0.5),
}


@pytest.mark.parametrize("name", list(GROWTH_CASES))
def test_growth_refit_equals_the_float64_value(orc, renderer, name):
    n, ids, scale = GROWTH_CASES[name]
    centres = _centres("uniform", n)
    build = _sphere_builder(centres)
    s = engine.Scene(); build(s); renderer.commit(s)
    st = renderer.update_instances([], [], T.REBUILD_FORCE_REBUILD)
    base, _, _ = _check_tlas(renderer, st, None)
    assert len(base) <= 65
    xfs = _scale_moves(ids, centres, scale)
    st = renderer.update_instances(ids, xfs, T.REBUILD_FORCE_REFIT)
    now = _check_refit(renderer, st, base)
    ref = R.growth(R.node_areas(*R.boxes_of(now)), R.node_areas(*R.boxes_of(base)))
    one_node = R.growth(R.node_areas(*R.boxes_of(now))[1:], R.node_areas(*R.boxes_of(base))[1:])
    print("growth_refit %s: device %.9g reference %.9g |device/ref - 1| = %.3g (without the root: %.3g)"
          % (name, st.growth_refit, ref, abs(st.growth_refit / ref - 1.0), abs(one_node / ref - 1.0)))
    assert abs(st.growth_refit / ref - 1.0) <= GROWTH_TOL
    assert st.growth_final == st.growth_refit
    # AUTO takes the reference's decision on the same moves, from a tree rebuilt with those instances back under the identity.
    # That is not the uploaded scene again: a moved instance gets the world bounds of its BLAS root box, which the reference's
    # position-indexed sphere builder (Scene.cs:386-395) makes another sphere's, so the base tree and the value are new ones.
    st = renderer.update_instances(ids, [T.identity_affine()] * len(ids), T.REBUILD_FORCE_REBUILD)
    base2, idx2, _ = _check_tlas(renderer, st, None)
    st = renderer.update_instances(ids, xfs, T.REBUILD_AUTO)
    _, _, inst2 = _download(renderer)
    now2 = _refit_numpy(base2, idx2, inst2)
    ref2 = R.growth(R.node_areas(*R.boxes_of(now2)), R.node_areas(*R.boxes_of(base2)))
    print("growth_refit %s under AUTO: device %.9g reference %.9g |device/ref - 1| = %.3g" % (name, st.growth_refit, ref2, abs(st.growth_refit / ref2 - 1.0)))
    assert not 1.4 <= ref2 <= 1.6, "the case must not sit on the threshold"
    assert st.action == (T.REBUILD_FORCE_REBUILD if ref2 > 1.5 else T.REBUILD_FORCE_REFIT)
    assert abs(st.growth_refit / ref2 - 1.0) <= GROWTH_TOL
    if ref2 > 1.5:
        assert st.growth_final == 1.0
        _check_tlas(renderer, st, None)
    else:
        assert st.growth_final == st.growth_refit
        assert _check_refit(renderer, st, base2).tobytes() == now2.tobytes()


@pytest.mark.parametrize("part,scale", [(0.25, 2.0), (1.0, 2.0), (0.5, 1.1), (1.0, 6.0)])
def test_blas_growth_equals_the_float64_value(orc, renderer, part, scale):
    build = _mesh_builder([K.random_mesh(60, 77)])
    s = engine.Scene(); build(s); renderer.commit(s)
    arrs = dict(s.arrays())
    b = arrs["instances"][arrs["instances"]["type"] == 2][0]
    root, cap = int(b["blasRoot"]), int(b["blasNodeCount"])
    assert cap <= 65
    base_nodes, _ = _refit_blas_numpy(arrs)
    pos = _xyz(arrs["meshPositions"])
    k = int(len(pos) * part) // 3 * 3
    new = pos.copy()
    tri = new[:k].reshape(-1, 3, 3)
    tri[:] = tri.mean(axis=1, keepdims=True) + (tri - tri.mean(axis=1, keepdims=True)) * scale     # whole triangles about their centres
    new = new.astype(np.float32)
    st = renderer.update_positions(0, new, T.REBUILD_AUTO)
    _set_positions(arrs, new)
    now_nodes, _ = _refit_blas_numpy(arrs)
    ref = R.growth(R.node_areas(*R.boxes_of(now_nodes[root:root + cap])), R.node_areas(*R.boxes_of(base_nodes[root:root + cap])))
    print("blas_growth part %.2f scale %.1f: device %.9g reference %.9g |device/ref - 1| = %.3g" % (part, scale, st.blas_growth, ref, abs(st.blas_growth / ref - 1.0)))
    assert abs(st.blas_growth / ref - 1.0) <= GROWTH_TOL
    assert not 1.4 <= ref <= 1.6
    if ref > 1.5:
        limits = _check_blas_rebuild(orc, renderer, arrs, st, frames=False)
        assert all(limits.values()) and st.blas_action == T.REBUILD_FORCE_REBUILD
    else:
        assert st.blas_action == T.REBUILD_FORCE_REFIT
        assert renderer.download_array("blasNodes").tobytes() == now_nodes.tobytes()
