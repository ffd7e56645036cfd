"""tests/lbvh_ref.py held to a second formulation (no GPU): Karras' construction with the position tie-break must emit the same
arrays as a top-down recursion over the unique integers key << 32 | sorted position, quant10 is checked by hand at its edges, and
the hand-made mesh cases of tests/test_lbvh_gpu.py must, by the restatement alone, cover leaf limit 4, two limits above it and
"does not fit" -- otherwise the GPU test could pass without the limit search ever leaving its first step."""
import numpy as np
import pytest

from tests import lbvh_cases as K, lbvh_ref as R

SIZES = [1, 2, 3, 4, 5, 14, 15, 128, 129, 256, 257]


def _keys(kind, n):
    rng = np.random.default_rng(1000 + n)
    if kind == "uniform":
        k = rng.integers(0, 1 << 30, n)
    elif kind == "runs":                       # 27 distinct values: long runs of duplicates at 257 items
        k = rng.integers(0, 1 << 30, 27)[rng.integers(0, 27, n)]
    else:
        k = np.full(n, 0x2AAAAAAA)
    return np.sort(k.astype(np.uint32), kind="stable")


@pytest.mark.parametrize("limit", [1, 2, 4, 7, 14])
@pytest.mark.parametrize("kind", ["uniform", "runs", "equal"])
@pytest.mark.parametrize("n", SIZES)
def test_karras_equals_top_down(n, kind, limit):
    keys = _keys(kind, n)
    a = R.emit(keys, limit, node_base=5, leaf_base=11)
    b = R.emit_topdown(keys, limit, node_base=5, leaf_base=11)
    for f in R.LINK_FIELDS:
        assert a[f].tolist() == b[f].tolist(), f
    sizes = R.check_tree(a, n, limit, node_base=5, leaf_base=11)
    assert sum(sizes) == n
    if kind == "equal" and n > limit:
        # all keys equal: the tie-break alone builds the tree, a balanced one over positions
        assert max(sizes) <= limit and min(sizes) >= 1


def test_equal_keys_split_by_position():
    # five equal keys, limit 2: positions 0..4 split at the highest differing position bit: [0..3] | [4], then [0,1] | [2,3]
    t = R.emit(np.full(5, 7, np.uint32), 2)
    assert t["count"].tolist() == [0, 0, 2, 2, 1] and t["first"].tolist() == [-1, -1, 0, 2, 4]
    assert t["left"].tolist() == [1, 2, -1, -1, -1] and t["right"].tolist() == [4, 3, -1, -1, -1]
    assert t["skipIndex"].tolist() == [-1, 4, 3, 4, -1]


def test_quant10_edges():
    f = np.float32
    assert R.quant10(f(2.0), f(2.0), f(6.0)) == 0                         # c == lo
    assert R.quant10(f(6.0), f(2.0), f(6.0)) == 1023                      # c == hi: 1024 clamps
    assert R.quant10(np.nextafter(f(6.0), f(0.0)), f(2.0), f(6.0)) == 1023
    assert R.quant10(f(4.0), f(2.0), f(6.0)) == 512
    assert R.quant10(f(2.0) + f(4.0) * f(1022.5 / 1024.0), f(2.0), f(6.0)) == 1022
    assert R.quant10(f(3.0), f(3.0), f(3.0)) == 0                         # ext == 0
    assert R.quant10(f(5.0), f(3.0), f(3.0)) == 0
    assert R.quant10(f(1.0), f(2.0), f(6.0)) == 0                         # below lo
    assert R.quant10(f("nan"), f(2.0), f(6.0)) == 0
    assert R.quant10(f("inf"), f(2.0), f(6.0)) == 1023
    assert R.quant10(f("-inf"), f(2.0), f(6.0)) == 0
    assert R.quant10(f(4.0), f(2.0), f("inf")) == 0                       # an infinite extent: every finite c lands in cell 0
    assert R.quant10(f("inf"), f(2.0), f("inf")) == 0                     # inf / inf
    assert R.quant10(f(4.0), f("nan"), f("nan")) == 0
    assert R.quant10(f(0.0), f(-0.0), f(1.0)) == 0                        # lo = -0.0
    assert R.quant10(f(-0.0), f(-0.0), f(1.0)) == 0
    assert R.quant10(f(0.5), f(-0.0), f(1.0)) == 512
    assert R.quant10(f(1.0), f(-0.0), f(1.0)) == 1023


def test_keys_of_a_small_set_by_hand():
    # cubic cells: ext = 4 (x); y spans 1 -> cells 0..256; z has no extent
    c = np.array([[0, 0, 5], [4, 1, 5], [2, 0.5, 5], [np.nan, 1, 5]], np.float32)
    k = R.morton_keys(c)

    def key(x, y, z):
        return (R._spread3(x) << 2) | (R._spread3(y) << 1) | R._spread3(z)
    assert k.tolist() == [key(0, 0, 0), key(1023, 256, 0), key(512, 128, 0), key(0, 256, 0)]
    assert R._spread3(0x3FF) == 0x09249249 and key(1023, 0, 0) == 0x24924924
    lo, hi = R.centroid_bounds(np.full((3, 3), np.nan, np.float32))
    assert np.isnan(lo).all() and np.isnan(hi).all()
    assert R.morton_keys(np.full((3, 3), np.nan, np.float32)).tolist() == [0, 0, 0]
    assert R.sort_items(np.array([3, 1, 3, 1, 0], np.uint32)).tolist() == [4, 1, 3, 0, 2]


def test_sums_in_the_device_order():
    # 300 nodes: two partial blocks; float32 pairwise order differs from a running sum
    rng = np.random.default_rng(5)
    v = rng.uniform(0.1, 3.0, 300).astype(np.float32)
    s0 = R._tree_sum(v[:256], 256)
    s1 = R._tree_sum(v[256:], 256)
    want = np.float32(s0 + s1)
    acc = np.zeros(1024, np.float32); acc[0], acc[1] = s0, s1
    assert R._tree_sum(acc, 1024) == want
    ref = float(np.sum(v.astype(np.float64)))
    assert abs(float(want) - ref) <= 300 * 2.0 ** -24 * ref
    assert R.growth([2.0, 8.0, 0.0, 3.0], [1.0, 2.0, 1.0, 0.0]) == pytest.approx(np.sqrt(8.0), rel=1e-12)
    assert R.growth([0.0], [1.0]) == 1.0


def _case_limit(mesh, leaf):
    pos, tris = mesh
    links, order = K.median_tree(pos, tris, leaf)
    cap = len(links["count"])
    R.check_tree(links, len(tris), leaf)
    n = len(tris)
    assert 2 * ((n + 13) // 14) - 1 <= cap, "the upload accepts this range for a rebuild"
    return R.blas(pos, tris, np.arange(n), cap), cap


def test_hand_made_cases_cover_the_limit_search():
    limits = {}
    for name, mesh, leaf in K.tight_cases():
        (limit, links, region, count), cap = _case_limit(mesh, leaf)
        limits[name] = limit
        if limit is not R.DOES_NOT_FIT:
            n = len(mesh[1])
            sizes = R.check_tree(links, n, limit, n_nodes=count)
            assert sorted(region.tolist()) == list(range(n)) and count <= cap
            assert (links["count"][count:] == 0).all() and all((links[f][count:] == -1).all() for f in ("left", "right", "first", "skipIndex"))
            if limit > 4:                         # the smallest that fits: one less does not
                keys = R.morton_keys(R.triangle_centroids(mesh[0], mesh[1], np.arange(n)))
                assert len(R.emit(np.sort(keys, kind="stable"), limit - 1)["count"]) > cap
                assert max(sizes) > 4
    got = set(limits.values())
    assert 4 in got, limits
    assert len({v for v in got if v is not None and v > 4}) >= 2, limits
    assert R.DOES_NOT_FIT in got, limits


def test_median_tree_is_a_valid_walk_ordered_blas():
    pos, tris = K.random_mesh(57, 3)
    for leaf in (1, 6, 14):
        links, order = K.median_tree(pos, tris, leaf, node_base=9, leaf_base=57)
        sizes = R.check_tree(links, 57, leaf, node_base=9, leaf_base=57)
        assert sorted(order.tolist()) == list(range(57)) and sum(sizes) == 57
