"""Inputs shared by tests/test_lbvh_ref.py (CPU) and tests/test_lbvh_gpu.py: small meshes as (positions, triangles), and a
walk-ordered median-split BLAS with a chosen leaf size, which makes the node range a rebuild has to fit into as tight as wanted."""
import numpy as np


def random_mesh(n, seed, flat=1.0):
    """n separate triangles (3 n vertices) scattered in a box around (0, 0.9, 0)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.0, 1.0, (n, 1, 3)) * np.array([1.2, 0.7 * flat, 0.9]) + np.array([0.0, 0.9, 0.0])
    pos = (c + rng.uniform(-0.08, 0.08, (n, 3, 3))).astype(np.float32).reshape(-1, 3)
    return pos, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def doubled_mesh(n, seed):
    """every triangle twice (the same three vertices): pairs of equal centroids"""
    pos, tris = random_mesh((n + 1) // 2, seed)
    return pos, np.repeat(tris, 2, axis=0)[:n].copy()


def one_centroid_mesh(n):
    """n copies of one triangle: every centroid equal, no extent on any axis"""
    pos = np.array([[-0.5, 0.4, 0.0], [0.5, 0.4, 0.1], [0.0, 1.3, -0.1]], np.float32)
    return pos, np.tile(np.array([[0, 1, 2]], np.int32), (n, 1))


def median_tree(pos, tris, leaf, node_base=0, leaf_base=0):
    """A median-split BLAS over all triangles, leaves of at most `leaf`, numbered in walk order.
    Returns (links {left, right, first, count, skipIndex}, triangle ids in leaf order)."""
    cent = pos[tris].astype(np.float64).mean(axis=1)
    out, order = [], []

    def rec(ids, after):
        i = len(out)
        out.append(None)
        if len(ids) <= leaf:
            out[i] = [-1, -1, leaf_base + len(order), len(ids), after]
            order.extend(ids)
            return
        c = cent[ids]
        ax = int(np.argmax(c.max(axis=0) - c.min(axis=0)))
        ids = [ids[k] for k in np.argsort(c[:, ax], kind="stable")]
        h = len(ids) // 2
        out[i] = [node_base + i + 1, None, -1, 0, after]
        # the right child's index is known once the left subtree is out: nodes of a subtree of m triangles are not known in advance
        mark = len(out)
        rec(ids[:h], None)
        r = len(out)
        for k in range(mark, r):                       # skip links that leave the left subtree point at the right child
            if out[k][4] is None:
                out[k][4] = node_base + r
        out[i][1] = node_base + r
        rec(ids[h:], after)

    rec(list(range(len(tris))), -1)
    arr = np.array(out, np.int32).reshape(-1, 5)
    return {f: arr[:, k].copy() for k, f in enumerate(("left", "right", "first", "count", "skipIndex"))}, np.array(order, np.int32)


# (name, mesh, leaf size of the uploaded median-split tree): the hand-made node ranges of the leaf-limit tests
def tight_cases():
    return [
        ("roomy_leaf2", random_mesh(97, 21), 2),
        ("leaf6", random_mesh(200, 22), 6),
        ("leaf10", random_mesh(200, 23), 10),
        ("leaf10_flat", random_mesh(150, 24, flat=0.05), 10),
        ("leaf14_full", random_mesh(224, 25), 14),
        ("leaf14_doubled", doubled_mesh(112, 26), 14),
    ]
