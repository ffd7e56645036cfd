"""Plain numpy restatement of the trees the device-side LBVH rebuild must produce (hrt_bvh.hip: TLAS rebuild of
hrt_scene_update_instances, mesh-BLAS rebuild of hrt_scene_update_positions) and of the numbers HRT_REBUILD_AUTO decides by.
Written from the contract in include/hip_raytrace.h and the comments of the kernels; it calls nothing of the library.

  centroid   instance: 0.5f * (worldBoundsMin + worldBoundsMax); triangle: ((a + b) + c) / 3.f; float32, per axis
  bounds     per-axis min / max over the centroids that are not NaN; an axis without one has no extent (NaN here)
  keys       ext = the longest extent (a NaN extent is ignored); 10 bits per axis by quant10(c, lo, lo + ext); 30-bit Morton key,
             x in the highest lane
  order      stable sort by key: equal keys keep item order
  tree       Karras 2012 over the sorted items, equal keys told apart by position: delta = 32 + clz(a ^ b)
  collapse   a node becomes a leaf when its subtree holds <= limit items and its parent's more
  limit      TLAS 2; BLAS the smallest of 4..14 whose tree (2 leaves - 1 nodes) fits the node range, else "does not fit"
  emission   walk order: left child at i + 1, skipIndex = the node after the subtree (-1 at the end), right = the other child

Boxes are not restated here (the refit restatements of tests/test_bvh_update_gpu.py do that)."""
import numpy as np

F32 = np.float32
DOES_NOT_FIT = None


# ------------------------------------------------------------------ keys
def instance_centroids(inst):
    """(n, 3) float32 from a structured instance array (worldBoundsMin / worldBoundsMax with X, Y, Z)."""
    with np.errstate(all="ignore"):
        return np.stack([F32(0.5) * (inst["worldBoundsMin"][f].astype(F32) + inst["worldBoundsMax"][f].astype(F32)) for f in "XYZ"], axis=1)


def triangle_centroids(pos, tris, items):
    """(n, 3) float32: pos (nv, 3) float32, tris (nt, 3) int, items = triangle ids in item order."""
    v = pos.astype(F32)[np.asarray(tris)[np.asarray(items)]]                       # (n, 3 vertices, 3 axes)
    with np.errstate(all="ignore"):
        return ((v[:, 0] + v[:, 1]) + v[:, 2]) / F32(3.0)


def centroid_bounds(cent):
    """(lo[3], hi[3]) float32; NaN on an axis where every centroid is NaN."""
    lo, hi = np.full(3, np.nan, F32), np.full(3, np.nan, F32)
    for k in range(3):
        c = cent[:, k]
        c = c[~np.isnan(c)]
        if c.size:
            lo[k], hi[k] = c.min(), c.max()
    return lo, hi


def quant10(c, lo, hi):
    c, lo, hi = F32(c), F32(lo), F32(hi)
    with np.errstate(all="ignore"):
        ext = F32(hi - lo)
        n = F32(F32(c - lo) / ext) if ext > 0 else F32(0.0)
        if not (n > 0):
            return 0
        s = F32(n * F32(1024.0))
        return 1023 if s >= F32(1023.0) else int(s)


def _spread3(v):
    out = 0
    for b in range(10):
        out |= ((v >> b) & 1) << (3 * b)
    return out


def morton_keys(cent):
    lo, hi = centroid_bounds(cent)
    with np.errstate(all="ignore"):
        e = (hi - lo).astype(F32)
    ext = F32(np.nan)
    for k in (2, 1, 0):                                      # max(ex, max(ey, ez)) with a NaN operand dropped
        if not np.isnan(e[k]) and (np.isnan(ext) or e[k] > ext):
            ext = e[k]
    keys = np.zeros(len(cent), np.uint32)
    with np.errstate(all="ignore"):
        top = [F32(lo[k] + ext) for k in range(3)]
    for i, c in enumerate(cent):
        x, y, z = (quant10(c[k], lo[k], top[k]) for k in range(3))
        keys[i] = (_spread3(x) << 2) | (_spread3(y) << 1) | _spread3(z)
    return keys


def sort_items(keys):
    """Stable: positions of the items in sorted order."""
    return np.argsort(np.asarray(keys, np.uint32), kind="stable")


# ------------------------------------------------------------------ Karras 2012
def _clz32(x):
    return 32 - int(x).bit_length()


def karras(keys):
    """keys: sorted.  Inner node j of the L - 1: (rngA, rngB, split).  Node 0 is the root."""
    keys = [int(k) for k in keys]
    L = len(keys)

    def delta(a, b):
        if b < 0 or b >= L:
            return -1
        return _clz32(keys[a] ^ keys[b]) if keys[a] != keys[b] else 32 + _clz32(a ^ b)

    A, B, G = [0] * max(L - 1, 0), [0] * max(L - 1, 0), [0] * max(L - 1, 0)
    for j in range(L - 1):
        d = 1 if delta(j, j + 1) - delta(j, j - 1) >= 0 else -1
        dmin = delta(j, j - d)
        lmax = 2
        while delta(j, j + lmax * d) > dmin:
            lmax <<= 1
        l, t = 0, lmax >> 1
        while t >= 1:
            if delta(j, j + (l + t) * d) > dmin:
                l += t
            t >>= 1
        e = j + l * d
        dnode = delta(j, e)
        s, t = 0, l
        while True:
            t = (t + 1) >> 1
            if delta(j, j + (s + t) * d) > dnode:
                s += t
            if t <= 1:
                break
        A[j], B[j], G[j] = min(j, e), max(j, e), j + s * d + min(d, 0)
    return A, B, G


def emit(keys, limit, node_base=0, leaf_base=0):
    """The emitted tree over sorted `keys` as link arrays {left, right, first, count, skipIndex} (int32, node_base / leaf_base added
    the way the reference-layout arrays carry them), in walk order."""
    L = len(keys)
    A, B, G = karras(keys)
    out = []

    def rec(a, b, inner):
        i = len(out)
        out.append(None)
        if b - a + 1 <= limit:
            out[i] = [-1, -1, leaf_base + a, b - a + 1, -1]
        else:
            g = G[inner]
            assert A[inner] == a and B[inner] == b
            rec(a, g, g)                       # Karras: the left child is inner node g (or leaf g), the right one g + 1
            r = len(out)
            rec(g + 1, b, g + 1)
            out[i] = [node_base + i + 1, node_base + r, -1, 0, -1]
        return i

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
    rec(0, L - 1, 0)
    n = len(out)
    # skip links: the node after the subtree
    end = [0] * n
    for i in range(n - 1, -1, -1):
        end[i] = i + 1 if out[i][3] > 0 else end[out[i][1] - node_base]
    for i in range(n):
        out[i][4] = -1 if end[i] >= n else node_base + end[i]
    arr = np.array(out, np.int32).reshape(-1, 5)
    return {f: arr[:, k].copy() for k, f in enumerate(("left", "right", "first", "count", "skipIndex"))}


def emit_topdown(keys, limit, node_base=0, leaf_base=0):
    """The second formulation: recursion over the unique 62-bit integers key << 32 | sorted position; a range splits where its highest
    differing bit flips and collapses at `limit`."""
    code = [(int(k) << 32) | i for i, k in enumerate(keys)]
    out = []

    def rec(a, b):
        i = len(out)
        out.append(None)
        if b - a + 1 <= limit:
            out[i] = [-1, -1, leaf_base + a, b - a + 1, None]
            return
        bit = (code[a] ^ code[b]).bit_length() - 1
        g = a
        while not (code[g + 1] >> bit) & 1:
            g += 1
        rec(a, g)
        r = len(out)
        rec(g + 1, b)
        out[i] = [node_base + i + 1, node_base + r, -1, 0, None]

    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
    rec(0, len(code) - 1)
    n = len(out)

    def close(i, after):
        out[i][4] = after
        if out[i][3] == 0:
            l, r = out[i][0] - node_base, out[i][1] - node_base
            close(l, node_base + r)
            close(r, after)
    close(0, -1)
    arr = np.array(out, np.int32).reshape(-1, 5)
    return {f: arr[:, k].copy() for k, f in enumerate(("left", "right", "first", "count", "skipIndex"))}


# ------------------------------------------------------------------ the two trees
def tlas(inst):
    """(links, tlasInstanceIndices) for a structured instance array."""
    n = len(inst)
    if n <= 2:                                           # the root is the only node, instances in id order
        links = {"left": [-1], "right": [-1], "first": [0], "count": [n], "skipIndex": [-1]}
        return {k: np.array(v, np.int32) for k, v in links.items()}, np.arange(n, dtype=np.int32)
    keys = morton_keys(instance_centroids(inst))
    order = sort_items(keys)
    return emit(keys[order], 2), order.astype(np.int32)


def blas(pos, tris, items, node_cap, node_base=0, leaf_base=0):
    """One mesh: (limit, links over the whole node range, leaf region, blasNodeCount), or (DOES_NOT_FIT, None, None, None).
    items = the instance's own item list triPrimIdx[primIndexFirst : primIndexFirst + primIndexCount]."""
    items = np.asarray(items, np.int32)
    keys = morton_keys(triangle_centroids(pos, tris, items))
    order = sort_items(keys)
    skeys = keys[order]
    for limit in range(4, 15):
        links = emit(skeys, limit, node_base, leaf_base)
        n = len(links["count"])
        if n <= node_cap:
            tail = node_cap - n                          # behind the emitted tree: owned by nobody
            for f in links:
                links[f] = np.concatenate([links[f], np.full(tail, 0 if f == "count" else -1, np.int32)])
            return limit, links, items[order], n
    return DOES_NOT_FIT, None, None, None


LINK_FIELDS = ("left", "right", "first", "count", "skipIndex")


def links_of(nodes):
    """The link fields of a structured hrt_bvh_node array, comparable with what emit() returns."""
    return {f: np.asarray(nodes[f], np.int32) for f in LINK_FIELDS}


def check_tree(links, n_items, limit, node_base=0, leaf_base=0, n_nodes=None):
    """The validity checks of the suite, limit-aware: every node on the walk, every item in exactly one leaf, leaves of at most
    `limit`, 2 leaves - 1 nodes.  Returns the leaf sizes in walk order."""
    n = len(links["count"]) if n_nodes is None else n_nodes
    cur, seen, slots, sizes = node_base, 0, [], []
    while cur != -1:
        i = cur - node_base
        assert 0 <= i < n and seen < n, "walk leaves the tree or does not end"
        seen += 1
        c = int(links["count"][i])
        if c > 0:
            assert c <= limit and links["left"][i] == -1 and links["right"][i] == -1
            slots.extend(range(int(links["first"][i]), int(links["first"][i]) + c))
            sizes.append(c)
            cur = int(links["skipIndex"][i])
        else:
            assert links["left"][i] == cur + 1 and links["right"][i] == links["skipIndex"][links["left"][i] - node_base]
            cur = int(links["left"][i])
    assert seen == n == 2 * len(sizes) - 1, "every node is on the walk, 2 leaves - 1 nodes"
    assert slots == list(range(leaf_base, leaf_base + n_items)), "every item in exactly one leaf"
    return sizes


# ------------------------------------------------------------------ stats
def node_areas(lo, hi):
    """float32 2 (dx dy + dy dz + dz dx) per node; lo, hi (n, 3) float32."""
    with np.errstate(all="ignore"):
        d = (hi.astype(F32) - lo.astype(F32)).astype(F32)
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        return (F32(2.0) * (((dx * dy).astype(F32) + (dy * dz).astype(F32)).astype(F32) + (dz * dx).astype(F32)).astype(F32)).astype(F32)


def boxes_of(nodes):
    lo = np.stack([nodes["boundsMin"][f] for f in "XYZ"], axis=1).astype(F32)
    hi = np.stack([nodes["boundsMax"][f] for f in "XYZ"], axis=1).astype(F32)
    return lo, hi


def _tree_sum(v, width):
    s = np.zeros(width, F32)
    s[:len(v)] = v
    d = width // 2
    with np.errstate(all="ignore"):
        while d > 0:
            s[:d] = (s[:d] + s[d:2 * d]).astype(F32)
            d //= 2
    return s[0]


def sah_cost(nodes):
    """sum(area x (leaf ? count : 1)) / area(root) in the device's two-stage float32 summation order (every node linked)."""
    lo, hi = boxes_of(nodes)
    sa = node_areas(lo, hi)
    w = np.where(nodes["count"] > 0, nodes["count"], 1).astype(F32)
    with np.errstate(all="ignore"):
        term = (sa * w).astype(F32)
        partial = [_tree_sum(term[b:b + 256], 256) for b in range(0, len(term), 256)]
        acc = np.zeros(1024, F32)
        for i, p in enumerate(partial):
            acc[i % 1024] = F32(acc[i % 1024] + p)
        total = _tree_sum(acc, 1024)
        return F32(total / sa[0]) if sa[0] > 0 else F32(0.0)


def growth(area_now, area_base):
    """exp(mean(log(float32(now / base)))) over nodes with both areas > 0, in float64; 1 when there is none."""
    a, b = np.asarray(area_now, F32), np.asarray(area_base, F32)
    with np.errstate(all="ignore"):
        m = (a > 0) & (b > 0)
        if not m.any():
            return 1.0
        q = (a[m] / b[m]).astype(F32).astype(np.float64)
        return float(np.exp(np.mean(np.log(q))))
