"""The yardstick of tests/test_rebuild_budget.py, independent of the code under test: the sort keys of pt_scene_rebuild_tree_ex
(include/pt_api.h: "Tree rebuild with a depth budget and two size classes") stated in numpy / plain Python and
handed to rebuild_ref.build, which builds the pinned topology over any sorted distinct keys.

    two size classes   large_i = ext_i > f * E;  each class quantises in its own centroid box;  key = large << 62 | morton << 32 | prim
    depth budget D     over the sorted keys: the radix tree, q(v) = depth(v) + clog2(size(v)); every triangle under a topmost v over more
                       than two triangles with q(v) >= D gets the key (key >> low << low) | rank in v, low = bit length of first ^ last of v

The budget is stated twice.  bottom_up_keys is the construction above (the device's, one walk up the parent links per triangle);
top_down_tree never forms a key: it splits a range as rebuild_ref.radix_tree does until depth + clog2(size) >= D and on the local rank
from there on.  tests/test_rebuild_budget.py asserts on the CPU that the two give the same tree.

Every float32 operation rounds once, as in rebuild_ref.  The prims of the tree order come from the ORIGINAL sorted keys: a rewritten
key no longer carries its prim."""
import bisect

import numpy as np

import rebuild_ref as B
from dynamic_ref import max2, min2

F = np.float32
DEFAULT_BUDGET, DEFAULT_FRACTION = 26, 0.0625


def clog2(m):
    """Bit length of m - 1: the depth of a balanced binary tree over m leaves."""
    return (int(m) - 1).bit_length()


def large_mask(pos, f):
    """(n,) bool: the triangle's own box is longer than f times the longest side of the box of all centroids."""
    p = np.ascontiguousarray(pos, F).reshape(-1, 3, 3)
    if not f > 0:
        return np.zeros(len(p), bool)
    c = B.centroids(p)
    E = (c.max(0) - c.min(0)).max()
    mn = min2(p[:, 0], min2(p[:, 1], p[:, 2]))
    mx = max2(p[:, 0], max2(p[:, 1], p[:, 2]))
    ext = (mx - mn).max(1)
    bound = F(f) * E
    assert ext.dtype == F and bound.dtype == F
    return ext > bound


def class_keys(pos, f):
    """(n,) uint64, unsorted: large << 62 | morton in the class's own centroid box << 32 | prim.  f = 0: rebuild_ref.keys_of."""
    if not f > 0:
        return B.keys_of(pos)
    c = B.centroids(pos)
    large = large_mask(pos, f)
    m = np.zeros(len(c), np.uint64)
    for cls in (False, True):
        sel = large == cls
        if sel.any():
            m[sel] = B.morton30(B.quantise(c[sel]))      # quantise takes the box of the centroids it is given
    return (large.astype(np.uint64) << np.uint64(62)) | (m << np.uint64(32)) | np.arange(len(c), dtype=np.uint64)


def _parents_and_depths(child, n):
    I = n - 1
    parent = np.full(2 * n - 1, -1, np.int64)
    for v in range(I):
        parent[child[v]] = v
    depth = np.zeros(2 * n - 1, np.int64)
    for v in range(2 * n - 1):
        p, d = parent[v], 0
        while p >= 0:
            p, d = parent[p], d + 1
        depth[v] = d
    return parent, depth


def bottom_up_keys(keys, D):
    """The new sorted keys for budget D over the sorted distinct keys `keys` (n >= 3 and D > 0, else a copy)."""
    k = [int(x) for x in keys]
    n = len(k)
    if D <= 0 or n < 3:
        return np.array(k, np.uint64)
    child, rng = B.radix_tree(keys)
    parent, depth = _parents_and_depths(child, n)
    out = list(k)
    for i in range(n):
        top, p = -1, parent[(n - 1) + i]
        while p >= 0:
            size = int(rng[p, 1] - rng[p, 0]) + 1
            if size > 2 and depth[p] + clog2(size) >= D:
                top = p
            p = parent[p]
        if top >= 0:
            f, l = int(rng[top, 0]), int(rng[top, 1])
            low = (k[f] ^ k[l]).bit_length()
            out[i] = ((k[i] >> low) << low) | (i - f)
    assert all(out[i] < out[i + 1] for i in range(n - 1))
    return np.array(out, np.uint64)


def top_down_tree(keys, D):
    """(child, rng) in rebuild_ref.radix_tree's numbering, for budget D, without new keys."""
    k = [int(x) for x in keys]
    n = len(k)
    child = np.full((n - 1, 2), -1, np.int64)
    rng = np.zeros((n - 1, 2), np.int64)
    todo = [(0, 0, n - 1, 0, None)]
    while todo:
        me, f, l, d, base = todo.pop()
        size = l - f + 1
        if base is None and D > 0 and size > 2 and d + clog2(size) >= D:
            base = f      # from here on the triangles are told apart by their rank in this range
        if base is None:
            b = (k[f] ^ k[l]).bit_length() - 1
            g = bisect.bisect_left(k, ((k[f] >> b) | 1) << b, f, l + 1) - 1
        else:
            a, z = f - base, l - base
            b = (a ^ z).bit_length() - 1
            g = base + (((a >> b) | 1) << b) - 1
        assert f <= g < l
        rng[me] = (f, l)
        for side, (cf, cl, idx) in enumerate(((f, g, g), (g + 1, l, g + 1))):
            if cf == cl:
                child[me, side] = (n - 1) + cf
            else:
                child[me, side] = idx
                todo.append((idx, cf, cl, d + 1, base))
    return child, rng


def build(pos, D=DEFAULT_BUDGET, f=DEFAULT_FRACTION):
    """rebuild_ref.build's dict for pt_scene_rebuild_tree_ex(pos; D, f), with the report: n_large, n_flattened_tris."""
    sorted_keys = np.sort(class_keys(pos, f))
    new = bottom_up_keys(sorted_keys, D)
    t = B.build(new)
    t["prim"] = B.prim_order(sorted_keys)
    t["n_large"] = int(large_mask(pos, f).sum())
    t["n_flattened_tris"] = int((new != sorted_keys).sum())
    return t


# ---- the chain scene: 72 triangles whose Morton tree is deeper than the kernels' stacks ----------------------------------------------
CHAIN_N = 72
CHAIN_OFFSET = (-16.0, 4.0, 40.0)      # the far corner cell's triangles sit at (0, 20, 56), in front of the camera below
CHAIN_CAMERA_POS = (0.0, 20.25, 59.0)


def chain_centres():
    """(72, 3) float32 box centres q / 64 + CHAIN_OFFSET, q in cells of 0 .. 1024, by index in `tris` order: 0, 1, 2, 4, .. 64 in cell
    (0, 0, 0) (a chain in the prim bits), the next thirty indices at the Morton codes 1 << j (a chain in the Morton bits), the rest in the
    far corner cell.  Every value is a multiple of 1 / 64 below 64: exact in float32, and so are the quantised cells."""
    origin = (0, 1, 2, 4, 8, 16, 32, 64)
    others = [i for i in range(CHAIN_N) if i not in origin]
    q = np.full((CHAIN_N, 3), 1024, np.int64)
    q[list(origin)] = 0
    for j, i in enumerate(others[:30]):
        q[i] = 0
        q[i, {2: 0, 1: 1, 0: 2}[j % 3]] = 1 << (j // 3)
    c = q.astype(np.float64) / 64.0 + np.asarray(CHAIN_OFFSET)
    assert (c.astype(F) == c).all()
    return c.astype(F)


def tris_at(centres, size=1.0):
    """tests/test_rebuild.py: _tris_at — (n, 3, 3) float32, a triangle around every centre whose box centre is the centre itself."""
    c = np.asarray(centres, F).reshape(-1, 1, 3)
    return (c + F(size) * F([[-1, -1, -1], [1, -1, 1], [-1, 1, 1]])[None]).astype(F)


def chain_positions():
    return tris_at(chain_centres(), 1.0)
