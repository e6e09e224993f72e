"""The yardstick of tests/test_rebuild.py, independent of the code under test: a numpy / plain-Python restatement of the tree that
pt_scene_rebuild_tree builds (include/pt_api.h: "Tree rebuild").

    centroid box -> quantised coordinates -> 30-bit Morton code -> key = morton << 32 | prim -> sorted order
    -> the binary radix tree over the sorted keys -> leaves of two -> numbering -> the refs of `nodes` and `quad`

Every float32 operation rounds once, as the device's do (no contraction, correctly rounded divide).  The radix tree is built top
down here (split a range at the highest bit in which its first and last key differ); the device builds the same tree bottom up, one
thread per internal node (Karras 2012).  The tree over a set of distinct keys is unique, so the two must agree.

Raw node v: v < n - 1 is the internal node whose range starts or ends at sorted triangle v (Karras' numbering: the left child of a
split at g is internal node g, the right child g + 1; the root is 0), v >= n - 1 is the leaf of sorted triangle v - (n - 1)."""
import bisect

import numpy as np

from dynamic_ref import max2, min2

F = np.float32
DEAD = -1


def centroids(pos):
    """(n, 3) float32: 0.5 * (box min + box max) of every triangle of pos (n, 3, 3)."""
    p = np.ascontiguousarray(pos, F).reshape(-1, 3, 3)
    mn = min2(p[:, 0], min2(p[:, 1], p[:, 2]))
    mx = max2(p[:, 0], max2(p[:, 1], p[:, 2]))
    c = F(0.5) * (mn + mx)
    assert c.dtype == F
    return c


def quantise(c):
    """(n, 3) int64 in 0..1023: the centroid's cell in the box of all centroids, 0 on an axis of no extent."""
    lo, hi = c.min(0), c.max(0)
    ext = hi - lo
    q = np.zeros(c.shape, np.int64)
    for a in range(3):
        if ext[a] > 0:
            x = ((c[:, a] - lo[a]) / ext[a]) * F(1024.0)
            assert x.dtype == F
            q[:, a] = np.minimum(1023, x.astype(np.int64))
    return q


def morton30(q):
    """Bit 3k + 2 from bit k of q_x, 3k + 1 from q_y, 3k from q_z."""
    m = np.zeros(len(q), np.uint64)
    for k in range(10):
        for a, off in ((0, 2), (1, 1), (2, 0)):
            m |= (((q[:, a] >> k) & 1).astype(np.uint64)) << np.uint64(3 * k + off)
    return m


def keys_of(pos):
    """(n,) uint64, unsorted: morton << 32 | prim."""
    c = centroids(pos)
    return (morton30(quantise(c)) << np.uint64(32)) | np.arange(len(c), dtype=np.uint64)


def sorted_keys(pos):
    return np.sort(keys_of(pos))


def prim_order(keys):
    """Tree order: the prim of every sorted key."""
    return (keys & np.uint64(0xffffffff)).astype(np.int64)


def radix_tree(keys):
    """child (n - 1, 2) raw ids, rng (n - 1, 2) first / last sorted triangle, for n >= 2 sorted distinct keys."""
    k = [int(x) for x in keys]
    n = len(k)
    assert n >= 2 and all(k[i] < k[i + 1] for i in range(n - 1))
    child = np.full((n - 1, 2), -1, np.int64)
    rng = np.zeros((n - 1, 2), np.int64)
    todo = [(0, 0, n - 1)]
    while todo:
        me, f, l = todo.pop()
        b = (k[f] ^ k[l]).bit_length() - 1                 # the highest bit in which the range differs
        pivot = ((k[f] >> b) | 1) << b                     # the smallest key of the range's prefix with that bit set
        g = bisect.bisect_left(k, pivot, f, l + 1) - 1      # last triangle of the left part
        assert f <= g < l
        rng[me] = (f, l)
        for side, (cf, cl, idx) in enumerate(((f, g, g), (g + 1, l, g + 1))):
            if cf == cl:
                child[me, side] = (n - 1) + cf
            else:
                child[me, side] = idx
                todo.append((idx, cf, cl))
    return child, rng


def build(keys):
    """The whole pinned topology for the sorted keys.  A dict:
    prim (n,), n_bn, n_wide, n_quad, depth, quad_depth, bn (n_bn, 4), order (n_bn,), level_start, wide_bn (n_wide, 2), quad_bn (n_quad, 4),
    node_refs (n_wide, 2) int32, quad_refs (n_quad, 4) int32."""
    n = len(keys)
    out = {"prim": prim_order(keys)}
    if n <= 2:      # the single-leaf scene (host/accel_build.cpp)
        leaf = ~n
        out.update(n_bn=1, n_wide=1, n_quad=1, depth=0, quad_depth=0, bn=np.array([[-1, -1, 0, n]]), order=np.array([0]), level_start=[0, 1],
                   wide_bn=np.array([[0, 0]]), quad_bn=np.array([[0, -1, -1, -1]]), node_refs=np.array([[leaf, -1]], np.int32),
                   quad_refs=np.array([[leaf, -1, -1, -1]], np.int32))
        return out
    child, rng = radix_tree(keys)
    I, N = n - 1, 2 * n - 1
    size = rng[:, 1] - rng[:, 0] + 1
    interior = np.zeros(N, bool)
    interior[:I] = size > 2
    live = np.ones(N, bool)
    for v in range(I):
        if size[v] == 2:
            live[child[v]] = False      # the two singletons under a leaf of two
    # depth from the root, height from the leaves
    depth = np.zeros(N, np.int64)
    height = np.zeros(N, np.int64)
    walk, stack = [], [0]
    while stack:
        v = stack.pop()
        walk.append(v)
        if interior[v]:
            for c in child[v]:
                depth[c] = depth[v] + 1
                stack.append(int(c))
    for v in reversed(walk):      # a node comes after its parent in `walk`
        if interior[v]:
            height[v] = 1 + max(height[child[v, 0]], height[child[v, 1]])
    # numbering: rank among the live / the interior raw nodes; 4-wide nodes by a stable sort on depth / 2
    newid = np.cumsum(live) - live
    widx = np.cumsum(interior) - interior
    is_quad = interior & (depth % 2 == 0)
    qraw = np.array(sorted(np.nonzero(is_quad)[0], key=lambda v: depth[v] // 2), np.int64)      # sorted() is stable
    qidx = np.full(N, -1, np.int64)
    qidx[qraw] = np.arange(len(qraw))

    def leaf_ref(c):
        return ~(((c - I) << 3) | 1) if c >= I else ~((int(rng[c, 0]) << 3) | 2)

    n_bn, n_wide, n_quad = int(live.sum()), int(interior.sum()), len(qraw)
    bn = np.zeros((n_bn, 4), np.int64)
    wide_bn, node_refs = np.zeros((n_wide, 2), np.int64), np.zeros((n_wide, 2), np.int32)
    quad_bn, quad_refs = np.full((n_quad, 4), -1, np.int64), np.full((n_quad, 4), -1, np.int32)
    for v in np.nonzero(live)[0]:
        v = int(v)
        if v >= I:
            bn[newid[v]] = (-1, -1, v - I, 1)
        elif not interior[v]:
            bn[newid[v]] = (-1, -1, rng[v, 0], 2)
        else:
            l, r = (int(c) for c in child[v])
            bn[newid[v]] = (newid[l], newid[r], 0, 0)
            wide_bn[widx[v]] = (newid[l], newid[r])
            node_refs[widx[v]] = [widx[c] if interior[c] else leaf_ref(c) for c in (l, r)]
            if is_quad[v]:
                ch = []
                for c in (l, r):
                    ch += [int(g) for g in child[c]] if interior[c] else [c]
                for k, c in enumerate(ch):
                    quad_bn[qidx[v], k] = newid[c]
                    quad_refs[qidx[v], k] = qidx[c] if interior[c] else leaf_ref(c)
    hl = height[live]
    top = int(hl.max())
    order = np.argsort(hl, kind="stable")      # builder nodes by height, ascending index within a height
    level_start = [int((hl < h).sum()) for h in range(top + 2)]
    out.update(n_bn=n_bn, n_wide=n_wide, n_quad=n_quad, depth=int(depth[live].max()), quad_depth=int(depth[qraw].max() // 2), bn=bn, order=order,
               level_start=level_start, wide_bn=wide_bn, quad_bn=quad_bn, node_refs=node_refs, quad_refs=quad_refs)
    return out


def walk_depths(nodes_arr, quad_arr):
    """(deepest node of the binary tree, deepest level of the 4-wide tree) from the downloaded arrays, the root at 0; a leaf of the
    binary tree counts as a node, as in the host build."""
    refs = np.ascontiguousarray(nodes_arr).reshape(-1, 16)[:, 12:14].view(np.int32)
    qrefs = np.ascontiguousarray(quad_arr).reshape(-1, 16)[:, 4:8].view(np.int32)
    single = refs[0, 0] < 0 and refs[0, 1] == -1
    deep, stack = 0, [(0, 0)]
    while stack and not single:
        w, d = stack.pop()
        for ref in refs[w]:
            deep = max(deep, d + 1)
            if ref >= 0:
                stack.append((int(ref), d + 1))
    qdeep, stack = 0, [(0, 0)]
    while stack:
        i, d = stack.pop()
        qdeep = max(qdeep, d)
        stack += [(int(ref), d + 1) for ref in qrefs[i] if ref >= 0]
    return deep, qdeep
