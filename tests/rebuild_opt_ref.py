"""The yardstick of tests/test_rebuild_opt.py, independent of the code under test: the treelet restructuring passes of
pt_scene_rebuild_tree_opt (include/pt_api.h: "Tree rebuild with treelet restructuring"; Karras and Aila 2013)
stated in numpy / plain Python over the radix tree of the existing yardsticks, and the numbering of rebuild_ref.build restated for an
arbitrary `child` array.

    keys      rebuild_budget_ref.class_keys -> sort -> bottom_up_keys -> rebuild_ref.radix_tree          (pt_scene_rebuild_tree_ex)
    nodes     raw nodes of the radix tree.  A LEAF is a singleton or an internal node over exactly two triangles; leaves are never
              opened, moved into or changed.  An INTERIOR node is an internal node over more than two triangles.
    boxes     singleton: min2 / max2 of its three vertices.  Leaf of two: min2 / max2 of (left child, right child).  Every other
              node: min2 / max2 of (left child, right child).  Subset S of a treelet's leaves: entry of the lowest bit, then min2 /
              max2 (so far, entry k) in ascending k.  area = 2 * (dx * dy + dy * dz + dz * dx), float32, every operation rounded once.
    one pass  heights (leaf = 0), depths and the depth of the tree are taken from the topology the pass starts from.  Interior nodes
              are processed in ascending start-of-pass height; nodes of one height are independent.  Per node v:
      1       box(v), h(v) = 1 + max h(children) from its current children
      2       L = [left, right]; while |L| < 7 and an entry is interior: the interior entry of largest area (the first of them in list
              order unless a later one is strictly larger) is replaced by its left child, its right child is appended, the node joins I.
              |L| < 3: nothing to do, and the treelet is not counted.
      3       a[S] = area of the box of S; c[singleton] = 0; c[S] = (S == full ? 0 : a[S]) + min over P of (c[P] + c[S \\ P]), P the proper
              subsets of S that contain S's lowest bit, in ascending numeric order, a later P only where strictly smaller.
              h[singleton k] = h(L[k]); h[S] = 1 + max(h[P], h[S \\ P]) for the chosen P.
      4       accept iff c[full] < area(I[0]) + area(I[1]) + ... (float32, in that order) and h[full] <= max(h(v), H_lim - depth(v));
              H_lim = D - 1 for a budget D > 0, else the depth of the tree this pass started from (deepest leaf, the root at 0).
      5       v is the node of `full`; the node of S has the node of P on the left and of S \\ P on the right; every other subset of two or
              more entries takes the next unused node of I in pre-order (node, left subtree, right subtree).  Boxes, heights, links.
    report    n_roots: treelets of >= 3 entries solved, n_restructured: treelets accepted, both summed over the passes.

The solve of a level is batched over its treelets with numpy (every element is the float32 operation named above); `solve_one` states
step 3 a second time for one treelet in plain Python, and tests/test_rebuild_opt.py states it a third time by enumeration."""
import math

import numpy as np

import rebuild_budget_ref as X
import rebuild_ref as B
from dynamic_ref import max2, min2, pad_hi, pad_lo

F = np.float32
DEFAULT_PASSES = 2
MAX_PASSES = 8
TREELET = 7


def area(lo, hi):
    """float32 area of boxes lo, hi (..., 3): dyn_area's expression."""
    d = (hi - lo).astype(F)
    d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
    a = F(2.0) * (d0 * d1 + d1 * d2 + d2 * d0)
    assert np.asarray(a).dtype == F
    return a


def partitions(S):
    """The proper subsets of S that contain its lowest bit, ascending."""
    low = S & -S
    rest = S ^ low
    out, sub = [], 0
    while sub != rest:
        out.append(low | sub)
        sub = (sub - rest) & rest
    return out


_PARTS = [np.array(partitions(S), np.int64) for S in range(1 << TREELET)]


def subset_boxes(llo, lhi, m):
    """(T, 2^m, 3) lo and hi of every subset of the m entries llo, lhi (T, m, 3): the lowest entry, then ascending."""
    T = llo.shape[0]
    lo, hi = np.zeros((T, 1 << m, 3), F), np.zeros((T, 1 << m, 3), F)
    for k in range(m):
        b = 1 << k
        lo[:, b], hi[:, b] = llo[:, k], lhi[:, k]
        if b > 1:
            lo[:, b + 1:2 * b] = min2(lo[:, 1:b], llo[:, k:k + 1])
            hi[:, b + 1:2 * b] = max2(hi[:, 1:b], lhi[:, k:k + 1])
    return lo, hi


def solve(llo, lhi, lh, m):
    """Step 3 for T treelets of m entries each: (a, c, part, h), arrays (T, 2^m)."""
    T, full = llo.shape[0], (1 << m) - 1
    lo, hi = subset_boxes(llo, lhi, m)
    a = area(lo, hi)
    c = np.zeros((T, 1 << m), F)
    part = np.zeros((T, 1 << m), np.int64)
    h = np.zeros((T, 1 << m), np.int64)
    rows = np.arange(T)
    for k in range(m):
        h[:, 1 << k] = lh[:, k]
    for S in range(1, full + 1):      # P and S \ P are below S
        P = _PARTS[S]
        if len(P) == 0:
            continue
        cand = c[:, P] + c[:, S ^ P]
        assert cand.dtype == F and not np.isnan(cand).any()
        j = np.argmin(cand, axis=1)      # the first of the smallest
        best = cand[rows, j]
        part[:, S] = P[j]
        c[:, S] = (F(0.0) if S == full else a[:, S]) + best
        h[:, S] = 1 + np.maximum(h[rows, part[:, S]], h[rows, S ^ part[:, S]])
    return a, c, part, h


def solve_one(llo, lhi, m):
    """Step 3 for one treelet in plain Python: (c[full], part) with the float32 operations one at a time."""
    full = (1 << m) - 1
    lo, hi = subset_boxes(np.asarray(llo, F)[None], np.asarray(lhi, F)[None], m)
    a = area(lo[0], hi[0])
    c, part = [F(0.0)] * (full + 1), [0] * (full + 1)
    for S in range(1, full + 1):
        best, best_p = None, 0
        for P in partitions(S):
            cand = F(c[P] + c[S ^ P])
            if best is None or cand < best:
                best, best_p = cand, P
        if best is not None:
            c[S], part[S] = F((F(0.0) if S == full else a[S]) + best), best_p
    return c[full], part


def _depth_height(child, interior):
    """depth (root 0) and height (leaf 0) of every raw node reached from the root, and the depth of the tree."""
    N = 2 * len(child) + 1
    depth, height = np.zeros(N, np.int64), np.zeros(N, np.int64)
    walk, stack = [], [0]
    while stack:
        v = stack.pop()
        walk.append(v)
        if interior[v]:
            for c in child[v]:
                depth[c] = depth[v] + 1
                stack.append(int(c))
    for v in reversed(walk):
        if interior[v]:
            height[v] = 1 + max(height[child[v, 0]], height[child[v, 1]])
    deepest = max(int(depth[v]) for v in walk if not interior[v])
    return depth, height, deepest


def leaf_boxes(pos_sorted, child, interior):
    """lo, hi (N, 3) float32 with the boxes of the singletons and of the leaves of two filled in."""
    n = len(pos_sorted)
    I, N = n - 1, 2 * n - 1
    p = np.ascontiguousarray(pos_sorted, F).reshape(-1, 3, 3)
    lo, hi = np.zeros((N, 3), F), np.zeros((N, 3), F)
    lo[I:] = min2(p[:, 0], min2(p[:, 1], p[:, 2]))
    hi[I:] = max2(p[:, 0], max2(p[:, 1], p[:, 2]))
    two = np.nonzero(~interior[:I])[0]
    lo[two] = min2(lo[child[two, 0]], lo[child[two, 1]])
    hi[two] = max2(hi[child[two, 0]], hi[child[two, 1]])
    return lo, hi


def one_pass(child, interior, lo, hi, D):
    """One restructuring pass, in place on child / lo / hi.  Returns (n_roots, n_restructured)."""
    depth, height, deepest = _depth_height(child, interior)
    h_lim = D - 1 if D > 0 else deepest
    hcur = np.zeros(len(depth), np.int64)      # leaves stay 0; an interior node's is written before it is read
    ar = area(lo, hi)                          # an interior node's is written before it is read
    I = len(child)
    roots = done = 0
    for level in range(1, int(height.max()) + 1):
        forms = {}
        for v in np.nonzero(interior[:I] & (height[:I] == level))[0]:
            v = int(v)
            l, r = int(child[v, 0]), int(child[v, 1])
            lo[v], hi[v] = min2(lo[l], lo[r]), max2(hi[l], hi[r])
            ar[v] = area(lo[v], hi[v])
            hcur[v] = 1 + max(hcur[l], hcur[r])
            L, Il = [l, r], []
            while len(L) < TREELET:
                pick = -1
                for k, e in enumerate(L):
                    if interior[e] and (pick < 0 or ar[e] > ar[L[pick]]):
                        pick = k
                if pick < 0:
                    break
                e = L[pick]
                Il.append(e)
                L[pick] = int(child[e, 0])
                L.append(int(child[e, 1]))
            if len(L) >= 3:
                forms.setdefault(len(L), []).append((v, L, Il))
        for m, group in forms.items():
            roots += len(group)
            Ls = np.array([L for _, L, _ in group], np.int64)
            a, c, part, h = solve(lo[Ls], hi[Ls], hcur[Ls], m)
            full = (1 << m) - 1
            for t, (v, L, Il) in enumerate(group):
                was = ar[Il[0]]
                for e in Il[1:]:
                    was = was + ar[e]
                assert was.dtype == F
                if not (c[t, full] < was and h[t, full] <= max(hcur[v], h_lim - depth[v])):
                    continue
                done += 1
                sub_lo, sub_hi = subset_boxes(lo[Ls[t]][None], hi[Ls[t]][None], m)
                nxt, stack = 0, [(full, -1, 0)]
                while stack:
                    S, pid, side = stack.pop()
                    single = S & (S - 1) == 0
                    if single:
                        node = L[S.bit_length() - 1]
                    elif pid < 0:
                        node = v
                    else:
                        node, nxt = Il[nxt], nxt + 1
                    if pid >= 0:
                        child[pid, side] = node
                    if not single:
                        if pid >= 0:
                            lo[node], hi[node], ar[node] = sub_lo[0, S], sub_hi[0, S], a[t, S]
                        hcur[node] = h[t, S]
                        P = int(part[t, S])
                        stack.append((S ^ P, node, 1))
                        stack.append((P, node, 0))
                assert nxt == len(Il)
    return roots, done


def interior_areas(child, interior, lo, hi):
    """Exact boxes of the interior nodes from the leaves up (lo, hi are rewritten): (raw ids in walk order, float32 areas)."""
    walk, stack = [], [0]
    while stack:
        v = stack.pop()
        if interior[v]:
            walk.append(v)
            stack += [int(c) for c in child[v]]
    for v in reversed(walk):
        lo[v], hi[v] = np.minimum(lo[child[v, 0]], lo[child[v, 1]]), np.maximum(hi[child[v, 0]], hi[child[v, 1]])
    w = np.array(walk, np.int64)
    return w, area(lo[w], hi[w])


def number(child, rng, interior_of_internal, n):
    """rebuild_ref.build's numbering for any topology `child` over the same leaves: rng is read only for a leaf of two's first
    triangle, interior_of_internal (n - 1,) says which internal nodes are interior."""
    I, N = n - 1, 2 * n - 1
    interior = np.zeros(N, bool)
    interior[:I] = interior_of_internal
    live = np.ones(N, bool)
    for v in range(I):
        if not interior[v]:
            live[child[v]] = False
    depth, height, _ = _depth_height(child, interior)
    newid = np.cumsum(live) - live
    widx = np.cumsum(interior) - interior
    is_quad = interior & (depth % 2 == 0)
    qraw = np.array(sorted(np.nonzero(is_quad)[0], key=lambda v: depth[v] // 2), np.int64)
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
    order = np.argsort(hl, kind="stable")
    level_start = [int((hl < h).sum()) for h in range(top + 2)]
    return dict(n_bn=n_bn, n_wide=n_wide, n_quad=n_quad, depth=int(depth[live].max()), quad_depth=int(depth[qraw].max() // 2), bn=bn, order=order,
                level_start=level_start, wide_bn=wide_bn, quad_bn=quad_bn, node_refs=node_refs, quad_refs=quad_refs)


def build(pos, D=X.DEFAULT_BUDGET, f=X.DEFAULT_FRACTION, passes=DEFAULT_PASSES, trace=None):
    """rebuild_ref.build's dict for pt_scene_rebuild_tree_opt(pos; D, f; passes) with the report (n_large, n_flattened_tris, n_roots,
    n_restructured) and the interior area sums: area_before / area_after, math.fsum of the float32 areas of the exact boxes of all
    interior nodes before the first and after the last pass, and nodes_area, the same sum over the boxes the `nodes` array holds
    (pad_lo / pad_hi of the exact box of every interior node but the root).  trace: a list that receives the area sum after each pass."""
    p = np.ascontiguousarray(pos, F).reshape(-1, 3, 3)
    n = len(p)
    sorted_keys = np.sort(X.class_keys(p, f))
    new = X.bottom_up_keys(sorted_keys, D)
    prim = B.prim_order(sorted_keys)
    report = dict(n_large=int(X.large_mask(p, f).sum()), n_flattened_tris=int((new != sorted_keys).sum()), n_roots=0, n_restructured=0)
    if n <= 2:      # the single-leaf scene: passes is ignored
        t = B.build(new)
        t.update(report, prim=prim, area_before=0.0, area_after=0.0, nodes_area=0.0)
        return t
    child, rng = B.radix_tree(new)
    I = n - 1
    interior = np.zeros(2 * n - 1, bool)
    interior[:I] = rng[:, 1] - rng[:, 0] > 1
    lo, hi = leaf_boxes(p[prim], child, interior)
    before = math.fsum(float(x) for x in interior_areas(child, interior, lo.copy(), hi.copy())[1])
    for _ in range(passes):
        roots, done = one_pass(child, interior, lo, hi, D)
        report["n_roots"] += roots
        report["n_restructured"] += done
        if trace is not None:
            trace.append(math.fsum(float(x) for x in interior_areas(child, interior, lo.copy(), hi.copy())[1]))
    t = number(child, rng, interior[:I], n)
    elo, ehi = lo.copy(), hi.copy()
    w, ar = interior_areas(child, interior, elo, ehi)
    t.update(report, prim=prim, area_before=before, area_after=math.fsum(float(x) for x in ar))
    t["nodes_area"] = math.fsum(float(x) for x in area(pad_lo(elo[w[1:]]), pad_hi(ehi[w[1:]]))) if len(w) > 1 else 0.0
    return t


def nodes_area(nodes_arr):
    """math.fsum of the float32 areas of the child boxes of `nodes` (16 floats per record: box of child 0, box of child 1, refs) whose
    child is itself a `nodes` record: every interior node but the root, once."""
    rec = np.ascontiguousarray(nodes_arr, F).reshape(-1, 16)
    refs = rec[:, 12:14].view(np.int32)
    total = []
    for side in (0, 1):
        sel = refs[:, side] >= 0
        total += [float(x) for x in area(rec[sel, 6 * side:6 * side + 3], rec[sel, 6 * side + 3:6 * side + 6])]
    return math.fsum(total)
