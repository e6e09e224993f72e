"""The scenes and CPU walkers of tests/test_deep_tree.py (pure numpy / plain Python, independent of the code under test; DESIGN.md
section 26).

The comb scene.  The chain scene of rebuild_budget_ref is deep, but every node on its chain has one leaf child, and trace_closest
(csrc/pt_trace.h) pushes only where both children are interior and both are hit: its stack stays near empty there.  The comb is a chain
whose every level has an interior sibling.  Morton-code placement as rebuild_budget_ref.chain_centres (cell q / 64 + CHAIN_OFFSET, bit b of
the code on axis {2: 0, 1: 1, 0: 2}[b % 3]):

    level j = 29 .. 2     three triangles at the codes (1 << j) | {0, 1, 2}: the right child of the chain's node at depth 29 - j
    codes 2 and 1         three coincident triangles each (told apart by their index in `tris`): two more levels in the Morton bits
    code 0                the triangles of index 80 + {0, 1, 2} and 80 + ((1 << k) | {0, 1, 2}), k = 2 .. 1 + index_levels: levels in the
                          index bits of the key (key = morton << 32 | index)
    three anchors         at cell (1024, 1024, 1024): the box of all centroids is the chain scene's

comb_positions(32) (index_levels = 1, 99 triangles) has binary depth 32 = pt_dbg_tree_limits' maximum and 4-wide depth 15, and every
node of its chain, depths 0 .. 30, has two interior children.  comb_positions(33) (102 triangles) is one level deeper: refused.
comb_positions(29) (90 triangles; single triangles at the codes 0, 1, 2) is the tree the comb started from: 29 / 14.
Every triangle is tris_at(centre, 8.0): its box is centre +- 8, and all centres but the anchors' lie within 8 + 1 / 64 of the origin cell,
so every box of the chain's side contains COMMON, a cube of side just under 8.  A ray that starts inside it enters every box at distance
0; trace_closest then takes the left child — the chain's side — first at every level and pushes the sibling: depth - 1 entries.

The walkers restate the CONTROL FLOW of trace_closest and of the 4-wide walk over the yardstick's topology (rebuild_ref.build's
node_refs / quad_refs) with the exact boxes of the positions and a float64 slab test.  They are an APPROXIMATION of the kernels'
arithmetic, as tools/stack_lab.cpp is (no padding or quantisation of the boxes, no reference leaf box, no parked leaves): good for an
upper figure of the stack, not for bits."""
import numpy as np

import rebuild_budget_ref as X

F = np.float32
AXIS_OF_BIT = {2: 0, 1: 1, 0: 2}
COMB_SIZE = 8.0
COMB_ANCHORS = 3
COMB_INDEX_BASE = 80      # the coincident triangles at code 0 have the indices 80, 81, 82 and 84, 85, 86 (and 88, 89, 90 in the 33-deep sibling)
# COMMON: what every box of the chain's side contains (centres are at most 8 + 1 / 64 from CHAIN_OFFSET on every axis)
COMMON_LO = np.asarray(X.CHAIN_OFFSET, np.float64) + (8.0 + 1.0 / 64.0 - COMB_SIZE)
COMMON_HI = np.asarray(X.CHAIN_OFFSET, np.float64) + COMB_SIZE
# The test camera of the comb: beyond the low corner of COMMON, looking along (2, 2, 1) / 3 (pitch = acos(2 / 3), yaw = 180 + atan(2)
# degrees).  Every triangle of tris_at faces it (normal (-1, -1, 1) / sqrt 3; Triangle::hit is one-sided), and its rays enter every box
# through a low face, the chain's side first or together with the sibling: the stack fills as it does for a ray that starts inside.
COMB_CAMERA_POS = (-30.0, -10.0, 35.0)
COMB_CAMERA_ROT = (0.0, 48.19, 243.435)


def cell_of_code(code):
    """The cell (qx, qy, qz) whose 30-bit Morton code is `code` (rebuild_ref.morton30's inverse)."""
    q = [0, 0, 0]
    for b in range(30):
        if (code >> b) & 1:
            q[AXIS_OF_BIT[b % 3]] |= 1 << (b // 3)
    return q


def comb_codes(depth):
    """(n,) list of Morton codes by index in `tris` order, -1 for an anchor; depth in (29, 32, 33)."""
    assert depth in (29, 32, 33)
    levels = [(1 << j) | k for j in range(2, 30) for k in (0, 1, 2)]
    if depth == 29:
        return [0, 1, 2] + levels + [-1] * COMB_ANCHORS
    at_zero = [COMB_INDEX_BASE + i for i in [0, 1, 2] + [(1 << k) | i for k in range(2, 2 + depth - 31) for i in (0, 1, 2)]]      # in the index bits of the key
    rest = [1] * 3 + [2] * 3 + levels + [-1] * COMB_ANCHORS
    n = len(at_zero) + len(rest)
    codes, it = [], iter(rest)
    for i in range(n):
        codes.append(0 if i in at_zero else next(it))
    return codes


def comb_centres(depth=32):
    codes = comb_codes(depth)
    q = np.array([[1024] * 3 if c < 0 else cell_of_code(c) for c in codes], np.int64)
    c = q.astype(np.float64) / 64.0 + np.asarray(X.CHAIN_OFFSET)
    assert (c.astype(F) == c).all()
    return c.astype(F)


def comb_positions(depth=32):
    """(n, 3, 3) float32: 99 triangles for depth 32, 102 for 33, 90 for 29."""
    return X.tris_at(comb_centres(depth), COMB_SIZE)


def other_face(pos, idx):
    """pos with vertices 1 and 2 of the listed triangles exchanged: the same boxes and centroids, hence the same tree, but those
    triangles face (1, 1, -1) / sqrt 3.  The tests turn the two lights round: a light that faces the way every other triangle faces
    lights none of them (Triangle::hit is one-sided)."""
    out = np.array(pos, F).reshape(-1, 3, 3)
    out[idx] = out[idx][:, [0, 2, 1]]
    return out


def comb_query_rays(seed, m):
    """2 m RAY8 records that start inside COMMON: m rays in unit normal directions with tmax 999999 (every 16th along an axis, the
    degenerate box test), then m segments to a point up to 40 away, tmax their length."""
    rs = np.random.RandomState(seed)
    o, a = (COMMON_LO + rs.uniform(0.02, 0.98, (m, 3)) * (COMMON_HI - COMMON_LO) for _ in range(2))
    d = rs.standard_normal((m, 3))
    d /= np.sqrt((d * d).sum(1, keepdims=True))
    d[::16] = np.eye(3)[np.arange(len(d[::16])) % 3] * np.where(np.arange(len(d[::16])) % 2 == 0, 1.0, -1.0)[:, None]
    seg = rs.standard_normal((m, 3))
    seg *= rs.uniform(1.0, 40.0, (m, 1)) / np.sqrt((seg * seg).sum(1, keepdims=True))
    ln = np.sqrt((seg * seg).sum(1, keepdims=True))
    rays = np.zeros((2 * m, 8), F)
    rays[:m, 0:3], rays[:m, 3:6], rays[:m, 7] = o, d, 999999.0
    rays[m:, 0:3], rays[m:, 3:6], rays[m:, 7] = a, seg / ln, ln[:, 0]
    return rays


COMB_LAST_ENTRY_PRIM = COMB_INDEX_BASE + 6


def comb_last_entry_rays(seed, m):
    """m RAY8 records whose closest hit is found through the LAST entry trace_closest can push on the 32-deep comb.  The six triangles at
    code 0 coincide; their plane touches COMMON only at a corner, so no ray from inside COMMON ever hits them.  These rays start
    1 / 512 in front of that plane (the next plane, code 1's, is 1 / (64 sqrt 3) away), at points of the triangle from which the line
    along -normal crosses COMMON, and head along -normal with a little jitter: inside every box of the chain's side from the start, into
    every sibling's box later, so 31 entries are pushed on the way down before the first triangle is tested; at the node over code 0 the
    walk goes left, to the indices 80, 81, 82, and pushes the indices 84, 85, 86 as its 31st entry.  All six tie in t and the largest
    index wins (Triangle::hit's tie rule): the hit is index 86 = COMB_LAST_ENTRY_PRIM, found only if that entry is kept.  (The triangle
    at code 5, index 7, lies in the same plane a sixty-fourth to the side; its index is lower.)"""
    rs = np.random.RandomState(seed)
    ab = rs.uniform(-2.0, -0.5, (m, 2))
    on_plane = np.concatenate([ab, 8.0 + ab.sum(1, keepdims=True)], 1)      # -x - y + z = 8 about the centre of cell 0
    normal = np.array([-1.0, -1.0, 1.0]) / np.sqrt(3.0)
    d = -normal + 0.05 * rs.standard_normal((m, 3))
    d /= np.sqrt((d * d).sum(1, keepdims=True))
    rays = np.zeros((m, 8), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 7] = np.asarray(X.CHAIN_OFFSET) + on_plane + normal / 512.0, d, 999999.0
    return rays


# ---- the yardstick's trees with boxes ----------------------------------------------------------------------------------------------
def _leaf_box(t, pos, ref):
    code = ~int(ref)
    p = pos[t["prim"][code >> 3:(code >> 3) + (code & 7)]].reshape(-1, 3).astype(np.float64)
    return p.min(0), p.max(0)


def child_boxes(t, pos, refs):
    """(lo, hi), each (len(refs), width, 3) float64: the exact box of every child of the tree `refs` (t["node_refs"] or t["quad_refs"]);
    a free slot (-1) gets an empty box."""
    pos = np.ascontiguousarray(pos, F).reshape(-1, 3, 3)
    n, w = refs.shape
    lo, hi = np.full((n, w, 3), np.inf), np.full((n, w, 3), -np.inf)
    done = np.zeros(n, bool)

    def fill(i):
        for k in range(w):
            ref = int(refs[i, k])
            if ref >= 0:
                if not done[ref]:
                    fill(ref)
                lo[i, k], hi[i, k] = lo[ref].min(0), hi[ref].max(0)
            elif ref != -1:
                lo[i, k], hi[i, k] = _leaf_box(t, pos, ref)
        done[i] = True

    fill(0)
    assert done.all()
    return lo, hi


def both_interior_path(node_refs):
    """The largest number of nodes with two interior children on one path from the root: what trace_closest's stack can hold at most,
    whatever the rays."""
    best = {}

    def count(i):
        if i not in best:
            l, r = (int(x) for x in node_refs[i])
            best[i] = int(l >= 0 and r >= 0) + max([count(c) for c in (l, r) if c >= 0], default=0)
        return best[i]

    return count(0)


def _slab(lo, hi, o, d, tmax):
    """(hit, entry distance) of the box against the ray's [0, tmax], float64; a zero direction component: inside the slab or not."""
    tn, tf = 0.0, tmax
    for a in range(3):
        if d[a] != 0.0:
            t0, t1 = (lo[a] - o[a]) / d[a], (hi[a] - o[a]) / d[a]
            if t0 > t1:
                t0, t1 = t1, t0
            tn, tf = max(tn, t0), min(tf, t1)
        elif not lo[a] <= o[a] <= hi[a]:
            return False, np.inf
    return tn <= tf, tn


def binary_walks(node_refs, boxes, rays):
    """trace_closest's control flow for every RAY8 record, no cull by a hit: (largest sp, node steps), each (len(rays),) int."""
    lo, hi, refs = boxes[0].tolist(), boxes[1].tolist(), node_refs.tolist()
    out = np.zeros((len(rays), 2), np.int64)
    for i, ray in enumerate(np.asarray(rays, np.float64).tolist()):
        o, d, tmax = ray[0:3], ray[3:6], ray[7]
        stack, cur, top, steps = [], 0, 0, 0
        while True:
            steps += 1
            refL, refR = refs[cur]
            okL, tnL = _slab(lo[cur][0], hi[cur][0], o, d, tmax)
            okR, tnR = _slab(lo[cur][1], hi[cur][1], o, d, tmax)
            okL, okR = okL and refL >= 0, okR and refR >= 0      # a leaf is tested on the spot and never pushed
            if okL and okR:
                near_left = tnL <= tnR
                stack.append(refR if near_left else refL)
                top = max(top, len(stack))
                cur = refL if near_left else refR
            elif okL:
                cur = refL
            elif okR:
                cur = refR
            elif not stack:
                break
            else:
                cur = stack.pop()
        out[i] = (top, steps)
    return out[:, 0], out[:, 1]


def _tri_hit(p, o, d, best):
    """Triangle::hit in float64 (one-sided, det >= 1e-4) on nested lists: the new closest t, or `best`."""
    cross = lambda a, b: (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])      # noqa: E731
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]      # noqa: E731
    e1, e2, T = [p[1][k] - p[0][k] for k in range(3)], [p[2][k] - p[0][k] for k in range(3)], [o[k] - p[0][k] for k in range(3)]
    P, Q = cross(d, e2), cross(T, e1)
    det = dot(P, e1)
    if det < 1e-4:
        return best
    t, u, v = dot(Q, e2) / det, dot(P, T), dot(Q, d)
    if t < 0 or t > best or u < 0 or u > det or v < 0 or u + v > det:
        return best
    return t


def quad_walks(t, pos, boxes, rays):
    """The 4-wide walk of tools/stack_lab.cpp for every RAY8 record over t["quad_refs"]: children nearest first, far side cut at the
    closest hit, up to three pushes per node, leaves pushed like nodes.  Returns (hist, largest stack per ray, node steps per ray):
    hist counts the stack depth after every node step in 32 bins, the last being 31 or more, as Scene.trace_depth_hist does for wf_trace."""
    lo, hi, refs = boxes[0].tolist(), boxes[1].tolist(), t["quad_refs"].tolist()
    tri = np.ascontiguousarray(pos, F).reshape(-1, 3, 3)[t["prim"]].astype(np.float64).tolist()      # in tree order
    hist, tops, steps = np.zeros(32, np.int64), np.zeros(len(rays), np.int64), np.zeros(len(rays), np.int64)
    for i, ray in enumerate(np.asarray(rays, np.float64).tolist()):
        ol, dl, best = ray[0:3], ray[3:6], ray[7]
        stack, cur, top = [], 0, 0
        while True:
            if cur >= 0:
                hit = []
                for k in range(4):
                    if refs[cur][k] != -1:
                        ok, tn = _slab(lo[cur][k], hi[cur][k], ol, dl, best)
                        if ok:
                            hit.append((tn, k))
                hit.sort()
                done = False
                if hit:
                    stack += [refs[cur][k] for _, k in reversed(hit[1:])]
                    top = max(top, len(stack))
                    cur = refs[cur][hit[0][1]]
                elif stack:
                    cur = stack.pop()
                else:
                    done = True
                hist[min(len(stack), 31)] += 1
                steps[i] += 1
                if done:
                    break
            else:
                code = ~cur
                for q in range(code >> 3, (code >> 3) + (code & 7)):
                    best = _tri_hit(tri[q], ol, dl, best)
                if not stack:
                    break
                cur = stack.pop()
        tops[i] = top
    return hist, tops, steps
