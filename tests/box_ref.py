"""The yardstick of tests/test_box_queries.py, independent of the code under test: the class key g(Q, k) of include/pt_api.h ("Box
queries") in numpy, transcribed from the header operation by operation; brute force over all primitives with the lists' order; the
families of (box, triangle) pairs the accuracy of the definition is measured on; and the box sets of the GPU tests.

Every function takes its precision from its arguments: float32 arrays give the header's arithmetic (numpy rounds every operation once
and contracts nothing), float64 arrays the same test in double."""
import numpy as np

import nearest_ref as N

F = np.float32
INF = F(np.inf)
CHUNK = 256      # triangles per block of the brute force: boxes x CHUNK x 3 floats per temporary
TOUCHING, INSIDE = 0, 1


def tri_key(lo, hi, a, ab, ac):
    """g(Q, triangle): 0 inside, 1 touching, +inf no member, for broadcastable (..., 3) arrays of one dtype."""
    lo, hi, a, ab, ac = np.broadcast_arrays(lo, hi, a, ab, ac)
    dt = a.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (lo <= hi).all(-1)
        b, c = a + ab, a + ac
        tlo, thi = np.fmin(np.fmin(a, b), c), np.fmax(np.fmax(a, b), c)
        overlap = ((tlo <= hi) & (thi >= lo)).all(-1)
        inside = ((tlo >= lo) & (thi <= hi)).all(-1)
        infinite = (np.isinf(lo) | np.isinf(hi)).any(-1)
        ctr = (lo + hi) * dt(0.5)
        h = np.fmax(hi - ctr, ctr - lo)
        v = (a - ctr, b - ctr, c - ctr)
        n = N.cross(ab, ac)
        d = N.dot(n, v[0])
        r = (h[..., 0] * np.abs(n[..., 0]) + h[..., 1] * np.abs(n[..., 1])) + h[..., 2] * np.abs(n[..., 2])
        sep = np.abs(d) > r
        for e in (ab, ac, ac - ab):
            for i in range(3):
                j, k = (i + 1) % 3, (i + 2) % 3
                p0, p1, p2 = (vm[..., k] * e[..., j] - vm[..., j] * e[..., k] for vm in v)
                rr = h[..., j] * np.abs(e[..., k]) + h[..., k] * np.abs(e[..., j])
                sep = sep | (np.fmin(np.fmin(p0, p1), p2) > rr) | (np.fmax(np.fmax(p0, p1), p2) < -rr)
    none, one = dt(np.inf), dt(1)
    return np.where(~valid | ~overlap, none, np.where(inside, dt(0), np.where(infinite, one, np.where(sep, none, one)))).astype(a.dtype)


def sphere_key(lo, hi, centre, rad):
    """g(Q, sphere): membership refers to the sphere's surface.  (..., 3) boxes and centres, (...) radii, one dtype."""
    rad = np.asarray(rad)
    lo, hi, centre = np.broadcast_arrays(lo, hi, centre)
    dt = lo.dtype.type
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (lo <= hi).all(-1)
        r3 = rad[..., None]
        inside = ((centre - r3 >= lo) & (centre + r3 <= hi)).all(-1)
        g = np.fmax(np.fmax(lo - centre, centre - hi), dt(0))
        near2 = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
        q = np.fmax(np.abs(lo - centre), np.abs(hi - centre))
        far2 = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]
        rr = rad * rad
        touch = (near2 <= rr) & (far2 >= rr)
    return np.where(~valid, dt(np.inf), np.where(inside, dt(0), np.where(touch, dt(1), dt(np.inf)))).astype(lo.dtype)


def split(boxes):
    """(lo, hi), each (n, 3), of (n, 8) BOX8 records."""
    b = np.ascontiguousarray(boxes, F).reshape(-1, 8)
    return b[:, 0:3], b[:, 4:7]


def make_boxes(lo, hi):
    """(n, 8) BOX8 records; the reserved floats hold a NaN, which nothing may read."""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    out = np.full((len(lo), 8), np.nan, F)
    out[:, 0:3], out[:, 4:7] = lo, hi
    return out


def key_matrix(boxes, positions, spheres=None):
    """(n boxes, n primitives) float32: g of every box against every primitive, triangles first."""
    lo, hi = split(boxes)
    a, ab, ac = N.edges(positions)
    cols = [tri_key(lo[:, None], hi[:, None], a[None, t:t + CHUNK], ab[None, t:t + CHUNK], ac[None, t:t + CHUNK]) for t in range(0, len(a), CHUNK)]
    if spheres is not None and len(spheres):
        s = np.ascontiguousarray(spheres, F)
        cols.append(sphere_key(lo[:, None], hi[:, None], s[None, :, 0:3], s[None, :, 3]))
    K = np.concatenate(cols, 1) if cols else np.zeros((len(lo), 0), F)
    assert K.dtype == F
    return K


def brute(boxes, positions, spheres=None, flags=TOUCHING, filter=None, K=None):
    """(counts, (offsets, cls, prim)) by definition: B(Q) = {k : g(Q, k) <= bound} without the primitives the filter drops, ordered by g
    ascending and among equal g the larger primitive first.  filter: None or (prim_bits, m, skip) — (n_prims,) uint32 or None, a word or
    (n,) uint32, (n,) ints or None.  K: key_matrix of the same arguments, if the caller has it."""
    if K is None:
        K = key_matrix(boxes, positions, spheres)
    member = K <= (F(0) if flags == INSIDE else F(1))
    if filter is not None:
        prim_bits, m, skip = filter
        words = np.full(K.shape[1], 0xFFFFFFFF, np.uint32) if prim_bits is None else np.asarray(prim_bits, np.uint32)
        member &= (words[None, :] & np.broadcast_to(np.asarray(m, np.uint32), (K.shape[0],))[:, None]) != 0
        if skip is not None:
            member &= np.arange(K.shape[1])[None, :] != np.asarray(skip, np.int64)[:, None]
    counts = member.sum(1).astype(np.int32)
    row, prim = np.nonzero(member)
    cls = K[row, prim]
    order = np.lexsort((-prim, cls, row))
    off = np.concatenate([np.zeros(1, np.int64), np.cumsum(counts, dtype=np.int64)])
    return counts, (off, np.ascontiguousarray(cls[order]), np.ascontiguousarray(prim[order].astype(np.int32)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the families of pairs the definition's accuracy is measured on (2 * 10^6 pairs each in the test)
# ---------------------------------------------------------------------------------------------------------------------------------
def _boxes_on(rs, pos, max_half, beside):
    """One box per triangle: centred on a point of the triangle moved by up to `beside` times the box's own half-size, half-sizes
    uniform in 0 .. max_half per axis.  beside = 1.5: inside, touching, grazing and disjoint pairs all occur; 0: the box sits ON the
    triangle, and the only question is whether float32 finds a thin box there."""
    n = len(pos)
    p = pos.astype(np.float64)
    u = rs.uniform(0, 1, (n, 2))
    flip = u.sum(1) > 1
    u[flip] = 1 - u[flip]
    on = p[:, 0] + u[:, :1] * (p[:, 1] - p[:, 0]) + u[:, 1:] * (p[:, 2] - p[:, 0])
    half = rs.uniform(0, max_half, (n, 3))
    ctr = on + rs.uniform(-beside, beside, (n, 3)) * half
    return (ctr - half).astype(F), (ctr + half).astype(F)


def ordinary_family(seed, n):
    """Triangles with edges of about 1.5 anywhere in the 40-wide room, boxes of half-size 0 .. 2 around them: (lo, hi, positions)."""
    rs = np.random.RandomState(seed)
    a = N.room_points(rs, n).astype(np.float64)
    pos = np.stack([a, a + rs.uniform(-1.5, 1.5, (n, 3)), a + rs.uniform(-1.5, 1.5, (n, 3))], 1).astype(F)
    lo, hi = _boxes_on(rs, pos, 2.0, 1.5)
    return lo, hi, pos


def needle_family(seed, n, beside=0.0):
    """Needles 30 long and 0.003 wide, boxes of half-size 0 .. 0.1 on them (beside > 0: next to them, a harder family that the test
    does not assert on: DESIGN.md section 41 has its figures)."""
    rs = np.random.RandomState(seed)
    pos = N.sliver_triangles(rs, n)
    lo, hi = _boxes_on(rs, pos, 0.1, beside)
    return lo, hi, pos


def far_family(seed, n):
    """The ordinary family translated by 2^17 along every axis, in float32: the coordinates lose 17 bits."""
    lo, hi, pos = ordinary_family(seed, n)
    t = F(131072.0)
    return lo + t, hi + t, pos + t


FAMILIES = {"ordinary": ordinary_family, "needles": needle_family, "far": far_family}


def accuracy(lo, hi, pos, shifts=(14, 16, 18, 20)):
    """The float32 key of every pair held against the float64 evaluation of the same test on the box grown and shrunk by
    delta = 2^-shift * M, M the largest absolute coordinate of the family (as tests/test_nearest.py takes the scene's: the error terms
    are products of an edge with a coordinate relative to the box, both bounded by the family's extent, not by a pair's own).
    Returns {shift: (members the grown box calls disjoint, non-members the shrunk box calls overlapping, pairs inside the shrunk box
    whose key is not 0)} and the float32 keys."""
    a, ab, ac = N.edges(pos)
    key = tri_key(lo, hi, a, ab, ac)
    M = float(max(np.abs(lo).max(), np.abs(hi).max(), np.abs(pos).max()))
    lo64, hi64, a64, ab64, ac64 = (x.astype(np.float64) for x in (lo, hi, a, ab, ac))
    out = {}
    for s in shifts:
        d = M * 2.0 ** -s
        grown = tri_key(lo64 - d, hi64 + d, a64, ab64, ac64)
        shrunk = tri_key(lo64 + d, hi64 - d, a64, ab64, ac64)
        out[s] = (int(((grown == np.inf) & (key != INF)).sum()), int(((shrunk <= 1) & ~(key <= 1)).sum()), int(((shrunk == 0) & (key != 0)).sum()))
    return out, key


# ---------------------------------------------------------------------------------------------------------------------------------
# the box sets of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
class BoxSets:
    """The boxes a scene is asked about, by kind (`parts`: name -> (n, 8) BOX8 records) and all together, shuffled so that every wave
    holds every kind (`boxes`; `kind[i]` names the part of row i).  positions: (m, 3, 3); spheres: None or (s, >= 4)."""

    def __init__(self, positions, spheres, seed, m=72):
        rs = np.random.RandomState(seed)
        pos = np.ascontiguousarray(positions, F).reshape(-1, 3, 3)
        v = pos.reshape(-1, 3)
        sph = None if spheres is None or not len(spheres) else np.ascontiguousarray(spheres, F)[:, 0:4]
        vlo, vhi = v.min(0), v.max(0)
        if sph is not None:
            vlo, vhi = np.minimum(vlo, (sph[:, 0:3] - sph[:, 3:4]).min(0)), np.maximum(vhi, (sph[:, 0:3] + sph[:, 3:4]).max(0))
        edge = np.sqrt((((pos[:, 1] - pos[:, 0]).astype(np.float64)) ** 2).sum(1))
        size = F(np.median(edge[edge > 0]))
        P = {}
        # about a triangle's size, around vertices (even rows) and centroids (odd rows)
        k = rs.randint(0, len(pos), m)
        c = np.where((np.arange(m) % 2 == 0)[:, None], pos[k, rs.randint(0, 3, m)], (pos[k].astype(np.float64).mean(1)).astype(F))
        half = (rs.uniform(0.2, 1.0, (m, 3)) * size).astype(F)
        P["around"] = make_boxes(c - half, c + half)
        # point boxes exactly on vertices and edge midpoints
        k, i = rs.randint(0, len(pos), m), rs.randint(0, 3, m)
        i[0::4] = 0               # every other vertex box sits on a V0: the one vertex a record holds exactly
        p = pos[k, i].copy()      # even rows: vertex i of triangle k; odd rows: (V_i + V_i+1) * 0.5 in float32, as N.vertex_and_edge_points
        p[1::2] = (pos[k[1::2], i[1::2]] + pos[k[1::2], (i[1::2] + 1) % 3]) * F(0.5)
        P["points"] = make_boxes(p, p)
        self.point_tri, self.point_vertex = k, np.where(np.arange(m) % 2 == 0, i, -1)      # -1: a midpoint, no vertex
        # slices: lo == hi on one axis, at a vertex coordinate
        k, ax = rs.randint(0, len(pos), m), rs.randint(0, 3, m)
        c = pos[k, rs.randint(0, 3, m)]
        half = (rs.uniform(0.5, 2.0, (m, 3)) * size).astype(F)
        half[np.arange(m), ax] = 0
        P["slices"] = make_boxes(c - half, c + half)
        # faces exactly through vertex coordinates: a triangle's own box (inside by equality); that box moved so that its hi face on one
        # axis is the triangle's lo (touching by one shared coordinate); a box that ends on a vertex coordinate of one axis
        k, ax = rs.randint(0, len(pos), m), rs.randint(0, 3, m)
        tlo, thi = N.tri_box(*N.edges(pos[k]))
        lo, hi = tlo.copy(), thi.copy()
        third = np.arange(m) % 3
        r = np.arange(m)
        shifted = third == 1
        hi[r[shifted], ax[shifted]] = tlo[r[shifted], ax[shifted]]
        lo[r[shifted], ax[shifted]] = tlo[r[shifted], ax[shifted]] - size
        ends = third == 2
        lo[ends] = tlo[ends] - size
        hi[ends] = thi[ends] + size
        hi[r[ends], ax[ends]] = pos[k[ends], 0, ax[ends]]
        P["faces"] = make_boxes(lo, hi)
        # the whole scene, exactly and with room to spare
        P["scene"] = make_boxes(np.stack([vlo, vlo - F(1)]), np.stack([vhi, vhi + F(1)]))
        # a half-space, a slab and a column
        mid = ((vlo.astype(np.float64) + vhi) * 0.5).astype(F)
        inf3 = np.full(3, np.inf, F)
        P["halfspace"] = make_boxes(np.stack([-inf3, np.array([-np.inf, mid[1], -np.inf], F), np.array([mid[0] - size, -np.inf, mid[2] - size], F)]),
                                    np.stack([np.array([np.inf, mid[1], np.inf], F), np.array([np.inf, mid[1] + size, np.inf], F),
                                              np.array([mid[0] + size, np.inf, mid[2] + size], F)]))
        # inverted boxes and boxes with a NaN, all around members of the scene
        lo, hi = split(P["around"][:14].copy())
        lo, hi = lo.copy(), hi.copy()
        for i in range(14):
            if i < 6:
                (lo if i < 3 else hi)[i, i % 3] = np.nan
            elif i < 12:
                lo[i, i % 3], hi[i, i % 3] = hi[i, i % 3], lo[i, i % 3]      # lo > hi on one axis
            else:
                lo[i], hi[i] = vhi + F(1), vlo - F(1)                        # the whole scene, inside out
        P["invalid"] = make_boxes(lo, hi)
        # far outside
        c = N.room_points(rs, m // 2) * F(300)
        P["far"] = make_boxes(c - size, c + size)
        if sph is not None:
            j = rs.randint(0, len(sph), 3 * (m // 3))
            u = rs.standard_normal((len(j), 3))
            u /= np.sqrt((u * u).sum(1, keepdims=True))
            ctr, rad = sph[j, 0:3].astype(np.float64), sph[j, 3:4].astype(np.float64)
            which = np.arange(len(j)) % 3
            c = np.where((which == 2)[:, None], ctr + rad * u, ctr)
            half = np.where((which == 0)[:, None], 0.3 * rad, np.where((which == 1)[:, None], 1.5 * rad, 0.4 * rad))
            P["spheres"] = make_boxes((c - half).astype(F), (c + half).astype(F))      # inside the ball, around it, across its surface
            self.sphere_kind, self.sphere_index = which, j
        self.parts = P
        names = list(P)
        boxes = np.concatenate([P[n] for n in names])
        kind = np.concatenate([np.full(len(P[n]), i) for i, n in enumerate(names)])
        order = rs.permutation(len(boxes))
        self.boxes, self.kind, self.names = np.ascontiguousarray(boxes[order]), kind[order], names
        self.order = order
        self.size, self.vlo, self.vhi = size, vlo, vhi

    def rows(self, name):
        """The rows of `boxes` that hold part `name`, in the part's own order."""
        i = self.names.index(name)
        start = sum(len(self.parts[n]) for n in self.names[:i])
        inv = np.empty(len(self.order), np.int64)
        inv[self.order] = np.arange(len(self.order))
        return inv[start:start + len(self.parts[name])]
