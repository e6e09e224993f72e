"""The yardstick of tests/test_convex_queries.py, independent of the code under test: the class key h(Q, k) of include/pt_api.h
("Convex-region queries") in numpy, transcribed from the header operation by operation; the node test of the walks; brute force over all
primitives with the lists' order; the families of pairs the kernels' own functions and the float32 vertex test are held to; a float64
polygon-clipping test that says what class 1 over-reports; and the region sets of the GPU tests.

Every function takes its precision from its arguments: float32 arrays give the header's arithmetic (numpy rounds every operation once
and contracts nothing), float64 arrays the same test in double.  A region is an (m, 4) array of PLANE4 records n.xyz | d."""
import numpy as np

import box_ref as B
import nearest_ref as N
import ptamd

F = np.float32
INF = F(np.inf)
CHUNK = 256
TOUCHING, INSIDE = 0, 1
MAXP = 8


def s_of(plane, v):
    """s(v) = (n.x*v.x + n.y*v.y) + n.z*v.z for broadcastable (..., 4) planes and (..., 3) points"""
    return (plane[..., 0] * v[..., 0] + plane[..., 1] * v[..., 1]) + plane[..., 2] * v[..., 2]


def _valid(pl):
    return np.isfinite(pl[..., 0:3]).all((-1, -2))


def tri_key(pl, a, ab, ac):
    """h(Q, triangle): pl (..., m, 4), a ab ac (..., 3), broadcastable, one dtype."""
    dt = a.dtype.type
    m = pl.shape[-2]
    with np.errstate(invalid="ignore", over="ignore"):
        b, c = a + ab, a + ac
        none, every = False, True
        for j in range(m):
            p = pl[..., j, :]
            ia, ib, ic = s_of(p, a) <= p[..., 3], s_of(p, b) <= p[..., 3], s_of(p, c) <= p[..., 3]
            none = none | ~(ia | ib | ic)
            every = every & (ia & ib & ic)
        bad = ~_valid(pl) | none
    return np.where(bad, dt(np.inf), np.where(every, dt(0), dt(1))).astype(a.dtype)


def sphere_key(pl, centre, rad):
    """h(Q, sphere): pl (..., m, 4), centre (..., 3), rad (...); membership refers to the sphere's surface."""
    rad = np.asarray(rad)
    dt = centre.dtype.type
    m = pl.shape[-2]
    with np.errstate(invalid="ignore", over="ignore"):
        none, every = False, True
        for j in range(m):
            p = pl[..., j, :]
            ln = np.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2])
            r = rad * ln
            sc = s_of(p, centre)
            none = none | ~(sc - r <= p[..., 3])
            every = every & (sc + r <= p[..., 3])
        bad = ~_valid(pl) | none
    return np.where(bad, dt(np.inf), np.where(every, dt(0), dt(1))).astype(centre.dtype)


def overlaps(pl, clo, chi):
    """The walks' node test: for no plane is the box's minimising corner outside.  pl (..., m, 4), clo chi (..., 3)."""
    ok = True
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(pl.shape[-2]):
            p = pl[..., j, :]
            corner = np.where(p[..., 0:3] >= 0, clo, chi)
            ok = ok & (s_of(p, corner) <= p[..., 3])
    return ok


def key_matrix(planes, positions, spheres=None):
    """(n regions, n primitives) float32: h of every region against every primitive, triangles first.  planes: (n, m, 4)."""
    pl = np.ascontiguousarray(planes, F)
    a, ab, ac = N.edges(positions)
    cols = [tri_key(pl[:, None], a[None, t:t + CHUNK], ab[None, t:t + CHUNK], ac[None, t:t + CHUNK]) for t in range(0, len(a), CHUNK)]
    if spheres is not None and len(spheres):
        s = np.ascontiguousarray(spheres, F)
        cols.append(sphere_key(pl[:, None], s[None, :, 0:3], s[None, :, 3]))
    K = np.concatenate(cols, 1) if cols else np.zeros((len(pl), 0), F)
    assert K.dtype == F
    return K


def brute(planes, positions, spheres=None, flags=TOUCHING, filter=None, K=None):
    """(counts, (offsets, cls, prim)) by definition, as box_ref.brute orders and filters them."""
    if K is None:
        K = key_matrix(planes, positions, spheres)
    return B.brute(None, None, None, flags, filter, K=K)


def natural_planes(pl):
    """Per region of (n, m, 4): the index of its last plane that is not neutral (a zero normal with d >= 0), plus one; at least 1."""
    neutral = (pl[..., 0:3] == 0).all(-1) & (pl[..., 3] >= 0)
    last = np.where(~neutral, np.arange(pl.shape[1])[None, :] + 1, 0).max(1)
    return np.maximum(last, 1)


def pad(pl, m=MAXP):
    """(n, k, 4) -> (n, m, 4) with neutral planes (0, 0, 0, 0) behind"""
    pl = np.ascontiguousarray(pl, F)
    out = np.zeros((pl.shape[0], m, 4), F)
    out[:, :pl.shape[1]] = pl
    return out


def obb_many(center, axes, half):
    """ptamd.obb_planes for n boxes at once: center (n, 3), axes (n, 3, 3), half (n, 3), float64 in, (n, 6, 4) float32 out."""
    c, a, h = np.asarray(center, np.float64), np.asarray(axes, np.float64), np.asarray(half, np.float64)
    n = np.stack([a[:, 0], -a[:, 0], a[:, 1], -a[:, 1], a[:, 2], -a[:, 2]], 1)
    d = (n * c[:, None, :]).sum(-1) + np.repeat(h, 2, 1)
    return np.concatenate([n, d[..., None]], -1).astype(F)


def aabb_many(lo, hi):
    """ptamd.aabb_planes for n boxes at once: (n, 6, 4) float32"""
    lo, hi = np.asarray(lo, F).reshape(-1, 3), np.asarray(hi, F).reshape(-1, 3)
    out = np.zeros((len(lo), 6, 4), F)
    for k in range(3):
        out[:, 2 * k, k], out[:, 2 * k, 3] = 1, hi[:, k]
        out[:, 2 * k + 1, k], out[:, 2 * k + 1, 3] = -1, -lo[:, k]
    return out


def rotations(rs, n):
    """n random rotations, (n, 3, 3) float64"""
    q, r = np.linalg.qr(rs.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


def widened(lo, hi):
    """A box as the binary tree's walk widens it (nearest_ref.binary_containment restates widen_binary)"""
    s = np.maximum(np.abs(lo), np.abs(hi)) * N.SLACK
    return lo - s, hi + s


# ---------------------------------------------------------------------------------------------------------------------------------
# the families of (region, triangle) pairs: box_ref.FAMILIES' positions, an oriented box on or beside each triangle
# ---------------------------------------------------------------------------------------------------------------------------------
def family(name, seed, n):
    """(planes (n, 6, 4), positions (n, 3, 3)): the box of the box family as an oriented box, turned at random about its centre.  The
    needles' boxes lie beside them as well as on them, and every 16th is large enough to hold a needle 30 long: all three classes occur."""
    lo, hi, pos = B.needle_family(seed, n, beside=1.0) if name == "needles" else B.FAMILIES[name](seed, n)
    rs = np.random.RandomState(seed + 1)
    lo64, hi64 = lo.astype(np.float64), hi.astype(np.float64)
    grow = rs.uniform(0.5, 2.0, (n, 1)) * (np.where(np.arange(n) % 16 == 0, 400.0, 1.0)[:, None] if name == "needles" else 1.0)
    return obb_many((lo64 + hi64) * 0.5, rotations(rs, n), (hi64 - lo64) * 0.5 * grow), pos


def vertex_accuracy(name, seed, n, shifts=(20, 22, 24)):
    """The float32 test s(v) <= d against float64 on n (plane, vertex) pairs of a family: the vertices are the family's, the planes
    pass them by within 2^-16 .. 2^-28 of M |n| on either side.  Returns {shift: exceptions at delta = 2^-shift * M * |n|} — a pair whose
    float64 signed distance e = n.v - d is above delta but float32 says inside, or below -delta but float32 says outside — and M."""
    _, _, pos = B.FAMILIES[name](seed, n)
    rs = np.random.RandomState(seed + 2)
    v = pos[np.arange(n), rs.randint(0, 3, n)]
    M = float(np.abs(pos).max())
    nrm = (rs.standard_normal((n, 3)) * np.exp(rs.uniform(-3, 3, (n, 1)))).astype(F)
    nrm[::5, rs.randint(0, 3)] = 0
    n64, v64 = nrm.astype(np.float64), v.astype(np.float64)
    ln = np.sqrt((n64 * n64).sum(1))
    off = rs.choice([-1.0, 1.0], n) * M * ln * 2.0 ** -rs.uniform(16, 28, n)
    d = ((n64 * v64).sum(1) + off).astype(F)
    inside32 = s_of(nrm, v) <= d
    e = (n64 * v64).sum(1) - d.astype(np.float64)
    out = {}
    for s in shifts:
        delta = 2.0 ** -s * M * ln
        out[s] = int(((e > delta) & inside32).sum() + ((e < -delta) & ~inside32).sum())
    return out, M


# ---------------------------------------------------------------------------------------------------------------------------------
# what class 1 over-reports: the triangle clipped against the region in float64
# ---------------------------------------------------------------------------------------------------------------------------------
def clipped_away(pl, tri):
    """Is the triangle (3, 3) disjoint from the region (m, 4)?  Sutherland-Hodgman in float64: the polygon that is left is empty."""
    poly = [np.asarray(p, np.float64) for p in tri]
    for p in np.asarray(pl, np.float64):
        if not np.isfinite(p).all():
            if p[3] == np.inf and (p[0:3] == 0).all():
                continue
            return True
        e = [float(p[0:3] @ q - p[3]) for q in poly]
        nxt = []
        for i in range(len(poly)):
            j = (i + 1) % len(poly)
            if e[i] <= 0:
                nxt.append(poly[i])
            if (e[i] <= 0) != (e[j] <= 0):
                t = e[i] / (e[i] - e[j])
                nxt.append(poly[i] + t * (poly[j] - poly[i]))
        poly = nxt
        if not poly:
            return True
    return False


def overreport(planes, positions, K=None):
    """(class-1 triangle pairs, those of them the float64 clipping calls disjoint) for regions (n, m, 4)"""
    pos = np.ascontiguousarray(positions, F).reshape(-1, 3, 3)
    if K is None:
        K = key_matrix(planes, pos)
    a, ab, ac = N.edges(pos)
    own = np.stack([a, a + ab, a + ac], 1)      # the record's own vertices
    q, k = np.nonzero(K[:, :len(pos)] == 1)
    return len(q), sum(clipped_away(planes[i], own[j]) for i, j in zip(q.tolist(), k.tolist()))


# ---------------------------------------------------------------------------------------------------------------------------------
# the region sets of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
class ConvexSets:
    """The regions a scene is asked about, by kind (`parts`: name -> (k, 8, 4), padded with neutral planes) and all together, shuffled so
    that every wave holds every kind (`planes`, (n, 8, 4); `kind[i]` names the part of row i; `natural[i]`: the planes row i needs).
    positions: (t, 3, 3); spheres: None or (s, >= 4)."""

    def __init__(self, positions, spheres, seed, m=80):
        rs = np.random.RandomState(seed)
        pos = np.ascontiguousarray(positions, F).reshape(-1, 3, 3)
        v = pos.reshape(-1, 3)
        sph = None if spheres is None or not len(spheres) else np.ascontiguousarray(spheres, F)[:, 0:4]
        boxes = B.BoxSets(pos, spheres, seed)
        size, vlo, vhi = boxes.size, boxes.vlo, boxes.vhi
        ctr, ext = (vlo.astype(np.float64) + vhi) * 0.5, (vhi.astype(np.float64) - vlo)
        P = {}
        # frusta: pixel windows, 1 x 1 to the whole frame, of small cameras inside the scene; every fourth with a near and a far plane
        fr = []
        self.cameras = []
        for i in range(m):
            W, H = int(rs.randint(4, 24)), int(rs.randint(4, 20))
            cam = ptamd.make_camera(W, H, pos=tuple((ctr + rs.uniform(-0.3, 0.3, 3) * ext).tolist()), rot_deg=tuple(rs.uniform(0, 360, 3).tolist()),
                                    fovy_deg=float(rs.uniform(20, 80)))
            x0, y0 = int(rs.randint(0, W)), int(rs.randint(0, H))
            if i % 2 == 0:      # every other camera looks at a vertex of the scene, through a window around the frame's centre
                f = pos[rs.randint(0, len(pos)), rs.randint(0, 3)].astype(np.float64) - np.array(cam.pos[:], np.float64)
                f /= np.sqrt((f * f).sum())
                r = np.cross(f, rs.standard_normal(3))
                r /= np.sqrt((r * r).sum())
                cam.forward[:], cam.right[:], cam.up[:] = f.tolist(), r.tolist(), np.cross(r, f).tolist()
                x0, y0 = int(rs.randint(0, (W - 1) // 2 + 1)), int(rs.randint(0, (H - 1) // 2 + 1))
                x1, y1 = int(rs.randint((W - 1) // 2 + 1, W + 1)), int(rs.randint((H - 1) // 2 + 1, H + 1))
            elif i % 5 == 0:
                x1, y1 = x0 + 1, y0 + 1
            else:
                x1, y1 = int(rs.randint(x0 + 1, W + 1)), int(rs.randint(y0 + 1, H + 1))
            if i % 7 == 0:
                x0, y0, x1, y1 = 0, 0, W, H
            if i % 10 == 2:
                x0, y0, x1, y1 = (W - 1) // 2, (H - 1) // 2, (W - 1) // 2 + 1, (H - 1) // 2 + 1      # one pixel, the one the vertex is seen through
            near, far = ((-1.0, np.inf) if i % 4 else (float(size), float(size) * float(rs.uniform(3, 30))))
            fr.append(ptamd.frustum_planes(cam, (x0, y0, x1, y1), near, far))
            self.cameras.append((cam, (x0, y0, x1, y1), near, far))
        P["frusta"] = pad(np.stack(fr))
        # oriented boxes about a triangle's size, around vertices (even rows) and centroids (odd rows)
        k = rs.randint(0, len(pos), m)
        c = np.where((np.arange(m) % 2 == 0)[:, None], pos[k, rs.randint(0, 3, m)].astype(np.float64), pos[k].astype(np.float64).mean(1))
        P["obb"] = pad(obb_many(c, rotations(rs, m), rs.uniform(0.2, 1.5, (m, 3)) * size * np.where(np.arange(m) % 8 == 0, 4.0, 1.0)[:, None]))
        # the boxes of the box tests, every kind of them, as six planes
        blo, bhi = B.split(boxes.boxes[:m])
        P["aabb"] = pad(aabb_many(blo, bhi))
        # oriented boxes with two more faces: eight planes that all cut
        k = rs.randint(0, len(pos), m // 4)
        c, rot, half = pos[k, 0].astype(np.float64), rotations(rs, m // 4), rs.uniform(0.5, 2.0, (m // 4, 3)) * size
        six = obb_many(c, rot, half)
        diag = (rot[:, 0] + rot[:, 1]) / np.sqrt(2.0)
        two = np.stack([np.concatenate([diag, ((diag * c).sum(1) + 0.8 * half[:, 0:2].sum(1) / np.sqrt(2.0))[:, None]], 1),
                        np.concatenate([-diag, (-(diag * c).sum(1) + 0.8 * half[:, 0:2].sum(1) / np.sqrt(2.0))[:, None]], 1)], 1).astype(F)
        P["prism8"] = np.concatenate([six, two], 1)
        # half-spaces and slabs through and beside vertices: axis-aligned (every third), unit and far from unit normals
        def normals(n):
            u = rs.standard_normal((n, 3)) * np.exp(rs.uniform(-2, 2, (n, 1)))
            ax = np.arange(n) % 3 == 0
            u[ax] = np.eye(3)[rs.randint(0, 3, ax.sum())] * rs.choice([-1.0, 1.0], (ax.sum(), 1))
            return u.astype(F)
        n4 = m // 4
        nrm, vert = normals(n4), pos[rs.randint(0, len(pos), n4), rs.randint(0, 3, n4)]
        P["halfspace"] = pad(np.concatenate([nrm, s_of(nrm, vert)[:, None]], 1)[:, None, :])      # the vertex lies ON the plane, by equality
        nrm, vert = normals(n4), pos[rs.randint(0, len(pos), n4), rs.randint(0, 3, n4)]
        t = (np.sqrt((nrm.astype(np.float64) ** 2).sum(1)) * size * rs.uniform(0.1, 3.0, n4)).astype(F)
        sv = s_of(nrm, vert)
        P["slab"] = pad(np.stack([np.concatenate([nrm, (sv + t)[:, None]], 1), np.concatenate([-nrm, (-sv + t)[:, None]], 1)], 1))
        nrm, vert = normals(n4), pos[rs.randint(0, len(pos), n4), rs.randint(0, 3, n4)]
        sv = s_of(nrm, vert)
        P["thin"] = pad(np.stack([np.concatenate([nrm, sv[:, None]], 1), np.concatenate([-nrm, -sv[:, None]], 1)], 1))      # zero thickness, through the vertex
        self.thin_vertex = vert
        # everything inside: the scene's box with room to spare, and a turned box around it
        big = obb_many(ctr[None], rotations(rs, 1), np.full((1, 3), ext.max() * 2.0 + 4.0))
        P["scene"] = pad(np.concatenate([aabb_many(vlo - F(1), vhi + F(1)), big]))
        # far outside
        c = (N.room_points(rs, m // 4) * F(300)).astype(np.float64)
        P["far"] = pad(obb_many(c, rotations(rs, m // 4), np.full((m // 4, 3), float(size))))
        # empty: (0, 0, 0, -1), d = -inf, opposed planes with a gap no triangle of the scene spans (one that did would be class 1: the
        # conservative case) — each among planes that would hold members
        e = P["obb"][:6].copy()
        e[0, 6], e[1, 0] = (0, 0, 0, -1), (0, 0, 0, -1)
        e[2, 7, 3], e[3, 2, 3] = -np.inf, -np.inf
        for i in (4, 5):
            e[i, 6] = e[i, 0]
            e[i, 7, 0:3], e[i, 7, 3] = -e[i, 0, 0:3], -e[i, 0, 3] - F(4 * ext.max())
        P["empty"] = e
        # invalid: a NaN or an infinite normal component, and a NaN d, in planes around members
        bad = P["obb"][6:18].copy()
        for i in range(12):
            j, comp = i % 6, i % 3
            bad[i, j, comp if i < 9 else 3] = (np.nan, np.inf, -np.inf)[i // 3] if i < 9 else np.nan
        P["invalid"] = bad
        if sph is not None:
            j = rs.randint(0, len(sph), 3 * (m // 6))
            u = rs.standard_normal((len(j), 3))
            u /= np.sqrt((u * u).sum(1, keepdims=True))
            sc, rad = sph[j, 0:3].astype(np.float64), sph[j, 3:4].astype(np.float64)
            which = np.arange(len(j)) % 3
            c = np.where((which == 2)[:, None], sc + rad * u, sc)
            half = np.where((which == 0)[:, None], 0.3 * rad, np.where((which == 1)[:, None], 1.5 * rad, 0.4 * rad)) * np.ones((1, 3))
            P["spheres"] = pad(obb_many(c, rotations(rs, len(j)), half))      # inside the ball, around it, across its surface
            self.sphere_kind, self.sphere_index = which, j
        self.parts = P
        names = list(P)
        planes = np.concatenate([P[n] for n in names])
        order = rs.permutation(len(planes))
        self.planes, self.names, self.order = np.ascontiguousarray(planes[order]), names, order
        self.kind = np.concatenate([np.full(len(P[n]), i) for i, n in enumerate(names)])[order]
        self.natural = natural_planes(self.planes)
        self.size, self.vlo, self.vhi = size, vlo, vhi

    def rows(self, name):
        """The rows of `planes` that hold part `name`, in the part's own order."""
        i = self.names.index(name)
        start = sum(len(self.parts[n]) for n in self.names[:i])
        inv = np.empty(len(self.order), np.int64)
        inv[self.order] = np.arange(len(self.order))
        return inv[start:start + len(self.parts[name])]

    def with_planes(self, m):
        """(rows, planes (k, m, 4)): the regions that need at most m planes, cut to m: the same regions, so the same keys"""
        rows = np.nonzero(self.natural <= m)[0]
        return rows, np.ascontiguousarray(self.planes[rows, :m])
