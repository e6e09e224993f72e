"""The yardstick of tests/test_nearest.py, independent of the code under test: the per-primitive function f of include/pt_api.h
("Closest-point queries") and its detail record in numpy, transcribed from the header operation by operation; the textbook
region-classification formula as an independent check of what f measures; and brute force over all primitives with the tie rule.

Every function takes its precision from its arguments: float32 arrays give the header's arithmetic (numpy rounds every operation once
and contracts nothing), float64 arrays the same formula in double."""
import numpy as np

F = np.float32
CHUNK = 256      # triangles per block of the brute force: points x CHUNK x 3 floats per temporary


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], -(a[..., 0] * b[..., 2] - a[..., 2] * b[..., 0]),
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def seg(q, e):
    """(seg, t) of the header: squared distance to the segment and the clamped parameter; a zero edge gives t = 0."""
    dt = q.dtype.type
    with np.errstate(invalid="ignore", divide="ignore"):
        t = dot(q, e) / dot(e, e)
        t = np.where(t > 0, t, dt(0))
    t = np.where(t < 1, t, dt(1))
    r = q - t[..., None] * e
    return dot(r, r), t


def boxdist2(p, lo, hi):
    g = np.maximum(np.maximum(lo - p, p - hi), p.dtype.type(0))
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def tri_box(a, ab, ac):
    """The box of the triangle the record describes: of (a, a + ab, a + ac)."""
    b, c = a + ab, a + ac
    return np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)


def tri_terms(p, a, ab, ac):
    """Everything f and the detail record are made of, for broadcastable (..., 3) arrays of one dtype."""
    p, a, ab, ac = np.broadcast_arrays(p, a, ab, ac)
    bc, ap = ac - ab, p - a
    bp = ap - ab
    (d1, t1), (d2, t2), (d3, t3) = seg(ap, ab), seg(ap, ac), seg(bp, bc)
    d_edge = np.minimum(np.minimum(d1, d2), d3)
    n = cross(ab, ac)
    nn, h = dot(n, n), dot(ap, n)
    sw, sa, sv = dot(cross(ab, ap), n), dot(cross(bc, bp), n), dot(cross(ap, ac), n)
    inside = (nn > 0) & (sw >= 0) & (sa >= 0) & (sv >= 0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d_plane = (h * h) / nn
        interior = inside & (d_plane < d_edge)
    d_raw = np.where(interior, d_plane, d_edge)
    lo, hi = tri_box(a, ab, ac)
    floor = boxdist2(p, lo, hi)
    return dict(p=p, a=a, ab=ab, ac=ac, bc=bc, ap=ap, t=(t1, t2, t3), d=(d1, d2, d3), d_edge=d_edge, n=n, nn=nn, h=h, sw=sw, sv=sv,
                interior=interior, d_raw=d_raw, floor=floor, f=np.maximum(d_raw, floor))


def tri_f(p, a, ab, ac):
    return tri_terms(p, a, ab, ac)["f"]


def sphere_f(p, centre, rad):
    pc = p - centre
    g = np.sqrt(dot(pc, pc)) - rad
    return g * g


def edges(positions):
    """(a, ab, ac), each (m, 3) float32, of (m, 3, 3) positions: the edges rounded once, as PtTriangle's E1 and E2 are."""
    pos = np.ascontiguousarray(positions, F).reshape(-1, 3, 3)
    return pos[:, 0], pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0]


def f_matrix(points, positions):
    """(n, m) float32: f of every point against every triangle.  For small inputs (the accuracy tests)."""
    a, ab, ac = edges(positions)
    p = np.ascontiguousarray(points, F)[:, None, 0:3]
    return tri_f(p, a[None], ab[None], ac[None])


def brute(points, positions, spheres=None):
    """(dist2, prim) of PT_NEAREST_CLOSEST by definition.  points: (n, 4) POINT4 records; positions: (m, 3, 3); spheres: None or (s, >= 4)
    records centre.xyz rad.  Primitives in index order, a candidate wins with f < best or f == best and a larger index, from (r2, -1)."""
    pts = np.ascontiguousarray(points, F)
    p = pts[:, None, 0:3]
    a, ab, ac = edges(positions)
    best, prim = pts[:, 3] * pts[:, 3], np.full(len(pts), -1, np.int32)
    rows = np.arange(len(pts))
    for lo in range(0, len(a), CHUNK):
        f = tri_f(p, a[None, lo:lo + CHUNK], ab[None, lo:lo + CHUNK], ac[None, lo:lo + CHUNK])
        k = f.shape[1] - 1 - np.argmin(f[:, ::-1], 1)      # the LAST minimum of the block: the largest index among equals
        fk = f[rows, k]
        with np.errstate(invalid="ignore"):
            take = fk <= best                              # every index here is above every earlier one
        best, prim = np.where(take, fk, best), np.where(take, (lo + k).astype(np.int32), prim)
    if spheres is not None:
        for j, s in enumerate(np.ascontiguousarray(spheres, F)):
            f = sphere_f(pts[:, 0:3], s[None, 0:3], s[3])
            with np.errstate(invalid="ignore"):
                take = f <= best
            best, prim = np.where(take, f, best), np.where(take, np.int32(len(a) + j), prim)
    assert best.dtype == F
    return np.where(prim < 0, F(0), best), prim


def f_of(points, prim, positions, spheres=None):
    """(n,) float32: f(p_i, prim_i) for the listed primitives (prim_i >= 0)."""
    pts = np.ascontiguousarray(points, F)[:, 0:3]
    a, ab, ac = edges(positions)
    prim = np.asarray(prim)
    out = np.zeros(len(pts), F)
    tri = prim < len(a)
    out[tri] = tri_f(pts[tri], a[prim[tri]], ab[prim[tri]], ac[prim[tri]])
    if (~tri).any():
        s = np.ascontiguousarray(spheres, F)[prim[~tri] - len(a)]
        out[~tri] = sphere_f(pts[~tri], s[:, 0:3], s[:, 3])
    return out


def detail(points, prim, positions, spheres=None):
    """(n, 8) float32 detail records of the header for the winning primitives: c.xyz v w side feature 0; zeros for prim < 0."""
    pts = np.ascontiguousarray(points, F)[:, 0:3]
    a, ab, ac = edges(positions)
    prim = np.asarray(prim)
    out = np.zeros((len(pts), 8), F)
    tri = (prim >= 0) & (prim < len(a))
    if tri.any():
        k = prim[tri]
        T = tri_terms(pts[tri], a[k], ab[k], ac[k])
        (t1, t2, t3), (d1, d2, _), e = T["t"], T["d"], T["d_edge"]
        one, zero = F(1), np.zeros(len(k), F)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            vi, wi = T["sv"] / T["nn"], T["sw"] / T["nn"]
            ci = T["p"] - (T["h"] / T["nn"])[:, None] * T["n"]
        feat = np.select([T["interior"], d1 == e, d2 == e], [0, 1, 2], 3)
        v = np.select([feat == 0, feat == 1, feat == 2], [vi, t1, zero], one - t3)
        w = np.select([feat == 0, feat == 1, feat == 2], [wi, zero, t2], t3)
        c = np.select([(feat == 0)[:, None], (feat == 1)[:, None], (feat == 2)[:, None]],
                      [ci, T["a"] + t1[:, None] * T["ab"], T["a"] + t2[:, None] * T["ac"]], (T["a"] + T["ab"]) + t3[:, None] * T["bc"])
        rec = np.zeros((len(k), 8), F)
        rec[:, 0:3], rec[:, 3], rec[:, 4] = c, v, w
        rec[:, 5], rec[:, 6] = np.where(T["h"] >= 0, one, -one), feat.astype(F)
        out[tri] = rec
    sph = prim >= len(a)
    if sph.any():
        s = np.ascontiguousarray(spheres, F)[prim[sph] - len(a)]
        ctr, rad = s[:, 0:3], s[:, 3]
        pc = pts[sph] - ctr
        l = np.sqrt(dot(pc, pc))
        with np.errstate(invalid="ignore", divide="ignore"):
            c = ctr + (rad / l)[:, None] * pc
        c0 = ctr.copy()
        c0[:, 0] = ctr[:, 0] + rad
        rec = np.zeros((int(sph.sum()), 8), F)
        rec[:, 0:3] = np.where((l > 0)[:, None], c, c0)
        rec[:, 5], rec[:, 6] = np.where(l >= rad, F(1), F(-1)), F(4)
        out[sph] = rec
    assert out.dtype == F
    return out


def textbook_d2(points, positions, dtype=np.float64):
    """(n, m) squared distance by the textbook formula (the seven Voronoi regions of a triangle, picked by the signs of d1 .. d6 and
    va, vb, vc), evaluated in `dtype` on the float32 inputs.  In float64 it is an independent statement of what f measures.  In float32
    (one rounding per operation, as numpy gives it) it is what the header decided against: on thin triangles va + vb + vc cancels and
    the distance is lost (tests/test_nearest.py: test_textbook_formula_in_float32_loses_thin_triangles)."""
    dt = np.dtype(dtype).type
    zero, one = dt(0), dt(1)
    a, ab, ac = (x.astype(dt)[None] for x in edges(positions))
    ap = np.ascontiguousarray(points, F)[:, None, 0:3].astype(dt) - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    bp = ap - ab
    d3, d4 = dot(ab, bp), dot(ac, bp)
    cp = ap - ac
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        den = one / ((va + vb) + vc)
        v, w = vb * den, vc * den
        e, g = d4 - d3, d5 - d6
        c = (va <= 0) & (e >= 0) & (g >= 0)
        v, w = np.where(c, one - e / (e + g), v), np.where(c, e / (e + g), w)
        c = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        v, w = np.where(c, zero, v), np.where(c, d2 / (d2 - d6), w)
        c = (d6 >= 0) & (d5 <= d6)
        v, w = np.where(c, zero, v), np.where(c, one, w)
        c = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        v, w = np.where(c, d1 / (d1 - d3), v), np.where(c, zero, w)
        c = (d3 >= 0) & (d4 <= d3)
        v, w = np.where(c, one, v), np.where(c, zero, w)
        c = (d1 <= 0) & (d2 <= 0)
        v, w = np.where(c, zero, v), np.where(c, zero, w)
    r = ap - (v[..., None] * ab + w[..., None] * ac)
    out = dot(r, r)
    assert out.dtype == dt
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# point sets
# ---------------------------------------------------------------------------------------------------------------------------------
def room_points(rs, n):
    """Uniform in the Cornell room (x, z in [-20, 20], y in [0, 40]; scenes_util.scene_rays8's origins)."""
    return np.stack([rs.uniform(-19, 19, n), rs.uniform(1, 39, n), rs.uniform(-19, 30, n)], 1).astype(F)


def surface_points(rs, n, positions, offset=1e-3):
    """On random triangles, every third one moved by a normal draw of size `offset`."""
    pos = np.ascontiguousarray(positions, F).reshape(-1, 3, 3).astype(np.float64)
    k = rs.randint(0, len(pos), n)
    u = rs.uniform(0, 1, (n, 2))
    flip = u.sum(1) > 1
    u[flip] = 1 - u[flip]
    p = pos[k, 0] + u[:, :1] * (pos[k, 1] - pos[k, 0]) + u[:, 1:] * (pos[k, 2] - pos[k, 0])
    p[::3] += rs.standard_normal((len(p[::3]), 3)) * offset
    return p.astype(F)


def vertex_and_edge_points(rs, n, positions):
    """Exactly on vertices (even rows) and exactly representable midpoints-ish of edges (odd rows: (V_i + V_j) * 0.5 in float32):
    points where neighbours sharing the vertex or edge tie."""
    pos = np.ascontiguousarray(positions, F).reshape(-1, 3, 3)
    k, i = rs.randint(0, len(pos), n), rs.randint(0, 3, n)
    p = pos[k, i].copy()
    p[1::2] = (pos[k[1::2], i[1::2]] + pos[k[1::2], (i[1::2] + 1) % 3]) * F(0.5)
    return p


def sliver_triangles(rs, n, length=30.0, width=0.003):
    """(n, 3, 3) float32: triangles `length` long and `width` wide (1:10,000), anywhere in the room and in any direction."""
    a = room_points(rs, n).astype(np.float64)
    u = rs.standard_normal((n, 3))
    u /= np.sqrt((u * u).sum(1, keepdims=True))
    w = np.cross(u, rs.standard_normal((n, 3)))
    w /= np.sqrt((w * w).sum(1, keepdims=True))
    return np.stack([a, a + length * u, a + length * u + width * w], 1).astype(F)


def with_radius(p, radius):
    out = np.zeros((len(p), 4), F)
    out[:, 0:3] = p
    out[:, 3] = radius
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the containment premise of the pruning, on downloaded arrays (Scene.dbg_array: quad, nodes, tri; layouts: csrc/pt_device.h)
# ---------------------------------------------------------------------------------------------------------------------------------
SLACK = F(9.5367431640625e-7)      # 2^-20


def record_boxes(tri_arr):
    """(lo, hi), each (n, 3) float32: the box of (a, a + ab, a + ac) of every tri record, in tree order."""
    t = np.ascontiguousarray(tri_arr, F).reshape(-1, 12)
    return tri_box(t[:, 0:3], t[:, 4:7], t[:, 8:11])


def _leaf_union(lo, hi, ref, seen):
    code = ~int(ref)
    first, cnt = code >> 3, code & 7
    seen[first:first + cnt] += 1
    return lo[first:first + cnt].min(0), hi[first:first + cnt].max(0)


def quad_containment(quad_arr, tri_arr):
    """Walks the 4-wide tree from the root.  Returns (violations, seen): the (node, child) pairs whose box, decoded and widened exactly as
    near_walk_quad does it in float32, does not contain the record box of every triangle below, and how often each triangle was reached."""
    q = np.ascontiguousarray(quad_arr, np.uint32).reshape(-1, 16)
    qf, refs = q.view(F), q[:, 4:8].view(np.int32)
    lo, hi = record_boxes(tri_arr)
    seen, bad = np.zeros(len(lo), np.int64), []

    def node(i):
        org, scl = qf[i, 0:3], np.array([qf[i, 3], qf[i, 14], qf[i, 15]], F)
        sl = (np.abs(org) + F(255) * scl) * SLACK
        got = None
        for k in range(4):
            ref = int(refs[i, k])
            if ref == -1:
                continue
            if ref < 0 and (~ref & 7) == 0:
                continue
            mn, mx = node(ref) if ref >= 0 else _leaf_union(lo, hi, ref, seen)
            blo = (org + scl * ((q[i, 8:11] >> np.uint32(8 * k)) & np.uint32(255)).astype(F)) - sl
            bhi = (org + scl * ((q[i, 11:14] >> np.uint32(8 * k)) & np.uint32(255)).astype(F)) + sl
            assert blo.dtype == F and bhi.dtype == F
            if not ((blo <= mn).all() and (bhi >= mx).all()):
                bad.append((i, k))
            got = (mn, mx) if got is None else (np.minimum(got[0], mn), np.maximum(got[1], mx))
        return got

    node(0)
    return bad, seen


def binary_containment(nodes_arr, tri_arr):
    """The same for the binary tree and widen_binary."""
    rec = np.ascontiguousarray(nodes_arr, F).reshape(-1, 16)
    refs = rec[:, 12:14].view(np.int32)
    lo, hi = record_boxes(tri_arr)
    seen, bad = np.zeros(len(lo), np.int64), []

    def node(i):
        got = None
        for side in (0, 1):
            ref = int(refs[i, side])
            if ref < 0 and (~ref & 7) == 0:
                continue
            mn, mx = node(ref) if ref >= 0 else _leaf_union(lo, hi, ref, seen)
            blo, bhi = rec[i, 6 * side:6 * side + 3], rec[i, 6 * side + 3:6 * side + 6]
            s = np.maximum(np.abs(blo), np.abs(bhi)) * SLACK
            if not ((blo - s <= mn).all() and (bhi + s >= mx).all()):
                bad.append((i, side))
            got = (mn, mx) if got is None else (np.minimum(got[0], mn), np.maximum(got[1], mx))
        return got

    node(0)
    return bad, seen
