"""The yardstick of tests/test_tri_queries.py, independent of the code under test: the membership of a query triangle and a primitive with
its section segment (include/pt_api.h, "Triangle queries") and the node test of its walks in numpy, transcribed from the header
operation by operation; brute force over every primitive with the lists' order; the float64 truths the definition is measured against
(the same definition in double, and the triangle-triangle distance); and the seeded families and query sets of the tests.

Every function takes its precision from its arguments: float32 arrays give the header's arithmetic (numpy rounds every operation once
and contracts nothing), float64 arrays the same definition in double.  dot, cross and seg are tests/nearest_ref.py's (the closest-point
section's, which the header refers to); min and max are the header's selects."""
import numpy as np

import nearest_ref as N

F = np.float32
NAN = F(np.nan)


def smin(a, b):
    return np.where(b < a, b, a)


def smax(a, b):
    return np.where(b > a, b, a)


def split(q, dtype=F):
    """(qa, qb, qc) of TRI12 records (n, 12)."""
    q = np.ascontiguousarray(q, F).reshape(-1, 12).astype(dtype)
    return q[:, 0:3], q[:, 4:7], q[:, 8:11]


def records(tri):
    """TRI12 records of (n, 3, 3) vertices; the reserved floats hold 7 (they are not read)."""
    tri = np.ascontiguousarray(tri, F).reshape(-1, 3, 3)
    out = np.full((len(tri), 12), 7, F)
    out[:, 0:3], out[:, 4:7], out[:, 8:11] = tri[:, 0], tri[:, 1], tri[:, 2]
    return out


def lane(qa, qb, qc):
    """What the header forms of the query once: n, the query's box, the inward edge normals."""
    n = N.cross(qb - qa, qc - qa)
    return dict(qa=qa, qb=qb, qc=qc, n=n, lo=smin(smin(qa, qb), qc), hi=smax(smax(qa, qb), qc), m0=N.cross(n, qb - qa), m1=N.cross(n, qc - qb),
                m2=N.cross(n, qa - qc))


def plane(L, v):
    n, qa = L["n"], L["qa"]
    return (n[..., 0] * (v[..., 0] - qa[..., 0]) + n[..., 1] * (v[..., 1] - qa[..., 1])) + n[..., 2] * (v[..., 2] - qa[..., 2])


def tri_key(L, a, ab, ac):
    """(member, p, q) of the header's steps 1 to 4 for pairs: L of (n, 3) arrays, a, ab, ac (n, 3).  p and q are zeros for a non-member."""
    dt = a.dtype.type
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        b, c = a + ab, a + ac
        tlo, thi = smin(smin(a, b), c), smax(smax(a, b), c)
        ok = ((tlo <= L["hi"]) & (thi >= L["lo"])).all(-1)
        da, db, dc = plane(L, a), plane(L, b), plane(L, c)
        ua, ub, uc = da >= 0, db >= 0, dc >= 0
        ok &= ~((ua == ub) & (ub == uc))
        la = (ua != ub) & (ua != uc)
        lb = ~la & (ub != ua) & (ub != uc)
        pick = lambda x, y, z: np.where(la[..., None] if x.ndim > la.ndim else la, x, np.where(lb[..., None] if x.ndim > la.ndim else lb, y, z))      # noqa: E731
        l, v1, v2 = pick(a, b, c), pick(b, c, a), pick(c, a, b)
        dl, d1, d2 = pick(da, db, dc), pick(db, dc, da), pick(dc, da, db)
        t1, t2 = dl / (dl - d1), dl / (dl - d2)
        P, Q = l + t1[..., None] * (v1 - l), l + t2[..., None] * (v2 - l)
        s0, s1 = np.zeros_like(da), np.ones_like(da)
        for m, v in ((L["m0"], L["qa"]), (L["m1"], L["qb"]), (L["m2"], L["qa"])):
            wp, wq = N.dot(m, P - v), N.dot(m, Q - v)
            ip, iq = wp >= 0, wq >= 0
            ok &= ip | iq
            s = wp / (wp - wq)
            s1 = np.where((ip != iq) & ip, smin(s1, s), s1)
            s0 = np.where((ip != iq) & ~ip, smax(s0, s), s0)
        ok &= s0 <= s1
        PQ = Q - P
        p, q = P + s0[..., None] * PQ, P + s1[..., None] * PQ
    z = dt(0)
    return ok, np.where(ok[..., None], p, z).astype(a.dtype), np.where(ok[..., None], q, z).astype(a.dtype)


def closest(p, a, ab, ac):
    """(f, c): f(p, triangle) of the closest-point section with min and max as selects, and the closest point as the detail record forms it."""
    dt = p.dtype.type
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        bc, ap = ac - ab, p - a
        bp = ap - ab
        (d1, t1), (d2, t2), (d3, t3) = N.seg(ap, ab), N.seg(ap, ac), N.seg(bp, bc)
        d_edge = smin(smin(d1, d2), d3)
        n = N.cross(ab, ac)
        nn, h = N.dot(n, n), N.dot(ap, n)
        sw, sa, sv = N.dot(N.cross(ab, ap), n), N.dot(N.cross(bc, bp), n), N.dot(N.cross(ap, ac), n)
        inside = (nn > 0) & (sw >= 0) & (sa >= 0) & (sv >= 0)
        d_plane = (h * h) / nn
        interior = inside & (d_plane < d_edge)
        u = h / nn
        c = np.where(interior[..., None], p - u[..., None] * n,
                     np.where((d1 == d_edge)[..., None], a + t1[..., None] * ab,
                              np.where((d2 == d_edge)[..., None], a + t2[..., None] * ac, (a + ab) + t3[..., None] * bc)))
        d_raw = np.where(interior, d_plane, d_edge)
        b, cc = a + ab, a + ac
        lo, hi = smin(smin(a, b), cc), smax(smax(a, b), cc)
        g = smax(smax(lo - p, p - hi), dt(0))
        floor = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]
        return smax(d_raw, floor), c.astype(p.dtype)


def sphere_key(qa, qb, qc, ctr, rad):
    """(member, c) of the header's sphere rule for pairs."""
    with np.errstate(invalid="ignore", over="ignore"):
        f, c = closest(ctr, qa, qb - qa, qc - qa)
        va, vb, vc = qa - ctr, qb - ctr, qc - ctr
        far2 = smax(smax(N.dot(va, va), N.dot(vb, vb)), N.dot(vc, vc))
        rr = rad * rad
        ok = (f <= rr) & (far2 >= rr)
    return ok, np.where(ok[..., None], c, ctr.dtype.type(0)).astype(ctr.dtype)


def node_test(L, lo, hi):
    """The walks' node test on the box (lo, hi)."""
    with np.errstate(invalid="ignore", over="ignore"):
        over = ((lo <= L["hi"]) & (hi >= L["lo"])).all(-1)
        pos = L["n"] >= 0
        cmin, cmax = np.where(pos, lo, hi), np.where(pos, hi, lo)
        return over & (plane(L, cmin) < 0) & (plane(L, cmax) >= 0)


KSLACK = F(2.0 ** -20)


def widen_binary(lo, hi):
    """The binary walk's widening of a node's box (csrc/pt_nearest.h: widen_binary), float32."""
    s = smax(np.abs(lo), np.abs(hi)) * KSLACK
    return lo - s, hi + s


def quad_box(lo, hi, plo, phi):
    """A box as the 4-wide walk sees it: quantised to 8 bits per axis in the frame of a parent box (plo, phi) that contains it, rounded
    outwards, decoded and widened as near_quad_child_box does: (org + scl * q) -+ (|org| + 255 scl) 2^-20, float32."""
    org = plo
    scl = np.maximum(((phi.astype(np.float64) - plo) / 255.0 * (1 + 1e-6)), 1e-30).astype(F)
    qlo = np.clip(np.floor((lo.astype(np.float64) - org) / scl), 0, 255).astype(F)
    qhi = np.clip(np.ceil((hi.astype(np.float64) - org) / scl), 0, 255).astype(F)
    sl = (np.abs(org) + F(255) * scl) * KSLACK
    return (org + scl * qlo) - sl, (org + scl * qhi) + sl


# ---------------------------------------------------------------------------------------------------------------------------------
# brute force over a scene
# ---------------------------------------------------------------------------------------------------------------------------------
def brute(queries, positions, spheres=None, chunk=64):
    """(counts, (offsets, cls, prim, detail)) by the definition: every query of the TRI12 records against every primitive, members in
    the lists' order (every key is 1: the larger index first), detail (total, 8) = p.xyz q.xyz kind 0."""
    qa, qb, qc = split(queries)
    a, ab, ac = N.edges(positions)
    with np.errstate(invalid="ignore"):
        b, c = a + ab, a + ac
        tlo, thi = smin(smin(a, b), c), smax(smax(a, b), c)
    Lall = lane(qa, qb, qc)
    rows = []
    for s in range(0, len(qa), chunk):
        e = min(s + chunk, len(qa))
        with np.errstate(invalid="ignore"):
            over = ((tlo[None] <= Lall["hi"][s:e, None]) & (thi[None] >= Lall["lo"][s:e, None])).all(-1)      # step 1 alone: the pairs worth a key
        qi, ti = np.nonzero(over)
        L = {k: v[s + qi] for k, v in Lall.items()}
        ok, p, q = tri_key(L, a[ti], ab[ti], ac[ti])
        det = np.zeros((int(ok.sum()), 8), F)
        det[:, 0:3], det[:, 3:6], det[:, 6] = p[ok], q[ok], 1
        rows.append((s + qi[ok], ti[ok].astype(np.int64), det))
    if spheres is not None and len(spheres):
        sp = np.ascontiguousarray(spheres, F)
        for j in range(len(sp)):
            ok, cpt = sphere_key(qa, qb, qc, np.broadcast_to(sp[j, 0:3], qa.shape), np.broadcast_to(sp[j, 3], qa.shape[:1]))
            det = np.zeros((int(ok.sum()), 8), F)
            det[:, 0:3], det[:, 3:6], det[:, 6] = cpt[ok], cpt[ok], 2
            rows.append((np.nonzero(ok)[0], np.full(int(ok.sum()), len(a) + j, np.int64), det))
    own = np.concatenate([r[0] for r in rows]) if rows else np.zeros(0, np.int64)
    prim = np.concatenate([r[1] for r in rows]) if rows else np.zeros(0, np.int64)
    det = np.concatenate([r[2] for r in rows]) if rows else np.zeros((0, 8), F)
    order = np.lexsort((-prim, own))
    own, prim, det = own[order], prim[order].astype(np.int32), det[order]
    counts = np.bincount(own, minlength=len(qa)).astype(np.int32)
    off = np.concatenate([np.zeros(1, np.int64), np.cumsum(counts, dtype=np.int64)])
    return counts, (off, np.ones(len(prim), F), prim, det)


def member_matrix(queries, positions, spheres=None):
    """(n queries, n primitives) bool from brute's list."""
    _, (off, _, prim, _) = brute(queries, positions, spheres)
    n_prims = len(positions) + (0 if spheres is None else len(spheres))
    M = np.zeros((len(off) - 1, n_prims), bool)
    M[np.repeat(np.arange(len(off) - 1), np.diff(off)), prim] = True
    return M


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 truths
# ---------------------------------------------------------------------------------------------------------------------------------
def member64(T, S):
    """The definition in float64 for pairs of (n, 3, 3) triangles: query T, scene triangle S."""
    T, S = T.astype(np.float64), S.astype(np.float64)
    return tri_key(lane(T[:, 0], T[:, 1], T[:, 2]), S[:, 0], S[:, 1] - S[:, 0], S[:, 2] - S[:, 0])[0]


def _segseg(p1, q1, p2, q2):
    """Distance between the segments p1 q1 and p2 q2, (n, 3) float64 (Ericson's closest points with every clamp; zero-length segments
    allowed)."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e, f = (d1 * d1).sum(1), (d2 * d2).sum(1), (d2 * r).sum(1)
    c, b = (d1 * r).sum(1), (d1 * d2).sum(1)
    den = a * e - b * b
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(den > 0, np.clip((b * f - c * e) / den, 0, 1), 0.0)
        s = np.where(a > 0, s, 0.0)
        t = np.where(e > 0, (b * s + f) / e, 0.0)
        s = np.where(t < 0, np.clip(np.where(a > 0, -c / a, 0.0), 0, 1), np.where(t > 1, np.clip(np.where(a > 0, (b - c) / a, 0.0), 0, 1), s))
        t = np.clip(t, 0, 1)
    g = (p1 + s[:, None] * d1) - (p2 + t[:, None] * d2)
    return np.sqrt((g * g).sum(1))


def point_tri64(p, S):
    """Distance from the points p (n, 3) to the triangles S (n, 3, 3), float64."""
    S = S.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(N.tri_f(p.astype(np.float64), S[:, 0], S[:, 1] - S[:, 0], S[:, 2] - S[:, 0]))


def distance64(T, S):
    """The float64 distance between the triangles of each pair: 0 where they cross (either as the query of the float64 definition), else the
    minimum over the nine edge pairs and the six vertex-face pairs."""
    T, S = T.astype(np.float64), S.astype(np.float64)
    d = np.full(len(T), np.inf)
    for i in range(3):
        for j in range(3):
            d = np.minimum(d, _segseg(T[:, i], T[:, (i + 1) % 3], S[:, j], S[:, (j + 1) % 3]))
    for i in range(3):
        d = np.minimum(d, point_tri64(T[:, i], S))
        d = np.minimum(d, point_tri64(S[:, i], T))
    return np.where(member64(T, S) | member64(S, T), 0.0, d)


def kappa(pos):
    """|E1| |E2| / |E1 x E2| in float64 (inf for a zero-area triangle)"""
    p = pos.astype(np.float64)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt((e1 * e1).sum(1) * (e2 * e2).sum(1)) / np.sqrt((np.cross(e1, e2) ** 2).sum(1))


def frame64(T):
    """(unit normal, two in-plane unit directions) of (n, 3, 3) triangles in float64; a zero-area triangle gets the axes."""
    T = T.astype(np.float64)
    e0 = T[:, 1] - T[:, 0]
    n = np.cross(e0, T[:, 2] - T[:, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        n = n / np.sqrt((n * n).sum(1, keepdims=True))
        u = e0 / np.sqrt((e0 * e0).sum(1, keepdims=True))
    bad = ~(np.isfinite(n).all(1) & np.isfinite(u).all(1))
    n[bad], u[bad] = [0, 0, 1], [1, 0, 0]
    return n, u, np.cross(n, u)


def truth(T, S, k, member32, p32, q32, by_kappa=False):
    """The two implications and the segment bound of a family at the factor k, delta = k 2^-24 scale (scale: the largest coordinate
    magnitude of the pair, times the scene triangle's kappa if asked for).  Returns boolean arrays (lower violated: a float64 member
    for T and its six translates by delta that float32 misses; upper violated: a float32 member farther than delta apart in float64;
    segment violated: p or q farther than delta from either triangle) and the mask of the pairs neither implication constrains."""
    scale = np.maximum(np.abs(T.astype(np.float64)).max((1, 2)), np.abs(S.astype(np.float64)).max((1, 2)))
    if by_kappa:
        scale = scale * np.minimum(kappa(S), 1e30)
    delta = k * 2.0 ** -24 * scale
    n, u, v = frame64(T)
    T64 = T.astype(np.float64)
    all7 = member64(T64, S)
    for d in (n, u, v):
        for sgn in (1.0, -1.0):
            all7 &= member64(T64 + (sgn * delta)[:, None, None] * d[:, None, :], S)
    dist = distance64(T, S)
    lower = all7 & ~member32
    upper = member32 & ~(dist <= delta)
    seg = np.zeros(len(T), bool)
    m = member32
    for x in (p32, q32):
        seg[m] |= ~(point_tri64(x[m], T[m]) <= delta[m]) | ~(point_tri64(x[m], S[m]) <= delta[m])
    free = ~all7 & (dist <= delta)
    return lower, upper, seg, free


# ---------------------------------------------------------------------------------------------------------------------------------
# the families of the CPU tests: pairs (query triangle, scene triangle) or (query triangle, sphere)
# ---------------------------------------------------------------------------------------------------------------------------------
def _unit(rs, n):
    u = rs.standard_normal((n, 3))
    return u / np.sqrt((u * u).sum(1, keepdims=True))


def _cube_tris(rs, n, centre, side):
    return centre[:, None, :] + rs.uniform(-side / 2, side / 2, (n, 3, 3))


def _ordinary(rs, n, centre_range=18.0, side=1.5):
    ctr = rs.uniform(-centre_range, centre_range, (n, 3)) + [0, 20, 0]
    S = _cube_tris(rs, n, ctr, side)
    T = _cube_tris(rs, n, ctr + rs.uniform(-0.3, 0.3, (n, 3)), side)
    return T, S


def family(name, seed, n):
    """(T, S): (n, 3, 3) float32 query and scene triangles of a family."""
    rs = np.random.RandomState(seed)
    if name == "ordinary":
        T, S = _ordinary(rs, n)
    elif name == "far":
        T, S = _ordinary(rs, n)
        shift = _unit(rs, n) * 2.0 ** 17
        T, S = T + shift[:, None, :], S + shift[:, None, :]
    elif name == "needles":
        a = rs.uniform(-18, 18, (n, 3)) + [0, 20, 0]
        d = _unit(rs, n)
        w = np.cross(d, _unit(rs, n))
        w /= np.sqrt((w * w).sum(1, keepdims=True))
        S = np.stack([a, a + 30.0 * d + 0.0015 * w, a + 30.0 * d - 0.0015 * w], 1)
        at = a + d * rs.uniform(3, 27, (n, 1))
        T = _cube_tris(rs, n, at + rs.uniform(-0.15, 0.15, (n, 3)), 1.5)
    elif name == "zero-area scene":
        T, S = _ordinary(rs, n, side=1.5)
        e0, e1 = S[:, 0].copy(), S[:, 1].copy()                                  # the segment the triangle collapses to
        k = np.arange(n) % 3
        S[k == 0, 2] = e1[k == 0]                                                # two vertices equal
        S[k == 1, 2] = (e0 + 0.5 * (e1 - e0))[k == 1]                            # three on a line (to rounding)
        S[k == 2, 1], S[k == 2, 2] = e0[k == 2], e1[k == 2]
        at = e0 + rs.uniform(0.2, 0.8, (n, 1)) * (e1 - e0)
        u = _unit(rs, n)                                                         # the query: a fat triangle about a point near the segment
        v = np.cross(u, _unit(rs, n))
        v /= np.sqrt((v * v).sum(1, keepdims=True))
        th = rs.uniform(0, 2 * np.pi, (n, 1)) + np.array([0.0, 2 * np.pi / 3, 4 * np.pi / 3]) + rs.uniform(-0.5, 0.5, (n, 3))
        r = rs.uniform(0.4, 1.2, (n, 3))
        T = at[:, None, :] + rs.uniform(-0.35, 0.35, (n, 1, 3)) + (r * np.cos(th))[:, :, None] * u[:, None, :] + (r * np.sin(th))[:, :, None] * v[:, None, :]
    elif name == "zero-area query":
        T, S = _ordinary(rs, n)
        k = np.arange(n) % 3
        T[k == 0, 2] = T[k == 0, 1]
        T[k == 1, 2] = T[k == 1, 0]
        T[k == 2] = T[k == 2, 0:1]                                               # a point
    elif name == "nan query":
        T, S = _ordinary(rs, n)
        T = T.astype(F)
        T[np.arange(n), rs.randint(0, 3, n), rs.randint(0, 3, n)] = NAN
        T[::5] = NAN
    elif name == "near-coplanar":
        T, S = _ordinary(rs, n)
        nrm = frame64(S)[0]
        tilt = _unit(rs, n) * rs.choice([1e-2, 1e-4, 1e-6], (n, 1))
        ctr = S.mean(1)
        rel = rs.uniform(-0.9, 0.9, (n, 3, 3))
        rel -= (rel * nrm[:, None, :]).sum(2, keepdims=True) * nrm[:, None, :]                       # in S's plane ...
        rel += (rel * tilt[:, None, :]).sum(2, keepdims=True) * nrm[:, None, :] * 1.0                # ... tilted about a line through its middle
        T = ctr[:, None, :] + rel
    elif name == "on the plane":
        # the query in an axis plane z = z0 with grid coordinates, the scene triangle's vertices on the grid with z in {z0 - 1, z0, z0 + 1}: exact
        # arithmetic, vertices ON the plane in most pairs — the half-open rule decides
        ax = rs.randint(0, 3, n)
        z0 = rs.randint(-8, 9, n).astype(np.float64)
        g = lambda lo, hi, shape: rs.randint(lo, hi + 1, shape).astype(np.float64)      # noqa: E731
        T = g(-4, 4, (n, 3, 3))
        S = g(-3, 3, (n, 3, 3))
        T[:, :, 2] = z0[:, None]
        S[:, :, 2] = z0[:, None] + g(-1, 1, (n, 3))
        roll = lambda X: np.where((ax == 0)[:, None, None], X[:, :, [2, 0, 1]], np.where((ax == 1)[:, None, None], X[:, :, [1, 2, 0]], X))      # noqa: E731
        T, S = roll(T), roll(S)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(T, F), np.ascontiguousarray(S, F)


TRI_FAMILIES = ("ordinary", "needles", "far", "zero-area scene", "zero-area query", "nan query", "near-coplanar", "on the plane")
NO_MEMBERS = ("zero-area query", "nan query")      # by definition no triangle member: exempt from the member half of the condition


def sphere_family(seed, n):
    """(T (n, 3, 3), spheres (n, 4)): query triangles against a sphere from outside, across its surface and within it."""
    rs = np.random.RandomState(seed)
    ctr = rs.uniform(-18, 18, (n, 3)) + [0, 20, 0]
    rad = rs.uniform(0.3, 3.0, n)
    k = np.arange(n) % 4
    dist = np.select([k == 0, k == 1, k == 2], [rs.uniform(1.0, 1.6, n), rs.uniform(0.7, 1.2, n), rs.uniform(0.0, 0.6, n)], 1.0) * rad
    at = ctr + _unit(rs, n) * dist[:, None]
    size = np.where(k == 2, rs.uniform(0.05, 0.5, n), rs.uniform(0.3, 1.5, n)) * rad
    T = at[:, None, :] + rs.uniform(-1, 1, (n, 3, 3)) * size[:, None, None]
    on = k == 3                                    # a vertex ON the surface, to rounding
    T[on, 0] = ctr[on] + _unit(rs, int(on.sum())) * rad[on, None]
    return np.ascontiguousarray(T, F), np.ascontiguousarray(np.concatenate([ctr, rad[:, None]], 1), F)


def closed_mesh(n_lat=9, n_lon=14, R=6.0, centre=(1.3, 17.0, -2.1)):
    """(m, 3, 3) float32 positions of a closed lat-lon sphere, bumpy so that no two vertices share a height: pole fans and split quads, every
    edge shared by exactly two triangles, the shared vertices the same floats, outward winding."""
    def P(i, j):
        j = j % n_lon
        th, ph = np.pi * i / n_lat, 2 * np.pi * j / n_lon
        r = R * (1.0 + 0.07 * np.sin(3.0 * th + 0.4) * np.cos(2.0 * ph + 0.3))
        if i in (0, n_lat):
            return np.asarray(centre) + [0.0, R if i == 0 else -R, 0.0]      # one pole whatever j
        return np.asarray(centre) + r * np.array([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)])
    tris = []
    for i in range(n_lat):
        for j in range(n_lon):
            p00, p01, p10, p11 = P(i, j), P(i, j + 1), P(i + 1, j), P(i + 1, j + 1)
            if i > 0:
                tris.append([p00, p01, p11] if i == n_lat - 1 else [p00, p01, p10])
            if 0 < i < n_lat - 1:
                tris.append([p01, p11, p10])
            if i == 0:
                tris.append([p00, p11, p10])
    return np.ascontiguousarray(tris, F)


# ---------------------------------------------------------------------------------------------------------------------------------
# query sets against a scene
# ---------------------------------------------------------------------------------------------------------------------------------
def scene_queries(positions, spheres, seed, n):
    """TRI12 records against a scene, every kind in every wave: triangles of the scene's own size placed on its surface, two slicing
    quads (four triangles) through the whole scene, zero-area and NaN queries, a few at the spheres."""
    rs = np.random.RandomState(seed)
    pos = np.ascontiguousarray(positions, F).reshape(-1, 3, 3).astype(np.float64)
    k = rs.randint(0, len(pos), n)
    tri = pos[k]
    e = tri[:, 1] - tri[:, 0]
    edge = float(np.median(np.sqrt((e * e).sum(1))))
    edge = edge if edge > 0 else 1.0
    w = rs.dirichlet([1, 1, 1], n)
    at = (tri * w[:, :, None]).sum(1)
    T = at[:, None, :] + rs.uniform(-1, 1, (n, 3, 3)) * edge * rs.choice([0.5, 1.0, 3.0], (n, 1, 1))
    kind = np.arange(n) % 16
    T[kind == 5, 2] = T[kind == 5, 1]                                       # zero area
    if spheres is not None and len(spheres):
        s = np.ascontiguousarray(spheres, F).astype(np.float64)
        idx = np.nonzero(kind == 9)[0]
        sj = s[rs.randint(0, len(s), len(idx))]
        T[idx] = (sj[:, 0:3] + _unit(rs, len(idx)) * (sj[:, 3] * rs.choice([0.3, 1.0, 1.5], len(idx)))[:, None])[:, None, :] + \
            rs.uniform(-1, 1, (len(idx), 3, 3)) * (sj[:, 3] * 0.6)[:, None, None]
    T = np.ascontiguousarray(T, F)
    nan_rows = np.nonzero(kind == 11)[0]
    T[nan_rows, rs.randint(0, 3, len(nan_rows)), rs.randint(0, 3, len(nan_rows))] = NAN
    # the slicing quads: one axis plane through the middle, one slanted, each larger than the scene
    v = pos.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    mid, ext = (lo + hi) / 2, float((hi - lo).max()) * 0.75 + 1.0
    quads = []
    for nrm in ([0.0, 1.0, 0.0], [0.3, 0.8, -0.52]):
        nrm = np.asarray(nrm) / np.linalg.norm(nrm)
        u = np.cross(nrm, [1.0, 0.0, 0.0])
        u /= np.linalg.norm(u)
        w2 = np.cross(nrm, u)
        c = mid + nrm * 0.013
        p00, p10, p11, p01 = c - ext * u - ext * w2, c + ext * u - ext * w2, c + ext * u + ext * w2, c - ext * u + ext * w2
        quads += [[p00, p10, p11], [p00, p11, p01]]
    quads = np.ascontiguousarray(quads, F)
    slots = np.nonzero(kind == 13)[0][:4]
    T[slots] = quads[:len(slots)]
    return records(T)
