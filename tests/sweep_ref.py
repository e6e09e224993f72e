"""The yardstick of tests/test_sweep.py, independent of the code under test: the first-contact parameter tau of include/pt_api.h ("Sphere
casts") and the node test of its walks in numpy, transcribed from the header operation by operation, and brute force over all primitives
with the tie rule.

Every function takes its precision from its arguments: float32 arrays give the header's arithmetic (numpy rounds every operation once
and contracts nothing), float64 arrays the same definition in double.  dot, cross and seg are tests/nearest_ref.py's (the closest-point
section's, which the header refers to); min and max are the header's selects."""
import numpy as np

import nearest_ref as N

F = np.float32
CHUNK = 256      # triangles per block of the brute force
NOW = 2.0 ** -126


def smin(a, b):
    return np.where(b < a, b, a)


def smax(a, b):
    return np.where(b > a, b, a)


def boxdist2(p, lo, hi):
    z = p.dtype.type(0)
    g = smax(smax(lo - p, p - hi), z)
    return (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2]


def tri_box(a, ab, ac):
    b, c = a + ab, a + ac
    return smin(smin(a, b), c), smax(smax(a, b), c)


def first(m, dv, R2):
    dt = m.dtype.type
    with np.errstate(all="ignore"):
        A = N.dot(dv, dv)
        t0 = -N.dot(m, dv) / A
        w = m + t0[..., None] * dv
        k = R2 - N.dot(w, w)
        t = t0 - np.sqrt(k / A)
        ok = (A > 0) & (k >= 0) & (t0 >= 0)
    return np.where(ok, smax(dt(NOW), t), dt(np.inf))


def slab(o, d, r, tmax, lo, hi):
    """Step 2 on the box (lo, hi) inflated by r: (passes, tn)."""
    dt = o.dtype.type
    shape = np.broadcast(o[..., 0], d[..., 0], r, tmax, lo[..., 0]).shape
    n, f, ok = np.zeros(shape, o.dtype), np.broadcast_to(tmax, shape).astype(o.dtype), np.ones(shape, bool)
    for ax in range(3):
        l, h = lo[..., ax] - r, hi[..., ax] + r
        dd, oo = d[..., ax], o[..., ax]
        with np.errstate(all="ignore"):
            inv = dt(1) / dd
            t1, t2 = (l - oo) * inv, (h - oo) * inv
            moving = np.broadcast_to(dd != 0, shape)
            n = np.where(moving, smax(n, smin(t1, t2)), n)
            f = np.where(moving, smin(f, smax(t1, t2)), f)
        ok = ok & (moving | ((l <= oo) & (oo <= h)))
    with np.errstate(invalid="ignore"):
        return ok & (n <= f), n


def node_test(o, d, r, tmax, bound, lo, hi):
    """(entered, key) of a node's box: key 0 where the sphere at its start may reach into the box, else tn."""
    dt = o.dtype.type
    near = boxdist2(o, lo, hi) <= r * r
    ok, tn = slab(o, d, r, tmax, lo, hi)
    with np.errstate(invalid="ignore"):
        return near | (ok & ~(tn > bound)), np.where(near | ~ok, dt(0), tn)


def _inside(ap, ab, ac, bc, n):
    bp = ap - ab
    with np.errstate(invalid="ignore"):
        return (N.dot(N.cross(ab, ap), n) >= 0) & (N.dot(N.cross(bc, bp), n) >= 0) & (N.dot(N.cross(ap, ac), n) >= 0)


def tri_parts(o, d, r, tmax, a, ab, ac):
    """Everything tau of a triangle is made of, for broadcastable arrays of one dtype: (..., 3) vectors, (...) scalars."""
    dt = o.dtype.type
    inf, now = dt(np.inf), dt(NOW)
    o, d, a, ab, ac = np.broadcast_arrays(o, d, a, ab, ac)
    r, tmax = np.broadcast_to(r, o.shape[:-1]), np.broadcast_to(tmax, o.shape[:-1])
    r2 = r * r
    b, c, bc = a + ab, a + ac, ac - ab
    tlo, thi = tri_box(a, ab, ac)
    n, oa = N.cross(ab, ac), o - a
    nn, h = N.dot(n, n), N.dot(oa, n)
    with np.errstate(all="ignore"):
        # 1. overlap
        floor2 = boxdist2(o, tlo, thi)
        d_edge = smin(smin(N.seg(oa, ab)[0], N.seg(oa, ac)[0]), N.seg(oa - ab, bc)[0])
        inside = (nn > 0) & _inside(oa, ab, ac, bc, n)
        d_plane = (h * h) / nn
        d_raw = np.where(inside & (d_plane < d_edge), d_plane, d_edge)
        f = smax(d_raw, floor2)
        overlap = f <= r2
        # 2. the floor
        ok, tn = slab(o, d, r, tmax, tlo, thi)
        # 3. the candidates
        best = np.full(o.shape[:-1], inf, o.dtype)
        dn = N.dot(d, n)
        s = np.where(h >= 0, dt(1), dt(-1))
        ln = np.sqrt(nn)
        g, sdn = s * h - r * ln, s * dn
        t = smax(now, np.where(g > 0, g / -sdn, dt(0)))
        q = (o + t[..., None] * d) - ((s * r) / ln)[..., None] * n
        take = (nn > 0) & (sdn < 0) & _inside(q - a, ab, ac, bc, n)
        best = np.where(take, smin(best, t), best)
        ob = o - b
        for m, e in ((oa, ab), (oa, ac), (ob, bc)):
            ee = N.dot(e, e)
            um, ud = N.dot(m, e) / ee, N.dot(d, e) / ee
            t = first(m - um[..., None] * e, d - ud[..., None] * e, r2)
            u = um + t * ud
            take = (ee > 0) & (0 <= u) & (u <= 1)
            best = np.where(take, smin(best, t), best)
        for m in (oa, ob, o - c):
            best = smin(best, first(m, d, r2))
        # 4. never before the floor
        tau = smax(best, tn)
        tau = np.where(tau <= tmax, tau, inf)
    return dict(f=f, overlap=overlap, ok=ok, tn=tn, raw=best, tau=np.where(overlap, dt(0), np.where(ok, tau, inf)), tlo=tlo, thi=thi)


def tri_tau(o, d, r, tmax, a, ab, ac):
    return tri_parts(o, d, r, tmax, a, ab, ac)["tau"]


def sphere_tau(o, d, r, tmax, ctr, rad):
    dt = o.dtype.type
    inf = dt(np.inf)
    pc = o - ctr
    with np.errstate(all="ignore"):
        l = np.sqrt(N.dot(pc, pc))
        g = l - rad
        out = first(pc, d, (rad + r) * (rad + r))
        R = rad - r
        A = N.dot(d, d)
        t0 = -N.dot(pc, d) / A
        w = pc + t0[..., None] * d
        k = R * R - N.dot(w, w)
        t = t0 + np.sqrt(k / A)
        deep = np.where((A > 0) & (k >= 0), smax(dt(NOW), t), inf)
        tau = np.where(l > rad, out, deep)
        tau = np.where(tau <= tmax, tau, inf)
        return np.where(g * g <= r * r, dt(0), tau)


def split(sweeps, dtype=F):
    """(o, r, d, tmax) of (n, 8) SWEEP8 records, in `dtype`."""
    s = np.ascontiguousarray(sweeps, F).astype(dtype)
    return s[:, 0:3], s[:, 3], s[:, 4:7], s[:, 7]


def tau_matrix(sweeps, positions, spheres=None):
    """(n, primitives) float32: tau of every sweep against every primitive, +inf where there is no contact within tmax."""
    o, r, d, tmax = split(sweeps)
    a, ab, ac = N.edges(positions)
    cols = [tri_tau(o[:, None], d[:, None], r[:, None], tmax[:, None], a[None, lo:lo + CHUNK], ab[None, lo:lo + CHUNK], ac[None, lo:lo + CHUNK])
            for lo in range(0, len(a), CHUNK)]
    if spheres is not None:
        s = np.ascontiguousarray(spheres, F)
        cols.append(sphere_tau(o[:, None], d[:, None], r[:, None], tmax[:, None], s[None, :, 0:3], s[None, :, 3]))
    K = np.concatenate(cols, 1) if cols else np.zeros((len(o), 0), F)
    assert K.dtype == F
    return K


def brute(K, allowed=None):
    """(t, prim) of PT_SWEEP_CLOSEST by definition from the tau matrix K: the smallest tau < +inf, among equals the largest index; a miss is
    (0, -1).  allowed: (n, primitives) bool, the primitives a filter keeps for each sweep."""
    if allowed is not None:
        K = np.where(allowed, K, F(np.inf))
    n, m = K.shape
    if m == 0:
        return np.zeros(n, F), np.full(n, -1, np.int32)
    k = m - 1 - np.argmin(K[:, ::-1], 1)
    t = K[np.arange(n), k]
    hit = t < np.inf
    return np.where(hit, t, F(0)), np.where(hit, k, -1).astype(np.int32)


def centres(sweeps, t):
    """The sphere's centre at contact, o + t * d in float32, as POINT4 records for nearest_ref.detail"""
    o, _, d, _ = split(sweeps)
    out = np.zeros((len(o), 4), F)
    out[:, 0:3] = o + np.asarray(t, F)[:, None] * d
    return out


def detail(sweeps, t, prim, positions, spheres=None):
    return N.detail(centres(sweeps, t), prim, positions, spheres)


# ---------------------------------------------------------------------------------------------------------------------------------
# the families of (sweep, triangle) pairs the definition is measured on
# ---------------------------------------------------------------------------------------------------------------------------------
def _on_triangle(rs, pos):
    p = pos.astype(np.float64)
    u = rs.uniform(0, 1, (len(p), 2))
    flip = u.sum(1) > 1
    u[flip] = 1 - u[flip]
    return p[:, 0] + u[:, :1] * (p[:, 1] - p[:, 0]) + u[:, 1:] * (p[:, 2] - p[:, 0])


def _unit(rs, n):
    u = rs.standard_normal((n, 3))
    return u / np.sqrt((u * u).sum(1, keepdims=True))


def _aimed(rs, pos, rmax, dist, miss):
    """Sweeps aimed at a point on (or, by up to `miss` radii, beside) their triangle from `dist` away, tmax around the distance, the
    direction of any length: hits, grazes, misses and sweeps that end short all occur.  (n, 8) float32."""
    n = len(pos)
    target = _on_triangle(rs, pos)
    r = rs.uniform(0, rmax, n)
    target = target + _unit(rs, n) * (r * rs.uniform(0, miss, n))[:, None]
    u = _unit(rs, n)
    far = rs.uniform(0, dist, n)
    speed = np.exp(rs.uniform(np.log(0.05), np.log(20), n))
    out = np.zeros((n, 8), F)
    out[:, 0:3], out[:, 3], out[:, 4:7] = target - u * far[:, None], r, u * speed[:, None]
    out[:, 7] = far / speed * rs.uniform(0.3, 2.0, n)
    return out


def _tris(name, rs, n):
    if name == "needles":
        return N.sliver_triangles(rs, n)
    a = N.room_points(rs, n).astype(np.float64)
    pos = np.stack([a, a + rs.uniform(-1.5, 1.5, (n, 3)), a + rs.uniform(-1.5, 1.5, (n, 3))], 1).astype(F)
    if name == "far":
        pos = pos + F(131072.0)
    if name == "zero area":
        k = np.arange(n) % 4
        pos[k == 0, 1] = pos[k == 0, 0]                                             # two equal vertices
        pos[k == 1, 2] = pos[k == 1, 1]
        pos[k == 2, 1] = pos[k == 2, 2] = pos[k == 2, 0]                            # a point
        pos[k == 3, 2] = ((pos[k == 3, 0] + pos[k == 3, 1]) * F(0.5)).astype(F)     # collinear
    return pos


FAMILIES = ("ordinary", "needles", "far", "zero area", "radius 0", "tmax 0", "zero direction", "axis parallel", "tmax inf", "starts")


def _shape(name, rs, sw, pos):
    """The sweeps `sw` aimed at the triangles `pos` (row by row), turned into the family `name`; returns them."""
    n = len(sw)
    if name == "radius 0":
        sw[:, 3] = 0
        sw[::2, 0:3] = (_on_triangle(rs, pos)[::2] - sw[::2, 4:7].astype(np.float64) * rs.uniform(0, 3, (n, 1))[::2]).astype(F)      # aimed at the triangle itself
    elif name == "tmax 0":
        sw[:, 7] = 0
        sw[:, 0:3] = (_on_triangle(rs, pos) + _unit(rs, n) * (sw[:, 3].astype(np.float64) * rs.uniform(0, 2, n))[:, None]).astype(F)
    elif name == "zero direction":
        sw[:, 4:7] = 0
        sw[1::2, 4:7] = F(-0.0)
        sw[:, 0:3] = (_on_triangle(rs, pos) + _unit(rs, n) * (sw[:, 3].astype(np.float64) * rs.uniform(0, 2, n))[:, None]).astype(F)
    elif name == "axis parallel":
        k = np.arange(n)
        zero = np.stack([(k % 3 == 0) | (k % 6 == 4), (k % 3 == 1) | (k % 6 == 5), (k % 3 == 2) | (k % 6 == 3)], 1)      # one or two components
        sw[:, 4:7][zero] = 0
        target = _on_triangle(rs, pos) + _unit(rs, n) * (sw[:, 3].astype(np.float64) * rs.uniform(0, 1.5, n))[:, None]
        sw[:, 0:3] = (target - sw[:, 4:7].astype(np.float64) * rs.uniform(0, 3, (n, 1))).astype(F)
    elif name == "tmax inf":
        sw[:, 7] = np.inf
    elif name == "starts":
        # the start inside (0.5 r), on (r, to rounding) and just outside (r + a few ulps .. r + 1e-3 r) the surface, moving any way
        k = np.arange(n) % 4
        away = np.select([k == 0, k == 1, k == 2], [0.5, 1.0, 1.0 + 1e-6 * rs.uniform(0, 1, n)], 1.0 + 1e-3 * rs.uniform(0, 1, n))
        nrm = np.cross(pos[:, 1].astype(np.float64) - pos[:, 0], pos[:, 2].astype(np.float64) - pos[:, 0])
        with np.errstate(invalid="ignore", divide="ignore"):
            nrm /= np.sqrt((nrm * nrm).sum(1, keepdims=True))
        nrm = np.where(np.isfinite(nrm).all(1, keepdims=True), nrm, _unit(rs, n))      # a zero-area triangle has no normal: any direction
        side = np.where(rs.uniform(0, 1, n) < 0.5, -1.0, 1.0)
        sw[:, 0:3] = (_on_triangle(rs, pos) + nrm * (side * away * sw[:, 3].astype(np.float64))[:, None]).astype(F)
        toward = rs.uniform(0, 1, n) < 0.7
        sw[toward, 4:7] = (-nrm * side[:, None] * rs.uniform(0.1, 3, (n, 1)) + _unit(rs, n) * 0.5)[toward].astype(F)
        sw[:, 7] = rs.uniform(0, 4, n)
    return sw


def family(name, seed, n):
    """(sweeps (n, 8), positions (n, 3, 3)) of a family, float32."""
    rs = np.random.RandomState(seed)
    pos = _tris(name, rs, n)
    sw = _aimed(rs, pos, 0.1 if name == "needles" else 2.0, 300.0 if name == "far" else 30.0, 2.5)
    return np.ascontiguousarray(_shape(name, rs, sw, pos), F), pos


KINDS = ("ordinary", "ordinary", "starts", "radius 0", "tmax 0", "zero direction", "axis parallel", "tmax inf", "vertex", "spheres")


def scene_sweeps(positions, spheres, seed, n):
    """n SWEEP8 records against a scene, every kind in every wave: long sweeps aimed at (or beside) random triangles, short ones that
    start inside, on and just outside the surface, thin rays, sweeps that stand still or have tmax 0, axis-parallel and unbounded ones,
    spheres that start exactly on a vertex (ties at tau = 0 among the triangles that share it), and sweeps at the scene's spheres from
    outside and from within."""
    rs = np.random.RandomState(seed)
    pos = np.ascontiguousarray(positions, F).reshape(-1, 3, 3)
    tri = pos[rs.randint(0, len(pos), n)]
    e = tri[:, 1].astype(np.float64) - tri[:, 0]
    edge = float(np.median(np.sqrt((e * e).sum(1))))
    sw = _aimed(rs, tri, min(2.0, 2.0 * edge), 30.0, 2.5)
    kind = np.arange(n) % len(KINDS)
    for j, name in enumerate(KINDS):
        idx = np.nonzero(kind == j)[0]
        if name == "vertex":
            sw[idx, 0:3] = tri[idx, rs.randint(0, 3, len(idx))]
            sw[idx[::2], 3] = 0
        elif name == "spheres":
            if spheres is None:
                continue
            s = np.ascontiguousarray(spheres, F)[rs.randint(0, len(spheres), len(idx))].astype(np.float64)
            u = _unit(rs, len(idx))
            inside = np.arange(len(idx)) % 3 == 0
            start = s[:, 0:3] + u * np.where(inside, 0.3 * s[:, 3], s[:, 3] + rs.uniform(0.5, 20, len(idx)))[:, None]
            aim = s[:, 0:3] + _unit(rs, len(idx)) * (s[:, 3] * rs.uniform(0, 1.3, len(idx)))[:, None]
            sw[idx, 0:3], sw[idx, 4:7] = start, (aim - start) * rs.uniform(0.05, 2, (len(idx), 1))
            sw[idx, 3] = np.where(inside, 0.2 * s[:, 3] * rs.uniform(0, 1, len(idx)), sw[idx, 3])
            sw[idx, 7] = rs.uniform(0.2, 60, len(idx))
        elif name != "ordinary":
            sw[idx] = _shape(name, rs, sw[idx].copy(), tri[idx])
    return np.ascontiguousarray(sw, F)


def kappa(pos):
    """|E1| |E2| / |E1 x E2| of the header's known-defect note, in float64 (inf for a zero-area triangle)"""
    p = pos.astype(np.float64)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt((e1 * e1).sum(1) * (e2 * e2).sum(1)) / np.sqrt((np.cross(e1, e2) ** 2).sum(1))


def sandwich(sweeps, pos, k, scale_by_kappa=False, t32=None):
    """The radius sandwich of a family at the factor k: tau64(r + delta) - eps <= tau32 <= tau64(r - delta) + eps with delta = k 2^-24
    scale (scale = the largest coordinate magnitude of the triangle, the segment's ends and r; times kappa if asked for) and eps =
    k 2^-24 max(tau, 1).  A radius below delta has no lower sphere: its upper bound is +inf.  t32: the float32 tau under test (None: this
    file's own).  Returns (violations below, violations above) as boolean arrays."""
    o, r, d, tmax = split(sweeps)
    a, ab, ac = N.edges(pos)
    t32 = (tri_tau(o, d, r, tmax, a, ab, ac) if t32 is None else np.asarray(t32, F)).astype(np.float64)
    o64, r64, d64, tmax64 = split(sweeps, np.float64)
    a64, ab64, ac64 = a.astype(np.float64), ab.astype(np.float64), ac.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        end = np.where(np.isfinite(tmax64)[:, None], o64 + np.where(np.isfinite(tmax64), tmax64, 0.0)[:, None] * d64, o64)
    scale = np.maximum.reduce([np.abs(pos.astype(np.float64)).max((1, 2)), np.abs(o64).max(1), np.abs(end).max(1), r64])
    if scale_by_kappa:
        scale = scale * np.minimum(kappa(pos), 1e30)
    delta = k * 2.0 ** -24 * scale
    lo = tri_tau(o64, d64, r64 + delta, tmax64, a64, ab64, ac64)
    hi = np.where(r64 - delta >= 0, tri_tau(o64, d64, np.maximum(r64 - delta, 0.0), tmax64, a64, ab64, ac64), np.inf)
    eps = lambda t: k * 2.0 ** -24 * np.maximum(np.where(np.isfinite(t), t, 0.0), 1.0)      # noqa: E731
    with np.errstate(invalid="ignore"):
        below = np.where(np.isfinite(lo), lo - eps(lo), np.inf) > t32
        above = t32 > np.where(np.isfinite(hi), hi + eps(hi), np.inf)
    return below, above
