"""The yardstick of tests/test_ray_hits.py: the first K hits along a ray and the hit count as include/pt_api.h defines them ("First K hits
along a ray and hit counts"), evaluated in numpy float32 over every (ray, primitive) pair.  No tree is walked and nothing of
csrc/pt_trace.h is compiled: the hit set H of a ray is what the header's acceptance rules admit, sorted by (t ascending as floats, the
larger prim first).  Every numpy float32 operation rounds once, as the device's do (no contraction, correctly rounded divide and sqrt).

Also the sheet-stack scene and the seeded ray sets of the tests (RAY8 records: org.xyz dir.xyz 0 tmax)."""
from collections import namedtuple

import numpy as np

from scenes_util import make_prims

F = np.float32
EPS = F(1e-4)            # kEps
K_FAR = F(1.00000024)    # the reference's scaling of the slab test's far side
T_FAR = F(999999.0)
KS = (1, 2, 5, 8, 9, 32)      # both sides of every capacity class (4, 8, 16, 32) and the ends of the range
KMAX = 32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _cross(ax, ay, az, bx, by, bz):
    return ay * bz - az * by, -(ax * bz - az * bx), ax * by - ay * bx


def tri_v0e1e2(tris88):
    """(m, 9) float32 V0 E1 E2 from PtTriangle records (the fields v0, E1, E2)."""
    t = np.ascontiguousarray(tris88, F)
    return np.ascontiguousarray(np.concatenate([t[:, 0:3], t[:, 39:42], t[:, 42:45]], 1))


def tri_eval(rays, tris9):
    """det, t, u, v of every (ray, triangle) pair, (n, m) float32 each, and the range tests of the two sides (no leaf box):
    front = Triangle::hit's tests for [0, tmax]; back = the same on -det, -u, -v where the front's det test fails."""
    r, q = np.asarray(rays, F), np.asarray(tris9, F)
    o = [r[:, k][:, None] for k in range(3)]
    d = [r[:, 3 + k][:, None] for k in range(3)]
    tmax = r[:, 7][:, None]
    v0 = [q[:, k][None, :] for k in range(3)]
    e1 = [q[:, 3 + k][None, :] for k in range(3)]
    e2 = [q[:, 6 + k][None, :] for k in range(3)]
    with np.errstate(all="ignore"):
        T = [o[k] - v0[k] for k in range(3)]
        P = _cross(*d, *e2)
        Q = _cross(*T, *e1)
        det = _dot(*P, *e1)
        t = _dot(*Q, *e2) * (F(1) / det)
        u = _dot(*P, *T)
        v = _dot(*Q, *d)
        ranges = lambda dd, uu, vv: ~(dd < EPS) & ~(t < 0) & ~(t > tmax) & ~((uu < 0) | (uu > dd)) & ~((vv < 0) | (vv + uu > dd))      # noqa: E731
        front = ranges(det, u, v)
        back = (det < EPS) & ranges(-det, -u, -v)
    assert det.dtype == F and t.dtype == F and u.dtype == F and v.dtype == F
    return det, t, u, v, front, back


def inv_dir(rays):
    """Normalize(1 / dir) as the reference forms it, (n, 3), and which rays are degenerate (its length not finite: a zero component)."""
    d = np.asarray(rays, F)[:, 3:6]
    with np.errstate(all="ignore"):
        inv = F(1) / d
        L = np.sqrt((inv[:, 0] * inv[:, 0] + inv[:, 1] * inv[:, 1]) + inv[:, 2] * inv[:, 2])
        return (inv / L[:, None]).astype(F), ~(L < F(np.inf))


def box_pass(rays, boxes6):
    """(n, b) bool: the reference's slab test (far side scaled by 1.00000024, entry clamped at 0, no cull) of every box (lo.xyz hi.xyz)
    for every ray, non-degenerate arithmetic (the caller overrides degenerate rays)."""
    r, b = np.asarray(rays, F), np.asarray(boxes6, F)
    invD, _ = inv_dir(r)
    with np.errstate(all="ignore"):
        mn, mx = [], []
        for k in range(3):
            t1 = (b[:, k][None, :] - r[:, k][:, None]) * invD[:, k][:, None]
            t2 = (b[:, 3 + k][None, :] - r[:, k][:, None]) * invD[:, k][:, None]
            mn.append(np.fmin(t1, t2))
            mx.append(np.fmax(t1, t2))
        tn = np.fmax(mn[2], np.fmax(mn[1], np.fmax(mn[0], F(0))))
        tf = np.fmin(mx[2], np.fmin(mx[1], mx[0])) * K_FAR
        return tn <= tf


def sphere_eval(rays, spheres):
    """r1, r2 (n, s) float32 and their validity (disc >= 0 included) for [0, tmax]."""
    r, s = np.asarray(rays, F), np.asarray(spheres, F).reshape(-1, 16)
    o = [r[:, k][:, None] for k in range(3)]
    d = [r[:, 3 + k][:, None] for k in range(3)]
    tmax = r[:, 7][:, None]
    with np.errstate(all="ignore"):
        oc = [o[k] - s[:, k][None, :] for k in range(3)]
        a = _dot(*d, *d)
        half_b = _dot(*oc, *d)
        c = _dot(*oc, *oc) - (s[:, 3] * s[:, 3])[None, :]
        disc = half_b * half_b - a * c
        sq = np.sqrt(disc)
        r1, r2 = (-half_b - sq) / a, (-half_b + sq) / a
        ok = ~(disc < 0)
        v1 = ok & ~(r1 < 0) & ~(tmax < r1)
        v2 = ok & ~(r2 < 0) & ~(tmax < r2)
    assert r1.dtype == F and r2.dtype == F
    return r1, r2, v1, v2


def leaf_of_tri(nodes):
    """For every triangle (the order of `tris`) the index of its reference leaf among the leaves in node order, and the leaves' boxes
    (n_leaves, 6): the leaf whose primStart..primEnd holds the triangle."""
    leaf = (nodes["primStart"] != -1) & (nodes["primEnd"] != -1)
    ls = nodes[leaf]
    n = int(ls["primEnd"].max()) + 1
    of = np.full(n, -1, np.int64)
    for i, (a, b) in enumerate(zip(ls["primStart"], ls["primEnd"])):
        assert (of[a:b + 1] == -1).all()
        of[a:b + 1] = i
    assert (of >= 0).all()
    return of, np.concatenate([ls["bMin"], ls["bMax"]], 1).astype(F)


Hits = namedtuple("Hits", "t prim facing bu bv count")      # (n, M) each, sorted, padded with (0, -1, 0, 0, 0); count (n,)


def brute(rays, tris9, leaf_boxes, spheres, both_sides):
    """The full sorted H of every ray.  tris9: (m, 9) V0 E1 E2; leaf_boxes: (m, 6), the reference leaf box of each triangle; spheres:
    (s, 16) or None.  bu, bv: u * (1 / det), v * (1 / det) of a triangle's record, 0 for a sphere's."""
    rays = np.ascontiguousarray(rays, F)
    n, m = len(rays), len(tris9)
    det, t, u, v, front, back = tri_eval(rays, tris9)
    _, deg = inv_dir(rays)
    acc = (front | back) if both_sides else front
    # the leaf-box condition, evaluated on the distinct boxes
    ub, which = np.unique(np.asarray(leaf_boxes, F), axis=0, return_inverse=True)
    acc &= box_pass(rays, ub)[:, which.reshape(-1)] | deg[:, None]
    with np.errstate(all="ignore"):
        inv_det = F(1) / det
        cols_t, cols_p = [t], [np.broadcast_to(np.arange(m)[None, :], (n, m))]
        cols_a, cols_f = [acc], [np.where(back, F(-1), F(1))]
        cols_u, cols_v = [u * inv_det], [v * inv_det]
    if spheres is not None and len(spheres):
        r1, r2, v1, v2 = sphere_eval(rays, spheres)
        s = r1.shape[1]
        sp = np.broadcast_to(m + np.arange(s)[None, :], (n, s))
        z = np.zeros((n, s), F)
        if both_sides:
            cols_t += [r1, r2]; cols_a += [v1, v2 & (r2 != r1)]; cols_f += [z + 1, z - 1]
        else:
            cols_t += [np.where(v1, r1, r2), r2]; cols_a += [v1 | v2, np.zeros((n, s), bool)]; cols_f += [np.where(v1, F(1), F(-1)), z - 1]
        cols_p += [sp, sp]; cols_u += [z, z]; cols_v += [z, z]
    t, p, a, f, bu, bv = (np.concatenate(c, 1) for c in (cols_t, cols_p, cols_a, cols_f, cols_u, cols_v))
    with np.errstate(all="ignore"):
        tkey = np.where(a, t + F(0), F(np.inf))      # -0 + 0 = +0: compared as floats
    order = np.lexsort((-p, tkey, ~a), axis=1)       # accepted first, t ascending, the larger prim first; stable: r1 before r2
    count = a.sum(1).astype(np.int32)
    M = max(int(count.max()) if n else 0, 1)
    order = order[:, :M]
    take = lambda x: np.take_along_axis(x, order, 1)      # noqa: E731
    live = np.arange(M)[None, :] < count[:, None]
    return Hits(np.where(live, take(t), F(0)).astype(F), np.where(live, take(p), -1).astype(np.int32), np.where(live, take(f), F(0)).astype(F),
                np.where(live, take(bu), F(0)).astype(F), np.where(live, take(bv), F(0)).astype(F), count)


def lists(h, k):
    """(t, prim, detail) of shape (n, k), (n, k), (n, k, 4): the first k members of H, the later slots the miss record and zeros."""
    n, M = h.t.shape
    pad = max(k - M, 0)
    cut = lambda x, fill: np.concatenate([x[:, :k], np.full((n, pad), fill, x.dtype)], 1)      # noqa: E731
    t, prim = cut(h.t, F(0)), cut(h.prim, np.int32(-1))
    det = np.stack([cut(h.bu, F(0)), cut(h.bv, F(0)), cut(h.facing, F(0)), np.zeros((n, k), F)], 2)
    return np.ascontiguousarray(t), np.ascontiguousarray(prim), np.ascontiguousarray(det)


def figures(h, k):
    """What a ray set holds at K = k: the numbers of rays with more than k members, with 1 .. k - 1, with none, with an exact tie in t
    between slot k - 1 and the first member left out, and with a tie between two slots of the list."""
    n, M = h.t.shape
    c = h.count
    cut = np.zeros(n, bool)
    if M > k:
        cut = (c > k) & (h.t[:, k - 1] == h.t[:, k])
    kk = min(k, M)
    inside = ((h.t[:, 1:kk] == h.t[:, :kk - 1]) & (np.arange(1, kk)[None, :] < c[:, None])).any(1) if kk > 1 else np.zeros(n, bool)
    return {"more": int((c > k).sum()), "fewer": int(((c >= 1) & (c < k)).sum()), "none": int((c == 0).sum()), "cut_ties": int(cut.sum()),
            "inside_ties": int(inside.sum())}


# ---------------------------------------------------------------------------------------------------------------------------------
# the sheet stack
# ---------------------------------------------------------------------------------------------------------------------------------
SHEET_LAYERS = 40
SHEET_DUPLICATED = (5, 17, 30)      # these layers are in the scene twice, at identical z
SHEET_X0, SHEET_Y0, SHEET_SIDE = -4.0, 16.0, 8.0
SHEET_Z0, SHEET_DZ = -10.0, 0.5


def sheet_z(i):
    return SHEET_Z0 + SHEET_DZ * i


def sheet_stack():
    """(87, 84) Primitive records: 40 parallel quads of two triangles each along z (x in [-4, 4], y in [16, 24], z = -10 + i / 2), the
    layers 5, 17 and 30 a second time at identical z (appended after the 40, so the copy has the larger index), every fourth layer
    (i % 4 == 3) wound the other way, so that it faces -z where the others face +z; one emissive triangle above them."""
    x0, y0, x1, y1 = SHEET_X0, SHEET_Y0, SHEET_X0 + SHEET_SIDE, SHEET_Y0 + SHEET_SIDE
    A, B, Cc = [], [], []
    for i in list(range(SHEET_LAYERS)) + list(SHEET_DUPLICATED):
        z = sheet_z(i)
        a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
        if i % 4 == 3:
            A += [a, a]; B += [c, d]; Cc += [b, c]
        else:
            A += [a, a]; B += [b, c]; Cc += [c, d]
    quads = make_prims(np.array(A, F), np.array(B, F), np.array(Cc, F))
    light = make_prims(np.array([[-3, 39, -3]], F), np.array([[3, 39, -3]], F), np.array([[0, 39, 3]], F), albedo=(0, 0, 0), emit=(6, 6, 6))
    return np.concatenate([quads, light])


def sheet_spheres():
    """Two spheres on the stack's axis: one in its middle (rays along z cross sheets inside it and on both sides), one in front of it."""
    def sph(c, r):
        return [*c, r, 0, 0, 0, 0.8, 0.8, 0.8, 0.04, 0.04, 0.04, 1.0, 0.5, 0.0]
    return np.array([sph((0.5, 20.5, 0.25), 2.25), sph((-1.0, 19.0, 14.0), 1.5)], F)


def rays8(org, d, tmax):
    n = len(d)
    org = np.broadcast_to(np.asarray(org, F), (n, 3))
    tmax = np.broadcast_to(np.asarray(tmax, F), (n,))
    return np.ascontiguousarray(np.concatenate([org, np.asarray(d, F), np.zeros((n, 1), F), tmax[:, None]], 1), F)


def sheet_rays(seed, m):
    """7 m rays: m along -z and m along +z through the quads' interiors (degenerate: two zero components), m / 2 each along the shared
    diagonal (x - x0 == y - y0 exactly) and along the edges x = x0 and y = y0, m oblique through the whole stack, m oblique segments
    with an un-normalised direction and tmax = 1 that start and end inside it, m short ones from between two layers (few hits or
    none), m from inside the first sphere."""
    rs = np.random.RandomState(seed)
    x0, y0, s = SHEET_X0, SHEET_Y0, SHEET_SIDE
    zlo, zhi = sheet_z(0), sheet_z(SHEET_LAYERS - 1)
    grid = lambda k: (rs.randint(1, 512, k) / 64.0).astype(F)      # noqa: E731  exact in float32, inside (0, 8)
    parts = []
    for sign in (-1.0, 1.0):
        org = np.stack([x0 + grid(m), y0 + grid(m), np.full(m, zhi + 8.0 if sign < 0 else zlo - 8.0)], 1)
        parts.append(rays8(org, np.tile(F([0, 0, sign]), (m, 1)), T_FAR))
    h = m // 2
    g = grid(h)
    sign = np.where(np.arange(h) % 2 == 0, -1.0, 1.0)
    z_of = np.where(sign < 0, zhi + 8.0, zlo - 8.0)
    parts.append(rays8(np.stack([x0 + g, y0 + g, z_of], 1), np.stack([0 * sign, 0 * sign, sign], 1), T_FAR))      # the diagonal
    e = np.arange(h) % 2 == 0
    parts.append(rays8(np.stack([np.where(e, x0, x0 + g), np.where(e, y0 + g, y0), z_of], 1), np.stack([0 * sign, 0 * sign, sign], 1), T_FAR))
    a = np.stack([x0 + rs.uniform(0.5, s - 0.5, m), y0 + rs.uniform(0.5, s - 0.5, m), np.full(m, zhi + 6.0)], 1)
    b = np.stack([x0 + rs.uniform(0.5, s - 0.5, m), y0 + rs.uniform(0.5, s - 0.5, m), np.full(m, zlo - 6.0)], 1)
    flip = (np.arange(m) % 2 == 1)[:, None]
    a, b = np.where(flip, b, a), np.where(flip, a, b)
    d = (b - a) / np.sqrt(((b - a) ** 2).sum(1, keepdims=True))
    parts.append(rays8(a, d, T_FAR))
    za, zb = rs.uniform(zlo + 0.1, zhi - 0.1, m), rs.uniform(zlo + 0.1, zhi - 0.1, m)
    a = np.stack([x0 + rs.uniform(0.5, s - 0.5, m), y0 + rs.uniform(0.5, s - 0.5, m), za], 1)
    b = np.stack([x0 + rs.uniform(0.5, s - 0.5, m), y0 + rs.uniform(0.5, s - 0.5, m), zb], 1)
    parts.append(rays8(a, b - a, 1.0))
    org = np.stack([x0 + rs.uniform(0.5, s - 0.5, m), y0 + rs.uniform(0.5, s - 0.5, m), rs.uniform(zlo, zhi, m)], 1)
    d = rs.standard_normal((m, 3))
    d /= np.sqrt((d * d).sum(1, keepdims=True))
    parts.append(rays8(org, d, rs.uniform(0.05, 1.5, m)))
    c = sheet_spheres()[0]
    w = rs.standard_normal((m, 3))
    w /= np.sqrt((w * w).sum(1, keepdims=True))
    org = c[None, 0:3] + w * rs.uniform(0, 0.9, (m, 1)) * c[3]
    d = rs.standard_normal((m, 3))
    d[: m // 2] = [0, 0, -1]
    d /= np.sqrt((d * d).sum(1, keepdims=True))
    parts.append(rays8(org, d, T_FAR))
    r = np.concatenate(parts)
    return np.ascontiguousarray(r[rs.permutation(len(r))], F)      # every wave holds every kind


def scene_rays(seed, m, pos, spheres):
    """About 5 m rays for a meshed room (positions (n, 3, 3); spheres (s, 16) or None): m long rays from the room's rim aimed at points of
    random triangles (interiors, vertices, edge midpoints) — they pass through the mesh, several hits each —, m of them continued from
    behind the mesh the other way, m un-normalised segments with tmax = 1 between points around the mesh, m axis-aligned rays through
    triangle points (degenerate), m / 2 short rays that stop before or just behind their first surface, and with spheres m / 2 aimed at
    them from outside and m / 2 starting inside one."""
    rs = np.random.RandomState(seed)
    pos = np.asarray(pos, F)
    v = pos.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    ctr, ext = 0.5 * (lo + hi), (hi - lo)

    def targets(k):
        idx = rs.randint(0, len(pos), k)
        w = rs.dirichlet((1, 1, 1), k)
        w[::8] = (1, 0, 0); w[1::8] = (0.5, 0.5, 0); w[2::8] = (0, 0.5, 0.5)
        return (pos[idx].astype(np.float64) * w[:, :, None]).sum(1)

    def around(k, scale):
        u = rs.standard_normal((k, 3))
        u /= np.sqrt((u * u).sum(1, keepdims=True))
        return ctr + u * scale * 0.5 * np.sqrt((ext * ext).sum())

    def unit(d):
        return d / np.sqrt((d * d).sum(1, keepdims=True))

    parts = []
    org, tgt = around(m, 1.3), targets(m)
    parts.append(rays8(org, unit(tgt - org), T_FAR))
    parts.append(rays8(tgt + unit(tgt - org) * 0.5 * np.sqrt((ext * ext).sum()), unit(org - tgt), T_FAR))
    a, b = around(m, 0.9), around(m, 0.9)
    parts.append(rays8(a, b - a, 1.0))
    tgt = targets(m)
    ax = rs.randint(0, 3, m)
    d = np.zeros((m, 3))
    d[np.arange(m), ax] = np.where(rs.uniform(0, 1, m) < 0.5, -1.0, 1.0)
    parts.append(rays8((tgt - d * ext.max()).astype(F), d, T_FAR))
    h = m // 2
    org, tgt = around(h, 1.1), targets(h)
    dist = np.sqrt(((tgt - org) ** 2).sum(1))
    parts.append(rays8(org, unit(tgt - org), dist * rs.uniform(0.5, 1.2, h)))
    if spheres is not None and len(spheres):
        s = np.asarray(spheres, np.float64).reshape(-1, 16)
        k = rs.randint(0, len(s), h)
        u = unit(rs.standard_normal((h, 3)))
        tgt = s[k, 0:3] + u * s[k, 3:4] * rs.uniform(0, 0.95, (h, 1))
        org = around(h, 1.2)
        parts.append(rays8(org, unit(tgt - org), T_FAR))
        k = rs.randint(0, len(s), h)
        org = s[k, 0:3] + unit(rs.standard_normal((h, 3))) * s[k, 3:4] * rs.uniform(0, 0.9, (h, 1))
        parts.append(rays8(org, unit(rs.standard_normal((h, 3))), T_FAR))
    r = np.concatenate(parts)
    return np.ascontiguousarray(r[rs.permutation(len(r))], F)
