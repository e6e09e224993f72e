"""The yardstick of tests/test_nearest_k.py, independent of the code under test: the K nearest primitives within a radius and the number
of primitives within it (include/pt_api.h, "K nearest and counts within a radius"), by brute force over the full matrix of
tests/nearest_ref.py's f, and the point sets the tests run on with the figures that say what those sets exercise."""
import numpy as np

import nearest_ref as N

F = N.F
INF = F(np.inf)
KS = (1, 2, 7, 8, 32)


def f_all(points, positions, spheres=None):
    """(n, m + s) float32: f of every point against every triangle, then every sphere, in primitive order."""
    pts = np.ascontiguousarray(points, F)
    p = pts[:, None, 0:3]
    a, ab, ac = N.edges(positions)
    cols = [N.tri_f(p, a[None, lo:lo + N.CHUNK], ab[None, lo:lo + N.CHUNK], ac[None, lo:lo + N.CHUNK]) for lo in range(0, len(a), N.CHUNK)]
    if spheres is not None:
        cols += [N.sphere_f(pts[:, 0:3], s[None, 0:3], s[3])[:, None] for s in np.ascontiguousarray(spheres, F)]
    f = np.concatenate(cols, 1)
    assert f.dtype == F
    return f


def _mask(points, f):
    pts = np.ascontiguousarray(points, F)
    with np.errstate(invalid="ignore"):
        return f <= (pts[:, 3] * pts[:, 3])[:, None]


def brute_k(points, positions, spheres, k, f=None):
    """(dist2, prim), each (n, k), of pt_nearest_k by definition: the members of C(p) = { j : f(p, j) <= r2 } ordered by f ascending, among
    equal f the larger index first, the first k of them, padded with the miss record (0, -1).  f: f_all of the same arguments, if the
    caller has it already."""
    f = f_all(points, positions, spheres) if f is None else f
    n, m = f.shape
    within = _mask(points, f)
    index = np.arange(m)
    d2, prim = np.zeros((n, k), F), np.full((n, k), -1, np.int32)
    for i in range(n):
        order = np.lexsort((-index, f[i]))
        order = order[within[i, order]][:k]
        d2[i, :len(order)], prim[i, :len(order)] = f[i, order], order
    return d2, prim


def count(points, positions, spheres, f=None):
    """(n,) int32: |C(p)|, the row sum of the mask."""
    f = f_all(points, positions, spheres) if f is None else f
    return _mask(points, f).sum(1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# point sets
# ---------------------------------------------------------------------------------------------------------------------------------
class PointSets:
    """The points of one scene, drawn once (RandomState 41, m per kind), and per K the POINT4 records made of them:
         m uniform in the room and in the scene's box, radius inf
         the same points, radius sqrt(median over them of the K-th smallest f): about half of them hold more than K candidates
         m exactly on vertices and edge midpoints, radius inf
         the same, radius 0: only the primitives that touch the point, which tie at f = 0
         m on triangles +- 1e-3, radius 7e-4
    permuted (one permutation per scene) so that every wave holds every kind.  The f matrix is computed once and shared by every K."""

    def __init__(self, positions, spheres, m=200, seed=41):
        rs = np.random.RandomState(seed)
        pos = np.ascontiguousarray(positions, F).reshape(-1, 3, 3)
        v = pos.reshape(-1, 3)
        lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
        box = (lo - 0.1 * (hi - lo) + rs.uniform(0, 1, (m // 2, 3)) * 1.2 * (hi - lo)).astype(F)
        self.space = np.concatenate([N.room_points(rs, m - m // 2), box])
        self.verts = N.vertex_and_edge_points(rs, m, pos)
        self.near = N.surface_points(rs, m, pos)
        self.perm = rs.permutation(5 * m)
        self.m, self.positions, self.spheres = m, pos, spheres
        base = np.concatenate([self.space, self.space, self.verts, self.verts, self.near])[self.perm]
        self.f = f_all(N.with_radius(base, INF), pos, spheres)
        self.f_space_sorted = np.sort(f_all(N.with_radius(self.space, INF), pos, spheres), 1)
        self._cache = {}

    def points(self, k):
        """(5 m, 4) POINT4 records for this K."""
        kth = self.f_space_sorted[:, min(k, self.f_space_sorted.shape[1]) - 1].astype(np.float64)
        cut = F(np.sqrt(np.median(kth)))
        parts = [N.with_radius(self.space, INF), N.with_radius(self.space, cut), N.with_radius(self.verts, INF), N.with_radius(self.verts, 0.0),
                 N.with_radius(self.near, F(7e-4))]
        return np.ascontiguousarray(np.concatenate(parts)[self.perm], F)

    def want(self, k):
        """(points, dist2 (n, k), prim (n, k), count (n,)) for this K, computed once."""
        if k not in self._cache:
            pts = self.points(k)
            self._cache[k] = (pts,) + brute_k(pts, self.positions, self.spheres, k, self.f) + (count(pts, self.positions, self.spheres, self.f),)
        return self._cache[k]

    def figures(self, k):
        """What the set exercises at this K: the shares of points with more than K candidates, with fewer than K but at least one, and
        with none; the number of points where slot K - 1 and the first excluded candidate have equal f (a tie exactly at the cut); and
        the number of points with two adjacent slots of equal f (a tie inside the list)."""
        pts, d2, prim, cnt = self.want(k)
        fs = np.sort(np.where(_mask(pts, self.f), self.f, INF), 1)      # the members of C in f order, padded with inf
        full = cnt > k
        cut_tie = full & (fs[:, k - 1] == fs[:, min(k, fs.shape[1] - 1)]) if fs.shape[1] > k else np.zeros(len(pts), bool)
        both = (prim[:, 1:] >= 0) if k > 1 else np.zeros((len(pts), 0), bool)
        inside = (both & (d2[:, 1:] == d2[:, :-1])).any(1) if k > 1 else np.zeros(len(pts), bool)
        return {"more": float(full.mean()), "fewer": float(((cnt < k) & (cnt > 0)).mean()), "none": float((cnt == 0).mean()),
                "cut_ties": int(cut_tie.sum()), "inside_ties": int(inside.sum()), "largest_finite": int(cnt[np.isfinite(pts[:, 3])].max())}
