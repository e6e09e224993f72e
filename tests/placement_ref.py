"""Scenes, placements and CPU-side transforms of tests/test_placement.py (pure numpy).

The "home" scene is kept as float64 positions in groups, so that it can be built again after any affine map: the ten wall triangles
of scenes_util._cornell_walls, a two-triangle ceiling light and the bumpy sphere of scenes_util._standin_positions(12) as a rough
metal, 276 triangles.  "mixed" adds two ground triangles of side 2^21 and a cluster of 64 triangles of side about 2^-6: 342.

A placement is a diagonal scale D and a translation t.  Vertices are mapped in float64 as x * D + t and rounded once to float32; the
flat frames are made again by scenes_util.make_prims from the rounded vertices.  The placed scene is simply another scene: every check
compares it with the oracle or with brute force on that same scene, so nothing depends on the map being exact.  Ray origins and
directions (renormalised), query points, radii and the camera position are mapped here as well."""
import numpy as np

import nearest_ref as N
from scenes_util import V_ALB, _aim, _cornell_walls, _facing, _standin_positions, make_prims, scene_rays8

F = np.float32
INF = F(np.inf)
T_FAR = 999999.0
GROUPS = ("walls", "light", "mesh", "ground", "cluster")
CLUSTER_CENTRE = (12.0, 5.0, 8.0)
CLUSTER_SIDE = 2.0 ** -6
CAMERA_POS = (0.0, 20.0, 60.0)      # ptamd.make_camera's default
# view: (home position, rotation, samples per pass).  `default` is the issue's frame.  `inside` stands by the left wall and looks along +x
# with 16 samples per pass, so that its streams outlive the 16 iterations after which the host first looks at the live count.
VIEWS = {"default": (CAMERA_POS, (0.0, 90.0, 0.0), 4), "inside": ((-18.0, 20.0, 0.0), (0.0, 90.0, -90.0), 16)}

_STRETCH = (256.0, 1.0, 1.0 / 64.0)
PLACEMENTS = {      # name: (D, t)
    "home": ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
    "far12": ((1.0, 1.0, 1.0), (4096.0, -8192.0, 2048.0)),
    "far17": ((1.0, 1.0, 1.0), (2.0 ** 17, -(2.0 ** 16), 2.0 ** 17)),
    "far20": ((1.0, 1.0, 1.0), (2.0 ** 20, 2.0 ** 20, -(2.0 ** 20))),
    "stretch": (_STRETCH, (0.0, 0.0, 0.0)),
    "stretch_far": (_STRETCH, (2.0 ** 15, 2.0 ** 10, -(2.0 ** 4))),
    "mixed": ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)),
    "tiny": ((2.0 ** -12,) * 3, (0.0, 0.0, 0.0)),
    "tiny_far": ((2.0 ** -12,) * 3, (64.0, -32.0, 16.0)),
    "huge": ((2.0 ** 20,) * 3, (0.0, 0.0, 0.0)),
}
ALL = tuple(PLACEMENTS)
RAYS = ("home", "far12", "far17", "far20", "stretch", "stretch_far", "mixed")      # the oracle is blind on the others
REFIT = ("far17", "far20", "stretch_far", "tiny_far")      # the moves the issue names ...
MOVES = tuple(n for n in PLACEMENTS if n not in ("home", "mixed"))      # ... and every placement that has home's 276 triangles
# Radius of the room points' queries: 6 * min(D).  On the two stretched placements that is 0.09 against a room 10,240 x 40 x 0.6; 16
# reaches across z, a good part of y and little of x, and the yardstick alone gives the shares that tests/test_placement.py asserts.
RADIUS = {name: 6.0 * min(PLACEMENTS[name][0]) for name in PLACEMENTS}
RADIUS["stretch"] = RADIUS["stretch_far"] = 16.0
# huge: the plane term of f overflows there and 6 * 2^20 leaves 0.42 - 0.53 of the lists non-empty, depending on
# the seed; with 8 * 2^20 the yardstick gives 0.63 - 0.74 and 0.24 - 0.33 over seeds 0 .. 39.
RADIUS["huge"] = 8.0 * 2.0 ** 20


def placement(name):
    D, t = PLACEMENTS[name]
    return np.array(D, np.float64), np.array(t, np.float64)


def _positions_of(prims):
    return prims.reshape(len(prims), 3, 28)[:, :, 0:3].astype(np.float64)


def home_scene(mixed=False, seed=3):
    """The scene before any placement, a dict: pos (n, 3, 3) float64, albedo and emit (n, 3), rough and metal (n,), group (n,) index into
    GROUPS."""
    walls = _cornell_walls()
    parts = [dict(pos=_positions_of(walls), albedo=walls[:, V_ALB:V_ALB + 3].astype(np.float64), emit=0.0, rough=1.0, metal=0.0, group=0)]
    y, h, down = 39.95, 5.0, np.array([0.0, -1.0, 0.0])
    q = [(-h, y, -h), (h, y, -h), (h, y, h), (-h, y, h)]
    light = np.array([_facing(q[i], q[j], q[k], down) for i, j, k in ((0, 1, 2), (0, 2, 3))], np.float64)
    parts.append(dict(pos=light, albedo=0.0, emit=15.0, rough=1.0, metal=0.0, group=1))
    mesh = np.stack([x.astype(np.float64) for x in _standin_positions(12)], 1)
    parts.append(dict(pos=mesh, albedo=(0.9, 0.8, 0.6), emit=0.0, rough=0.3, metal=1.0, group=2))
    if mixed:
        rs = np.random.RandomState(seed)
        s, up = 2.0 ** 20, np.array([0.0, 1.0, 0.0])
        g = [(-s, -1.0, -s), (s, -1.0, -s), (s, -1.0, s), (-s, -1.0, s)]
        ground = np.array([_facing(g[i], g[j], g[k], up) for i, j, k in ((0, 1, 2), (0, 2, 3))], np.float64)
        parts.append(dict(pos=ground, albedo=(0.5, 0.5, 0.5), emit=0.0, rough=1.0, metal=0.0, group=3))
        c = np.array(CLUSTER_CENTRE) + rs.uniform(-0.5, 0.5, (64, 1, 3))
        cluster = c + rs.uniform(-0.5, 0.5, (64, 3, 3)) * (2.0 * CLUSTER_SIDE)
        parts.append(dict(pos=cluster, albedo=(0.2, 0.4, 0.9), emit=0.0, rough=1.0, metal=0.0, group=4))
    out = {}
    for key in ("albedo", "emit"):
        out[key] = np.concatenate([np.broadcast_to(np.asarray(p[key], np.float64), (len(p["pos"]), 3)) for p in parts])
    for key in ("rough", "metal"):
        out[key] = np.concatenate([np.full(len(p["pos"]), p[key], np.float64) for p in parts])
    out["group"] = np.concatenate([np.full(len(p["pos"]), p["group"], np.int64) for p in parts])
    out["pos"] = np.concatenate([p["pos"] for p in parts])
    return out


def map_positions(pos, D, t):
    """x * D + t in float64, rounded once to float32."""
    return (np.asarray(pos, np.float64) * D + t).astype(F)


def placed_prims(scene, D, t):
    """((n, 84) float32 Primitive records of the scene after the placement, (n, 3, 3) float32 positions), both in input order."""
    p = map_positions(scene["pos"], D, t)
    prims = make_prims(p[:, 0], p[:, 1], p[:, 2], albedo=scene["albedo"].astype(F), emit=scene["emit"].astype(F), rough=scene["rough"].astype(F),
                       metal=scene["metal"].astype(F))
    return np.ascontiguousarray(prims, F), p


def frames_of(prims):
    """(n, 27) float32 N0 N1 N2 T0 T1 T2 B0 B1 B2 of Primitive records: pt_scene_update_vertices' frames."""
    v = prims.reshape(len(prims), 3, 28)
    return np.ascontiguousarray(np.concatenate([v[:, :, 3:6].reshape(-1, 9), v[:, :, 8:11].reshape(-1, 9), v[:, :, 11:14].reshape(-1, 9)], 1), F)


def tri_to_input(tris88, placed):
    """For every TRI record of a BVH built from the placed primitives, the index of its primitive in input order, by the nine vertex
    floats (no two triangles of these scenes share all three vertices)."""
    key = {np.ascontiguousarray(p, F).tobytes(): i for i, p in enumerate(placed.reshape(len(placed), 9))}
    assert len(key) == len(placed)
    return np.array([key[np.ascontiguousarray(tr[0:9], F).tobytes()] for tr in np.ascontiguousarray(tris88, F)])


def map_rays(rays8, D, t):
    """RAY8 records after the placement: the origin as a vertex, the direction dir * D made a unit vector, a finite tmax stretched with
    the direction so that it ends at the image of the same point (999999, the integrator's t_max, stays)."""
    r = np.ascontiguousarray(rays8, F)
    o = r[:, 0:3].astype(np.float64) * D + t
    d = r[:, 3:6].astype(np.float64) * D
    ln = np.sqrt((d * d).sum(1))
    out = np.zeros_like(r)
    out[:, 0:3], out[:, 3:6] = o, d / ln[:, None]
    out[:, 7] = np.where(r[:, 7] < F(T_FAR), r[:, 7].astype(np.float64) * ln, T_FAR)
    return out


def map_camera_pos(D, t, pos=CAMERA_POS):
    """pos * D + t in float32 (the rotation stays)."""
    return tuple(float(x) for x in (np.asarray(pos, np.float64) * D + t).astype(F))


def aimed_rays(scene, placed, D, t, idx, rs):
    """One RAY8 record per entry of idx, aimed in float32 (scenes_util._aim) at a point of that triangle of the PLACED scene: its
    vertices bit for bit, its edge midpoints as float32 gives them, interior points.  The origin is drawn in the home room, off the
    front of the triangle, and mapped."""
    n = len(idx)
    v = scene["pos"][idx]
    w = rs.dirichlet((1, 1, 1), n)
    tgt = map_positions((v * w[:, :, None]).sum(1), D, t)
    p = placed[idx]
    for k in range(3):
        tgt[k::8] = p[k::8, k]
        tgt[3 + k::8] = (p[3 + k::8, k] + p[3 + k::8, (k + 1) % 3]) * F(0.5)
    w[0::8], w[1::8], w[2::8], w[3::8], w[4::8], w[5::8] = (1, 0, 0), (0, 1, 0), (0, 0, 1), (0.5, 0.5, 0), (0, 0.5, 0.5), (0.5, 0, 0.5)
    at = (v * w[:, :, None]).sum(1)
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nrm /= np.sqrt((nrm * nrm).sum(1, keepdims=True))
    off = nrm + 0.6 * rs.standard_normal((n, 3))
    off /= np.sqrt((off * off).sum(1, keepdims=True))
    off = np.where(((off * nrm).sum(1) < 0.2)[:, None], nrm, off)
    org = np.clip(at + off * rs.uniform(4, 14, (n, 1)), [-19.5, 0.5, -19.5], [19.5, 39.5, 19.5])
    return _aim(map_positions(org, D, t), tgt)


def afar_rays(scene, placed, D, t, idx, rs):
    """One RAY8 record per entry of idx, aimed like aimed_rays' at a point of that triangle, from 2^10 .. 2^19.5 home units away through
    the open front of the room (home direction (dx, dy, 1), |dx| <= 0.15, 0 <= dy <= 0.3): the origin is far from the scene while the
    scene's own coordinates stay what they are, which is where t(q) = q*A + B of quad_order has a large B over small boxes."""
    n = len(idx)
    v = scene["pos"][idx]
    w = rs.dirichlet((1, 1, 1), n)
    tgt = map_positions((v * w[:, :, None]).sum(1), D, t)
    p = placed[idx]
    for k in range(3):
        tgt[k::8] = p[k::8, k]
        w[k::8] = np.eye(3)[k]
    at = (v * w[:, :, None]).sum(1)
    d = np.stack([rs.uniform(-0.15, 0.15, n), rs.uniform(0.0, 0.3, n), np.ones(n)], 1)
    d /= np.sqrt((d * d).sum(1, keepdims=True))
    org = at + d * (2.0 ** rs.uniform(10, 19.5, n))[:, None]
    return _aim(map_positions(org, D, t), tgt)


def ray_sets(name, scene, placed, seed, n=4000):
    """{set: RAY8 records} of a placement: `scene` (n scenes_util.scene_rays8 rays, mapped), `aimed` (n / 2 rays at vertices, edge midpoints
    and interior points of every triangle in turn), `afar` (n / 2 rays at the mesh from far outside the room) and, where the scene has
    the cluster, `cluster` (n / 2 rays aimed at its triangles)."""
    D, t = placement(name)
    rs = np.random.RandomState(seed)
    out = {"scene": map_rays(scene_rays8(n, rs), D, t)}
    m = n // 2
    out["aimed"] = aimed_rays(scene, placed, D, t, np.arange(m) % len(placed), rs)
    mesh = np.nonzero(scene["group"] == GROUPS.index("mesh"))[0]
    out["afar"] = afar_rays(scene, placed, D, t, mesh[np.arange(m) % len(mesh)], np.random.RandomState(seed + 1))
    cluster = np.nonzero(scene["group"] == GROUPS.index("cluster"))[0]
    if len(cluster):
        out["cluster"] = aimed_rays(scene, placed, D, t, cluster[np.arange(m) % len(cluster)], rs)
    return out


def query_points(name, positions, seed, m=300):
    """(POINT4 records (3 m, 4), mask of the room points) against the placed positions (k, 3, 3) float32: m nearest_ref.room_points
    mapped by the placement with radius RADIUS[name]; m surface points +- 1e-3 min(D), radius RADIUS[name] and 7e-4 min(D) in turn; m
    points exactly on vertices and edge midpoints with radius inf, 0, RADIUS[name] in turn.  Permuted, so that every wave holds every kind."""
    D, t = placement(name)
    rs = np.random.RandomState(seed)
    r, small = F(RADIUS[name]), float(min(D))
    room = map_positions(N.room_points(rs, m), D, t)
    surf = N.surface_points(rs, m, positions, offset=1e-3 * small)
    vert = N.vertex_and_edge_points(rs, m, positions)
    k = np.arange(m)
    pts = np.concatenate([N.with_radius(room, r), N.with_radius(surf, np.where(k % 2 == 0, r, F(7e-4 * small)).astype(F)),
                          N.with_radius(vert, np.select([k % 3 == 0, k % 3 == 1], [INF, F(0)], r).astype(F))])
    perm = rs.permutation(len(pts))
    return np.ascontiguousarray(pts[perm], F), (perm < m)
