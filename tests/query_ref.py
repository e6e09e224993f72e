"""Seeded ray sets for the ray-query tests (tests/test_query.py) and for tools/query_time.py (pure numpy; RAY8 records: org.xyz dir.xyz
0 tmax).  The room of the generated scenes is x, z in [-20, 20], y in [0, 40], open towards +z where the camera stands.

  set A   the camera rays of a frame: one per pixel, directions as pt_dbg_pixel_dir gives them (the caller passes them in)
  set B   incoherent bounce rays: from A's hit points, lifted off the surface along the shading normal, in a random direction of the
          hemisphere around it; a pixel whose camera ray missed gets a random ray inside the room instead
  set C   segments between random pairs of points in the room: dir = b - a (not normalised), tmax = 1 — the visibility question"""
import numpy as np

CAM_POS = (0.0, 20.0, 60.0)       # ptamd.make_camera's default
T_FAR = 999999.0                  # the integrator's t_max for a path ray
ROOM_LO = np.float32([-19.0, 1.0, -19.0])
ROOM_HI = np.float32([19.0, 39.0, 30.0])


def pixel_list(W, H, pass_=0):
    """(W * H, 3) int32 rows px py pass, row-major: the input of pt_dbg_pixel_dir."""
    py, px = np.mgrid[0:H, 0:W]
    return np.stack([px.ravel(), py.ravel(), np.full(W * H, pass_)], 1).astype(np.int32)


def rays8(org, d, tmax):
    n = len(d)
    org = np.broadcast_to(np.asarray(org, np.float32), (n, 3))
    tmax = np.broadcast_to(np.asarray(tmax, np.float32), (n,))
    return np.ascontiguousarray(np.concatenate([org, np.asarray(d, np.float32), np.zeros((n, 1), np.float32), tmax[:, None]], 1), np.float32)


def set_a(pixel_dir_out8, cam_pos=CAM_POS):
    """Camera rays from the (n, 8) rows of pt_dbg_pixel_dir (columns 2..4 are the direction)."""
    return rays8(cam_pos, pixel_dir_out8[:, 2:5], T_FAR)


def _unit(v):
    return (v / np.sqrt((v * v).sum(1, keepdims=True))).astype(np.float32)


def set_b(prim, hits29, rs):
    """Bounce rays from the closest hits of set A: prim (n,), hits29 (n, 29) as pt_dbg_raycast / trace_rays(surface=True) give them."""
    n = len(prim)
    p, nrm = hits29[:, 5:8], hits29[:, 8:11]
    d = _unit(rs.standard_normal((n, 3)).astype(np.float32))
    flip = (d * nrm).sum(1) < 0
    d[flip] = -d[flip]
    org = (p + np.float32(1e-3) * nrm).astype(np.float32)
    miss = (prim < 0) | ~np.isfinite(org).all(1) | ~np.isfinite(nrm).all(1)
    org[miss] = rs.uniform(ROOM_LO, ROOM_HI, (n, 3)).astype(np.float32)[miss]
    return rays8(org, d, T_FAR)


def set_c(n, rs):
    a = rs.uniform(ROOM_LO, ROOM_HI, (n, 3)).astype(np.float32)
    b = rs.uniform(ROOM_LO, ROOM_HI, (n, 3)).astype(np.float32)
    return rays8(a, (b - a).astype(np.float32), 1.0)


def sphere_only_rays():
    """Rays that only the rough-metal sphere of scenes_util.test_spheres (centre (-9, 30, -8), radius 6) blocks: no triangle lies between
    their origin and tmax (the wall at x = -20 is behind them, the mesh sits low in the middle of the room).  An axis-aligned ray, a segment
    with an un-normalised direction, and one of each that stops short of the sphere (misses)."""
    org = np.float32([[-19, 30, -8], [-19, 30, -8], [-19, 30, -8], [-19, 30, -8]])
    d = np.float32([[1, 0, 0], [10, 0.5, 0.5], [1, 0, 0], [10, 0.5, 0.5]])
    return rays8(org, d, np.float32([6.0, 1.0, 3.5, 0.3]))


def odd_rays():
    """Rays whose result is unspecified but which must not stall the walk: zero direction, NaN and inf components, a huge origin."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rows = [
        ([0, 20, 10], [0, 0, 0], T_FAR),
        ([0, 20, 10], [nan, 0, -1], T_FAR),
        ([0, 20, 10], [nan, nan, nan], T_FAR),
        ([nan, 20, 10], [0, 0, -1], T_FAR),
        ([0, 20, 10], [inf, 0, -1], T_FAR),
        ([0, 20, 10], [-inf, inf, inf], T_FAR),
        ([inf, 20, 10], [0, 0.1, -1], T_FAR),
        ([0, 20, 10], [0, 0.1, -1], nan),
        ([0, 20, 10], [0, 0.1, -1], inf),
        ([0, 20, 10], [0, 0.1, -1], -1.0),
        ([3e38, -3e38, 3e38], [1e-30, 1e30, -1e-38], T_FAR),
        ([0, 20, 10], [1e-45, 0, 0], T_FAR),
    ]
    return rays8(np.float32([r[0] for r in rows]), np.float32([r[1] for r in rows]), np.float32([r[2] for r in rows]))
