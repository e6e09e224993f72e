"""The yardstick of tests/test_lists.py (include/pt_api.h, "Variable-length query results"), independent of the code under test: the CSR
form of every H(ray) and every C(p), cut out of the existing brute forces (ray_hits_ref.brute, nearest_k_ref.brute_k with k = the number
of primitives), and a sheet stack tall enough that one ray's list outgrows every fixed capacity of the sort."""
import numpy as np

import nearest_k_ref as K
import nearest_ref as N
import ray_hits_ref as H
from scenes_util import make_prims

F = np.float32
SORT_TILE = 512            # records of the sort's LDS tile (csrc/pt_lists.hip: kSortTile); a list longer than this takes its global steps
SCAN_CHUNK = 2048          # counts of one chunk of pt_list_offsets (kScanChunk)
SCAN_GRID = 256            # its most workgroups (kScanGrid): the spans grow past SCAN_GRID * SCAN_CHUNK counts


def csr(count):
    """(n + 1,) int64: 0, then the running sum of max(count, 0)."""
    c = np.maximum(np.asarray(count, np.int64), 0)
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(c, dtype=np.int64)])


def ray_lists(h):
    """(offsets, t, prim, detail (total, 4)) of a ray_hits_ref.Hits: every row cut at its count, concatenated in ray order."""
    n, M = h.t.shape
    live = np.arange(M)[None, :] < h.count[:, None]
    det = np.stack([h.bu, h.bv, h.facing, np.zeros_like(h.t)], 2)
    return csr(h.count), np.ascontiguousarray(h.t[live]), np.ascontiguousarray(h.prim[live]), np.ascontiguousarray(det[live])


def point_lists(points, positions, spheres, f=None):
    """(offsets, dist2, prim) of pt_within_radius_list by definition: brute_k with k = the number of primitives, every row cut at |C(p)|."""
    f = K.f_all(points, positions, spheres) if f is None else f
    d2, prim = K.brute_k(points, positions, spheres, f.shape[1], f)
    cnt = K.count(points, positions, spheres, f)
    live = np.arange(f.shape[1])[None, :] < cnt[:, None]
    assert ((prim >= 0) == live).all()
    return csr(cnt), np.ascontiguousarray(d2[live]), np.ascontiguousarray(prim[live])


def point_detail(points, off, prim, positions, spheres):
    """(total, 8): nearest_ref.detail of every slot, the slot's point found through the offsets."""
    owner = np.repeat(np.arange(len(points)), np.diff(off))
    return N.detail(np.asarray(points, F)[owner], prim, positions, spheres)


def segments(off, cap):
    """(b, e) of every query: b = clamp(off[i], 0, cap), e = clamp(off[i + 1], b, cap) (the header's rule)."""
    off = np.asarray(off, np.int64)
    b = np.clip(off[:-1], 0, cap)
    e = np.minimum(np.maximum(off[1:], b), cap)
    return b, e


# ---------------------------------------------------------------------------------------------------------------------------------
# the tall sheet stack: ray_hits_ref.sheet_stack's recipe with 600 layers
# ---------------------------------------------------------------------------------------------------------------------------------
TALL_LAYERS = 600
TALL_DUPLICATED = (5, 17, 30, 250, 251, 480)      # a second time at identical z, appended after the others: ties deep in long lists


def tall_stack():
    """ray_hits_ref.sheet_stack with TALL_LAYERS layers (x in [-4, 4], y in [16, 24], z = -10 + i / 2, every fourth wound the other way)
    and TALL_DUPLICATED twice, then the emissive triangle: 1,213 Primitive records."""
    x0, y0, x1, y1 = H.SHEET_X0, H.SHEET_Y0, H.SHEET_X0 + H.SHEET_SIDE, H.SHEET_Y0 + H.SHEET_SIDE
    A, B, Cc = [], [], []
    for i in list(range(TALL_LAYERS)) + list(TALL_DUPLICATED):
        z = H.sheet_z(i)
        a, b, c, d = (x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)
        if i % 4 == 3:
            A += [a, a]; B += [c, d]; Cc += [b, c]
        else:
            A += [a, a]; B += [b, c]; Cc += [c, d]
    quads = make_prims(np.array(A, F), np.array(B, F), np.array(Cc, F))
    light = make_prims(np.array([[-3, 39, -3]], F), np.array([[3, 39, -3]], F), np.array([[0, 39, 3]], F), albedo=(0, 0, 0), emit=(6, 6, 6))
    return np.concatenate([quads, light])


def tall_rays(seed, m):
    """About 5.5 m + 160 rays: m along -z and m along +z through the quads' interiors (one hit per layer crossed, ties at the duplicated
    layers), m / 2 along the shared diagonal (both triangles of a quad at one t: up to 2 per layer), m oblique through the whole stack,
    m un-normalised segments between two layers, m short ones from between two layers, and two sweeps along +z whose tmax grows by one
    layer per ray: from below layer 0 (91 rays) and from below layer 40 (71 rays, no duplicate there), so that every list length from 0
    to 70 occurs."""
    rs = np.random.RandomState(seed)
    x0, y0, s = H.SHEET_X0, H.SHEET_Y0, H.SHEET_SIDE
    zlo, zhi = H.sheet_z(0), H.sheet_z(TALL_LAYERS - 1)
    grid = lambda k: (rs.randint(1, 512, k) / 64.0).astype(F)      # noqa: E731  exact in float32, inside (0, 8)
    parts = []
    for sign in (-1.0, 1.0):
        org = np.stack([x0 + grid(m), y0 + grid(m), np.full(m, zhi + 8.0 if sign < 0 else zlo - 8.0)], 1)
        parts.append(H.rays8(org, np.tile(F([0, 0, sign]), (m, 1)), H.T_FAR))
    h = m // 2
    g = grid(h)
    sign = np.where(np.arange(h) % 2 == 0, -1.0, 1.0)
    z_of = np.where(sign < 0, zhi + 8.0, zlo - 8.0)
    parts.append(H.rays8(np.stack([x0 + g, y0 + g, z_of], 1), np.stack([0 * sign, 0 * sign, sign], 1), H.T_FAR))
    a = np.stack([x0 + rs.uniform(0.5, s - 0.5, m), y0 + rs.uniform(0.5, s - 0.5, m), np.full(m, zhi + 6.0)], 1)
    b = np.stack([x0 + rs.uniform(0.5, s - 0.5, m), y0 + rs.uniform(0.5, s - 0.5, m), np.full(m, zlo - 6.0)], 1)
    flip = (np.arange(m) % 2 == 1)[:, None]
    a, b = np.where(flip, b, a), np.where(flip, a, b)
    d = (b - a) / np.sqrt(((b - a) ** 2).sum(1, keepdims=True))
    parts.append(H.rays8(a, d, H.T_FAR))
    za, zb = rs.uniform(zlo + 0.1, zhi - 0.1, m), rs.uniform(zlo + 0.1, zhi - 0.1, m)
    a = np.stack([x0 + rs.uniform(0.5, s - 0.5, m), y0 + rs.uniform(0.5, s - 0.5, m), za], 1)
    b = np.stack([x0 + rs.uniform(0.5, s - 0.5, m), y0 + rs.uniform(0.5, s - 0.5, m), zb], 1)
    parts.append(H.rays8(a, b - a, 1.0))
    org = np.stack([x0 + rs.uniform(0.5, s - 0.5, m), y0 + rs.uniform(0.5, s - 0.5, m), rs.uniform(zlo, zhi, m)], 1)
    d = rs.standard_normal((m, 3))
    d /= np.sqrt((d * d).sum(1, keepdims=True))
    parts.append(H.rays8(org, d, rs.uniform(0.05, 1.5, m)))
    for first, count in ((0, 91), (40, 71)):
        c = np.arange(count)
        org = np.stack([np.full(count, x0 + 3.0), np.full(count, y0 + 5.0), np.full(count, H.sheet_z(first) - 0.25)], 1)
        parts.append(H.rays8(org, np.tile(F([0, 0, 1]), (count, 1)), (0.5 * c).astype(F)))      # layer first + j at t = 0.25 + j / 2
    r = np.concatenate(parts)
    return np.ascontiguousarray(r[rs.permutation(len(r))], F)
