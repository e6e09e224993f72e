"""The yardstick of tests/test_dynamic.py, independent of the code under test: numpy float32 restatements of what pt_bvh_build_sah
writes for a triangle and for the boxes of the reference tree (host/bvh_build.cpp: flatten_tri, build), numpy walks of the two
downloaded traversal trees, and the moves the tests apply (written once for numpy and torch: `xp` is either module).

Every numpy float32 operation rounds once, as the host's and the device's do (no contraction, correctly rounded divide and sqrt)."""
import math

import numpy as np

F = np.float32
# float offsets in a PtTriangle (include/pt_api.h)
T_V0, T_T, T_B, T_N, T_NORMAL, T_E1, T_E2, T_MAT0, T_AREA = 0, 9, 18, 27, 36, 39, 42, 51, 87


def min2(a, b):
    return np.where(b < a, b, a)      # glm::min: b < a ? b : a


def max2(a, b):
    return np.where(a < b, b, a)      # glm::max: a < b ? b : a


def positions(tris):
    """(n, 3, 3) float32: V0 V1 V2 of every triangle."""
    return np.ascontiguousarray(tris[:, 0:9], F).reshape(-1, 3, 3).copy()


def restate_tris(tris, pos, frames=None):
    """tris' of include/pt_api.h ("Dynamic geometry"): tris with the vertices pos (n x 9) and everything derived from them."""
    t = np.ascontiguousarray(tris, F).copy()
    p = np.ascontiguousarray(pos, F).reshape(-1, 9)
    assert p.shape[0] == t.shape[0]
    t[:, 0:9] = p
    v0, v1, v2 = p[:, 0:3], p[:, 3:6], p[:, 6:9]
    e1, e2 = v1 - v0, v2 - v0
    cx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    cy = -(e1[:, 0] * e2[:, 2] - e1[:, 2] * e2[:, 0])
    cz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
        t[:, T_NORMAL + 0], t[:, T_NORMAL + 1], t[:, T_NORMAL + 2] = cx / ln, cy / ln, cz / ln
    t[:, T_E1:T_E1 + 3], t[:, T_E2:T_E2 + 3] = e1, e2
    t[:, T_AREA] = ln * F(0.5)
    assert t.dtype == F and ln.dtype == F
    if frames is not None:
        f = np.ascontiguousarray(frames, F).reshape(-1, 27)      # N0 N1 N2 T0 T1 T2 B0 B1 B2
        t[:, T_N:T_N + 9], t[:, T_T:T_T + 9], t[:, T_B:T_B + 9] = f[:, 0:9], f[:, 9:18], f[:, 18:27]
    return t


def is_leaf(nodes):
    return (nodes["primStart"] != -1) & (nodes["primEnd"] != -1)


def refit_nodes(nodes, tris):
    """nodes': every leaf's box the min / max over its triangles in index order, every interior box min2 / max2 of Child[0] = childR
    and Child[1] = childL; children visited in descending index order (a child's index is above its parent's)."""
    out = nodes.copy()
    leaf = is_leaf(nodes)
    big = np.finfo(F).max
    for i in range(len(nodes) - 1, -1, -1):
        if leaf[i]:
            mn, mx = np.full(3, big, F), np.full(3, -big, F)
            for k in range(int(nodes["primStart"][i]), int(nodes["primEnd"][i]) + 1):
                a, b, c = tris[k, 0:3], tris[k, 3:6], tris[k, 6:9]
                mn = min2(mn, min2(a, min2(b, c)))
                mx = max2(mx, max2(a, max2(b, c)))
        else:
            c0, c1 = int(nodes["childR"][i]), int(nodes["childL"][i])
            mn = min2(out["bMin"][c0], out["bMin"][c1])
            mx = max2(out["bMax"][c0], out["bMax"][c1])
        out["bMin"][i], out["bMax"][i] = mn, mx
    return out


def leaf_boxes(nodes):
    """(n_leaves, 8) float32 as the `leafbox` device array: bMin bMax 0 0 of the leaves in node order."""
    l = is_leaf(nodes)
    out = np.zeros((int(l.sum()), 8), F)
    out[:, 0:3], out[:, 3:6] = nodes["bMin"][l], nodes["bMax"][l]
    return out


def tri_records(tris, nodes, prim, ref_leaf):
    """The `tri` (n, 12) and `tripair` (n, 32) device arrays for the tree order given by prim / ref_leaf (csrc/pt_device.h)."""
    n = len(prim)
    lb = leaf_boxes(nodes)
    tri = np.zeros((n, 12), F)
    tri[:, 0:3], tri[:, 4:7], tri[:, 8:11] = tris[prim, 0:3], tris[prim, T_E1:T_E1 + 3], tris[prim, T_E2:T_E2 + 3]
    tri[:, 3], tri[:, 7] = prim.astype(np.int32).view(F), ref_leaf.astype(np.int32).view(F)
    nxt = np.minimum(np.arange(n) + 1, n - 1)
    pair = np.zeros((n, 32), F)
    for k, src in enumerate((0, 1, 2, 4, 5, 6, 8, 9, 10)):
        pair[:, 2 * k], pair[:, 2 * k + 1] = tri[:, src], tri[nxt, src]
    pair[:, 18], pair[:, 19] = tri[:, 3], tri[nxt, 3]
    pair[:, 20:26], pair[:, 26:32] = lb[ref_leaf, 0:6], lb[ref_leaf[nxt], 0:6]
    return tri, pair


def pad_lo(v):
    v = np.asarray(v, F)
    return v - (np.abs(v) * F(1.52587890625e-5) + F(1e-30))


def pad_hi(v):
    v = np.asarray(v, F)
    return v + (np.abs(v) * F(1.52587890625e-5) + F(1e-30))


def box_area(mn, mx):
    """Builder::area in float32."""
    d = np.asarray(mx, F) - np.asarray(mn, F)
    return F(2.0) * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0])


def _leaf_bounds(tri, pos, first, count, seen):
    prim = tri[first:first + count, 3].view(np.int32)
    seen[prim] += 1
    v = pos[prim].reshape(-1, 3)
    return v.min(0), v.max(0)


def walk_nodes(nodes_arr, tri_arr, pos):
    """Walks the binary traversal tree (`nodes`, 16 floats per record) from the root.  Returns (mismatches, seen, boxes): child boxes
    that are not pad_lo / pad_hi of the exact bounds of the triangles below them, how often each triangle was reached, and the
    exact (mn, mx) of every node of the tree, root included."""
    rec, tri = nodes_arr.reshape(-1, 16), tri_arr.reshape(-1, 12)
    refs = rec[:, 12:14].view(np.int32)
    seen = np.zeros(len(tri), np.int64)
    boxes, bad = [], []

    def below(ref):
        if ref < 0:
            code = ~int(ref)
            mn, mx = _leaf_bounds(tri, pos, code >> 3, code & 7, seen)
        else:
            mn, mx = node(int(ref))
        boxes.append((mn, mx))
        return mn, mx

    def node(w):
        got = None
        for side in (0, 1):
            ref = refs[w, side]
            if ref < 0 and (~int(ref) & 7) == 0:
                continue      # no child
            mn, mx = below(ref)
            b = rec[w, 6 * side:6 * side + 6]
            if not (np.array_equal(b[0:3], pad_lo(mn)) and np.array_equal(b[3:6], pad_hi(mx))):
                bad.append((w, side))
            got = (mn, mx) if got is None else (np.minimum(got[0], mn), np.maximum(got[1], mx))
        return got

    single = refs[0, 1] < 0 and (~int(refs[0, 1]) & 7) == 0 and refs[0, 0] < 0
    root = node(0)
    if not single:
        boxes.append(root)      # a single leaf is the root itself, already listed
    return bad, seen, boxes


def walk_quad(quad_arr, tri_arr, pos):
    """Walks the 4-wide tree (`quad`, 16 dwords per record).  Returns (violations, seen, scales_ok): child boxes origin + scale * q
    that do not contain pad -/+ absPad of the exact bounds below them, how often each triangle was reached, and whether every scale is
    a power of two."""
    q, tri = quad_arr.reshape(-1, 16), tri_arr.reshape(-1, 12)
    qf, refs = q.view(F), q[:, 4:8].view(np.int32)
    seen = np.zeros(len(tri), np.int64)
    every = pos[tri[:, 3].view(np.int32)].reshape(-1, 3)
    abs_pad = F(np.abs(every).max()) * F(9.5367431640625e-7)
    bad, scales_ok = [], True

    def below(ref):
        if ref < 0:
            code = ~int(ref)
            return _leaf_bounds(tri, pos, code >> 3, code & 7, seen)
        return node(int(ref))

    def node(i):
        nonlocal scales_ok
        org = qf[i, 0:3].astype(np.float64)
        scale = np.array([qf[i, 3], qf[i, 14], qf[i, 15]], np.float64)
        scales_ok = scales_ok and all(math.frexp(float(s))[0] == 0.5 for s in scale)
        got = None
        for k in range(4):
            ref = int(refs[i, k])
            lo = np.array([(int(q[i, 8 + a]) >> (8 * k)) & 255 for a in range(3)], np.float64)
            hi = np.array([(int(q[i, 11 + a]) >> (8 * k)) & 255 for a in range(3)], np.float64)
            if ref == -1:
                if not ((lo == 255).all() and (hi == 0).all()):
                    bad.append((i, k, "empty slot"))
                continue
            mn, mx = below(ref)
            want_lo = (pad_lo(mn) - abs_pad).astype(np.float64)
            want_hi = (pad_hi(mx) + abs_pad).astype(np.float64)
            if not ((org + scale * lo <= want_lo).all() and (org + scale * hi >= want_hi).all()):
                bad.append((i, k, "box"))
            got = (mn, mx) if got is None else (np.minimum(got[0], mn), np.maximum(got[1], mx))
        return got

    node(0)
    return bad, seen, scales_ok


def core_box(tris_uploaded, pos):
    """The `core` device array (6 floats, lo.xyz hi.xyz) after a move to pos (n, 3, 3): the box of the triangles pt_scene_create
    classified small on the uploaded geometry (box diagonal * 8 < the scene's), at their new positions, padded by
    0.01 * extent + 1e-4 * (diagonal of the moved scene box) — csrc/pt_scene.hip: core_box, all in float32."""
    def diag(lo, hi):
        d = (hi - lo).astype(F)
        return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    p0 = positions(tris_uploaded)
    v0 = p0.reshape(-1, 3)
    small = diag(p0.min(1), p0.max(1)) * F(8.0) < diag(v0.min(0), v0.max(0))
    p = np.ascontiguousarray(pos, F).reshape(-1, 3, 3)
    v, c = p.reshape(-1, 3), p[small].reshape(-1, 3)
    sd = diag(v.min(0), v.max(0))
    lo, hi = c.min(0), c.max(0)
    pad = F(0.01) * (hi - lo) + F(1e-4) * sd
    return np.concatenate([lo - pad, hi + pad]).astype(F)


def area_sum(boxes):
    """float64 sum of the float32 areas of a list of (mn, mx)."""
    return float(sum(np.float64(box_area(mn, mx)) for mn, mx in boxes))


# ---------------------------------------------------------------------------------------------------------------------------------
# moves: pos is (n, 3, 3) float32, numpy (xp = numpy) or torch on the device (xp = torch); sel is a boolean (n,) array of the same kind
# ---------------------------------------------------------------------------------------------------------------------------------
def emissive(tris):
    """pt_scene_create's light test: any vertex material with |emittance| > 1e-4."""
    e = np.stack([np.sqrt((tris[:, o:o + 3].astype(np.float64) ** 2).sum(1)) for o in (T_MAT0, T_MAT0 + 12, T_MAT0 + 24)])
    return (e > 0.0001).any(0)


def mesh_mask(tris):
    """The stand-in mesh: not emissive and small (the room's triangles have a 56.6 diagonal, the mesh's < 5 at lat_lon 16)."""
    p = positions(tris)
    diag = np.sqrt(((p.max(1) - p.min(1)).astype(np.float64) ** 2).sum(1))
    return (~emissive(tris)) & (diag < 10.0)


def wall_mask(tris):
    """The two triangles of the room's wall at x = -20."""
    p = positions(tris)
    return (p[:, :, 0] == -20.0).all(1)


def _apply(pos, sel, moved, xp):
    return xp.where(sel[:, None, None], moved, pos)


def _centroid(pos, sel):
    return pos[sel].reshape(-1, 3).mean(0)


def move_rigid_wobble(pos, sel, xp, deg=25.0, shift=(3.0, 1.5, -2.0)):
    """Rotate the selected triangles by deg about y through their centroid, add a sine wobble in y, translate."""
    c = _centroid(pos, sel)
    p = pos - c
    cs, sn = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    moved = xp.stack([cs * x + sn * z + shift[0], y + 0.6 * xp.sin(0.7 * x + 0.4 * z) + shift[1], -sn * x + cs * z + shift[2]], -1) + c
    return _apply(pos, sel, moved, xp)


def move_translate(pos, sel, xp, shift=(2.0, 0.0, 1.0)):
    moved = xp.stack([pos[..., 0] + shift[0], pos[..., 1] + shift[1], pos[..., 2] + shift[2]], -1)
    return _apply(pos, sel, moved, xp)


def move_scale(pos, sel, xp, factor=3.0):
    c = _centroid(pos, sel)
    return _apply(pos, sel, (pos - c) * factor + c, xp)


def move_wall_wobble(pos, sel, xp):
    """Displace the selected vertices along x by a function of their own position, so that shared vertices stay shared."""
    y, z = pos[..., 1], pos[..., 2]
    moved = xp.stack([pos[..., 0] + 1.5 * xp.sin(0.11 * y + 0.07 * z + 0.5), y, z], -1)
    return _apply(pos, sel, moved, xp)


def rotate_frames(tris, deg):
    """(n, 27) float32 N0 N1 N2 T0 T1 T2 B0 B1 B2 of tris rotated by deg about y and normalised."""
    cs, sn = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    f = np.concatenate([tris[:, T_N:T_N + 9], tris[:, T_T:T_T + 9], tris[:, T_B:T_B + 9]], 1).reshape(-1, 9, 3).astype(np.float64)
    r = np.stack([cs * f[..., 0] + sn * f[..., 2], f[..., 1], -sn * f[..., 0] + cs * f[..., 2]], -1)
    r /= np.sqrt((r * r).sum(-1, keepdims=True))
    return np.ascontiguousarray(r.reshape(-1, 27), F)
