"""The numpy side of tests/test_large_scene.py: the scenes, the material sets and the move that take the scene-edit kernels past
65,536 triangles, and the split of an array at that index which the premises of the CPU tests are stated with.
Nothing here restates a yardstick: the light and emittance tests are materials_ref's, the core box dynamic_ref's, the centroid and
class boxes rebuild_ref's and rebuild_budget_ref's.

65,536 = 256 workgroups of 256 threads = kCoreBlocks * 256 = 256 * kMatBlock: the first triangle a grid-stride reduction meets on its
second trip, and the first whose block count the material update's scan meets in its second round.  Every index is in reference order,
the order of `tris` as ptamd.build_bvh returns it."""
import numpy as np

import materials_ref as M
import rebuild_budget_ref as X
import rebuild_ref as B
from scenes_util import make_prims

F = np.float32
SPLIT = 65536
SEED = 20                      # tests/test_materials.py's
STANDIN_LAT_LON = 187          # ptamd.gen_scene(1, 187): the benchmark's own scene
STANDIN_TRIS = 69576
SHEET_SIZES = (65536, 65537)
LARGE_FRACTION = 1.0 / 16.0
DEPTH_BUDGET = 26
SHEET_NX, SHEET_NZ = 128, 256      # 2 * 128 * 256 = 65,536 cells' triangles: two more than the smaller sheet takes


def blocks(n):
    """Workgroups of 256 threads over n triangles."""
    return (n + 255) // 256


def sheet_prims(n_total, seed=7):
    """(n_total, 84) Primitive records: n_total - 2 small triangles of a jittered height field (x, z in [-18, 18], y in [4, 6]; the cells
    in a seeded random order, so that the triangle left out is none in particular) and one emissive quad of two big triangles at y = 30,
    facing down.  The quad gives the scene a light, a second size class and, its box being far larger than the field's, a core box."""
    rs = np.random.RandomState(seed)
    n_small = n_total - 2
    assert 0 < n_small <= 2 * SHEET_NX * SHEET_NZ
    xs = np.linspace(-18.0, 18.0, SHEET_NX + 1)[:, None] + rs.uniform(-0.04, 0.04, (SHEET_NX + 1, SHEET_NZ + 1))
    zs = np.linspace(-18.0, 18.0, SHEET_NZ + 1)[None, :] + rs.uniform(-0.02, 0.02, (SHEET_NX + 1, SHEET_NZ + 1))
    ys = 5.0 + rs.uniform(-1.0, 1.0, (SHEET_NX + 1, SHEET_NZ + 1))
    p = np.stack([xs, ys, zs], -1).astype(F)
    p00, p10, p11, p01 = p[:-1, :-1], p[1:, :-1], p[1:, 1:], p[:-1, 1:]
    a = np.stack([p00, p00], 2).reshape(-1, 3)
    b = np.stack([p11, p01], 2).reshape(-1, 3)
    c = np.stack([p10, p11], 2).reshape(-1, 3)
    pick = rs.permutation(len(a))[:n_small]
    field = make_prims(a[pick], b[pick], c[pick], albedo=(0.6, 0.7, 0.5))
    q = F([[-14, 30, -14], [14, 30, -14], [14, 30, 14], [-14, 30, 14]])
    quad = make_prims(q[[0, 0]], q[[1, 2]], q[[2, 3]], albedo=(0, 0, 0), emit=(6, 6, 6))      # (b - a) x (c - a) points down
    return np.ascontiguousarray(np.concatenate([field, quad]), F)


# ---------------------------------------------------------------------------------------------------------------------------------
# material sets: materials_ref's (a) .. (e), and set (f) in two variants
# ---------------------------------------------------------------------------------------------------------------------------------
def bad_triangle(n):
    """The triangle set (f) spoils: the middle of the second stride; in a scene that has none, the last triangle."""
    return SPLIT + (n - SPLIT) // 2 if n > SPLIT else n - 1


HEAD_TRIANGLE = SPLIT // 2      # block 128 of the scan's first round; no light of any of the three scenes


def set_f(tris, value, at=None):
    """The uploaded materials, and one triangle — bad_triangle(n), at or above SPLIT, unless `at` names another — whose first emittance
    component is `value`: 2e8 (above the 1e8 the emittance test allows, and a light) or NaN (fails the test, and no light)."""
    m = M.materials(tris)
    m[bad_triangle(len(tris)) if at is None else at, 0] = value
    return m


def material_sets(tris, seed=SEED, names="abcdef"):
    """(label, mat12) in the order the tests apply them: materials_ref.material_sets' (a) .. (e), then "f 2e8", "f nan" and "f head".
    In "f head" the spoiled triangle is HEAD_TRIANGLE and every row from SPLIT on is fine: the scan's second round is clean, and the
    flag is down only if the first round's is carried into it."""
    out = [(k, m) for k, m in M.material_sets(tris, seed) if k in names]
    if "f" in names:
        out += [("f 2e8", set_f(tris, 2e8)), ("f nan", set_f(tris, np.nan)), ("f head", set_f(tris, 2e8, HEAD_TRIANGLE))]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the move `far_tail`
# ---------------------------------------------------------------------------------------------------------------------------------
def tail_picks(n):
    """Up to three triangles of the second stride: its first, its middle and its last."""
    return sorted({i for i in (SPLIT, SPLIT + (n - SPLIT) // 2, n - 1) if SPLIT <= i < n})


FAR = 8.0      # extents of the scene in x.  The distance decides how the Morton cells fall on the mesh: at 2 the plain radix tree over the
               # moved standin187 is 33 levels deep, one more than the kernels' stacks hold, and pt_scene_rebuild_tree would refuse it;
               # at 8 it is 31 (tests/test_large_scene.py asserts on the CPU that it is within the limit)


def far_tail(pos, factor=FAR):
    """pos (n, 3, 3) with every triangle at or above SPLIT translated along +x by `factor` times the scene's extent in x (their box
    then lies wholly beyond the scene's), and tail_picks(n) scaled about their own centroids until the longest side of their box is an
    eighth of the longest side of the translated centroid box: twice what makes a triangle large at a fraction of 1 / 16.  float32
    throughout, one operation at a time.  A scene of SPLIT triangles or fewer comes back as it is."""
    p = np.ascontiguousarray(pos, F).reshape(-1, 3, 3).copy()
    n = len(p)
    if n <= SPLIT:
        return p
    v = p.reshape(-1, 3)
    shift = F(factor) * (v[:, 0].max() - v[:, 0].min())
    p[SPLIT:, :, 0] = p[SPLIT:, :, 0] + shift
    c = B.centroids(p)
    E = (c.max(0) - c.min(0)).max()
    for i in tail_picks(n):
        ext = (p[i].max(0) - p[i].min(0)).max()
        mid = ((p[i, 0] + p[i, 1]) + p[i, 2]) / F(3.0)
        p[i] = (p[i] - mid) * ((F(0.125) * E) / ext) + mid
    assert p.dtype == F
    return p


def without_tail(a):
    """The part of a per-triangle array a reduction sees that loses its second trip."""
    return a[:SPLIT]


def class_boxes(pos, f=LARGE_FRACTION, keep=None):
    """((lo, hi) of the small class, (lo, hi) of the large class): the centroid boxes rebuild_budget_ref.class_keys quantises in, over
    the triangles keep (a boolean mask; all of them by default).  The classes are those of the whole scene either way."""
    c, large = B.centroids(pos), X.large_mask(pos, f)
    keep = np.ones(len(c), bool) if keep is None else keep
    return tuple((c[keep & (large == cls)].min(0), c[keep & (large == cls)].max(0)) for cls in (False, True))
