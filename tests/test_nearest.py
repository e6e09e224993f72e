"""Closest-point queries on an uploaded scene (pt_closest_points, pt_closest_points_host, Scene.closest_points).

On the CPU: the C-ABI surface, the argument checks with a fake scene and fake device addresses, the accuracy of the header's float32
function against the float64 textbook formula, its totality on zero-area triangles, its floor and the tie rule of brute force.

On the GPU: bits only, no tolerance, and no query left out of a comparison.  (dist2, prim) of every point against brute force over all
primitives (tests/nearest_ref.py, transcribed from the header), the detail records against numpy, the any-within contract, the same
bits whatever tree the scene holds (upload, refit, three rebuilds, the binary walk by depth and by its knob), stream order behind an
update, the containment premise of the pruning on downloaded arrays, no side effects on renders, and a batch with odd records."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import deep_tree_ref as Dp
import dynamic_ref as R
import nearest_ref as N
import ptamd
import rebuild_budget_ref as X
from scenes_util import attribute_scene, make_prims, needle_scene
from scenes_util import test_spheres as make_test_spheres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pathtrace-on-cuda_amd")
F = np.float32
INF = F(np.inf)
ATTR_SEED, NEEDLE_SEED = 7, 5
# The largest error of sqrt(f) against the float64 textbook distance over the three point sets of test_formula_accuracy, per triangle, in
# units of 2^-24 * M (M = the largest absolute coordinate among the point and the scene), as measured when the test was written
# (DESIGN.md section 29); the test asserts 4 x it, the margin being there because the scenes are seeded.
MEASURED_ERR = {"attribute": 3.07, "needle512": 23.2}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def prim_positions(prims):
    """(n, 3, 3) float32 vertex positions of (n, 84) Primitive records."""
    return np.ascontiguousarray(prims.reshape(len(prims), 3, 28)[:, :, 0:3])


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound():
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in ("pt_closest_points", "pt_closest_points_host"):
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    assert callable(ptamd.Scene.closest_points)
    assert "#define PT_NEAREST_CLOSEST 0" in hdr and "#define PT_NEAREST_ANY     1" in hdr
    assert (ptamd.NEAREST_CLOSEST, ptamd.NEAREST_ANY) == (0, 1)
    assert hdr.index("Closest-point queries") > hdr.index("Ray queries (new")


def test_nearest_record_is_eight_bytes_in_c_and_in_python(tmp_path):
    assert C.sizeof(ptamd.PtNearest) == 8 and ptamd.NEAREST_DTYPE.itemsize == 8
    assert ptamd.PtNearest.dist2.offset == 0 and ptamd.PtNearest.prim.offset == 4
    assert ptamd.NEAREST_DTYPE.fields["dist2"][1] == 0 and ptamd.NEAREST_DTYPE.fields["prim"][1] == 4
    src = tmp_path / "nearest.c"
    src.write_text('#include <stddef.h>\n#include "pt_api.h"\n_Static_assert(sizeof(PtNearest) == 8, "PtNearest");\n'
                   '_Static_assert(offsetof(PtNearest, dist2) == 0 && offsetof(PtNearest, prim) == 4, "fields");\n'
                   '_Static_assert(PT_NEAREST_CLOSEST == 0 && PT_NEAREST_ANY == 1, "modes");\n')
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_bad_arguments_are_rejected_before_any_device_call():
    """A fake scene and fake device addresses: never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    base = 1 << 40
    scene, pts, out, det = (C.c_void_p(base + (i << 20)) for i in range(4))
    off = lambda p, k: C.c_void_p(p.value + k)      # noqa: E731
    dev = [
        ("NULL scene", (None, pts, 64, 0, out, None)),
        ("NULL points", (scene, None, 64, 0, out, None)),
        ("NULL out", (scene, pts, 64, 0, None, None)),
        ("n < 0", (scene, pts, -1, 0, out, None)),
        ("mode 2", (scene, pts, 64, 2, out, None)),
        ("mode -1", (scene, pts, 64, -1, out, None)),
        ("points + 4", (scene, off(pts, 4), 64, 0, out, None)),
        ("points + 8", (scene, off(pts, 8), 64, 0, out, None)),
        ("out + 4", (scene, pts, 64, 0, off(out, 4), None)),
        ("detail + 2", (scene, pts, 64, 0, out, off(det, 2))),
        ("detail with any-within", (scene, pts, 64, 1, out, det)),
        ("n = 0 does not excuse a NULL", (scene, None, 0, 0, out, None)),
    ]
    for what, a in dev:
        assert l.pt_closest_points(*a, None) == -1, what
        assert b"pt_closest_points:" in l.pt_last_error(), (what, l.pt_last_error())
    h_pts, h_out, h_det = np.zeros((64, 4), F), np.zeros(64, ptamd.NEAREST_DTYPE), np.zeros((64, 8), F)
    P = ptamd._ptr
    host = [
        ("NULL scene", (None, P(h_pts), 64, 0, P(h_out), None)),
        ("NULL points", (scene, None, 64, 0, P(h_out), None)),
        ("NULL out", (scene, P(h_pts), 64, 0, None, None)),
        ("n < 0", (scene, P(h_pts), -5, 0, P(h_out), None)),
        ("mode 7", (scene, P(h_pts), 64, 7, P(h_out), None)),
        ("detail with any-within", (scene, P(h_pts), 64, 1, P(h_out), P(h_det))),
    ]
    for what, a in host:
        assert l.pt_closest_points_host(*a) == -1, what
        assert b"pt_closest_points_host:" in l.pt_last_error(), (what, l.pt_last_error())
    # nothing to do: PT_OK, still without touching the scene or the device
    assert l.pt_closest_points(scene, pts, 0, 0, out, None, None) == 0
    assert l.pt_closest_points(scene, pts, 0, 1, out, None, None) == 0
    assert l.pt_closest_points(scene, pts, 0, 0, out, det, None) == 0
    assert l.pt_closest_points_host(scene, P(h_pts), 0, 0, P(h_out), None) == 0


class _FakeScene:
    n_tris, device, _h = 5, 0, C.c_void_p(1 << 40)


def test_wrapper_checks_shape_dtype_and_device_on_the_host():
    import torch
    fake = _FakeScene()
    cp = ptamd.Scene.closest_points
    for pts in (np.zeros((4, 3), F), np.zeros(16, F), np.zeros((2, 4, 4), F)):
        with pytest.raises(ptamd.PtError):
            cp(fake, pts)
    for pts in (torch.zeros((5, 4)), torch.zeros((5, 4), dtype=torch.float64), torch.zeros((5, 3)), torch.zeros((4, 5)).t(), [[0.0] * 4]):
        with pytest.raises(ptamd.PtError):      # a CPU tensor, a wrong dtype, a wrong shape, not contiguous, not an array
            cp(fake, pts)
    with pytest.raises(ptamd.PtError):
        cp(fake, np.zeros((4, 4), F), any_within=True, detail=True)
    d2, prim = cp(fake, np.zeros((0, 4), F))      # n = 0: PT_OK without a device
    assert d2.shape == (0,) and prim.shape == (0,) and d2.dtype == F and prim.dtype == np.int32


def _accuracy_scenes():
    prims, groups = attribute_scene(ATTR_SEED, 12)
    return {"attribute": (prim_positions(prims), groups["zero"]), "needle512": (prim_positions(needle_scene(NEEDLE_SEED, 512)[0]), np.zeros(0, int))}


@pytest.mark.parametrize("name", ["attribute", "needle512"])
def test_formula_accuracy_against_the_float64_textbook_distance(name):
    """sqrt(f) in float32 against the float64 evaluation of the textbook formula, per triangle, on points in the room, points on the
    surface +- 1e-3 and points 300 times farther out.  The textbook formula is 0 / 0 on a triangle with two equal vertices; there, and
    only there, the yardstick is the float64 distance to its three edges, which is what such a triangle is."""
    pos, zero = _accuracy_scenes()[name]
    rs = np.random.RandomState(31)
    room = N.room_points(rs, 300)
    sets = {"room": room, "near": N.surface_points(rs, 300, pos), "far": room * F(300)}
    scene_max = np.abs(pos).max()
    worst = 0.0
    for what, p in sets.items():
        f = N.f_matrix(p, pos)
        assert f.dtype == F and np.isfinite(f).all() and (f >= 0).all()
        d64 = N.textbook_d2(p, pos)
        undefined = np.isnan(d64)
        assert np.isin(np.nonzero(undefined)[1], zero).all(), "the textbook formula is undefined on zero-area triangles only"
        if undefined.any():
            a, ab, ac = (x.astype(np.float64)[None] for x in N.edges(pos))
            ap = p[:, None, :].astype(np.float64) - a
            edge = np.minimum(np.minimum(N.seg(ap, ab)[0], N.seg(ap, ac)[0]), N.seg(ap - ab, ac - ab)[0])
            d64 = np.where(undefined, edge, d64)
        M = np.maximum(np.abs(p).max(1), scene_max).astype(np.float64)
        err = np.abs(np.sqrt(f.astype(np.float64)) - np.sqrt(d64)) / (2.0 ** -24 * M[:, None])
        print(f"{name} {what}: largest error {err.max():.2f} x 2^-24 M")
        worst = max(worst, float(err.max()))
    print(f"{name}: largest error {worst:.2f} x 2^-24 M, recorded {MEASURED_ERR[name]}")
    assert worst <= 4 * MEASURED_ERR[name]


def test_textbook_formula_in_float32_loses_thin_triangles():
    """Why the header does not use the textbook formula: evaluated in float32 on 300 triangles 30 long and 0.003 wide, for points on
    them +- 1e-3, its va + vb + vc cancels and the distance is off by scene units (3.37, 8.3e5 x 2^-24 M when this was written), where
    f is off by 1.4e-3, 343 x 2^-24 M.  Asserted: the textbook error is beyond the slivers' own width (the result no longer tells the
    sliver from a line somewhere else) and two orders of magnitude beyond f's — bounds chosen before the figures were read."""
    rs = np.random.RandomState(17)
    width = 0.003
    pos = N.sliver_triangles(rs, 300, 30.0, width)
    p = N.surface_points(rs, 300, pos)
    d64 = np.sqrt(N.textbook_d2(p, pos))
    assert np.isfinite(d64).all()
    t32, f = N.textbook_d2(p, pos, F), N.f_matrix(p, pos)
    assert t32.dtype == F and f.dtype == F
    with np.errstate(invalid="ignore"):
        e_t = np.abs(np.sqrt(t32.astype(np.float64)) - d64)
    e_t = np.where(np.isnan(e_t), np.inf, e_t)      # a NaN is a loss, too
    e_f = np.abs(np.sqrt(f.astype(np.float64)) - d64)
    unit = 2.0 ** -24 * np.maximum(np.abs(p).max(1), np.abs(pos).max()).astype(np.float64)[:, None]
    print(f"slivers 1:10,000: textbook in float32 off by {e_t.max():.3g} ({(e_t / unit).max():.3g} x 2^-24 M), f by {e_f.max():.3g} ({(e_f / unit).max():.3g} x 2^-24 M)")
    assert e_t.max() > width
    assert e_t.max() > 100 * e_f.max()


def test_f_is_total_on_zero_area_triangles_and_never_below_its_floor():
    rs = np.random.RandomState(3)
    v = rs.uniform(-5, 5, (40, 3)).astype(F)
    w = rs.uniform(-5, 5, (40, 3)).astype(F)
    pos = np.concatenate([np.stack([v, v, v], 1), np.stack([v, v, w], 1), np.stack([v, w, v], 1), np.stack([v, w, w], 1),
                          np.stack([v, (v + w) * F(0.5), w], 1)])      # three equal, two equal (three ways), collinear
    p = np.concatenate([N.room_points(rs, 200), v, w, (v + w) * F(0.5), N.room_points(rs, 50) * F(300)])
    f = N.f_matrix(p, pos)
    assert np.isfinite(f).all() and (f >= 0).all()
    exact = np.sqrt(((p[:, None, :].astype(np.float64) - v[None].astype(np.float64)) ** 2).sum(-1))      # a point triangle is its vertex
    assert np.allclose(np.sqrt(f[:, :40].astype(np.float64)), exact, rtol=1e-5, atol=1e-5)
    assert (f[200:240, :40][np.arange(40), np.arange(40)] == 0).all()                              # the point itself
    # the floor, on real scenes and on the degenerate ones: f >= boxdist2(p, box of the record's triangle), exactly
    prims, _ = attribute_scene(ATTR_SEED, 12)
    for q in (pos, prim_positions(prims), prim_positions(needle_scene(NEEDLE_SEED, 512)[0])):
        for pts in (p, N.surface_points(rs, 300, q)):
            a, ab, ac = N.edges(q)
            T = N.tri_terms(pts[:, None, :], a[None], ab[None], ac[None])
            assert (T["f"] >= T["floor"]).all() and (T["f"] >= T["d_raw"]).all()
            assert ((T["f"] == T["floor"]) | (T["f"] == T["d_raw"])).all()


def test_brute_force_breaks_exact_ties_towards_the_larger_index():
    prims, g = attribute_scene(ATTR_SEED, 12)
    pos = prim_positions(prims)
    assert len(g["dups"]) == 40 and np.array_equal(bits(pos[g["dups"]]), bits(pos[g["dup_of"]])) and (g["dups"] > g["dup_of"]).all()
    rs = np.random.RandomState(8)
    pts = N.with_radius(np.concatenate([N.surface_points(rs, 400, pos[g["dup_of"]]), N.vertex_and_edge_points(rs, 200, pos[g["dup_of"]])]), INF)
    d2, prim = N.brute(pts, pos)
    f = N.f_matrix(pts, pos)
    assert np.array_equal(bits(d2), bits(f.min(1)))
    for i in range(len(pts)):
        assert prim[i] == np.nonzero(f[i] == f[i].min())[0].max()
    won = np.isin(prim, g["dups"])
    print(f"a duplicate wins {won.mean():.3f} of the points on duplicated triangles; the copied triangle {np.isin(prim, g['dup_of']).mean():.3f}")
    assert won.mean() > 0.5 and not np.isin(prim, g["dup_of"]).any()
    # a radius that admits exactly the tie, and one just below it
    r = np.sqrt(d2.astype(np.float64))
    cut = pts.copy()
    cut[:, 3] = np.nextafter(r.astype(F), F(0))
    keep = (cut[:, 3] * cut[:, 3] < d2)
    d2c, primc = N.brute(cut, pos)
    assert (primc[keep] == -1).all() and (d2c[keep] == 0).all() and keep.sum() > 100


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


SCENES = ("cornell", "standin24_spheres", "attribute", "needle4096", "chain28", "comb32")
N_POINTS = {"needle4096": 200}      # per set; the others take 400
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _host_scene(name):
    """(nodes, tris, spheres) of a host-built scene."""
    def make():
        prims = {"cornell": lambda: ptamd.gen_scene(0, 187), "standin24_spheres": lambda: ptamd.gen_scene(1, 24),
                 "attribute": lambda: attribute_scene(ATTR_SEED, 12)[0], "needle4096": lambda: needle_scene(NEEDLE_SEED, 4096)[0]}[name]()
        nodes, tris, _ = ptamd.build_bvh(prims)
        return nodes, tris, make_test_spheres() if name == "standin24_spheres" else None
    return _cached(("host", name), make)


# The deep trees of tests/deep_tree_ref.py: the positions, and the depth budget of the rebuild that makes the tree deep (None: the plain call)
DEEP = {"chain28": (X.chain_positions, 28), "comb32": (lambda: Dp.comb_positions(32), None)}


def _positions(name):
    """(n, 3, 3) float32 in the order of `tris`: what brute force runs over."""
    if name in DEEP:
        return _cached(("pos", name), lambda: np.ascontiguousarray(DEEP[name][0](), F).reshape(-1, 3, 3))
    return R.positions(_host_scene(name)[1])


def _deep_scene(name):
    """Any host-built scene of as many triangles (two of them lights), moved to the deep tree's positions and rebuilt: the tree depends
    on the positions and the index in `tris` order alone."""
    pos = _positions(name)
    n = len(pos)
    rs = np.random.RandomState(23)
    a = rs.uniform(-8, 8, (n, 3)).astype(F) + F([0, 20, 0])
    b, c = a + rs.uniform(-3, 3, a.shape).astype(F), a + rs.uniform(-3, 3, a.shape).astype(F)
    prims = np.concatenate([make_prims(a[:n - 2], b[:n - 2], c[:n - 2]), make_prims(a[n - 2:], b[n - 2:], c[n - 2:], albedo=(0, 0, 0), emit=(6, 6, 6))])
    nodes, tris, _ = ptamd.build_bvh(prims)
    assert len(tris) == n
    sc = ptamd.Scene(nodes, tris)
    sc.update_vertices(pos.reshape(-1, 9))
    if DEEP[name][1] is None:
        sc.rebuild_tree()
    else:
        sc.rebuild_tree(depth_budget=DEEP[name][1], large_fraction=0.0)
    return sc


def _spheres(name):
    return None if name in DEEP else _host_scene(name)[2]


def _scene(name):
    """The device scene; chain28 and comb32 after the rebuild that makes them deep."""
    if name in DEEP:
        return _deep_scene(name)
    return ptamd.Scene(*_host_scene(name))


def _n_prims(name):
    sph = _spheres(name)
    return len(_positions(name)) + (0 if sph is None else len(sph))


def make_points(pos, spheres, seed, m):
    """POINT4 records against the positions: m uniform in the room and in the scene's box with an infinite radius; the same points with
    radii that cut roughly half of them off; m on triangles +- 1e-3; m exactly on vertices and edge midpoints; m / 2 vertices with
    radius 0; m / 2 points 300 times farther out; a few on and inside the spheres."""
    rs = np.random.RandomState(seed)
    v = pos.reshape(-1, 3)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    box = (lo - 0.1 * (hi - lo) + rs.uniform(0, 1, (m // 2, 3)) * 1.2 * (hi - lo)).astype(F)
    space = np.concatenate([N.room_points(rs, m - m // 2), box])
    d2, _ = N.brute(N.with_radius(space, INF), pos, spheres)
    half = F(np.sqrt(np.median(d2.astype(np.float64))))
    near = N.surface_points(rs, m, pos)
    near_r = np.where(np.arange(m) % 2 == 0, INF, F(7e-4)).astype(F)      # 1e-3 normal draws: a tight radius cuts some of them off
    verts = N.vertex_and_edge_points(rs, m, pos)
    zero_r = pos[rs.randint(0, len(pos), m // 2), rs.randint(0, 3, m // 2)]
    parts = [N.with_radius(space, INF), N.with_radius(space, half), N.with_radius(near, near_r), N.with_radius(verts, INF),
             N.with_radius(zero_r, 0.0), N.with_radius(N.room_points(rs, m // 2) * F(300), INF)]
    if spheres is not None:
        s = np.ascontiguousarray(spheres, F)
        k = rs.randint(0, len(s), 60)
        u = rs.standard_normal((60, 3))
        u /= np.sqrt((u * u).sum(1, keepdims=True))
        scale = np.where(np.arange(60) % 3 == 0, 0.0, np.where(np.arange(60) % 3 == 1, 0.6, 1.0))      # the centre, inside, on the surface
        parts.append(N.with_radius((s[k, 0:3] + (scale * s[k, 3])[:, None] * u).astype(F), INF))
    pts = np.ascontiguousarray(np.concatenate(parts), F)
    return pts[rs.permutation(len(pts))]      # every wave holds every kind


def _points(name):
    return _cached(("points", name), lambda: make_points(_positions(name), _spheres(name), 40 + SCENES.index(name), N_POINTS.get(name, 400)))


def _want(name):
    """(dist2, prim, detail) by brute force and numpy, computed once per scene."""
    def make():
        pts, pos, sph = _points(name), _positions(name), _spheres(name)
        d2, prim = N.brute(pts, pos, sph)
        return d2, prim, N.detail(pts, prim, pos, sph)
    return _cached(("want", name), make)


def assert_closest(got, want, what):
    d2, prim = np.asarray(got[0]), np.asarray(got[1])
    assert np.array_equal(prim, want[1]), f"{what}: {(prim != want[1]).sum()} prims differ, first at {np.nonzero(prim != want[1])[0][:5]}"
    assert np.array_equal(bits(d2), bits(want[0])), f"{what}: dist2 differs at {np.nonzero(bits(d2) != bits(want[0]))[0][:5]}"
    if len(got) > 2:
        ok = (bits(got[2]) == bits(want[2])).all(1)
        assert ok.all(), f"{what}: {(~ok).sum()} detail records differ, first at {np.nonzero(~ok)[0][:5]}: {np.asarray(got[2])[~ok][:2]} want {want[2][~ok][:2]}"


def assert_any(got, want, pts, pos, sph, what):
    d2, prim = np.asarray(got[0]), np.asarray(got[1])
    hit = want[1] >= 0
    assert np.array_equal(prim >= 0, hit), f"{what}: {((prim >= 0) != hit).sum()} points decide differently from the closest query"
    assert (prim[~hit] == -1).all() and (bits(d2[~hit]) == 0).all(), what
    assert (prim < len(pos) + (0 if sph is None else len(sph))).all(), what
    f = N.f_of(pts[hit], prim[hit], pos, sph)
    assert np.array_equal(bits(d2[hit]), bits(f)), f"{what}: dist2 is not f(p, prim)"
    assert (f <= pts[hit, 3] * pts[hit, 3]).all() and (f >= want[0][hit]).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_closest_point_is_brute_forces(_gpu, name):
    pts, pos, sph, want = _points(name), _positions(name), _spheres(name), _want(name)
    hit = want[1] >= 0
    print(f"{name}: {len(pts)} points, {len(pos)} triangles, found {hit.mean():.3f}, spheres win {(want[1] >= len(pos)).sum()}, "
          f"features {np.bincount(want[2][hit, 6].astype(int), minlength=5).tolist()}, dist2 == 0 at {(hit & (want[0] == 0)).sum()}")
    m = N_POINTS.get(name, 400)
    assert hit.mean() > 0.4 and (~hit).sum() >= m // 4 and (hit & (want[0] == 0)).sum() >= m // 2      # radii cut answers off; radius 0 on a vertex hits
    sc = _scene(name)
    info = sc.tree_info()
    assert (3 * info["quad_depth"] + 2 > 40) == (name in DEEP)      # the deep trees take the binary walk
    assert_closest(sc.closest_points(pts, detail=True), want, name)
    assert_closest(sc.closest_points(pts), want, name + " without detail")
    assert_any(sc.closest_points(pts, any_within=True), want, pts, pos, sph, name + " any")
    for lo, m in ((0, 1), (7, 63), (100, 64), (33, 65), (211, 130)):      # partial waves
        sub = tuple(x[lo:lo + m] for x in want)
        assert_closest(sc.closest_points(pts[lo:lo + m], detail=True), sub, f"{name}, n = {m}")
        assert_any(sc.closest_points(pts[lo:lo + m], any_within=True), sub, pts[lo:lo + m], pos, sph, f"{name} any, n = {m}")


CHILD = r"""
import sys
import numpy as np
import ptamd
from scenes_util import test_spheres
pts, out = np.load(sys.argv[1]), sys.argv[2]
nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, 24))
sc = ptamd.Scene(nodes, tris, test_spheres())
d2, prim, det = sc.closest_points(pts, detail=True)
ad2, aprim = sc.closest_points(pts, any_within=True)
np.savez(out, d2=d2, prim=prim, det=det, ad2=ad2, aprim=aprim)
"""


@pytest.mark.gpu
def test_binary_walk_forced_by_its_knob_gives_the_same_bits(_gpu, tmp_path):
    """PTAMD_QUERY_QUAD=0 in a fresh process (the knob is read when a scene is created), as tests/test_query.py sets it."""
    name = "standin24_spheres"
    pts_file, out = str(tmp_path / "pts.npy"), str(tmp_path / "child.npz")
    np.save(pts_file, _points(name))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]), PTAMD_QUERY_QUAD="0")
    subprocess.run([sys.executable, "-c", CHILD, pts_file, out], check=True, env=env, timeout=600)
    g = np.load(out)
    assert_closest((g["d2"], g["prim"], g["det"]), _want(name), "PTAMD_QUERY_QUAD=0")
    assert_any((g["ad2"], g["aprim"]), _want(name), _points(name), _positions(name), _spheres(name), "PTAMD_QUERY_QUAD=0 any")


def _turned(tris):
    """The stand-in mesh turned and wobbled; in a scene without one (the needles), every triangle."""
    mask = R.mesh_mask(tris)
    if not mask.any():
        mask = np.ones(len(tris), bool)
    return R.move_rigid_wobble(R.positions(tris), mask, np).reshape(-1, 9).astype(F)


@pytest.mark.gpu
def test_the_result_does_not_depend_on_the_tree(_gpu):
    """A refit tree, a fresh upload at the same pose and the three rebuilds hold different boxes and different topologies over the same
    positions: the same bits from all of them, and they are brute force's."""
    name = "standin24_spheres"
    nodes, tris, sph = _host_scene(name)
    pts = _points(name)
    pos2 = _turned(tris)
    want = N.brute(pts, pos2.reshape(-1, 3, 3), sph)
    want += (N.detail(pts, want[1], pos2.reshape(-1, 3, 3), sph),)
    moved = (want[1] != _want(name)[1]) | (bits(want[0]) != bits(_want(name)[0]))
    print(f"the move changed {moved.mean():.3f} of the results")
    assert moved.mean() > 0.2
    sc = ptamd.Scene(nodes, tris, sph)
    sc.update_vertices(pos2)
    assert_closest(sc.closest_points(pts, detail=True), want, "after update_vertices")
    tris2 = R.restate_tris(tris, pos2)
    fresh = ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph)
    assert_closest(fresh.closest_points(pts, detail=True), want, "fresh scene at the pose")
    info = [sc.tree_info()]
    sc.rebuild_tree()
    assert_closest(sc.closest_points(pts, detail=True), want, "after rebuild_tree")
    info.append(sc.tree_info())
    sc.rebuild_tree(depth_budget=26, large_fraction=1 / 16)
    assert_closest(sc.closest_points(pts, detail=True), want, "after rebuild_tree(26, 1/16)")
    info.append(sc.tree_info())
    sc.rebuild_tree_optimized()
    assert_closest(sc.closest_points(pts, detail=True), want, "after rebuild_tree_optimized")
    assert_any(sc.closest_points(pts, any_within=True), want, pts, pos2.reshape(-1, 3, 3), sph, "any after rebuild_tree_optimized")
    info.append(sc.tree_info())
    print("trees:", info)
    assert info[-1]["rebuilds"] == 3


@pytest.mark.gpu
def test_query_after_an_update_on_the_same_stream_sees_the_moved_geometry(_gpu):
    import torch
    name = "standin24_spheres"
    nodes, tris, sph = _host_scene(name)
    pts = _points(name)
    pos2 = _turned(tris)
    want = N.brute(pts, pos2.reshape(-1, 3, 3), sph)
    want += (N.detail(pts, want[1], pos2.reshape(-1, 3, 3), sph),)
    sc = ptamd.Scene(nodes, tris, sph)
    sc.update_vertices(R.positions(tris).reshape(-1, 9))      # the first update allocates the scene's maps: not what is measured below
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    bytes0 = sc.device_bytes
    with torch.cuda.stream(st):
        d_pos = torch.from_numpy(pos2).to(dev)
        d_pts = torch.from_numpy(pts).to(dev)
        sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
        got = sc.closest_points(d_pts, detail=True, stream_ptr=st.cuda_stream)      # no host wait in between
        got_any = sc.closest_points(d_pts, any_within=True, stream_ptr=st.cuda_stream)
        assert sc.device_bytes == bytes0      # a query allocates nothing
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].shape == (len(pts), 8) and got[0].device == dev
        host = [x.cpu().numpy() for x in got + got_any]
    st.synchronize()
    assert_closest(tuple(host[:3]), want, "device path behind an update")
    assert_any(tuple(host[3:]), want, pts, pos2.reshape(-1, 3, 3), sph, "device path, any")


def _assert_contained(sc, n_tris, what):
    tri = sc.dbg_array("tri")
    for tree, walk in (("quad", N.quad_containment), ("nodes", N.binary_containment)):
        bad, seen = walk(sc.dbg_array(tree), tri)
        assert (seen[:n_tris] == 1).all(), f"{what}, {tree}: not every triangle is reached exactly once"
        assert not bad, f"{what}, {tree}: {len(bad)} child boxes do not contain the triangles below them, first {bad[:5]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["standin24_spheres", "attribute", "needle4096"])
def test_widened_child_boxes_contain_the_record_boxes_below_them(_gpu, name):
    """The premise of the pruning, on the arrays the kernel reads: every child box of either tree, widened exactly
    as the kernel widens it, contains the box of (a, a + ab, a + ac) of every triangle below it — after upload, a refit and each of the
    three rebuilds."""
    nodes, tris, sph = _host_scene(name)
    sc = ptamd.Scene(nodes, tris, sph)
    _assert_contained(sc, len(tris), "upload")
    sc.update_vertices(_turned(tris))
    _assert_contained(sc, len(tris), "refit")
    sc.rebuild_tree()
    _assert_contained(sc, len(tris), "rebuild_tree")
    sc.rebuild_tree(depth_budget=26, large_fraction=1 / 16)
    _assert_contained(sc, len(tris), "rebuild_tree(26, 1/16)")
    sc.rebuild_tree_optimized()
    _assert_contained(sc, len(tris), "rebuild_tree_optimized")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DEEP))
def test_widened_child_boxes_contain_the_record_boxes_in_the_deep_trees(_gpu, name):
    """The same premise on the trees the binary walk takes by depth."""
    _assert_contained(_deep_scene(name), len(_positions(name)), name)


@pytest.mark.gpu
def test_queries_leave_renders_alone(_gpu):
    import torch
    name = "standin24_spheres"
    pts = _points(name)
    cam, prm = ptamd.make_camera(100, 52), ptamd.default_params(passes=3, spp_per_pass=4)
    sc = _scene(name)
    sc.closest_points(pts)      # before the first render, too
    img = sc.render(cam, prm)
    state = (sc.last_iterations(), sc.device_bytes)
    d_pts = torch.from_numpy(pts).cuda()
    sc.closest_points(pts, detail=True)
    sc.closest_points(pts, any_within=True)
    sc.closest_points(d_pts, detail=True)
    sc.closest_points(d_pts, any_within=True)
    torch.cuda.synchronize()
    assert (sc.last_iterations(), sc.device_bytes) == state
    img2 = sc.render(cam, prm)
    assert np.array_equal(bits(img), bits(img2)) and np.array_equal(bits(img), bits(_scene(name).render(cam, prm)))
    assert (sc.last_iterations(), sc.device_bytes) == state


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["standin24_spheres", "comb32"])
def test_odd_records_end_and_leave_their_neighbours_alone(_gpu, name):
    """A NaN coordinate, an infinite coordinate and a negative radius in one batch of 130: the call returns, those rows keep prim in
    range, and every other row is brute force's."""
    pts, want = _points(name)[:130].copy(), tuple(x[:130] for x in _want(name))
    odd = [5, 70, 100]
    pts[5, 1], pts[70, 0], pts[100, 3] = np.nan, np.inf, -1.0
    keep = np.ones(130, bool)
    keep[odd] = False
    sc = _scene(name)
    got = sc.closest_points(pts, detail=True)
    assert ((got[1] >= -1) & (got[1] < _n_prims(name))).all()
    assert_closest(tuple(x[keep] for x in got), tuple(x[keep] for x in want), name + ", the rows beside the odd ones")
    got_any = sc.closest_points(pts, any_within=True)
    assert ((got_any[1] >= -1) & (got_any[1] < _n_prims(name))).all()
    assert_any(tuple(x[keep] for x in got_any), tuple(x[keep] for x in want), pts[keep], _positions(name), _spheres(name), name + " any")
