"""The K nearest primitives and the count within a radius (pt_nearest_k, pt_count_within and their _host variants, Scene.nearest_k,
Scene.count_within).

On the CPU: the C-ABI surface, the argument checks with a fake scene and fake device addresses, the wrapper's own checks, and the
yardstick's properties (tests/nearest_k_ref.py: k = 1 is the closest query's brute force, a shorter list is a prefix of a longer one,
a duplicated triangle precedes the one it copies).

On the GPU: bits only, no tolerance, and no point left out of a comparison.  Every slot of every list against brute force over the
full f matrix, the detail records against numpy, column 0 against Scene.closest_points, the counts against the mask's row sums, the
same bits whatever tree the scene holds, stream order behind an update, no side effects on renders, the exactly-once premise on the
downloaded arrays of the tree that was walked, and a batch with odd records.  The scenes are tests/test_nearest.py's, built by its
helpers; the point sets are nearest_k_ref.PointSets, and every test asserts on its own reference that the sets hold what they are
meant to hold (lists that overflow, lists that stay short, empty lists, ties at the cut and inside the list) before it compares."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dynamic_ref as R
import nearest_k_ref as K
import nearest_ref as N
import ptamd
import test_nearest as T
from scenes_util import attribute_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pathtrace-on-cuda_amd")
F = np.float32
INF = F(np.inf)
bits = T.bits
SLICES = ((0, 1), (7, 63), (100, 64), (33, 65), (211, 130))      # partial waves, one wave, a wave and a lane, two waves and two lanes


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
NEW = ("pt_nearest_k", "pt_nearest_k_host", "pt_count_within", "pt_count_within_host")


def test_new_symbols_are_exported_declared_and_bound(tmp_path):
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    assert callable(ptamd.Scene.nearest_k) and callable(ptamd.Scene.count_within)
    assert ptamd.NEAREST_KMAX == 32
    src = tmp_path / "kmax.c"
    src.write_text('#include "pt_api.h"\n_Static_assert(PT_NEAREST_KMAX == 32, "PT_NEAREST_KMAX");\n')
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    at = hdr.index("K nearest and counts within a radius")
    assert hdr.index("Closest-point queries") < at < hdr.index("Radiance along the caller's own rays")
    assert hdr.index(" pt_closest_points_host(") < at      # directly after that section: its last declaration comes before, the next section after


def test_bad_arguments_are_rejected_before_any_device_call():
    """A fake scene and fake device addresses: never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    base = 1 << 40
    scene, pts, out, det, cnt = (C.c_void_p(base + (i << 20)) for i in range(5))
    off = lambda p, k: C.c_void_p(p.value + k)      # noqa: E731
    dev = [
        ("NULL scene", (None, pts, 64, 8, out, None)),
        ("NULL points", (scene, None, 64, 8, out, None)),
        ("NULL out", (scene, pts, 64, 8, None, None)),
        ("n < 0", (scene, pts, -1, 8, out, None)),
        ("k = 0", (scene, pts, 64, 0, out, None)),
        ("k = 33", (scene, pts, 64, 33, out, None)),
        ("k = -1", (scene, pts, 64, -1, out, None)),
        ("points + 4", (scene, off(pts, 4), 64, 8, out, None)),
        ("points + 8", (scene, off(pts, 8), 64, 8, out, None)),
        ("out + 4", (scene, pts, 64, 8, off(out, 4), None)),
        ("detail + 2", (scene, pts, 64, 8, out, off(det, 2))),
        ("n = 0 does not excuse a NULL", (scene, None, 0, 8, out, None)),
        ("n = 0 does not excuse k = 0", (scene, pts, 0, 0, out, None)),
    ]
    for what, a in dev:
        assert l.pt_nearest_k(*a, None) == -1, what
        assert b"pt_nearest_k:" in l.pt_last_error(), (what, l.pt_last_error())
    dev_count = [
        ("NULL scene", (None, pts, 64, cnt)),
        ("NULL points", (scene, None, 64, cnt)),
        ("NULL out", (scene, pts, 64, None)),
        ("n < 0", (scene, pts, -1, cnt)),
        ("points + 8", (scene, off(pts, 8), 64, cnt)),
        ("count + 2", (scene, pts, 64, off(cnt, 2))),
        ("n = 0 does not excuse a NULL", (scene, pts, 0, None)),
    ]
    for what, a in dev_count:
        assert l.pt_count_within(*a, None) == -1, what
        assert b"pt_count_within:" in l.pt_last_error(), (what, l.pt_last_error())
    h_pts, h_out, h_det, h_cnt = np.zeros((64, 4), F), np.zeros((64, 8), ptamd.NEAREST_DTYPE), np.zeros((64, 8, 8), F), np.zeros(64, np.int32)
    P = ptamd._ptr
    host = [
        ("NULL scene", (None, P(h_pts), 64, 8, P(h_out), None)),
        ("NULL points", (scene, None, 64, 8, P(h_out), None)),
        ("NULL out", (scene, P(h_pts), 64, 8, None, P(h_det))),
        ("n < 0", (scene, P(h_pts), -5, 8, P(h_out), None)),
        ("k = 0", (scene, P(h_pts), 64, 0, P(h_out), None)),
        ("k = 33", (scene, P(h_pts), 64, 33, P(h_out), None)),
        ("k = -1", (scene, P(h_pts), 64, -1, P(h_out), None)),
    ]
    for what, a in host:
        assert l.pt_nearest_k_host(*a) == -1, what
        assert b"pt_nearest_k_host:" in l.pt_last_error(), (what, l.pt_last_error())
    host_count = [
        ("NULL scene", (None, P(h_pts), 64, P(h_cnt))),
        ("NULL points", (scene, None, 64, P(h_cnt))),
        ("NULL out", (scene, P(h_pts), 64, None)),
        ("n < 0", (scene, P(h_pts), -5, P(h_cnt))),
    ]
    for what, a in host_count:
        assert l.pt_count_within_host(*a) == -1, what
        assert b"pt_count_within_host:" in l.pt_last_error(), (what, l.pt_last_error())
    # nothing to do: PT_OK, still without touching the scene or the device
    assert l.pt_nearest_k(scene, pts, 0, 1, out, None, None) == 0
    assert l.pt_nearest_k(scene, pts, 0, 32, out, det, None) == 0
    assert l.pt_nearest_k_host(scene, P(h_pts), 0, 8, P(h_out), None) == 0
    assert l.pt_count_within(scene, pts, 0, cnt, None) == 0
    assert l.pt_count_within_host(scene, P(h_pts), 0, P(h_cnt)) == 0


class _FakeScene:
    n_tris, device, _h = 5, 0, C.c_void_p(1 << 40)


def test_wrapper_checks_shape_dtype_device_and_k_on_the_host():
    import torch
    fake = _FakeScene()
    nk, cw = ptamd.Scene.nearest_k, ptamd.Scene.count_within
    for pts in (np.zeros((4, 3), F), np.zeros(16, F), np.zeros((2, 4, 4), F)):
        with pytest.raises(ptamd.PtError):
            nk(fake, pts, 4)
        with pytest.raises(ptamd.PtError):
            cw(fake, pts)
    for pts in (torch.zeros((5, 4)), torch.zeros((5, 4), dtype=torch.float64), torch.zeros((5, 3)), torch.zeros((4, 5)).t(), [[0.0] * 4]):
        with pytest.raises(ptamd.PtError):      # a CPU tensor, a wrong dtype, a wrong shape, not contiguous, not an array
            nk(fake, pts, 4)
        with pytest.raises(ptamd.PtError):
            cw(fake, pts)
    for k in (0, 33, -1):
        with pytest.raises(ptamd.PtError):
            nk(fake, np.zeros((4, 4), F), k)
    d2, prim, det = nk(fake, np.zeros((0, 4), F), 7, detail=True)      # n = 0: PT_OK without a device
    assert d2.shape == (0, 7) and prim.shape == (0, 7) and det.shape == (0, 7, 8) and d2.dtype == F and prim.dtype == np.int32
    cnt = cw(fake, np.zeros((0, 4), F))
    assert cnt.shape == (0,) and cnt.dtype == np.int32


def _attribute():
    prims, g = attribute_scene(T.ATTR_SEED, 12)
    return T.prim_positions(prims), g


def test_yardstick_with_k_1_is_the_closest_querys_brute_force():
    pos, _ = _attribute()
    sph = T.make_test_spheres()
    ps = K.PointSets(pos, sph)
    for k in (1, 8):
        pts = ps.points(k)
        d2, prim = K.brute_k(pts, pos, sph, 1, ps.f)
        want = N.brute(pts, pos, sph)
        assert np.array_equal(bits(d2[:, 0]), bits(want[0])) and np.array_equal(prim[:, 0], want[1])
        assert (want[1] >= len(pos)).any(), "no sphere wins anywhere: the spheres' columns go unchecked"


def test_yardstick_lists_are_prefixes_of_longer_lists_and_counts_are_their_lengths():
    pos, _ = _attribute()
    ps = K.PointSets(pos, None)
    pts = ps.points(8)
    lists = {k: K.brute_k(pts, pos, None, k, ps.f) for k in K.KS}
    cnt = K.count(pts, pos, None, ps.f)
    for k in K.KS:
        for k2 in K.KS:
            if k < k2:
                assert np.array_equal(bits(lists[k][0]), bits(lists[k2][0][:, :k])) and np.array_equal(lists[k][1], lists[k2][1][:, :k]), (k, k2)
        d2, prim = lists[k]
        assert np.array_equal((prim >= 0).sum(1), np.minimum(cnt, k))
        assert ((prim >= 0)[:, :-1] >= (prim >= 0)[:, 1:]).all(), "a miss slot before a candidate"
        assert (bits(d2)[prim < 0] == 0).all()
        r2 = (pts[:, 3] * pts[:, 3])[:, None]
        assert (d2[prim >= 0] <= np.broadcast_to(r2, d2.shape)[prim >= 0]).all()
        later = prim[:, 1:] >= 0
        assert ((d2[:, 1:] > d2[:, :-1]) | ((d2[:, 1:] == d2[:, :-1]) & (prim[:, 1:] < prim[:, :-1])) | ~later).all(), "the order of the definition"
        for i in range(0, len(pts), 37):      # no primitive twice in a list
            p = prim[i][prim[i] >= 0]
            assert len(np.unique(p)) == len(p)


def test_yardstick_puts_a_duplicated_triangle_before_the_one_it_copies():
    pos, g = _attribute()
    assert len(g["dups"]) == 40 and np.array_equal(bits(pos[g["dups"]]), bits(pos[g["dup_of"]])) and (g["dups"] > g["dup_of"]).all()
    rs = np.random.RandomState(8)
    pts = N.with_radius(np.concatenate([N.surface_points(rs, 200, pos[g["dup_of"]]), N.vertex_and_edge_points(rs, 100, pos[g["dup_of"]])]), INF)
    d2, prim = K.brute_k(pts, pos, None, 8)
    copy_of = dict(zip(g["dups"].tolist(), g["dup_of"].tolist()))
    pairs = 0
    for i in range(len(pts)):
        for j in range(8):
            if int(prim[i, j]) not in copy_of:
                continue
            tied = (bits(d2[i]) == bits(d2[i, j])) & (prim[i] >= 0)
            at = np.nonzero(prim[i] == copy_of[int(prim[i, j])])[0]
            if len(at) == 0:      # the copied triangle fell off the end of the list: everything from the duplicate on ties with it
                assert tied[j:].all(), (i, j, prim[i])
                continue
            assert at[0] > j and tied[j:at[0] + 1].all(), (i, j, prim[i])      # the duplicate first, equal f in between
            if tied.sum() == 2:      # no third triangle shares the f (a neighbour across a vertex or an edge would sit between them)
                assert at[0] == j + 1, (i, j, prim[i])
                pairs += 1
    print(f"{pairs} duplicate pairs in adjacent slots over {len(pts)} lists")
    assert pairs >= 200      # the 200 points inside duplicated triangles: the pair leads the list, nothing else ties with it


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


ALL_KS = ("standin24_spheres", "attribute")      # K in (1, 2, 7, 8, 32); the others K in (1, 8, 32)
# Every scene's point sets are asserted to hold every kind of list in the shares of the recipe: more than K candidates at >= 0.4 of the
# points, fewer than K but some at >= 0.15 (K >= 2), none at >= 0.05.  Cornell alone cannot hold two of them, and is asserted on what it
# can: its 12 triangles overflow no list of 32 (more = 0 at K = 32; 0.62 at K = 1, 0.461 at K = 8), and at K = 8 and 32 the cut radius,
# the median 8th (12th) smallest of 12 distances, spans the room, so that only surface points moved off by more than their 7e-4 radius
# find nothing (none = 0.031 at K = 8 and 32; 0.131 at K = 1).  Its short lists are plenty: fewer = 0.469 at K = 8, 0.969 at K = 32.
_SETS = {}


def _ks(name):
    return K.KS if name in ALL_KS else (1, 8, 32)


def _sets(name):
    if name not in _SETS:
        _SETS[name] = K.PointSets(T._positions(name), T._spheres(name))
    return _SETS[name]


def _want_detail(ps, k):
    key = ("detail", k)
    if key not in ps._cache:
        pts, _, prim, _ = ps.want(k)
        ps._cache[key] = N.detail(np.repeat(pts, k, 0), prim.reshape(-1), ps.positions, ps.spheres).reshape(len(pts), k, 8)
    return ps._cache[key]


def assert_sets_hold_what_they_should(name, k):
    fig = _sets(name).figures(k)
    print(f"{name}, K = {k}: {fig}")
    if name == "cornell":
        assert (fig["more"] >= 0.4 or k >= T._n_prims(name)) and (fig["none"] >= 0.05 if k == 1 else fig["none"] > 0), (name, k, fig)
    else:
        assert fig["more"] >= 0.4 and fig["none"] >= 0.05, (name, k, fig)
    assert k < 2 or fig["fewer"] >= 0.15, (name, k, fig)
    if name == "attribute":
        assert fig["cut_ties"] >= 100 and (k < 2 or fig["inside_ties"] >= 200), (name, k, fig)


def assert_lists(got, want, what):
    """got: (dist2, prim[, detail]) of shape (n, k[, 8]); want: the same from the yardstick."""
    d2, prim = np.asarray(got[0]), np.asarray(got[1])
    assert d2.shape == want[0].shape and prim.shape == want[1].shape and d2.dtype == F and prim.dtype == np.int32, what
    bad = (prim != want[1]).any(1)
    assert not bad.any(), f"{what}: the prims of {bad.sum()} points differ, first at {np.nonzero(bad)[0][:5]}: {prim[bad][:2]} want {want[1][bad][:2]}"
    bad = (bits(d2) != bits(want[0])).any(1)
    assert not bad.any(), f"{what}: dist2 differs at {np.nonzero(bad)[0][:5]}"
    if len(got) > 2:
        det = np.asarray(got[2])
        assert det.shape == want[2].shape, what
        bad = (bits(det) != bits(want[2])).any((1, 2))
        assert not bad.any(), f"{what}: the detail records of {bad.sum()} points differ, first at {np.nonzero(bad)[0][:5]}"


def _assert_walk(sc, name):
    info = sc.tree_info()
    assert (3 * info["quad_depth"] + 2 > 40) == (name in T.DEEP)      # the deep trees take the binary walk


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.SCENES)
def test_nearest_k_is_brute_forces(_gpu, name):
    ps, sc = _sets(name), T._scene(name)
    _assert_walk(sc, name)
    for k in _ks(name):
        assert_sets_hold_what_they_should(name, k)
        pts, d2, prim, _ = ps.want(k)
        det = _want_detail(ps, k)
        assert_lists(sc.nearest_k(pts, k, detail=True), (d2, prim, det), f"{name}, K = {k}")
        assert_lists(sc.nearest_k(pts, k), (d2, prim), f"{name}, K = {k}, without detail")
        c2, cprim = sc.closest_points(pts)
        assert np.array_equal(bits(c2), bits(d2[:, 0])) and np.array_equal(cprim, prim[:, 0]), f"{name}, K = {k}: column 0 is not closest_points'"
        for lo, m in SLICES:
            assert_lists(sc.nearest_k(pts[lo:lo + m], k, detail=True), (d2[lo:lo + m], prim[lo:lo + m], det[lo:lo + m]), f"{name}, K = {k}, n = {m}")
    if name == "cornell":
        assert (ps.want(32)[2][:, 12:] == -1).all()      # 12 triangles: k = 32 pads every list


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.SCENES)
def test_count_within_is_the_masks_row_sum(_gpu, name):
    ps, sc = _sets(name), T._scene(name)
    _assert_walk(sc, name)
    for k in _ks(name):
        assert_sets_hold_what_they_should(name, k)
        pts, _, _, cnt = ps.want(k)
        got = sc.count_within(pts)
        assert got.dtype == np.int32 and np.array_equal(got, cnt), f"{name}, K = {k}: {(got != cnt).sum()} counts differ, first at {np.nonzero(got != cnt)[0][:5]}"
        for lo, m in SLICES:
            assert np.array_equal(sc.count_within(pts[lo:lo + m]), cnt[lo:lo + m]), f"{name}, K = {k}, n = {m}"
        slots = (sc.nearest_k(pts, k)[1] >= 0).sum(1)
        assert np.array_equal(np.minimum(got, k), slots), f"{name}, K = {k}: min(k, count) is not the number of slots filled"
    if name in ("cornell", "standin24_spheres"):      # an infinite radius counts every primitive, spheres included
        everything = pts.copy()
        everything[:, 3] = INF
        assert (sc.count_within(everything) == T._n_prims(name)).all()
        assert T._n_prims(name) > len(T._positions(name)) or name == "cornell"


CHILD = r"""
import sys
import numpy as np
import ptamd
from scenes_util import test_spheres
out = sys.argv[2]
nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, 24))
sc = ptamd.Scene(nodes, tris, test_spheres())
res = {}
with np.load(sys.argv[1]) as sets:
    for key in sets.files:
        d2, prim, det = sc.nearest_k(sets[key], int(key), detail=True)
        res.update({"d2_" + key: d2, "prim_" + key: prim, "det_" + key: det, "cnt_" + key: sc.count_within(sets[key])})
np.savez(out, **res)
"""


@pytest.mark.gpu
def test_binary_walk_forced_by_its_knob_gives_the_same_bits(_gpu, tmp_path):
    """PTAMD_QUERY_QUAD=0 in a fresh process (the knob is read when a scene is created), as tests/test_nearest.py sets it."""
    name = "standin24_spheres"
    ps = _sets(name)
    pts_file, out = str(tmp_path / "pts.npz"), str(tmp_path / "child.npz")
    np.savez(pts_file, **{str(k): ps.points(k) for k in K.KS})
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]), PTAMD_QUERY_QUAD="0")
    subprocess.run([sys.executable, "-c", CHILD, pts_file, out], check=True, env=env, timeout=600)
    g = np.load(out)
    for k in K.KS:
        assert_sets_hold_what_they_should(name, k)
        _, d2, prim, cnt = ps.want(k)
        assert_lists((g[f"d2_{k}"], g[f"prim_{k}"], g[f"det_{k}"]), (d2, prim, _want_detail(ps, k)), f"PTAMD_QUERY_QUAD=0, K = {k}")
        assert np.array_equal(g[f"cnt_{k}"], cnt), f"PTAMD_QUERY_QUAD=0, K = {k}: counts"


def _moved_want(name, ks):
    """The yardstick at the turned pose of tests/test_nearest.py, for the scene's own point sets: {k: (pts, d2, prim, detail, count)}."""
    def make():
        _, tris, sph = T._host_scene(name)
        ps = _sets(name)
        pos2 = T._turned(tris)
        p3 = pos2.reshape(-1, 3, 3)
        f = K.f_all(ps.points(1), p3, sph)      # the radius is not part of f: one matrix serves every K
        res = {}
        for k in ks:
            pts = ps.points(k)
            d2, prim = K.brute_k(pts, p3, sph, k, f)
            res[k] = (pts, d2, prim, N.detail(np.repeat(pts, k, 0), prim.reshape(-1), p3, sph).reshape(len(pts), k, 8), K.count(pts, p3, sph, f))
        return pos2, res
    return T._cached(("moved_k", name, ks), make)


def _assert_pose(sc, res, what):
    for k, (pts, d2, prim, det, cnt) in res.items():
        assert_lists(sc.nearest_k(pts, k, detail=True), (d2, prim, det), f"{what}, K = {k}")
        assert np.array_equal(sc.count_within(pts), cnt), f"{what}, K = {k}: counts"


@pytest.mark.gpu
def test_the_result_does_not_depend_on_the_tree(_gpu):
    """A refit tree, a fresh upload at the same pose and the three rebuilds hold different boxes and different topologies over the same
    positions: the same bits from all of them, and they are brute force's."""
    name = "standin24_spheres"
    nodes, tris, sph = T._host_scene(name)
    pos2, res = _moved_want(name, K.KS)
    for k in K.KS:
        assert_sets_hold_what_they_should(name, k)
        moved = (res[k][2] != _sets(name).want(k)[2]).any(1)
        print(f"K = {k}: the move changed {moved.mean():.3f} of the lists")
        assert moved.mean() > 0.2
    sc = ptamd.Scene(nodes, tris, sph)
    sc.update_vertices(pos2)
    _assert_pose(sc, res, "after update_vertices")
    tris2 = R.restate_tris(tris, pos2)
    _assert_pose(ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph), res, "fresh scene at the pose")
    sc.rebuild_tree()
    _assert_pose(sc, res, "after rebuild_tree")
    sc.rebuild_tree(depth_budget=26, large_fraction=1 / 16)
    _assert_pose(sc, res, "after rebuild_tree(26, 1/16)")
    sc.rebuild_tree_optimized()
    _assert_pose(sc, res, "after rebuild_tree_optimized")
    assert sc.tree_info()["rebuilds"] == 3


@pytest.mark.gpu
def test_queries_after_an_update_on_the_same_stream_see_the_moved_geometry(_gpu):
    import torch
    name = "standin24_spheres"
    nodes, tris, sph = T._host_scene(name)
    pos2, res = _moved_want(name, K.KS)
    sc = ptamd.Scene(nodes, tris, sph)
    sc.update_vertices(R.positions(tris).reshape(-1, 9))      # the first update allocates the scene's maps: not what is measured below
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    bytes0 = sc.device_bytes
    host = {}
    with torch.cuda.stream(st):
        d_pos = torch.from_numpy(pos2).to(dev)
        d_pts = {k: torch.from_numpy(res[k][0]).to(dev) for k in (7, 32)}
        sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
        got = {k: sc.nearest_k(d_pts[k], k, detail=True, stream_ptr=st.cuda_stream) + (sc.count_within(d_pts[k], stream_ptr=st.cuda_stream),)
               for k in (7, 32)}      # no host wait in between
        assert sc.device_bytes == bytes0      # a query allocates nothing
        g = got[7]
        assert g[0].dtype == torch.float32 and g[1].dtype == torch.int32 and g[0].shape == g[1].shape == (len(res[7][0]), 7)
        assert g[2].shape == (len(res[7][0]), 7, 8) and g[3].dtype == torch.int32 and g[0].device == dev
        for k in got:
            host[k] = [x.cpu().numpy() for x in got[k]]
    st.synchronize()
    for k, h in host.items():
        _, d2, prim, det, cnt = res[k]
        assert_lists((np.ascontiguousarray(h[0]), np.ascontiguousarray(h[1]), h[2]), (d2, prim, det), f"device path behind an update, K = {k}")
        assert np.array_equal(h[3], cnt), f"device path behind an update, K = {k}: counts"


@pytest.mark.gpu
def test_queries_leave_renders_alone(_gpu):
    import torch
    name = "standin24_spheres"
    pts = _sets(name).points(8)
    cam, prm = ptamd.make_camera(100, 52), ptamd.default_params(passes=3, spp_per_pass=4)
    sc = T._scene(name)
    sc.nearest_k(pts, 8)      # before the first render, too
    sc.count_within(pts)
    img = sc.render(cam, prm)
    state = (sc.last_iterations(), sc.device_bytes)
    d_pts = torch.from_numpy(pts).cuda()
    sc.nearest_k(pts, 32, detail=True)
    sc.count_within(pts)
    sc.nearest_k(d_pts, 3, detail=True)
    sc.count_within(d_pts)
    torch.cuda.synchronize()
    assert (sc.last_iterations(), sc.device_bytes) == state
    img2 = sc.render(cam, prm)
    assert np.array_equal(bits(img), bits(img2)) and np.array_equal(bits(img), bits(T._scene(name).render(cam, prm)))
    assert (sc.last_iterations(), sc.device_bytes) == state


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.SCENES)
def test_every_triangle_sits_below_exactly_one_leaf_of_the_tree_walked(_gpu, name):
    """The premise a list needs and the closest query did not: a triangle met twice would fill two slots and be
    counted twice.  On the downloaded arrays of whichever tree the queries walk."""
    sc = T._scene(name)
    _assert_walk(sc, name)
    tree, walk = ("nodes", N.binary_containment) if name in T.DEEP else ("quad", N.quad_containment)
    bad, seen = walk(sc.dbg_array(tree), sc.dbg_array("tri"))
    n = len(T._positions(name))
    assert (seen[:n] == 1).all() and (seen[n:] == 0).all(), f"{name}, {tree}: {(seen[:n] != 1).sum()} triangles are not reached exactly once"
    assert not bad, f"{name}, {tree}: {len(bad)} child boxes do not contain the triangles below them"


@pytest.mark.gpu
def test_slot_numbers_past_two_to_the_31(_gpu):
    """2^26 + 65 points at k = 32 are 2^31 + 2080 slots in one launch: the record offsets need 64 bits, and nothing smaller reaches
    them.  DEVICE MEMORY: 16 GB of records (2^31 slots of 8 bytes, no less can be resident) and 1 GB of points; the checks go over
    the records in pieces of 2^21 points, 0.5 GB, with temporaries of 0.2 GB; under 4 s on an MI355X.  No detail records (they
    would be 64 GB more).  All but the last 65 points are far outside the room with radius 0 (the root's boxes are out of reach: a
    miss at once); the last 65 are the first 65 of the Cornell set, and their lists, which sit past slot 2^31, are brute force's.
    The 2^31 miss slots before them are checked on the device."""
    import torch
    name, k, tail, piece = "cornell", 32, 65, 1 << 21
    pts, d2, prim, _ = (x[:tail] for x in _sets(name).want(k))
    n = (1 << 26) + tail
    dev = torch.device("cuda:0")
    d_pts = torch.empty((n, 4), dtype=torch.float32, device=dev)
    d_pts[:, 0:3] = 1e6
    d_pts[:, 3] = 0.0
    d_pts[n - tail:] = torch.from_numpy(pts).to(dev)
    got_d2, got_prim = T._scene(name).nearest_k(d_pts, k)
    torch.cuda.synchronize()
    assert got_prim.shape == (n, k) and n * k > 1 << 31
    wrong = torch.zeros((), dtype=torch.int64, device=dev)
    for lo in range(0, n - tail, piece):
        hi = min(lo + piece, n - tail)
        wrong += (got_prim[lo:hi] != -1).sum() + (got_d2[lo:hi].view(torch.int32) != 0).sum()
    assert int(wrong) == 0, f"{int(wrong)} of the 2^31 miss slots are not (0, -1)"
    assert_lists((got_d2[n - tail:].cpu().numpy(), got_prim[n - tail:].cpu().numpy()), (d2, prim), "the lists past slot 2^31")
    assert (prim >= 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["standin24_spheres", "comb32"])
def test_odd_records_end_and_leave_their_neighbours_alone(_gpu, name):
    """A NaN coordinate, an infinite coordinate and a negative radius in one batch of 130: the calls return, those rows keep every prim
    and count in range, and every other row is brute force's."""
    ps = _sets(name)
    n_prims = T._n_prims(name)
    keep = np.ones(130, bool)
    keep[[5, 70, 100]] = False
    sc = T._scene(name)
    for k in (1, 8, 32):
        pts, d2, prim, cnt = (x[:130] for x in ps.want(k))
        det = _want_detail(ps, k)[:130]
        pts = pts.copy()
        pts[5, 1], pts[70, 0], pts[100, 3] = np.nan, np.inf, -1.0
        got = sc.nearest_k(pts, k, detail=True)
        assert ((got[1] >= -1) & (got[1] < n_prims)).all()
        assert_lists(tuple(x[keep] for x in got), (d2[keep], prim[keep], det[keep]), f"{name}, K = {k}, the rows beside the odd ones")
        got_cnt = sc.count_within(pts)
        assert ((got_cnt >= 0) & (got_cnt <= n_prims)).all()
        assert np.array_equal(got_cnt[keep], cnt[keep]), f"{name}, K = {k}: counts beside the odd ones"
