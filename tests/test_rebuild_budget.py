"""The tree rebuild with a depth budget and two size classes (pt_scene_rebuild_tree_ex; include/pt_api.h: "Tree rebuild with a depth
budget and two size classes").  On the CPU: the C-ABI surface, the parameter checks, and the numpy yardstick
(tests/rebuild_budget_ref.py: the keys stated independently of the device code, the budget stated twice) on the chain scene, whose
plain Morton tree is deeper than the kernels' stacks.  On the GPU, with the small frames, sample counts and helpers of
tests/test_rebuild.py: {0, 0} is pt_scene_rebuild_tree byte for byte; the trees are the yardstick's, are trees and keep the budget; the
chain scene is refused by the plain call and accepted by the new one with every result unchanged; the rebuilt arrays are a function of
the positions and the two parameters; later updates work on the new trees.  Bits everywhere; the one exception is the oracle frame of
the chain scene, compared by scenes_util.check_image as test_rebuild.py compares the attribute and needle scenes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import dynamic_ref as R
import ptamd
import rebuild_budget_ref as X
import rebuild_ref as B
import test_rebuild as T
from scenes_util import check_image, make_prims, pinhole_rays, scene_rays8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pt_rebuild_params_default", "pt_scene_rebuild_tree_ex")
PT_ERR_INVALID, PT_ERR_UNSUPPORTED = -1, -5
MAX_DEPTH = 32      # ptd::kStackDepth, as test_rebuild.py's limit test reads it back


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound():
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW_SYMBOLS:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    assert "typedef struct PtRebuildReport { int32_t n_large, n_flattened_tris; } PtRebuildReport;" in hdr
    assert "int32_t depth_budget;" in hdr and "float   large_fraction;" in hdr
    assert [(f, t) for f, t in ptamd.PtRebuildParams._fields_] == [("depth_budget", C.c_int32), ("large_fraction", C.c_float)]
    assert [(f, t) for f, t in ptamd.PtRebuildReport._fields_] == [("n_large", C.c_int32), ("n_flattened_tris", C.c_int32)]
    p = ptamd.PtRebuildParams(-7, -7.0)
    ptamd.lib().pt_rebuild_params_default(C.byref(p))
    assert (p.depth_budget, p.large_fraction) == (26, 0.0625) == (X.DEFAULT_BUDGET, X.DEFAULT_FRACTION)
    import inspect
    assert list(inspect.signature(ptamd.Scene.rebuild_tree).parameters) == ["self", "stream_ptr", "depth_budget", "large_fraction"]


def test_bad_parameters_are_rejected_before_any_device_call():
    """A fake scene address: never dereferenced, and no HIP call is made, when a parameter is bad."""
    l = ptamd.lib()
    scene = C.c_void_p(1 << 40)
    rep = ptamd.PtRebuildReport(-3, -3)
    ok = ptamd.PtRebuildParams(26, 0.0625)
    cases = [("NULL scene", None, ok), ("NULL params", scene, None)]
    for d, f in ((-1, 0.0), (33, 0.0), (1 << 30, 0.0), (26, -0.5), (26, float("nan")), (26, float("inf")), (26, float("-inf")), (0, -1e-30)):
        cases.append((f"depth_budget {d}, large_fraction {f}", scene, ptamd.PtRebuildParams(d, f)))
    for what, s, p in cases:
        assert l.pt_scene_rebuild_tree_ex(s, C.byref(p) if p is not None else None, C.byref(rep), None) == PT_ERR_INVALID, what
        assert "pt_scene_rebuild_tree_ex" in l.pt_last_error().decode(), (what, l.pt_last_error())
        assert (rep.n_large, rep.n_flattened_tris) == (-3, -3), what


def _tree_numbers(t):
    return t["depth"], t["quad_depth"]


def test_chain_scene_numbers():
    """Today's tree over the chain scene breaks the limit of 32; a budget D gives depth D - 1 exactly."""
    pos = X.chain_positions()
    assert pos.shape == (72, 3, 3) and (B.centroids(pos) == X.chain_centres()).all()
    keys = B.sorted_keys(pos)
    codes = sorted(int(k) >> 32 for k in keys)
    assert codes == [0] * 8 + [1 << j for j in range(30)] + [(1 << 30) - 1] * 34
    assert sorted(int(k) & 0xffffffff for k in keys if int(k) >> 32 == 0) == [0, 1, 2, 4, 8, 16, 32, 64]
    assert _tree_numbers(B.build(keys)) == (36, 17) and 36 > MAX_DEPTH
    for D, want in ((32, (31, 15)), (26, (25, 12)), (12, (11, 5)), (8, (7, 3)), (7, (6, 2))):
        t = X.build(pos, D, 0.0)
        assert _tree_numbers(t) == want, (D, _tree_numbers(t))
        assert np.array_equal(t["prim"], B.prim_order(keys)) and 0 < t["n_flattened_tris"] <= 72 and t["n_large"] == 0
        T._check_ref_is_a_tree(t, 72)
    assert X.clog2(72) == 7 and [X.clog2(m) for m in (1, 2, 3, 4, 5, 8, 9)] == [0, 1, 2, 2, 3, 3, 4]


def _key_sets():
    rs = np.random.RandomState(17)
    yield "chain", B.sorted_keys(X.chain_positions())
    yield "random", B.sorted_keys(T._tris_at(rs.uniform(-5, 5, (300, 3)).astype(np.float32)))
    yield "clustered", B.sorted_keys(T._tris_at((rs.uniform(-1, 1, (200, 3)) ** 7 * 40).astype(np.float32)))
    yield "coincident", np.arange(64, dtype=np.uint64)
    yield "three", B.sorted_keys(T._tris_at([[0, 0, 0], [8, 8, 8], [1, 0, 0]]))


def test_the_two_statements_of_the_budget_agree():
    """Bottom up (new keys, then the radix tree over them) against top down (split on the local rank once depth + clog2(size) >= D)."""
    for name, keys in _key_sets():
        n = len(keys)
        deep = B.build(keys)["depth"] + 1      # a leaf counts as a node
        for D in sorted({0, X.clog2(n), X.clog2(n) + 1, 8, 12, 26, 32, deep - 1, deep}):
            if 0 < D < X.clog2(n) or D > 32:
                continue
            new = X.bottom_up_keys(keys, D)
            c1, r1 = B.radix_tree(new)
            c2, r2 = X.top_down_tree(keys, D)
            assert np.array_equal(c1, c2) and np.array_equal(r1, r2), (name, D)
            if D:
                assert B.build(new)["depth"] + 1 <= D, (name, D)


def test_a_budget_the_tree_already_keeps_changes_no_key():
    """The tree's depth, a leaf counting as a node, is H + 1 for a radix tree whose deepest triangle is H links below the root.  A node
    at depth d over m triangles has a subtree at least clog2(m) high, so d + clog2(m) <= H < D for every D >= H + 1: no node is chosen."""
    for name, keys in _key_sets():
        child, _ = B.radix_tree(keys)
        H = int(X._parents_and_depths(child, len(keys))[1].max())
        assert B.build(keys)["depth"] in (H - 1, H), name      # H - 1 where the deepest triangles sit in a leaf of two
        for D in range(H + 1, 33):
            assert np.array_equal(X.bottom_up_keys(keys, D), keys), (name, D)


def test_zero_parameters_give_todays_keys():
    for pos in (X.chain_positions(), T._tris_at(np.random.RandomState(2).uniform(-5, 5, (100, 3)).astype(np.float32))):
        assert np.array_equal(X.class_keys(pos, 0.0), B.keys_of(pos))
        t, want = X.build(pos, 0, 0.0), B.build(B.sorted_keys(pos))
        assert (t["n_large"], t["n_flattened_tris"]) == (0, 0)
        for k in want:
            assert np.array_equal(t[k], want[k]), k


def test_the_root_joins_the_two_classes():
    """Cornell room + stand-in mesh at lat_lon 16, f = 1 / 16: both classes have members, and the root's children are exactly
    the two classes — with and without a budget."""
    _, tris, _ = T._build("standin")
    pos = R.positions(tris)
    large = X.large_mask(pos, 1 / 16)
    # the walls are large; at 16 x 16 so are the mesh's triangles near its equator, those near its poles are small
    assert 0 < large.sum() < len(pos) and large[R.wall_mask(tris)].all() and 0 < large[R.mesh_mask(tris)].sum() < R.mesh_mask(tris).sum()
    keys = np.sort(X.class_keys(pos, 1 / 16))
    n_small = int((~large).sum())
    assert not large[B.prim_order(keys)[:n_small]].any() and large[B.prim_order(keys)[n_small:]].all()
    for D in (0, 26, X.clog2(len(pos))):
        child, rng = B.radix_tree(X.bottom_up_keys(keys, D))
        l, r = (int(c) for c in child[0])
        span = lambda c: (int(rng[c, 0]), int(rng[c, 1])) if c < len(pos) - 1 else (c - (len(pos) - 1),) * 2      # noqa: E731
        if D != X.clog2(len(pos)):      # a root that is itself flattened splits on the rank instead
            assert span(l) == (0, n_small - 1) and span(r) == (n_small, len(pos) - 1), D


def _chain_tris():
    """(nodes, tris) of any 72 triangles with a light: the scene the chain positions are moved into (prim = index in `tris` order)."""
    if "chain" not in T._SCENES:
        rs = np.random.RandomState(23)
        a = rs.uniform(-8, 8, (X.CHAIN_N, 3)).astype(np.float32) + np.float32([0, 20, 0])
        b, c = a + rs.uniform(-3, 3, a.shape).astype(np.float32), a + rs.uniform(-3, 3, a.shape).astype(np.float32)
        prims = np.concatenate([make_prims(a[:70], b[:70], c[:70]), make_prims(a[70:], b[70:], c[70:], albedo=(0, 0, 0), emit=(6, 6, 6))])
        nodes, tris, _ = ptamd.build_bvh(prims)
        assert len(tris) == X.CHAIN_N and R.emissive(tris).sum() == 2
        T._SCENES["chain"] = (nodes, tris, None, X.CHAIN_CAMERA_POS)
    return T._SCENES["chain"][:2]


def _chain_moved():
    """(nodes', tris') of the chain scene at the chain positions, as the oracle takes them."""
    nodes, tris = _chain_tris()
    tris2 = R.restate_tris(tris, X.chain_positions().reshape(-1, 9))
    return R.refit_nodes(nodes, tris2), tris2


def test_chain_camera_sees_the_chain():
    """At least a tenth of the camera's pinhole rays hit the moved scene (the oracle's ray cast, on the CPU)."""
    import oracle_lib as O
    nodes2, tris2 = _chain_moved()
    W, H = T.FRAMES[0]
    _, prim, _ = O.Scene(nodes2.tobytes(), tris2).raycast(pinhole_rays(ptamd.make_camera(W, H, pos=X.CHAIN_CAMERA_POS)))
    print(f"chain scene: {np.mean(prim >= 0):.3f} of the pinhole rays hit, {len(np.unique(prim[prim >= 0]))} triangles seen")
    assert np.mean(prim >= 0) >= 0.10


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    import oracle_lib as O
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    O.set_libm(1)            # the pinned contract: correctly rounded float transcendentals
    yield


def _make(name, golden_dir):
    """(scene at its positions, positions (n, 3, 3), camera position or None); the chain scene is created elsewhere and moved."""
    if name == "chain":
        nodes, tris = _chain_tris()
        sc = ptamd.Scene(nodes, tris)
        sc.update_vertices(X.chain_positions().reshape(-1, 9))
        return sc, X.chain_positions(), X.CHAIN_CAMERA_POS
    nodes, tris, sph, cam = T._scene_data(name, golden_dir)
    return ptamd.Scene(nodes, tris, sph), R.positions(tris), cam


def _refused(call):
    with pytest.raises(ptamd.PtError) as e:
        call()
    assert f"({PT_ERR_UNSUPPORTED})" in str(e.value), str(e.value)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("cornell", "standin", "single1", "single2", "three"))
def test_zero_parameters_are_the_plain_rebuild(_gpu, golden_dir, name):
    plain, _, _ = _make(name, golden_dir)
    plain.rebuild_tree()
    ex, _, _ = _make(name, golden_dir)
    assert ex.rebuild_tree(depth_budget=0, large_fraction=0.0) == {"n_large": 0, "n_flattened_tris": 0}
    T._assert_arrays(T._arrays(ex), T._arrays(plain), f"{name}: {{0, 0}} against pt_scene_rebuild_tree")
    assert ex.tree_info() == plain.tree_info() and ex.tree_inflation() == 1.0


PINNED_SCENES = ("cornell", "standin", "standin_spheres", "three", "attribute", "needle", "chain")
PINNED_PARAMS = ((26, 1 / 16), (26, 0.0), (0, 1 / 16), ("clog2(n)", 0.0))
_YARD = {}


@pytest.mark.gpu
@pytest.mark.parametrize("D,f", PINNED_PARAMS)
@pytest.mark.parametrize("name", PINNED_SCENES)
def test_trees_are_the_pinned_build(_gpu, golden_dir, name, D, f):
    sc, pos, _ = _make(name, golden_dir)
    if D == "clog2(n)":
        D = X.clog2(len(pos)) if len(pos) >= 3 else 1
    t = X.build(pos, D, f)
    before = T._arrays(sc)
    if t["depth"] > MAX_DEPTH:
        # only without a budget: the chain scene, whose 72 triangles are all large, under (0, 1/16).  The call is refused as the plain one is.
        assert D == 0 and name == "chain"
        _refused(lambda: sc.rebuild_tree(depth_budget=D, large_fraction=f))
        T._assert_arrays(T._arrays(sc), before, f"{name}: refused")
        assert sc.tree_info()["rebuilds"] == 0
        return
    report = sc.rebuild_tree(depth_budget=D, large_fraction=f)
    a, info = T._arrays(sc), sc.tree_info()
    what = f"{name} ({D}, {f})"
    print(f"{what}: {info} {report}")
    assert report == {"n_large": t["n_large"], "n_flattened_tris": t["n_flattened_tris"]}, what
    assert np.array_equal(a["tri"].reshape(-1, 12)[:, 3].view(np.int32), t["prim"]), f"{what}: tree order"
    nrefs = a["nodes"].reshape(-1, 16)[:, 12:16].view(np.int32)
    assert nrefs.shape[0] == t["n_wide"] and np.array_equal(nrefs[:, 0:2], t["node_refs"]) and (nrefs[:, 2:4] == 0).all(), f"{what}: refs of nodes"
    qrefs = a["quad"].reshape(-1, 16)[:, 4:8].view(np.int32)
    assert qrefs.shape[0] == t["n_quad"] and np.array_equal(qrefs, t["quad_refs"]), f"{what}: refs of quad"
    assert (info["n_wide"], info["n_quad"], info["depth"], info["quad_depth"], info["rebuilds"]) == (t["n_wide"], t["n_quad"], t["depth"], t["quad_depth"], 1)
    T._assert_arrays(a, before, f"{what}: arrays a rebuild does not touch", T.KEPT)
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 10000))
    try:
        T._assert_is_a_tree(a, info, pos, what)      # tree_info against walk_depths of the arrays; walk_nodes and walk_quad
    finally:
        sys.setrecursionlimit(limit)
    if D:
        assert info["depth"] <= D and info["depth"] + 1 <= D and info["quad_depth"] <= (D - 1) // 2, what
    assert sc.tree_inflation() == 1.0


@pytest.mark.gpu
def test_chain_scene_refused_by_the_plain_call_accepted_with_a_budget(_gpu, golden_dir):
    import oracle_lib as O
    sc, pos, cam_pos = _make("chain", golden_dir)
    W, H = T.FRAMES[0]
    cam, prm = ptamd.make_camera(W, H, pos=cam_pos), T.params(passes=2, spp_per_pass=2)
    rays = np.concatenate([scene_rays8(3000, np.random.RandomState(5)), pinhole_rays(cam)[::3]]).astype(np.float32)
    hit = np.mean(sc.trace_rays(pinhole_rays(cam))[1] >= 0)
    print(f"chain scene: {hit:.3f} of the pinhole rays hit")
    assert hit >= 0.10
    before, was = T._arrays(sc), T._everything(sc, cam, prm, rays)
    _refused(sc.rebuild_tree)
    assert "depth 36" in ptamd.lib().pt_last_error().decode()
    T._assert_arrays(T._arrays(sc), before, "chain: all nine arrays after the refused rebuild")
    assert sc.tree_info()["rebuilds"] == 0
    report = sc.rebuild_tree(depth_budget=26, large_fraction=0)
    info = sc.tree_info()
    print(f"chain scene, budget 26: {info} {report}")
    assert info["depth"] <= 26 and info["quad_depth"] <= 12 and info["rebuilds"] == 1 and report == {"n_large": 0, "n_flattened_tris": 14}
    after = T._arrays(sc)
    T._assert_arrays(after, before, "chain: arrays a rebuild does not touch", T.KEPT)
    assert any(after[a].shape != before[a].shape or not np.array_equal(after[a], before[a]) for a in T.REBUILT)
    now = T._everything(sc, cam, prm, rays)
    for what in was:
        if was[what].dtype == np.float32:
            assert T._same_or_nan(now[what], was[what]), what
        else:
            assert np.array_equal(now[what], was[what]), what
    assert (was["any"] == (was["closest prim"] >= 0)).all() and np.isfinite(was["render"]).all()
    nodes2, tris2 = _chain_moved()
    ref, _ = O.Scene(nodes2.tobytes(), tris2).render(O.make_camera(W, H, pos=cam_pos), O.make_params(W, H, prm.passes, prm.spp_per_pass), 16)
    check_image(now["render"], ref, "chain: rebuilt with a budget, against the oracle")


@pytest.mark.gpu
def test_rebuilt_arrays_are_a_function_of_positions_and_parameters(_gpu):
    nodes, tris, sph = T._build("standin_spheres")
    d_pos, h_pos = T._move(tris, "rigid")
    moved = ptamd.Scene(nodes, tris, sph)
    moved.update_vertices(d_pos)
    rep = moved.rebuild_tree(depth_budget=26, large_fraction=1 / 16)
    tris2 = R.restate_tris(tris, h_pos)
    created = ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph)
    assert created.rebuild_tree(depth_budget=None, large_fraction=1 / 16) == rep and rep["n_large"] > 0      # None: the default, 26
    a = T._arrays(moved)
    T._assert_arrays(a, T._arrays(created), "moved and rebuilt against created there and rebuilt")
    held = moved.device_bytes
    assert moved.rebuild_tree(depth_budget=26) == rep      # None: the default, 1 / 16
    T._assert_arrays(T._arrays(moved), a, "a second identical call")
    assert moved.device_bytes == held and moved.tree_info()["rebuilds"] == 2 and moved.tree_inflation() == 1.0
    after_plain = ptamd.Scene(nodes, tris, sph)
    after_plain.update_vertices(d_pos)
    after_plain.rebuild_tree()
    plain = T._arrays(after_plain)
    assert any(plain[k].shape != a[k].shape or not np.array_equal(plain[k], a[k]) for k in T.REBUILT)
    assert after_plain.rebuild_tree(depth_budget=26, large_fraction=1 / 16) == rep
    T._assert_arrays(T._arrays(after_plain), a, "the new call after a plain rebuild")
    other = moved.rebuild_tree(depth_budget=X.clog2(len(tris)), large_fraction=0.0)
    assert other["n_large"] == 0 and other["n_flattened_tris"] > rep["n_flattened_tris"]


@pytest.mark.gpu
def test_what_a_rebuild_holds_follows_its_parameters(_gpu):
    """pt_scene_device_bytes after a rebuild follows the parameters of the calls a scene has seen, not the name of the entry point
    (include/pt_api.h: "Memory"): the class boxes (16,384 + 64 bytes, and the 64-bit sort's storage where it applies) with a
    large_fraction > 0, 28 bytes per raw node and the level offsets of a pass with passes > 0, and nothing else beyond the plain call."""
    nodes, tris, sph = T._build("standin_spheres")
    N = 2 * len(tris) - 1

    def rebuilt(call):
        sc = ptamd.Scene(nodes, tris, sph)
        call(sc)
        assert sc.tree_inflation() == 1.0
        return sc, sc.device_bytes

    def again(sc, call):
        held = sc.device_bytes
        call(sc)
        assert sc.device_bytes == held and sc.tree_inflation() == 1.0

    sc_plain, plain = rebuilt(lambda sc: sc.rebuild_tree())
    for D, f in ((0, 0.0), (26, 0.0)):
        assert rebuilt(lambda sc: sc.rebuild_tree(depth_budget=D, large_fraction=f))[1] == plain, (D, f)
    assert rebuilt(lambda sc: sc.rebuild_tree_optimized(passes=0, depth_budget=26, large_fraction=0.0))[1] == plain
    classes = lambda sc: sc.rebuild_tree(depth_budget=0, large_fraction=1 / 16)
    sc_classes, with_classes = rebuilt(classes)
    print(f"plain {plain}, classes + {with_classes - plain}")
    assert with_classes - plain >= 16448 and rebuilt(classes)[1] == with_classes
    passes = lambda sc: sc.rebuild_tree_optimized(passes=2, depth_budget=26, large_fraction=0.0)
    sc_passes, with_passes = rebuilt(passes)
    print(f"passes + {with_passes - plain}, 28 N = {28 * N}")
    assert 28 * N <= with_passes - plain <= 28 * N + 8192
    again(sc_plain, lambda sc: sc.rebuild_tree())
    again(sc_classes, classes)
    again(sc_passes, passes)
    again(sc_passes, lambda sc: sc.rebuild_tree())      # a plain call after an opt call


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"PTAMD_TREE": "0"}, {"PTAMD_LEAF": "4"}])
def test_rebuild_does_not_depend_on_the_build_at_upload(_gpu, monkeypatch, env):
    nodes, tris, sph = T._build("standin")
    sc = ptamd.Scene(nodes, tris, sph)
    want_report = sc.rebuild_tree(depth_budget=26, large_fraction=1 / 16)
    want = T._arrays(sc)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc = ptamd.Scene(nodes, tris, sph)
    up = T._arrays(sc)
    assert any(up[a].shape != want[a].shape or not np.array_equal(up[a], want[a]) for a in T.REBUILT)
    assert sc.rebuild_tree(depth_budget=26, large_fraction=1 / 16) == want_report
    T._assert_arrays(T._arrays(sc), want, str(env), T.REBUILT)


@pytest.mark.gpu
def test_update_rebuild_update_render(_gpu):
    """Update -> rebuild with the defaults -> update -> render is the oracle's frame of the last pose, in both modes."""
    nodes, tris, sph = T._build("standin_spheres")
    sc = ptamd.Scene(nodes, tris, sph)
    d_pos, h_pos = T._move(tris, "rigid")
    sc.update_vertices(d_pos)
    assert sc.tree_inflation() != 1.0
    sc.rebuild_tree(depth_budget=26, large_fraction=1 / 16)
    assert sc.tree_inflation() == 1.0
    tris2 = R.restate_tris(tris, h_pos)
    T._assert_renders(sc, R.refit_nodes(nodes, tris2), tris2, sph, "rigid, rebuilt with budget and classes")
    refs = T._refs_of(T._arrays(sc))
    d_pos3, h_pos3 = T._move(tris, "scale3")
    sc.update_vertices(d_pos3)
    tris3 = R.restate_tris(tris, h_pos3)
    T._assert_renders(sc, R.refit_nodes(nodes, tris3), tris3, sph, "rigid, rebuilt with budget and classes, scale3")
    a = T._arrays(sc)
    T._assert_is_a_tree(a, None, h_pos3.reshape(-1, 3, 3), "rigid, rebuilt, scale3")
    assert all(np.array_equal(x, y) for x, y in zip(T._refs_of(a), refs)), "an update changed the refs of the rebuilt trees"
    assert sc.tree_inflation() != 1.0


@pytest.mark.gpu
def test_update_rebuild_render_in_stream_order(_gpu):
    """Update, the new rebuild and a render enqueued on a side stream with no synchronisation in between from the caller."""
    import torch
    nodes, tris, sph = T._build("standin_spheres")
    W, H = T.FRAMES[1]
    cam, prm = ptamd.make_camera(W, H), T.params(rank=0, world=1)
    sc = ptamd.Scene(nodes, tris, sph)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d_pos, h_pos = T._move(tris, "rigid")
        tiles = torch.empty(ptamd.tiles_floats(cam, prm), dtype=torch.float32, device=dev)
        work = torch.empty(ptamd.work_bytes(cam, prm), dtype=torch.uint8, device=dev)
        frame = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
        report = sc.rebuild_tree(stream_ptr=st.cuda_stream, depth_budget=26, large_fraction=1 / 16)
        sc.render_tiles(cam, prm, tiles.data_ptr(), work.data_ptr(), st.cuda_stream)
        ptamd.untile(tiles.data_ptr(), cam, 1, frame.data_ptr(), st.cuda_stream)
        got = frame.cpu().numpy()
    st.synchronize()
    tris2 = R.restate_tris(tris, h_pos)
    T._assert_same(got, ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph).render(cam, prm), "stream-ordered update + rebuild with a budget + render")
    assert sc.tree_info()["rebuilds"] == 1 and report["n_large"] > 0
