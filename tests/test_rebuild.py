"""Rebuilding the traversal trees of an uploaded scene on the GPU (pt_scene_rebuild_tree, pt_scene_tree_info; include/pt_api.h: "Tree
rebuild").  On the CPU: the C-ABI surface, the argument checks, the limit check as a host function, and the numpy yardstick
(tests/rebuild_ref.py) on hand-made inputs.  On the GPU, on the small scenes the suite already uses: a rebuild changes no result
(bits), the rebuilt trees are trees (numpy walks of the downloaded arrays), they are the pinned linear BVH of rebuild_ref, they are a
function of the positions alone, and every later update works on them.  Bits everywhere; the two exceptions are stated where they are
used: the float64 area sum of pt_scene_tree_inflation (1e-12, as tests/test_dynamic.py) and the oracle frames of the attribute and
needle scenes, which are compared by the bar of their own test files (scenes_util.check_image)."""
import ctypes as C
import os

import numpy as np
import pytest

import dynamic_ref as R
import ptamd
import rebuild_ref as B
from scenes_util import NEEDLE_CAMERA_POS, NEEDLE_SEED, check_image, load_ref_attr, make_prims, needle_scene, pinhole_rays, scene_rays8
from scenes_util import test_spheres as make_test_spheres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pt_scene_rebuild_tree", "pt_scene_tree_info", "pt_dbg_tree_limits")
REBUILT = ("nodes", "quad", "tri", "tripair")
KEPT = ("leafbox", "surf", "lights", "spheres", "core")
SCENES = ("cornell", "standin", "standin_spheres", "single1", "single2", "three", "attribute", "needle")
# the small frames, sample counts and scene arrays of tests/test_dynamic.py
FRAMES = ((64, 48), (100, 52))
PASSES, SPP = 3, 4
ARRAYS = REBUILT + KEPT
PT_ERR_UNSUPPORTED = -5      # include/pt_api.h: PtStatus


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def params(**kw):
    return ptamd.default_params(**{**dict(passes=PASSES, spp_per_pass=SPP), **kw})


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
    assert "typedef struct PtTreeInfo { int32_t n_wide, n_quad, depth, quad_depth, rebuilds; } PtTreeInfo;" in hdr
    assert callable(ptamd.Scene.rebuild_tree) and callable(ptamd.Scene.tree_info)
    assert [f for f, _ in ptamd.PtTreeInfo._fields_] == ["n_wide", "n_quad", "depth", "quad_depth", "rebuilds"]
    assert "a rebuild on the GPU" not in hdr      # no longer out of scope


def test_null_arguments_are_rejected_before_any_device_call():
    """A fake scene address: never dereferenced, and no HIP call is made, when an argument is NULL."""
    l = ptamd.lib()
    scene = C.c_void_p(1 << 40)
    info = ptamd.PtTreeInfo()
    for what, call in [("rebuild_tree: NULL scene", lambda: l.pt_scene_rebuild_tree(None, None)),
                       ("tree_info: NULL scene", lambda: l.pt_scene_tree_info(None, C.byref(info))),
                       ("tree_info: NULL out", lambda: l.pt_scene_tree_info(scene, None))]:
        assert call() == -1, what
        assert what.split(":")[0] in l.pt_last_error().decode(), (what, l.pt_last_error())


def test_limit_check_refuses_a_tree_that_is_too_deep():
    """The check pt_scene_rebuild_tree applies to the depths it reads back (and pt_scene_create to the host build's), fed depths: no GPU
    test builds a scene that breaks a kernel limit."""
    l = ptamd.lib()
    md, mq = C.c_int32(0), C.c_int32(0)
    assert l.pt_dbg_tree_limits(0, 0, C.byref(md), C.byref(mq)) == 0
    # ptd::kStackDepth = 32; wf_trace's stack holds 16 + 48 = 64 entries (csrc/pt_wavefront.hip) and a walk needs 3 * depth + 2: (64 - 2) // 3
    assert md.value == 32 and mq.value == 20
    assert l.pt_dbg_tree_limits(32, mq.value, None, None) == 0
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    assert f"PT_ERR_UNSUPPORTED = {PT_ERR_UNSUPPORTED} " in hdr
    assert l.pt_dbg_tree_limits(33, 0, None, None) == PT_ERR_UNSUPPORTED and "depth 33" in l.pt_last_error().decode()
    assert l.pt_dbg_tree_limits(0, mq.value + 1, None, None) == PT_ERR_UNSUPPORTED and "4-wide" in l.pt_last_error().decode()
    assert l.pt_dbg_tree_limits(33, mq.value + 1, None, None) == PT_ERR_UNSUPPORTED


def _tris_at(centres, size=0.25):
    """(n, 3, 3) float32: a small triangle around every centre whose box centre is the centre itself (exactly: powers of two)."""
    c = np.asarray(centres, np.float32).reshape(-1, 1, 3)
    return (c + np.float32(size) * np.float32([[-1, -1, -1], [1, -1, 1], [-1, 1, 1]])[None]).astype(np.float32)


def _check_ref_is_a_tree(t, n):
    """Every triangle under exactly one leaf, reached once from the root, in both of rebuild_ref's trees."""
    for refs, what in ((t["node_refs"], "nodes"), (t["quad_refs"], "quad")):
        seen, stack, visited = np.zeros(n, int), [0], set()
        while stack:
            i = stack.pop()
            assert i not in visited, what
            visited.add(i)
            for ref in refs[i]:
                ref = int(ref)
                if ref >= 0:
                    stack.append(ref)
                elif ref != -1:
                    seen[(~ref) >> 3:((~ref) >> 3) + ((~ref) & 7)] += 1
        assert (seen == 1).all() and len(visited) == len(refs), what


def test_yardstick_three_triangles():
    """The smallest tree with an interior node: a leaf of two and a leaf of one."""
    pos = _tris_at([[0, 0, 0], [8, 8, 8], [1, 0, 0]])
    keys = B.sorted_keys(pos)
    assert list(B.prim_order(keys)) == [0, 2, 1]                                 # x is the most significant axis of every bit triple
    assert [int(k) >> 32 for k in keys] == [0, 1 << 23, (1 << 30) - 1]      # q = (0,0,0), (128,0,0), (1023,1023,1023)
    t = B.build(keys)
    assert (t["n_bn"], t["n_wide"], t["n_quad"], t["depth"], t["quad_depth"]) == (3, 1, 1, 1, 0)
    assert t["node_refs"].tolist() == [[~((0 << 3) | 2), ~((2 << 3) | 1)]]
    assert t["quad_refs"].tolist() == [[~((0 << 3) | 2), ~((2 << 3) | 1), -1, -1]]
    assert t["bn"].tolist() == [[1, 2, 0, 0], [-1, -1, 0, 2], [-1, -1, 2, 1]] and t["quad_bn"].tolist() == [[1, 2, -1, -1]]
    assert list(t["order"]) == [1, 2, 0] and t["level_start"] == [0, 2, 3]
    _check_ref_is_a_tree(t, 3)


def test_yardstick_coincident_centroids():
    """64 triangles with one centroid: every Morton code is equal, the tree comes from the prim bits."""
    pos = _tris_at(np.tile(np.float32([[3, 4, 5]]), (64, 1)), size=np.float32(2.0) ** -np.arange(64).reshape(-1, 1, 1))
    assert np.unique(B.centroids(pos), axis=0).shape == (1, 3)
    keys = B.sorted_keys(pos)
    assert list(keys) == list(range(64))
    child, rng = B.radix_tree(keys)
    depth = {0: 0}
    for v in sorted(range(63), key=lambda v: rng[v, 1] - rng[v, 0], reverse=True):      # parents before children
        for c in child[v]:
            depth[int(c)] = depth[v] + 1
    assert max(depth.values()) == 6 and all(depth[63 + j] == 6 for j in range(64))      # the radix tree of 6 prim bits is balanced
    t = B.build(keys)
    # 32 leaves of two at depth 5 under 31 interior nodes; 4-wide nodes at depths 0, 2, 4: 1 + 4 + 16
    assert (t["n_bn"], t["n_wide"], t["n_quad"], t["depth"], t["quad_depth"]) == (63, 31, 21, 5, 2)
    assert t["level_start"] == [0, 32, 48, 56, 60, 62, 63]
    # numbered breadth-first: the root and its four children are full; the 16 below hold two leaves of two and two free slots each
    assert (t["quad_refs"][:5] >= 0).all() and (t["quad_refs"][5:, :2] < -1).all() and (t["quad_refs"][5:, 2:] == -1).all()
    _check_ref_is_a_tree(t, 64)


def test_yardstick_flat_scene():
    """Centroids that share one coordinate: an axis of extent 0 quantises to 0 and takes no part."""
    rs = np.random.RandomState(3)
    c = rs.uniform(-5, 5, (40, 3)).astype(np.float32)
    c[:, 1] = 2.5
    pos = _tris_at(c)
    q = B.quantise(B.centroids(pos))
    assert (q[:, 1] == 0).all() and q[:, 0].max() == 1023 and q[:, 2].max() == 1023 and q.min() == 0
    m = B.morton30(q)
    assert (m & np.uint64(0x12492492)).max() == 0      # the y bits (3k + 1)
    keys = B.sorted_keys(pos)
    assert sorted(B.prim_order(keys)) == list(range(40))
    t = B.build(keys)
    assert t["n_bn"] == 2 * t["n_wide"] + 1
    _check_ref_is_a_tree(t, 40)
    # a degenerate box in all three axes is the coincident case; two triangles are the single-leaf scene
    one = B.build(B.sorted_keys(_tris_at([[1, 1, 1], [1, 1, 1]])))
    assert one["node_refs"].tolist() == [[~2, -1]] and one["quad_refs"].tolist() == [[~2, -1, -1, -1]] and one["level_start"] == [0, 1]


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


_BUILT = {}


def _build(name):
    """(nodes, tris, spheres) of cornell / standin / standin_spheres, as tests/test_dynamic.py builds them."""
    if name not in _BUILT:
        prims = ptamd.gen_scene(0, 187) if name == "cornell" else ptamd.gen_scene(1, 16)
        nodes, tris, _ = ptamd.build_bvh(prims)
        _BUILT[name] = (nodes, tris, make_test_spheres() if name == "standin_spheres" else None)
    return _BUILT[name]


def _move(tris, move, device="cuda:0"):
    """The `rigid` and `scale3` moves of tests/test_dynamic.py, made with torch on the device: (tensor (n, 9) there, the same as numpy)."""
    import torch
    pos = torch.from_numpy(R.positions(tris)).to(device)
    sel = lambda m: torch.from_numpy(m).to(device)      # noqa: E731
    if move == "rigid":
        pos = R.move_rigid_wobble(pos, sel(R.mesh_mask(tris)), torch)
        pos = R.move_translate(pos, sel(R.emissive(tris)), torch)
    elif move == "scale3":
        pos = R.move_scale(pos, sel(R.mesh_mask(tris)), torch, 3.0)
    else:
        raise KeyError(move)
    pos = pos.reshape(-1, 9).contiguous()
    assert pos.dtype == torch.float32
    return pos, pos.cpu().numpy()


def _arrays(sc):
    return {a: sc.dbg_array(a) for a in ARRAYS}


def _assert_arrays(got, want, what, names=ARRAYS):
    for a in names:
        assert got[a].shape == want[a].shape, (what, a)
        if want[a].dtype == np.float32:
            g, w = got[a], want[a]
            same = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
        else:
            same = got[a] == want[a]
        assert same.all(), (what, a, np.argwhere(~same)[:5].ravel())


def _assert_same(got, want, what):
    same = (bits(got) == bits(want))
    print(f"{what}: bit-identical floats {same.mean():.6f}")
    assert got.shape == want.shape and same.all(), what


def _oracle(nodes, tris, sph):
    import oracle_lib as O
    return O.Scene(nodes.tobytes(), tris, sph)


def _oracle_render(so, W, H, prm):
    import oracle_lib as O
    ref, _ = so.render(O.make_camera(W, H), O.make_params(W, H, prm.passes, prm.spp_per_pass, first_pass=prm.first_pass), 16)
    return ref


_SCENES = {}


def _scene_data(name, golden_dir):
    """(nodes, tris, spheres, camera position or None)."""
    if name not in _SCENES:
        cam = None
        if name in ("cornell", "standin", "standin_spheres"):
            nodes, tris, sph = _build(name)
        elif name == "attribute":
            g, prims, _, _, _ = load_ref_attr(golden_dir)
            nodes, tris, _ = ptamd.build_bvh(prims)
            sph = g["spheres"]
        elif name == "needle":
            nodes, tris, _ = ptamd.build_bvh(needle_scene(NEEDLE_SEED)[0])      # the scene of tests/test_needle_scene.py
            sph, cam = None, NEEDLE_CAMERA_POS
        else:
            a = np.float32([[-6, 12, -3], [-6, 12, -3], [-9, 2, 4]])
            b = np.float32([[6, 12, -3], [6, 24, -3], [-3, 2, 4]])
            c = np.float32([[6, 24, -3], [-6, 24, -3], [-6, 7, 2]])
            k = {"single1": 1, "single2": 2, "three": 3}[name]
            nodes, tris, _ = ptamd.build_bvh(make_prims(a[:k], b[:k], c[:k], emit=(5, 5, 5)))
            assert len(tris) == k
            sph = None
        _SCENES[name] = (nodes, tris, sph, cam)
    return _SCENES[name]


def _camera(W, H, pos):
    return ptamd.make_camera(W, H) if pos is None else ptamd.make_camera(W, H, pos=pos)


def _same_or_nan(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and ((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all()


def _everything(sc, cam, prm, rays):
    """What a rebuild must leave bit for bit as it was."""
    out = {}
    sc.set_mode(1)
    out["render"] = sc.render(cam, prm)
    sc.set_mode(0)
    sc.enable_counters(True)
    out["mode 0"] = sc.render(cam, prm)
    sc.enable_counters(False)
    sc.set_mode(1)
    out["aov"], out["aov prim"] = sc.aov(cam, prm)
    out["raycast"], out["raycast prim"] = sc.raycast(rays)
    out["closest t"], out["closest prim"], out["closest surface"] = sc.trace_rays(rays, surface=True)
    out["any"] = sc.trace_rays(rays, any_hit=True)[1] >= 0
    out["render_rays"] = sc.render_rays(pinhole_rays(cam), prm)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_rebuild_of_an_untouched_scene_changes_nothing(_gpu, golden_dir, name):
    nodes, tris, sph, cam_pos = _scene_data(name, golden_dir)
    sc = ptamd.Scene(nodes, tris, sph)
    W, H = FRAMES[0]
    cam, prm = _camera(W, H, cam_pos), params(passes=2, spp_per_pass=2)
    rays = np.concatenate([scene_rays8(3000, np.random.RandomState(5)), pinhole_rays(cam)[::3]]).astype(np.float32)
    assert sc.tree_info()["rebuilds"] == 0
    before, was = _arrays(sc), _everything(sc, cam, prm, rays)
    sc.rebuild_tree()
    after = _arrays(sc)
    _assert_arrays(after, before, f"{name}: arrays a rebuild does not touch", KEPT)
    tri0, tri1 = before["tri"].reshape(-1, 12), after["tri"].reshape(-1, 12)
    o0, o1 = np.argsort(tri0[:, 3].view(np.int32), kind="stable"), np.argsort(tri1[:, 3].view(np.int32), kind="stable")
    assert np.array_equal(tri1[o1][:, 3].view(np.int32), np.arange(len(tris)))
    assert np.array_equal(bits(tri1[o1]), bits(tri0[o0])), f"{name}: tri is not a permutation of its records"
    assert sc.tree_inflation() == 1.0 and sc.tree_info()["rebuilds"] == 1
    now = _everything(sc, cam, prm, rays)
    for what in was:
        if was[what].dtype == np.float32:
            assert _same_or_nan(now[what], was[what]), (name, what)
        else:
            assert np.array_equal(now[what], was[what]), (name, what)
    assert (was["any"] == (was["closest prim"] >= 0)).all() and np.isfinite(was["render"]).all()
    if name in ("attribute", "needle"):      # ... and the frame is the oracle's, by the bar of the scene's own test file
        import oracle_lib as O
        so = O.Scene(nodes.tobytes(), tris, sph)
        ocam = O.make_camera(W, H) if cam_pos is None else O.make_camera(W, H, pos=cam_pos)
        ref, _ = so.render(ocam, O.make_params(W, H, prm.passes, prm.spp_per_pass), 16)
        check_image(now["render"], ref, f"{name}: rebuilt, against the oracle")


_REBUILT = {}


def _rebuilt(name, golden_dir):
    """(arrays, tree_info, positions (n, 3, 3)) of a scene created and rebuilt, shared by the tests that only read them."""
    if name not in _REBUILT:
        nodes, tris, sph, _ = _scene_data(name, golden_dir)
        sc = ptamd.Scene(nodes, tris, sph)
        sc.rebuild_tree()
        _REBUILT[name] = (_arrays(sc), sc.tree_info(), R.positions(tris))
    return _REBUILT[name]


def _assert_is_a_tree(a, info, pos, what):
    bad, seen, boxes = R.walk_nodes(a["nodes"], a["tri"], pos)
    assert not bad, (what, "nodes: boxes that are not the padded exact bounds", bad[:5])
    assert (seen == 1).all(), (what, "nodes: triangles not reached exactly once")
    qbad, qseen, scales_ok = R.walk_quad(a["quad"], a["tri"], pos)
    assert not qbad, (what, "quad: boxes that do not contain the padded bounds", qbad[:5])
    assert (qseen == 1).all() and scales_ok, what
    if info is not None:
        depth, quad_depth = B.walk_depths(a["nodes"], a["quad"])
        assert (info["n_wide"], info["n_quad"]) == (a["nodes"].size // 16, a["quad"].size // 16), what
        assert (info["depth"], info["quad_depth"]) == (depth, quad_depth), (what, info, depth, quad_depth)
        md, mq = C.c_int32(0), C.c_int32(0)
        assert ptamd.lib().pt_dbg_tree_limits(depth, quad_depth, C.byref(md), C.byref(mq)) == 0 and depth <= md.value and quad_depth <= mq.value
        print(f"{what}: {info}")
    return boxes


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_rebuilt_trees_are_trees(_gpu, golden_dir, name):
    import sys
    a, info, pos = _rebuilt(name, golden_dir)
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 10000))
    try:
        _assert_is_a_tree(a, info, pos, name)
    finally:
        sys.setrecursionlimit(limit)
    assert info["rebuilds"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_rebuilt_trees_are_the_pinned_build(_gpu, golden_dir, name):
    a, info, pos = _rebuilt(name, golden_dir)
    t = B.build(B.sorted_keys(pos))
    assert np.array_equal(a["tri"].reshape(-1, 12)[:, 3].view(np.int32), t["prim"]), f"{name}: tree order"
    nrefs = a["nodes"].reshape(-1, 16)[:, 12:16].view(np.int32)
    assert nrefs.shape[0] == t["n_wide"] and np.array_equal(nrefs[:, 0:2], t["node_refs"]) and (nrefs[:, 2:4] == 0).all(), f"{name}: refs of nodes"
    qrefs = a["quad"].reshape(-1, 16)[:, 4:8].view(np.int32)
    assert qrefs.shape[0] == t["n_quad"] and np.array_equal(qrefs, t["quad_refs"]), f"{name}: refs of quad"
    assert (info["n_wide"], info["n_quad"], info["depth"], info["quad_depth"]) == (t["n_wide"], t["n_quad"], t["depth"], t["quad_depth"])


def _with_materials(tris, mat):
    t = tris.copy()
    for o in (R.T_MAT0, R.T_MAT0 + 12, R.T_MAT0 + 24):
        t[:, o:o + 12] = mat
    return t


def _refs_of(a):
    """The child refs of `nodes` and `quad`, as integers."""
    return a["nodes"].reshape(-1, 16)[:, 12:16].view(np.uint32).copy(), a["quad"].reshape(-1, 16)[:, 4:8].copy()


def _assert_renders(sc, nodes2, tris2, sph, what, oracle=True):
    fresh = ptamd.Scene(nodes2, tris2, sph)
    W, H = FRAMES[0]
    cam, prm = ptamd.make_camera(W, H), params()
    ref = _oracle_render(_oracle(nodes2, tris2, sph), W, H, prm) if oracle else None
    for mode in (1, 0):
        sc.set_mode(mode)
        fresh.set_mode(mode)
        got = sc.render(cam, prm)
        _assert_same(got, fresh.render(cam, prm), f"{what}, mode {mode}, against a fresh upload")
        if oracle:
            _assert_same(got, ref, f"{what}, mode {mode}, against the oracle")
    sc.set_mode(1)


@pytest.mark.gpu
@pytest.mark.parametrize("move,then", [("rigid", "scale3"), ("scale3", "rigid")])
def test_update_rebuild_update(_gpu, move, then):
    name = "standin_spheres"
    nodes, tris, sph = _build(name)
    sc = ptamd.Scene(nodes, tris, sph)
    d_pos, h_pos = _move(tris, move)
    sc.update_vertices(d_pos)
    assert sc.tree_inflation() != 1.0
    sc.rebuild_tree()
    assert sc.tree_inflation() == 1.0
    tris2 = R.restate_tris(tris, h_pos)
    _assert_renders(sc, R.refit_nodes(nodes, tris2), tris2, sph, f"{move}, rebuilt")
    a = _arrays(sc)
    boxes1 = _assert_is_a_tree(a, sc.tree_info(), h_pos.reshape(-1, 3, 3), f"{move}, rebuilt")
    refs = _refs_of(a)
    # a second, different update refits the NEW trees
    d_pos3, h_pos3 = _move(tris, then)
    sc.update_vertices(d_pos3)
    tris3 = R.restate_tris(tris, h_pos3)
    nodes3 = R.refit_nodes(nodes, tris3)
    _assert_renders(sc, nodes3, tris3, sph, f"{move}, rebuilt, {then}")
    a = _arrays(sc)
    boxes3 = _assert_is_a_tree(a, None, h_pos3.reshape(-1, 3, 3), f"{move}, rebuilt, {then}")
    assert all(np.array_equal(x, y) for x, y in zip(_refs_of(a), refs)), "an update changed the refs of the rebuilt trees"
    # float64 summation order is the device reduction's, not numpy's: 1e-12 relative, as tests/test_dynamic.py argues
    want, got = R.area_sum(boxes3) / R.area_sum(boxes1), sc.tree_inflation()
    print(f"{move} -> rebuild -> {then}: tree inflation {got:.6f}")
    assert len(boxes3) == len(boxes1) and abs(got - want) <= 1e-12 * want and got != 1.0, (got, want)
    # a light off, another on
    mat = tris3[:, R.T_MAT0:R.T_MAT0 + 12].copy()
    lights = np.nonzero(R.emissive(tris3))[0]
    mesh = np.nonzero(R.mesh_mask(tris3))[0]
    mat[lights[0], 0:3] = 0.0
    mat[mesh[7], 0:3] = (9.0, 7.0, 5.0)
    sc.update_materials(mat)
    assert sc.num_lights == len(lights)
    _assert_renders(sc, nodes3, _with_materials(tris3, mat), sph, f"{move}, rebuilt, {then}, materials", oracle=False)


@pytest.mark.gpu
def test_rebuilt_arrays_are_a_function_of_the_positions(_gpu):
    name, move = "standin_spheres", "rigid"
    nodes, tris, sph = _build(name)
    moved = ptamd.Scene(nodes, tris, sph)
    d_pos, h_pos = _move(tris, move)
    moved.update_vertices(d_pos)
    moved.rebuild_tree()
    tris2 = R.restate_tris(tris, h_pos)
    created = ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph)
    created.rebuild_tree()
    a, b = _arrays(moved), _arrays(created)
    _assert_arrays(a, b, "moved and rebuilt against created there and rebuilt")
    held = moved.device_bytes
    moved.rebuild_tree()
    _assert_arrays(_arrays(moved), a, "a second rebuild")
    assert moved.device_bytes == held and moved.tree_info()["rebuilds"] == 2 and moved.tree_inflation() == 1.0
    assert held > ptamd.Scene(nodes, tris, sph).device_bytes


@pytest.mark.gpu
def test_update_rebuild_render_in_stream_order(_gpu):
    """Update, rebuild and render enqueued on a non-default stream with no synchronisation in between from the caller."""
    import torch
    nodes, tris, sph = _build("standin_spheres")
    W, H = FRAMES[1]
    cam, prm = ptamd.make_camera(W, H), params(rank=0, world=1)
    sc = ptamd.Scene(nodes, tris, sph)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d_pos, h_pos = _move(tris, "rigid")
        tiles = torch.empty(ptamd.tiles_floats(cam, prm), dtype=torch.float32, device=dev)
        work = torch.empty(ptamd.work_bytes(cam, prm), dtype=torch.uint8, device=dev)
        frame = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
        sc.rebuild_tree(stream_ptr=st.cuda_stream)
        sc.render_tiles(cam, prm, tiles.data_ptr(), work.data_ptr(), st.cuda_stream)
        ptamd.untile(tiles.data_ptr(), cam, 1, frame.data_ptr(), st.cuda_stream)
        got = frame.cpu().numpy()
    st.synchronize()
    tris2 = R.restate_tris(tris, h_pos)
    _assert_same(got, ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph).render(cam, prm), "stream-ordered update + rebuild + render")
    assert sc.tree_info()["rebuilds"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"PTAMD_TREE": "0"}, {"PTAMD_LEAF": "4"}])
def test_rebuild_does_not_depend_on_the_build_at_upload(_gpu, golden_dir, monkeypatch, env):
    want, _, _ = _rebuilt("standin", golden_dir)      # under the default build
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nodes, tris, sph = _build("standin")
    sc = ptamd.Scene(nodes, tris, sph)
    up = _arrays(sc)
    assert any(up[a].shape != want[a].shape or not np.array_equal(up[a], want[a]) for a in REBUILT)
    sc.rebuild_tree()
    _assert_arrays(_arrays(sc), want, str(env), REBUILT)
