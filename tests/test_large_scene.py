"""Scene edits above 65,536 triangles: pt_scene_update_materials, pt_scene_update_vertices and the three rebuild
calls on scenes where the scan of the material update runs a second round, the grid-stride reductions of the vertex update and of the
rebuild take a second trip, a level of the treelet pass holds more treelets than ro_solve has waves, and rocPRIM sorts and scans four
times what any other test hands it.  The scenes, the sets and the move are tests/large_scene_ref.py's; every yardstick and helper is
the one its feature's own test file uses (materials_ref, dynamic_ref, rebuild_ref, rebuild_budget_ref, rebuild_opt_ref; the helpers of
tests/test_materials.py and tests/test_rebuild.py).

On the CPU: the premises.  Each shows in numpy alone that the input's answer changes if the triangles at and above 65,536 are lost,
so that a GPU test which passes has run the second stride and got it right.  On the GPU: bits, no tolerance anywhere but the float64
area sum of pt_scene_tree_inflation (1e-12 relative, as tests/test_dynamic.py argues it).  Two NaNs count as equal, as in
tests/test_materials.py: the second variant of set (f) puts a NaN emittance into `surf`, where a fresh upload has one too.

One thing a vertex update cannot be held to: the four tree arrays of a FRESH upload of moved geometry.  A fresh upload builds its own
traversal trees over the moved triangles; an update refits the trees it has.  As in tests/test_dynamic.py, `nodes` and `quad` are
checked by numpy walks (every box of `nodes` IS the padded exact bound of what lies below it), `tri` and `tripair` against
dynamic_ref.tri_records, `core` against dynamic_ref.core_box, and the other four arrays against the fresh upload.  Where the move is the
identity (far_tail on sheet65536) all nine arrays are compared."""
import contextlib
import ctypes as C
import sys

import numpy as np
import pytest

import dynamic_ref as R
import large_scene_ref as L
import materials_ref as M
import ptamd
import rebuild_budget_ref as X
import rebuild_opt_ref as P
import rebuild_ref as B
import test_materials as TM
import test_rebuild as T
from scenes_util import pinhole_rays, scene_rays8

SCENES = ("standin187", "sheet65536", "sheet65537")
SIZES = {"standin187": L.STANDIN_TRIS, "sheet65536": 65536, "sheet65537": 65537}
FRAMES = ((64, 48), (100, 52))
PASSES, SPP = 2, 2
REBUILDS = ("plain", "budget", "treelets")
UNTOUCHED_BY_THE_TREES = ("surf", "lights", "leafbox", "spheres")
TREE_LIMIT = 32      # ptd::kStackDepth, as tests/test_rebuild.py's limit test reads it back


def params(**kw):
    return ptamd.default_params(**{**dict(passes=PASSES, spp_per_pass=SPP), **kw})


# ---------------------------------------------------------------------------------------------------------------------------------
# module-level caches: every scene, moved position set and yardstick is computed once
# ---------------------------------------------------------------------------------------------------------------------------------
_BUILT, _MOVED, _UPLOAD, _YARD, _ORACLE = {}, {}, {}, {}, {}


def _build(name):
    """(nodes, tris) of a scene; tris in reference order."""
    if name not in _BUILT:
        prims = ptamd.gen_scene(1, L.STANDIN_LAT_LON) if name == "standin187" else L.sheet_prims(SIZES[name])
        nodes, tris, _ = ptamd.build_bvh(prims)
        _BUILT[name] = (nodes, tris)
    return _BUILT[name]


def _moved(name, move="far_tail"):
    """(n, 3, 3) float32 positions after a move: far_tail, or tests/test_dynamic.py's `rigid` stated in numpy."""
    if (name, move) not in _MOVED:
        _, tris = _build(name)
        pos = R.positions(tris)
        if move == "far_tail":
            pos = L.far_tail(pos)
        elif move == "rigid":
            pos = R.move_translate(R.move_rigid_wobble(pos, R.mesh_mask(tris), np), R.emissive(tris), np).astype(np.float32)
        else:
            raise KeyError(move)
        _MOVED[(name, move)] = pos
    return _MOVED[(name, move)]


def _upload_of(name, pos, key, mat=None):
    """(nodes', tris') a fresh upload of the scene at pos takes, with the materials mat where given."""
    if (name, key) not in _UPLOAD:
        nodes, tris = _build(name)
        tris2 = R.restate_tris(tris if mat is None else M.apply_materials(tris, mat), pos.reshape(-1, 9))
        _UPLOAD[(name, key)] = (R.refit_nodes(nodes, tris2), tris2)
    return _UPLOAD[(name, key)]


def _yard(kind):
    """The pinned tree of a rebuild of standin187 after far_tail."""
    if kind not in _YARD:
        pos = _moved("standin187")
        _YARD[kind] = {"plain": lambda: B.build(B.sorted_keys(pos)), "budget": lambda: X.build(pos, L.DEPTH_BUDGET, L.LARGE_FRACTION),
                       "treelets": lambda: P.build(pos, L.DEPTH_BUDGET, L.LARGE_FRACTION, 1)}[kind]()
    return _YARD[kind]


def _oracle_frame(name, key, nodes2, tris2):
    """The oracle's 64 x 48 frame of a scene state at PASSES x SPP."""
    import oracle_lib as O
    if (name, key) not in _ORACLE:
        W, H = FRAMES[0]
        ref, _ = O.Scene(nodes2.tobytes(), tris2, None).render(O.make_camera(W, H), O.make_params(W, H, PASSES, SPP), 16)
        assert np.isfinite(ref).all()
        _ORACLE[(name, key)] = ref
    return _ORACLE[(name, key)]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the premises
# ---------------------------------------------------------------------------------------------------------------------------------
def test_sizes_and_block_counts():
    """Premise 4.  69,576 triangles are 272 blocks, 4,040 triangles in the second stride; the sheets are the last size with one stride
    and 256 blocks and the first with two."""
    counts = [len(_build(name)[1]) for name in SCENES]
    assert counts == [69576, 65536, 65537] == [SIZES[name] for name in SCENES]
    assert [L.blocks(n) for n in counts] == [272, 256, 257]
    assert counts[0] - L.SPLIT == 4040 and L.SPLIT == 256 * 256
    for name in SCENES:      # both size classes, two lights, and triangles small enough for a core box
        _, tris = _build(name)
        pos = R.positions(tris)
        large = X.large_mask(pos, L.LARGE_FRACTION)
        assert 2 <= large.sum() <= 16 and M.lights_of(tris).sum() == 2, name
        assert np.isfinite(R.core_box(tris, pos)).all(), name
    for name in SCENES[1:]:      # the sheets: the quad's two triangles are the large class and the lights, and are counted in the total
        _, tris = _build(name)
        assert np.array_equal(X.large_mask(R.positions(tris), L.LARGE_FRACTION), M.lights_of(tris)), name


def test_material_sets_have_lights_on_both_sides_of_the_split():
    """Premise 1.  A scan that loses its second round, or its carry, changes the light count, the slots of the lights at and above 65,536,
    or the emittance flag; one that drops the flag of an earlier round reports "f head" as ok."""
    for name in ("standin187", "sheet65537"):
        _, tris = _build(name)
        n = len(tris)
        sets = dict(L.material_sets(tris))
        assert list(sets) == ["a", "b", "c", "d", "e", "f 2e8", "f nan", "f head"]
        lit = M.is_light(sets["b"])
        assert lit[:L.SPLIT].any() and lit[L.SPLIT:].any(), name
        assert 0 < lit[:L.SPLIT].sum() < lit.sum(), name
        # ... and more than a block's worth of partial sums reach the second round with a carry that is not zero
        if name == "standin187":
            per_block = np.add.reduceat(lit.astype(np.int64), np.arange(0, n, 256))
            assert len(per_block) == 272 and (per_block[256:] > 0).all() and per_block[:256].sum() > 10000
        only = np.flatnonzero(M.is_light(sets["c"]))
        assert only.tolist() == [n - 1] and n - 1 >= L.SPLIT, name
        assert not M.is_light(sets["d"]).any(), name
        bad = L.bad_triangle(n)
        assert bad >= L.SPLIT, name
        for label, light in (("f 2e8", True), ("f nan", False)):
            mat = sets[label]
            assert M.emittance_ok(L.without_tail(mat)) and not M.emittance_ok(mat), (name, label)
            assert bool(M.is_light(mat)[bad]) == light, (name, label)
            want = M.lights_of(tris).copy()
            want[bad] = light
            assert np.array_equal(M.is_light(mat), want), (name, label)
        # ... and the other way round: the first round's flag is down, the second round's rows are all fine.  A scan that kept only
        # its last round's flag would report the scene ok.
        mat = sets["f head"]
        assert L.HEAD_TRIANGLE < L.SPLIT and not M.lights_of(tris)[L.HEAD_TRIANGLE], name
        assert not M.emittance_ok(L.without_tail(mat)) and M.emittance_ok(mat[L.SPLIT:]) and not M.emittance_ok(mat), name
        assert M.is_light(mat).sum() == 3 and M.is_light(mat)[L.HEAD_TRIANGLE], name
    # the sheet with one stride: the spoiled triangle is its last, the last thread of block 255
    _, tris = _build("sheet65536")
    assert L.bad_triangle(len(tris)) == 65535 and not M.emittance_ok(L.set_f(tris, 2e8)) and M.emittance_ok(L.set_f(tris, 2e8)[:-1])


def _boxes_differ(a, b):
    return not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))


def test_far_tail_changes_what_every_reduction_returns():
    """Premise 2.  The core box, the centroid box, both class boxes and the count of large triangles of the moved scene all differ from
    what the triangles below 65,536 alone give."""
    _, tris = _build("standin187")
    before, pos = R.positions(tris), _moved("standin187")
    n = len(pos)
    head = np.arange(n) < L.SPLIT
    assert np.array_equal(pos[head], before[head]) and (pos[~head, :, 0].min() > before[:, :, 0].max())      # clear of the scene's box
    core, core_head = R.core_box(tris, pos), R.core_box(L.without_tail(tris), L.without_tail(pos))
    assert not np.array_equal(core, core_head) and core[3] > core_head[3] + 100.0
    c = B.centroids(pos)
    assert _boxes_differ((c.min(0), c.max(0)), (c[head].min(0), c[head].max(0)))
    small_box, large_box = L.class_boxes(pos)
    small_head, large_head = L.class_boxes(pos, keep=head)
    assert _boxes_differ(small_box, small_head) and _boxes_differ(large_box, large_head)
    large = X.large_mask(pos, L.LARGE_FRACTION)
    assert large[head].sum() >= 1 and large[~head].sum() >= 1 and large[L.tail_picks(n)].all() and len(L.tail_picks(n)) == 3
    assert (~large[~head]).sum() >= 1000
    assert large.sum() != X.large_mask(pos[head], L.LARGE_FRACTION).sum()
    # the sheet with one triangle in the second stride: that triangle alone moves the core box; the other sheet stays where it is
    _, st = _build("sheet65537")
    sp = _moved("sheet65537")
    assert not np.array_equal(R.core_box(st, sp), R.core_box(L.without_tail(st), L.without_tail(sp)))
    assert not np.array_equal(R.core_box(st, sp), R.core_box(st, R.positions(st)))
    assert np.array_equal(_moved("sheet65536"), R.positions(_build("sheet65536")[1]))


def test_plain_tree_of_the_moved_scene_is_within_the_kernels_limits():
    """pt_scene_rebuild_tree takes no budget and refuses a tree deeper than the stacks: far_tail's distance is chosen so that it need not."""
    t = _yard("plain")
    md, mq = C.c_int32(0), C.c_int32(0)
    assert ptamd.lib().pt_dbg_tree_limits(t["depth"], t["quad_depth"], C.byref(md), C.byref(mq)) == 0
    assert t["depth"] <= md.value == TREE_LIMIT and t["quad_depth"] <= mq.value


def test_a_level_of_the_treelet_pass_has_more_treelets_than_the_grid():
    """Premise 3.  ro_solve runs 4,096 waves per height: the interior nodes of one height of the tree the pass starts from (the budget
    rebuild's), and of the tree it leaves, from the yardsticks' own level tables."""
    start, end = _yard("budget"), _yard("treelets")
    for t in (start, end):
        per_height = np.diff(t["level_start"])      # height 0: the leaves
        assert per_height[1:].max() > 4096, per_height[:8]
        assert per_height[1:].sum() == t["n_wide"]
    assert np.diff(start["level_start"])[1] > 2 * 4096      # a third treelet for some waves
    assert end["n_roots"] > 4096 and 0 < end["n_restructured"] < end["n_roots"]
    assert end["n_large"] == start["n_large"] >= 4 and end["n_flattened_tris"] == start["n_flattened_tris"]


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


def _device(a, per):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1, per)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_material_arrays_after_each_set(_gpu, name):
    """Test 5.  One scene through the device entry point, a second through the host one: after every set the nine arrays, the light
    count and the pruning flag are a fresh upload's and each other's; the lights are materials_ref.light_records.  The flag is 0 after
    each of the three variants of (f) — the bad emittance in the scan's second round, or in its first with a clean second — and 1 again
    after the good set that follows."""
    nodes, tris = _build(name)
    names = "abcdef" if name == "standin187" else "bcf"
    sets = L.material_sets(tris, names=names)
    sets.append(sets[0])      # after (f), a good set again — (a), or (b) on the sheets: the flag comes back
    dev_sc, host_sc = ptamd.Scene(nodes, tris), ptamd.Scene(nodes, tris)
    pos = R.positions(tris)
    counts = {}
    for label, mat in sets:
        dev_sc.update_materials(_device(mat, 12))
        host_sc.update_materials(mat)
        tris2 = R.restate_tris(M.apply_materials(tris, mat), pos)
        got, want = TM._state(dev_sc), TM._state(ptamd.Scene(nodes, tris2))
        what = f"{name} ({label})"
        TM._assert_state(got, want, what + " against a fresh upload")
        TM._assert_state(TM._state(host_sc), got, what + " host against device entry point")
        TM._assert_same(got["lights"].reshape(-1, 16), M.light_records(tris2), what + " light records from numpy")
        TM._assert_same(got["surf"].reshape(-1, 48)[:, 36:48], mat, what + " surface floats 36..47")
        assert int(got["num_lights"]) == int(M.is_light(mat).sum()), what
        assert int(got["nee_prune"]) == (0 if label.startswith("f") else 1) == int(M.emittance_ok(mat)), what
        counts[label] = int(got["num_lights"])
        print(f"{what}: {counts[label]} lights, nee_prune {int(got['nee_prune'])}")
    assert counts["c"] == 1 and counts["b"] > 0.2 * len(tris)
    assert counts["f 2e8"] == 3 and counts["f nan"] == 2 and counts["f head"] == 3
    if name == "standin187":
        assert counts["d"] == 0 and counts["a"] == counts["e"] == 2


def _results(sc):
    """Tests 6 and 8: two frames, 3,000 closest-hit rays with their surface records, and next-event estimation at their hit points."""
    out = {}
    for W, H in FRAMES:
        out[f"render {W}x{H}"] = sc.render(ptamd.make_camera(W, H), params())
    t, prim, surf = sc.trace_rays(scene_rays8(3000, np.random.RandomState(11)), surface=True)
    out["trace t"], out["trace prim"], out["trace surface"] = t, prim, surf
    pts = surf[prim >= 0][:, 5:8]
    seeds = np.random.RandomState(12).randint(0, 2**32, (pts.shape[0], 2), dtype=np.uint64).astype(np.uint32)
    out["nee in"] = np.concatenate([pts, seeds.view(np.float32)], 1)
    out["nee"] = sc.nee(out["nee in"])
    return out


def _assert_results(sc, fresh, oracle_frame, what):
    got, want = _results(sc), _results(fresh)
    for k in want:
        TM._assert_same(got[k], want[k], f"{what}: {k} against a fresh upload")
    assert (got["trace prim"] >= 0).mean() > 0.7 and len(got["nee in"]) == (got["trace prim"] >= 0).sum() > 2100
    TM._assert_same(got["render 64x48"], oracle_frame, f"{what}: 64 x 48 against the oracle")
    return got


@pytest.mark.gpu
def test_material_results_after_set_b(_gpu):
    """Test 6.  20,766 lights, 1,224 of them past the first round of the scan: a light's slot decides which one NEE samples."""
    nodes, tris = _build("standin187")
    mat = M.set_b(tris, L.SEED)
    sc = ptamd.Scene(nodes, tris)
    before = sc.render(ptamd.make_camera(*FRAMES[0]), params())
    sc.update_materials(_device(mat, 12))
    tris2 = R.restate_tris(M.apply_materials(tris, mat), R.positions(tris))
    got = _assert_results(sc, ptamd.Scene(nodes, tris2), _oracle_frame("standin187", "b", nodes, tris2), "standin187 (b)")
    assert not TM._same(got["render 64x48"], before).all()      # the new lights are visible
    assert (got["nee"][:, 8:11].sum(1) > 0).sum() > 100


VERTEX_CASES = (("standin187", "far_tail"), ("standin187", "rigid"), ("sheet65536", "far_tail"), ("sheet65537", "far_tail"))
_UPDATED = {}


def _updated(name, move):
    """(arrays, tree_inflation) of a scene after one vertex update, shared by the tests that only read them."""
    if (name, move) not in _UPDATED:
        nodes, tris = _build(name)
        sc = ptamd.Scene(nodes, tris)
        sc.update_vertices(_device(_moved(name, move), 9))
        _UPDATED[(name, move)] = (T._arrays(sc), sc.tree_inflation())
    return _UPDATED[(name, move)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,move", VERTEX_CASES)
def test_vertex_update_arrays(_gpu, name, move):
    """Test 7, the arrays: the records against a fresh upload of the moved geometry and against numpy, the core box against
    dynamic_ref.core_box, the refs of both trees as they were."""
    nodes, tris = _build(name)
    pos = _moved(name, move)
    what = f"{name} {move}"
    got, _ = _updated(name, move)
    nodes2, tris2 = _upload_of(name, pos, move)
    fresh, never = T._arrays(ptamd.Scene(nodes2, tris2)), T._arrays(ptamd.Scene(nodes, tris))
    identity = np.array_equal(pos, R.positions(tris))
    assert identity == (name == "sheet65536")
    T._assert_arrays(got, fresh, what + " against a fresh upload", T.ARRAYS if identity else UNTOUCHED_BY_THE_TREES)
    assert np.array_equal(T.bits(got["leafbox"].reshape(-1, 8)), T.bits(R.leaf_boxes(nodes2)))
    tri = got["tri"].reshape(-1, 12)
    prim, leaf = tri[:, 3].view(np.int32), tri[:, 7].view(np.int32)
    assert np.array_equal(np.sort(prim), np.arange(len(tris)))
    want_tri, want_pair = R.tri_records(tris2, nodes2, prim, leaf)
    T._assert_arrays(got, {"tri": want_tri.ravel(), "tripair": want_pair.ravel()}, what + " records from numpy", ("tri", "tripair"))
    assert all(np.array_equal(x, y) for x, y in zip(T._refs_of(got), T._refs_of(never))), what + ": an update changed the refs"
    want_core = R.core_box(tris, pos)
    assert never["core"].size == 6 and np.array_equal(got["core"], want_core), (what, got["core"], want_core)
    assert np.array_equal(R.core_box(tris, R.positions(tris)), never["core"])      # the rule is the upload's
    if identity:
        T._assert_arrays(got, never, what + " against the scene never updated")
    else:
        assert not np.array_equal(got["core"], never["core"]) and not np.array_equal(T.bits(got["surf"]), T.bits(never["surf"]))
        if move == "far_tail":      # what the first stride alone would have given
            assert not np.array_equal(got["core"], R.core_box(L.without_tail(tris), L.without_tail(pos)))


@contextlib.contextmanager
def _deep_recursion():
    """The numpy walks recurse once per level of a tree; room for that, and the limit as it was afterwards."""
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 10000))
    try:
        yield
    finally:
        sys.setrecursionlimit(limit)


def _walk_nodes(arrays, pos, what):
    with _deep_recursion():
        bad, seen, boxes = R.walk_nodes(arrays["nodes"], arrays["tri"], pos)
    assert not bad, (what, "nodes: boxes that are not the padded exact bounds", bad[:5])
    assert (seen == 1).all(), (what, "nodes: triangles not reached exactly once")
    return boxes


_UPLOADED_BOXES = {}


def _uploaded_boxes(name):
    """The exact boxes of the binary tree of a scene never updated: the denominator of the inflation ratio."""
    if name not in _UPLOADED_BOXES:
        nodes, tris = _build(name)
        _UPLOADED_BOXES[name] = _walk_nodes(T._arrays(ptamd.Scene(nodes, tris)), R.positions(tris), f"{name} as uploaded")
    return _UPLOADED_BOXES[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name,move", VERTEX_CASES)
def test_vertex_update_binary_tree_and_inflation(_gpu, name, move):
    """Test 7, the binary tree: every box of `nodes` after the move is the padded exact bound of the triangles below it — `rigid` changes
    every box of the mesh, level by level — and pt_scene_tree_inflation, dyn_area's block partials (one per 1,024 builder nodes) summed
    on the host, is numpy's ratio (1e-12: the order of a float64 sum)."""
    what = f"{name} {move}"
    got, inflation = _updated(name, move)
    boxes, ref_boxes = _walk_nodes(got, _moved(name, move), what), _uploaded_boxes(name)
    assert len(boxes) == len(ref_boxes) > 65536
    want = R.area_sum(boxes) / R.area_sum(ref_boxes)
    print(f"{what}: tree inflation {inflation:.9f}, numpy {want:.9f}")
    assert abs(inflation - want) <= 1e-12 * want, (what, inflation, want)
    if name == "sheet65536":      # the identity
        assert inflation == 1.0 == want
    else:
        assert inflation != 1.0 and (move != "far_tail" or inflation > 1.0), (what, inflation)
        moved_boxes = sum(not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])) for a, b in zip(boxes, ref_boxes))
        print(f"{what}: {moved_boxes} of {len(boxes)} boxes differ from the uploaded ones")
        if move == "rigid":
            assert moved_boxes > 0.9 * len(boxes), (what, moved_boxes)


@pytest.mark.gpu
@pytest.mark.parametrize("name,move", VERTEX_CASES)
def test_vertex_update_quad_tree(_gpu, name, move):
    """Test 7, the 4-wide tree after the move: every quantised child box contains the padded bound below it, every scale is a power of two."""
    got, _ = _updated(name, move)
    with _deep_recursion():
        qbad, qseen, scales_ok = R.walk_quad(got["quad"], got["tri"], _moved(name, move))
    assert not qbad, (name, move, "quad: boxes that do not contain the padded bounds", qbad[:5])
    assert (qseen == 1).all() and scales_ok, (name, move)


def _moved_scene():
    """standin187 after far_tail, its upload (nodes', tris') and the moved positions."""
    nodes, tris = _build("standin187")
    pos = _moved("standin187")
    sc = ptamd.Scene(nodes, tris)
    sc.update_vertices(_device(pos, 9))
    nodes2, tris2 = _upload_of("standin187", pos, "far_tail")
    return sc, nodes2, tris2, pos


@pytest.mark.gpu
def test_vertex_update_results_after_far_tail(_gpu):
    """Test 8."""
    sc, nodes2, tris2, _ = _moved_scene()
    still = ptamd.Scene(*_build("standin187")).render(ptamd.make_camera(*FRAMES[0]), params())
    got = _assert_results(sc, ptamd.Scene(nodes2, tris2), _oracle_frame("standin187", "far_tail", nodes2, tris2), "standin187 far_tail")
    assert not TM._same(got["render 64x48"], still).all()      # the move is visible


def _rebuild(sc, kind):
    if kind == "plain":
        sc.rebuild_tree()
        return {}
    if kind == "budget":
        return sc.rebuild_tree(depth_budget=L.DEPTH_BUDGET, large_fraction=L.LARGE_FRACTION)
    return sc.rebuild_tree_optimized(passes=1, depth_budget=L.DEPTH_BUDGET, large_fraction=L.LARGE_FRACTION)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", REBUILDS)
def test_rebuilt_trees_are_the_pinned_build(_gpu, kind):
    """Test 9.  The tree order and the refs of both trees are the yardstick's: a wrong centroid or class box moves Morton cells, a wrong
    sort or scan moves everything, a treelet left out leaves its nodes where the budget rebuild put them."""
    sc, _, _, pos = _moved_scene()
    t = _yard(kind)
    before = T._arrays(sc)
    report = _rebuild(sc, kind)
    a, info = T._arrays(sc), sc.tree_info()
    what = f"standin187 far_tail, {kind}"
    print(f"{what}: {info} {report}")
    assert report == {k: t[k] for k in ("n_large", "n_flattened_tris", "n_roots", "n_restructured") if k in report}, what
    assert len(report) == {"plain": 0, "budget": 2, "treelets": 4}[kind]
    assert np.array_equal(a["tri"].reshape(-1, 12)[:, 3].view(np.int32), t["prim"]), f"{what}: tree order"
    nrefs = a["nodes"].reshape(-1, 16)[:, 12:16].view(np.int32)
    assert nrefs.shape[0] == t["n_wide"] and np.array_equal(nrefs[:, 0:2], t["node_refs"]) and (nrefs[:, 2:4] == 0).all(), f"{what}: refs of nodes"
    qrefs = a["quad"].reshape(-1, 16)[:, 4:8].view(np.int32)
    assert qrefs.shape[0] == t["n_quad"] and np.array_equal(qrefs, t["quad_refs"]), f"{what}: refs of quad"
    assert (info["n_wide"], info["n_quad"], info["depth"], info["quad_depth"], info["rebuilds"]) == (t["n_wide"], t["n_quad"], t["depth"], t["quad_depth"], 1)
    T._assert_arrays(a, before, f"{what}: arrays a rebuild does not touch", T.KEPT)
    assert sc.tree_inflation() == 1.0
    if kind != "plain":
        assert info["depth"] <= L.DEPTH_BUDGET - 1 and info["quad_depth"] <= (L.DEPTH_BUDGET - 1) // 2, what
    if kind == "treelets":
        got = P.nodes_area(a["nodes"])
        assert got == t["nodes_area"], (what, got, t["nodes_area"])
        assert t["n_restructured"] > 0 and t["area_after"] < t["area_before"]
    if kind == "plain":
        with _deep_recursion():
            T._assert_is_a_tree(a, info, pos, what)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", REBUILDS)
def test_rebuilds_keep_every_result(_gpu, kind):
    """Test 10."""
    sc, nodes2, tris2, _ = _moved_scene()
    W, H = FRAMES[0]
    cam, prm = ptamd.make_camera(W, H), params()
    rays = np.concatenate([scene_rays8(3000, np.random.RandomState(5)), pinhole_rays(cam)[::3]]).astype(np.float32)
    before, was = T._arrays(sc), T._everything(sc, cam, prm, rays)
    _rebuild(sc, kind)
    after = T._arrays(sc)
    T._assert_arrays(after, before, f"{kind}: arrays a rebuild does not touch", T.KEPT)
    assert any(after[a].shape != before[a].shape or not np.array_equal(after[a], before[a]) for a in T.REBUILT)
    assert sc.tree_info()["rebuilds"] == 1 and sc.tree_inflation() == 1.0
    now = T._everything(sc, cam, prm, rays)
    for what in was:
        if was[what].dtype == np.float32:
            assert T._same_or_nan(now[what], was[what]), (kind, what)
        else:
            assert np.array_equal(now[what], was[what]), (kind, what)
    assert (was["any"] == (was["closest prim"] >= 0)).all() and np.isfinite(was["render"]).all()
    TM._assert_same(now["render"], _oracle_frame("standin187", "far_tail", nodes2, tris2), f"{kind}: rebuilt, against the oracle")


@pytest.mark.gpu
def test_materials_move_rebuild_move_render_in_stream_order(_gpu):
    """Test 11.  Materials (b), far_tail, the rebuild with a budget, `rigid` and a render enqueued on a side stream; the caller waits for
    nothing but what the calls themselves wait for.  The frame and the arrays are a fresh upload's of the final state."""
    import torch
    nodes, tris = _build("standin187")
    mat = M.set_b(tris, L.SEED)
    final = _moved("standin187", "rigid")
    W, H = FRAMES[1]
    cam, prm = ptamd.make_camera(W, H), params(rank=0, world=1)
    sc = ptamd.Scene(nodes, tris)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    src = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (mat, _moved("standin187").reshape(-1, 9), final.reshape(-1, 9))]
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        d_mat, d_far, d_rigid = (torch.zeros_like(a).add_(a) for a in src)      # filled on the side stream, with no wait after
        tiles = torch.empty(ptamd.tiles_floats(cam, prm), dtype=torch.float32, device=dev)
        work = torch.empty(ptamd.work_bytes(cam, prm), dtype=torch.uint8, device=dev)
        frame = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        sc.update_materials(d_mat, stream_ptr=st.cuda_stream)
        sc.update_vertices(d_far, stream_ptr=st.cuda_stream)
        report = sc.rebuild_tree(stream_ptr=st.cuda_stream, depth_budget=L.DEPTH_BUDGET, large_fraction=L.LARGE_FRACTION)
        sc.update_vertices(d_rigid, stream_ptr=st.cuda_stream)
        sc.render_tiles(cam, prm, tiles.data_ptr(), work.data_ptr(), st.cuda_stream)
        ptamd.untile(tiles.data_ptr(), cam, 1, frame.data_ptr(), st.cuda_stream)
        got = frame.cpu().numpy()
    st.synchronize()
    t = _yard("budget")
    assert report == {"n_large": t["n_large"], "n_flattened_tris": t["n_flattened_tris"]} and sc.tree_info()["rebuilds"] == 1
    nodes2, tris2 = _upload_of("standin187", final, "b, rigid", mat)
    fresh = ptamd.Scene(nodes2, tris2)
    TM._assert_same(got, fresh.render(cam, prm), "stream-ordered materials + far_tail + rebuild + rigid + render")
    a = TM._state(sc)
    TM._assert_state(a, TM._state(fresh), "the final state against a fresh upload", UNTOUCHED_BY_THE_TREES)
    TM._assert_same(a["lights"].reshape(-1, 16), M.light_records(tris2), "light records from numpy")
    tri = a["tri"].reshape(-1, 12)
    prim, leaf = tri[:, 3].view(np.int32), tri[:, 7].view(np.int32)
    assert np.array_equal(prim, t["prim"])      # the rebuilt order, refitted
    want_tri, want_pair = R.tri_records(tris2, nodes2, prim, leaf)
    T._assert_arrays(a, {"tri": want_tri.ravel(), "tripair": want_pair.ravel()}, "records from numpy", ("tri", "tripair"))
    assert np.array_equal(a["core"], R.core_box(tris, final)) and sc.tree_inflation() != 1.0
