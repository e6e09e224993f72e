"""The tree rebuild with treelet restructuring (pt_scene_rebuild_tree_opt; include/pt_api.h: "Tree rebuild with treelet restructuring";
DESIGN.md section 25).  On the CPU: the C-ABI surface, the parameter checks, and the numpy yardstick (tests/rebuild_opt_ref.py: the pass
stated independently of the device code, its dynamic programme stated three times).  On the GPU, with the small frames, sample counts
and helpers of tests/test_rebuild.py and tests/test_rebuild_budget.py: passes = 0 is pt_scene_rebuild_tree_ex byte for byte; the trees
are the yardstick's, are trees, keep the budget and have the yardstick's interior area; every result keeps its bits; the rebuilt arrays
are a function of the positions and the parameters; later updates work on the new trees.  Bits everywhere; the one exception is the
oracle frame of the chain scene, compared by scenes_util.check_image as tests/test_rebuild_budget.py compares it."""
import ctypes as C
import inspect
import itertools
import os
import sys

import numpy as np
import pytest

import dynamic_ref as R
import ptamd
import rebuild_budget_ref as X
import rebuild_opt_ref as P
import rebuild_ref as B
import test_rebuild as T
import test_rebuild_budget as TB
from scenes_util import check_image, pinhole_rays, scene_rays8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pt_rebuild_opt_passes_default", "pt_scene_rebuild_tree_opt")
PT_ERR_INVALID = -1
F = np.float32


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
    assert "typedef struct PtRebuildOptReport { int32_t n_large, n_flattened_tris, n_roots, n_restructured; } PtRebuildOptReport;" in hdr
    assert [(f, t) for f, t in ptamd.PtRebuildOptReport._fields_] == [(f, C.c_int32) for f in ("n_large", "n_flattened_tris", "n_roots", "n_restructured")]
    assert C.sizeof(ptamd.PtRebuildOptReport) == 16
    assert ptamd.lib().pt_rebuild_opt_passes_default() == P.DEFAULT_PASSES == 2
    assert list(inspect.signature(ptamd.Scene.rebuild_tree_optimized).parameters) == ["self", "passes", "depth_budget", "large_fraction", "stream_ptr"]
    assert list(inspect.signature(ptamd.Scene.rebuild_tree).parameters) == ["self", "stream_ptr", "depth_budget", "large_fraction"]


def test_bad_parameters_are_rejected_before_any_device_call():
    """A fake scene address: never dereferenced, and no HIP call is made, when a parameter is bad."""
    l = ptamd.lib()
    scene = C.c_void_p(1 << 40)
    rep = ptamd.PtRebuildOptReport(-3, -3, -3, -3)
    ok = ptamd.PtRebuildParams(26, 0.0625)
    cases = [("NULL scene", None, ok, 2), ("NULL params", scene, None, 2)]
    for d, f in ((-1, 0.0), (33, 0.0), (1 << 30, 0.0), (26, -0.5), (26, float("nan")), (26, float("inf")), (26, float("-inf")), (0, -1e-30)):
        cases.append((f"depth_budget {d}, large_fraction {f}", scene, ptamd.PtRebuildParams(d, f), 2))
    for passes in (-1, 9, P.MAX_PASSES + 1, 1 << 30, -(1 << 31)):
        cases.append((f"passes {passes}", scene, ok, passes))
    for what, s, p, passes in cases:
        assert l.pt_scene_rebuild_tree_opt(s, C.byref(p) if p is not None else None, passes, C.byref(rep), None) == PT_ERR_INVALID, what
        assert "pt_scene_rebuild_tree_opt" in l.pt_last_error().decode(), (what, l.pt_last_error())
        assert (rep.n_large, rep.n_flattened_tris, rep.n_roots, rep.n_restructured) == (-3, -3, -3, -3), what


def _grids():
    """The chain scene and two grids of 216 triangles: regular, and jittered with triangles of mixed size."""
    rs = np.random.RandomState(41)
    g = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    yield "chain", X.chain_positions()
    yield "grid", X.tris_at((2.0 * g).astype(F), 0.5)
    c = (3.0 * g + rs.uniform(-1.2, 1.2, g.shape)).astype(F)
    size = (F(2.0) ** rs.randint(-3, 2, (len(c), 1, 1))).astype(F)
    yield "jittered", (c.reshape(-1, 1, 3) + size * F([[-1, -1, -1], [1, -1, 1], [-1, 1, 1]])[None]).astype(F)


def _leaf_refs(t):
    return sorted(int(r) for r in t["node_refs"].ravel() if r < 0)


def test_zero_passes_give_the_extended_rebuild():
    for name, pos in _grids():
        for D, f in ((26, 1 / 16), (0, 0.0), (8, 0.0)):
            t, want = P.build(pos, D, f, 0), X.build(pos, D, f)
            assert (t["n_roots"], t["n_restructured"]) == (0, 0) and t["area_after"] == t["area_before"]
            for k in want:
                assert np.array_equal(t[k], want[k]), (name, D, f, k)


def test_yardstick_trees_are_trees_with_less_area():
    any_done = False
    for name, pos in _grids():
        for D, f in ((26, 1 / 16), (26, 0.0), (0, 0.0)):
            if D == 0 and name == "chain":
                continue      # the plain tree over the chain scene is 36 deep: no budget, no rebuild
            base = X.build(pos, D, f)
            was, trace = None, []
            for passes in (1, 2, 3):
                t = P.build(pos, D, f, passes)
                what = (name, D, f, passes)
                T._check_ref_is_a_tree(t, len(pos))
                assert np.array_equal(t["prim"], base["prim"]) and _leaf_refs(t) == _leaf_refs(base), what
                assert (t["n_large"], t["n_flattened_tris"], t["n_wide"], t["n_bn"]) == (base["n_large"], base["n_flattened_tris"], base["n_wide"], base["n_bn"]), what
                assert 0 <= t["n_restructured"] <= t["n_roots"] <= passes * t["n_wide"], what
                if t["n_restructured"] > 0:
                    assert t["area_after"] < t["area_before"], what
                    any_done = True
                else:
                    assert t["area_after"] == t["area_before"] and np.array_equal(t["node_refs"], base["node_refs"]), what
                assert t["depth"] <= (D - 1 if D else base["depth"]), what
                assert was is None or t["area_after"] <= was, what      # a pass accepts only what is cheaper
                was = t["area_after"]
                trace.append(t["area_after"] / t["area_before"])
            print(f"{name} ({D}, {f}): area sum after 1, 2, 3 passes / before: " + ", ".join(f"{x:.4f}" for x in trace))
    assert any_done


def test_depth_budget_survives_the_passes_on_the_chain_scene():
    pos = X.chain_positions()
    for D in (26, 12, 8):
        base = X.build(pos, D, 0.0)
        for passes in (1, 2):
            t = P.build(pos, D, 0.0, passes)
            assert t["depth"] <= D - 1 and t["quad_depth"] <= (D - 1) // 2, (D, passes, t["depth"])
            T._check_ref_is_a_tree(t, 72)
        if D == 8:
            assert base["depth"] == 7      # the budget binds: the tree is as deep as it may be before the first pass


def _all_trees(leaves):
    """Every binary topology over the tuple of leaves, as nested pairs (each unordered pair once)."""
    if len(leaves) == 1:
        yield leaves[0]
        return
    first, rest = leaves[0], leaves[1:]
    for k in range(len(rest)):
        for with_first in itertools.combinations(rest, k):
            other = tuple(x for x in rest if x not in with_first)
            for a in _all_trees((first,) + with_first):
                for b in _all_trees(other):
                    yield (a, b)


def test_dynamic_programme_against_enumeration():
    """Step 3 a third time: every topology over up to 5 entries is enumerated and its internal boxes summed.  Integer coordinates below
    64 make every area an integer below 2^15 and every sum exact, so the comparison is of bits whatever the order of the additions."""
    rs = np.random.RandomState(7)
    counts = {3: 3, 4: 15, 5: 105}
    for m in (3, 4, 5):
        assert sum(1 for _ in _all_trees(tuple(range(m)))) == counts[m]
        for _ in range(20):
            lo = rs.randint(0, 32, (m, 3)).astype(F)
            hi = lo + rs.randint(0, 32, (m, 3)).astype(F)

            def cost(tree, root=True):
                """(leaf set, summed area of the internal nodes below the root)"""
                if not isinstance(tree, tuple):
                    return [tree], 0.0
                la, ca = cost(tree[0], False)
                lb, cb = cost(tree[1], False)
                both = la + lb
                own = 0.0 if root else float(P.area(lo[both].min(0), hi[both].max(0)))
                return both, ca + cb + own

            best = min(cost(t)[1] for t in _all_trees(tuple(range(m))))
            c_full, part = P.solve_one(lo, hi, m)
            assert float(c_full) == best, (m, lo, hi)
            a, c, parts, h = P.solve(lo[None], hi[None], np.zeros((1, m), np.int64), m)
            assert float(c[0, -1]) == best and list(parts[0]) == list(part)
    # and the two statements of the yardstick agree on float boxes, ties included (coincident boxes)
    for m in (3, 5, 7):
        for _ in range(5):
            lo = rs.uniform(-5, 5, (m, 3)).astype(F)
            hi = lo + rs.uniform(0, 3, (m, 3)).astype(F)
            lo[1], hi[1] = lo[0], hi[0]
            c_full, part = P.solve_one(lo, hi, m)
            a, c, parts, h = P.solve(lo[None], hi[None], np.zeros((1, m), np.int64), m)
            assert c[0, -1].view(np.uint32) == F(c_full).view(np.uint32) and list(parts[0]) == list(part)


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


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("cornell", "standin", "three", "single1", "single2"))
def test_zero_passes_are_the_extended_rebuild(_gpu, golden_dir, name):
    ex, _, _ = TB._make(name, golden_dir)
    want = ex.rebuild_tree(depth_budget=26, large_fraction=1 / 16)
    opt, _, _ = TB._make(name, golden_dir)
    assert opt.rebuild_tree_optimized(passes=0, depth_budget=26, large_fraction=1 / 16) == {**want, "n_roots": 0, "n_restructured": 0}
    T._assert_arrays(T._arrays(opt), T._arrays(ex), f"{name}: passes = 0 against pt_scene_rebuild_tree_ex")
    assert opt.tree_info() == ex.tree_info() and opt.tree_inflation() == 1.0
    if name in ("single1", "single2"):      # the single-leaf path ignores passes
        two, _, _ = TB._make(name, golden_dir)
        assert two.rebuild_tree_optimized(passes=2, depth_budget=26, large_fraction=1 / 16) == {**want, "n_roots": 0, "n_restructured": 0}
        T._assert_arrays(T._arrays(two), T._arrays(ex), f"{name}: passes = 2 on a single leaf")
        assert two.tree_info() == ex.tree_info() and two.tree_inflation() == 1.0


PINNED_SCENES = ("cornell", "three", "standin", "standin_spheres", "attribute", "chain", "needle")
PINNED_PARAMS = ((26, 1 / 16), (26, 0.0), ("tight", 0.0))
_YARD, _PLAIN_AREA = {}, {}


def _tight(n):
    """8 where a tree over n triangles can be that shallow (it binds on the chain scene), else one level above the balanced tree."""
    return max(8, X.clog2(n) + 1)


def _yard(name, pos, D, f, passes):
    key = (name, D, f, passes)
    if key not in _YARD:
        _YARD[key] = P.build(pos, D, f, passes)
    return _YARD[key]


# the needle scene (16,386 triangles) runs with one pass only, to keep the numpy side short
PINNED_CASES = [(name, D, f, passes) for name in PINNED_SCENES for D, f in PINNED_PARAMS for passes in (1, 2) if not (name == "needle" and passes == 2)]
# without a budget the limit of step 4 is the depth of the tree a pass starts from, and the launches cover heights 1 .. 63
PINNED_CASES += [("standin", 0, 1 / 16, 2), ("attribute", 0, 0.0, 1), ("three", 0, 0.0, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,D,f,passes", PINNED_CASES)
def test_trees_are_the_pinned_build(_gpu, golden_dir, name, D, f, passes):
    sc, pos, _ = TB._make(name, golden_dir)
    if D == "tight":
        D = _tight(len(pos))
    t = _yard(name, pos, D, f, passes)
    before = T._arrays(sc)
    report = sc.rebuild_tree_optimized(passes=passes, depth_budget=D, large_fraction=f)
    a, info = T._arrays(sc), sc.tree_info()
    what = f"{name} ({D}, {f}) x {passes}"
    print(f"{what}: {info} {report}; area sum {t['area_after'] / max(t['area_before'], 1e-300):.4f} of the unoptimised tree's")
    assert report == {k: t[k] for k in ("n_large", "n_flattened_tris", "n_roots", "n_restructured")}, what
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
        T._assert_is_a_tree(a, info, pos, what)
    finally:
        sys.setrecursionlimit(limit)
    if D:
        assert info["depth"] <= D - 1 and info["quad_depth"] <= (D - 1) // 2, what
    else:      # no deeper than it was
        assert info["depth"] <= X.build(pos, 0, f)["depth"], what
    assert sc.tree_inflation() == 1.0
    # the area the pass is about, from the boxes the render reads
    got = P.nodes_area(a["nodes"])
    assert got == t["nodes_area"], (what, got, t["nodes_area"])
    if (name, D, f) not in _PLAIN_AREA:
        plain, _, _ = TB._make(name, golden_dir)
        plain.rebuild_tree_optimized(passes=0, depth_budget=D, large_fraction=f)
        _PLAIN_AREA[(name, D, f)] = P.nodes_area(T._arrays(plain)["nodes"])
    if t["n_restructured"] > 0:
        # The pass guarantees a strictly lower sum for the EXACT boxes (the yardstick's figures, which the equality above ties to the
        # device's tree).  `nodes` holds them padded by 2^-16 of each coordinate, which moves a sum by a few 2^-16 of itself: the
        # inequality between the padded sums is the issue's check and holds while a pass gains more than that, as it does here.
        assert t["area_after"] < t["area_before"], what
        assert got < _PLAIN_AREA[(name, D, f)], (what, got, _PLAIN_AREA[(name, D, f)])
    else:      # nothing was cheaper: the tree is pt_scene_rebuild_tree_ex's
        assert got == _PLAIN_AREA[(name, D, f)], what


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("standin", "attribute", "needle", "chain"))
def test_results_keep_their_bits(_gpu, golden_dir, name):
    sc, pos, cam_pos = TB._make(name, golden_dir)
    W, H = T.FRAMES[0]
    cam, prm = T._camera(W, H, cam_pos), T.params(passes=2, spp_per_pass=2)
    rays = np.concatenate([scene_rays8(3000, np.random.RandomState(5)), pinhole_rays(cam)[::3]]).astype(np.float32)
    before, was = T._arrays(sc), T._everything(sc, cam, prm, rays)
    report = sc.rebuild_tree_optimized(passes=2, depth_budget=26, large_fraction=1 / 16)
    print(f"{name}: {sc.tree_info()} {report}")
    after = T._arrays(sc)
    T._assert_arrays(after, before, f"{name}: arrays a rebuild does not touch", T.KEPT)
    assert any(after[a].shape != before[a].shape or not np.array_equal(after[a], before[a]) for a in T.REBUILT)
    assert sc.tree_info()["rebuilds"] == 1 and sc.tree_inflation() == 1.0
    now = T._everything(sc, cam, prm, rays)
    for what in was:
        if was[what].dtype == np.float32:
            assert T._same_or_nan(now[what], was[what]), (name, what)
        else:
            assert np.array_equal(now[what], was[what]), (name, what)
    assert (was["any"] == (was["closest prim"] >= 0)).all() and np.isfinite(was["render"]).all()
    if name == "chain":
        import oracle_lib as O
        nodes2, tris2 = TB._chain_moved()
        ref, _ = O.Scene(nodes2.tobytes(), tris2).render(O.make_camera(W, H, pos=cam_pos), O.make_params(W, H, prm.passes, prm.spp_per_pass), 16)
        check_image(now["render"], ref, "chain: rebuilt with two passes, against the oracle")


@pytest.mark.gpu
def test_rebuilt_arrays_are_a_function_of_positions_and_parameters(_gpu):
    nodes, tris, sph = T._build("standin_spheres")
    d_pos, h_pos = T._move(tris, "rigid")
    moved = ptamd.Scene(nodes, tris, sph)
    moved.update_vertices(d_pos)
    rep = moved.rebuild_tree_optimized(passes=2, depth_budget=26, large_fraction=1 / 16)
    assert rep["n_restructured"] > 0
    tris2 = R.restate_tris(tris, h_pos)
    created = ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph)
    assert created.rebuild_tree_optimized() == rep      # None: the defaults, 2 passes and (26, 1 / 16)
    a = T._arrays(moved)
    T._assert_arrays(a, T._arrays(created), "moved and rebuilt against created there and rebuilt")
    held = moved.device_bytes
    assert moved.rebuild_tree_optimized(passes=2) == rep
    T._assert_arrays(T._arrays(moved), a, "a second identical call")
    assert moved.device_bytes == held and moved.tree_info()["rebuilds"] == 2 and moved.tree_inflation() == 1.0
    # the older calls allocate nothing of the new call's: 28 bytes per raw node and the words
    older = ptamd.Scene(nodes, tris, sph)
    older.update_vertices(d_pos)
    older.rebuild_tree(depth_budget=26, large_fraction=1 / 16)
    assert 28 * (2 * len(tris) - 1) <= held - older.device_bytes <= 28 * (2 * len(tris) - 1) + 8192
    ex = T._arrays(older)
    assert any(ex[k].shape != a[k].shape or not np.array_equal(ex[k], a[k]) for k in T.REBUILT)
    assert older.rebuild_tree_optimized(passes=2) == rep
    T._assert_arrays(T._arrays(older), a, "the new call after an extended rebuild")
    one = moved.rebuild_tree_optimized(passes=1)
    assert one["n_roots"] < rep["n_roots"] and 0 < one["n_restructured"] < rep["n_restructured"]


@pytest.mark.gpu
def test_update_rebuild_update_render(_gpu):
    """Update -> optimised rebuild -> update -> render is the oracle's frame of the last pose, in both modes."""
    nodes, tris, sph = T._build("standin_spheres")
    sc = ptamd.Scene(nodes, tris, sph)
    d_pos, h_pos = T._move(tris, "rigid")
    sc.update_vertices(d_pos)
    assert sc.tree_inflation() != 1.0
    sc.rebuild_tree_optimized()
    assert sc.tree_inflation() == 1.0
    tris2 = R.restate_tris(tris, h_pos)
    T._assert_renders(sc, R.refit_nodes(nodes, tris2), tris2, sph, "rigid, rebuilt with two passes")
    refs = T._refs_of(T._arrays(sc))
    d_pos3, h_pos3 = T._move(tris, "scale3")
    sc.update_vertices(d_pos3)
    tris3 = R.restate_tris(tris, h_pos3)
    T._assert_renders(sc, R.refit_nodes(nodes, tris3), tris3, sph, "rigid, rebuilt with two passes, scale3")
    a = T._arrays(sc)
    T._assert_is_a_tree(a, None, h_pos3.reshape(-1, 3, 3), "rigid, rebuilt, scale3")
    assert all(np.array_equal(x, y) for x, y in zip(T._refs_of(a), refs)), "an update changed the refs of the rebuilt trees"
    assert sc.tree_inflation() != 1.0


@pytest.mark.gpu
def test_update_rebuild_render_in_stream_order(_gpu):
    """Update, the optimised rebuild and a render enqueued on a side stream with no synchronisation in between from the caller."""
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
        report = sc.rebuild_tree_optimized(stream_ptr=st.cuda_stream)
        sc.render_tiles(cam, prm, tiles.data_ptr(), work.data_ptr(), st.cuda_stream)
        ptamd.untile(tiles.data_ptr(), cam, 1, frame.data_ptr(), st.cuda_stream)
        got = frame.cpu().numpy()
    st.synchronize()
    tris2 = R.restate_tris(tris, h_pos)
    T._assert_same(got, ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph).render(cam, prm), "stream-ordered update + optimised rebuild + render")
    assert sc.tree_info()["rebuilds"] == 1 and report["n_restructured"] > 0
