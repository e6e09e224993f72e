"""Trees 27 to 32 levels deep on every GPU walk.  include/pt_api.h promises that every entry point keeps its bits
on any tree the limit check accepts, and that the ray queries and the render's drain "walk the 4-wide tree only up to level 12 and the
binary tree beyond".  Three accepted trees, built by the GPU rebuild over about 100 triangles (tests/deep_tree_ref.py,
tests/rebuild_budget_ref.py):

    comb32    the comb scene under pt_scene_rebuild_tree:          binary depth 32 (the limit), 4-wide depth 15
    chain28   the chain scene under pt_scene_rebuild_tree_ex (28, 0):           27,                          13 (the first past the cut at 12)
    chain32   the chain scene under pt_scene_rebuild_tree_ex (32, 0):           31,                          15

and one refused: the comb's sibling with one level more, 33 deep.  With 3 * quad_depth + 2 > 40 the render's tail runs in
wf_drain<false> and pt_trace_rays in its binary fallback, both on trace_closest, whose 32-entry stack the comb fills to 31; wf_trace walks
the 4-wide tree with up to 48 of its 16 + 48 stack entries.

On the CPU: the premises — the depths, the limit check, which walk is taken, and the stack figures of the numpy walkers — before any
device call.  On the GPU, with the helpers of tests/test_rebuild.py (64 x 48, 2 passes x 2 spp): every result of the shallow host-built
tree is kept bit for bit by the deep one; closest hits and NEE rows are the oracle's in every bit; the frame passes
scenes_util.check_image against the oracle, the bar the chain scene already uses; every schedule gives the same bits; the overflow of
wf_trace's stack is seen in the device's own histogram and survives time slicing; the 33-deep tree is refused with nothing changed;
vertex updates and the treelet passes work on the 32-deep tree."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import deep_tree_ref as Dp
import dynamic_ref as R
import oracle_lib as O
import ptamd
import rebuild_budget_ref as X
import rebuild_opt_ref as P
import rebuild_ref as B
import test_rebuild as T
import test_rebuild_budget as TB
from scenes_util import check_image, make_prims, pinhole_rays, scene_rays8
from test_query import _assert_any, _assert_closest, same_bits_or_nan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, PASSES, SPP = 64, 48, 2, 2
STREAMS = W * H * PASSES
MAX_DEPTH, MAX_QUAD_DEPTH = 32, 20      # pt_dbg_tree_limits, as tests/test_rebuild.py reads them back
DRAIN_QUAD_STACK, TRACE_STACK = 40, 64      # csrc/pt_wavefront.hip: kDrainQuadStack (pt_query.hip: kQueryStack), kWfLdsStack + kWfOvfLevels
# name: scene, depth budget (None: the plain call), (depth, quad_depth), nodes with two interior children on the longest such path
TREES = {"comb32": ("comb", None, (32, 15), 31),
         "chain28": ("chain", 28, (27, 13), 5),
         "chain32": ("chain", 32, (31, 15), 5)}
# The share of the 4-wide walk's node steps that leave 31 or more entries on the stack, for the comb camera's 3072 pinhole rays, by the
# CPU walker (deep_tree_ref.quad_walks): 0.2896.  The device's own histogram must show half of it (the issue's bar, set before any run).
CPU_DEEP_SHARE = 0.2896
DEVICE_DEEP_SHARE_BAR = CPU_DEEP_SHARE / 2
LAST_ENTRY_RAYS = 64
MAX_RAY_STEPS = 128      # no ray of the comb takes as many node steps in the CPU's 4-wide walk (asserted there)

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _host(n):
    """(nodes, tris) of any n triangles with two lights, host-built: the shallow tree that is the "before" of every comparison."""
    def make():
        rs = np.random.RandomState(23)
        a = rs.uniform(-8, 8, (n, 3)).astype(np.float32) + np.float32([0, 20, 0])
        b, c = a + rs.uniform(-3, 3, a.shape).astype(np.float32), a + rs.uniform(-3, 3, a.shape).astype(np.float32)
        prims = np.concatenate([make_prims(a[:n - 2], b[:n - 2], c[:n - 2]), make_prims(a[n - 2:], b[n - 2:], c[n - 2:], albedo=(0, 0, 0), emit=(6, 6, 6))])
        nodes, tris, _ = ptamd.build_bvh(prims)
        assert len(tris) == n and R.emissive(tris).sum() == 2
        return nodes, tris
    return _cached(("host", n), make)


def host_tris(name):
    return TB._chain_tris() if name.startswith("chain") else _host(len(Dp.comb_positions(int(name[4:]))))


def positions(name):
    """The chain scene as it is; the comb with its two lights (wherever the host build put them) turned to face the other triangles."""
    if name.startswith("chain"):
        return X.chain_positions()
    return _cached(("pos", name), lambda: Dp.other_face(Dp.comb_positions(int(name[4:])), np.nonzero(R.emissive(host_tris(name)[1]))[0]))


def yardstick(name):
    return _cached(("yard", name), lambda: X.build(positions(name), TREES[name][1] or 0, 0.0))


def moved(name, pos=None):
    """(nodes', tris') at the positions, as the oracle and a fresh upload take them."""
    nodes, tris = host_tris(name)
    tris2 = R.restate_tris(tris, (positions(name) if pos is None else pos).reshape(-1, 9))
    return R.refit_nodes(nodes, tris2), tris2


def camera_of(name, lib=ptamd, pos=None):
    if name.startswith("chain"):
        return lib.make_camera(W, H, pos=X.CHAIN_CAMERA_POS)
    kw = {"rot_deg" if lib is ptamd else "rot": Dp.COMB_CAMERA_ROT}
    return lib.make_camera(W, H, pos=pos or Dp.COMB_CAMERA_POS, **kw)


def params(**kw):
    return ptamd.default_params(**{**dict(passes=PASSES, spp_per_pass=SPP), **kw})


def query_rays(name):
    """The closest-hit rays of a tree: the comb's start inside the region all boxes share (512) or hit the triangles behind the last stack
    entry (LAST_ENTRY_RAYS), plus every third pinhole ray and rays about the room (axis-aligned and shortened ones among them,
    scenes_util.scene_rays8); the chain's are its own test's."""
    cam = camera_of(name)
    if name.startswith("chain"):
        return np.concatenate([scene_rays8(3000, np.random.RandomState(5)), pinhole_rays(cam)[::3]]).astype(np.float32)
    return np.concatenate([Dp.comb_query_rays(11, 256), Dp.comb_last_entry_rays(13, LAST_ENTRY_RAYS), pinhole_rays(cam)[::3],
                           scene_rays8(500, np.random.RandomState(5))]).astype(np.float32)


def oracle_scene(name):
    def make():
        O.set_libm(1)
        nodes2, tris2 = moved(name)
        return O.Scene(nodes2.tobytes(), tris2)
    return _cached(("oracle", name), make)


def oracle_frame(name):
    return _cached(("oframe", name), lambda: oracle_scene(name).render(camera_of(name, O), O.make_params(W, H, PASSES, SPP), 16)[0])


def device_scene(name, rebuild=True):
    """The host-built scene moved to the positions and, with rebuild, given its deep tree."""
    nodes, tris = host_tris(name)
    sc = ptamd.Scene(nodes, tris)
    sc.update_vertices(positions(name).reshape(-1, 9))
    if rebuild:
        D = TREES[name][1]
        if D is None:
            sc.rebuild_tree()
        else:
            sc.rebuild_tree(depth_budget=D, large_fraction=0.0)
    return sc


def _limits(depth, quad_depth):
    return ptamd.lib().pt_dbg_tree_limits(depth, quad_depth, None, None)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the premises
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tree_numbers_limits_and_which_walk_is_taken():
    md, mq = C.c_int32(0), C.c_int32(0)
    assert ptamd.lib().pt_dbg_tree_limits(0, 0, C.byref(md), C.byref(mq)) == 0 and (md.value, mq.value) == (MAX_DEPTH, MAX_QUAD_DEPTH)
    assert (len(positions("comb32")), len(positions("comb33")), len(positions("comb29"))) == (99, 102, 90)
    assert np.array_equal(B.keys_of(positions("comb32")), B.keys_of(Dp.comb_positions(32)))      # a light turned round keeps its key
    for name, (_, D, numbers, _) in TREES.items():
        t = yardstick(name)
        assert (t["depth"], t["quad_depth"]) == numbers, (name, t["depth"], t["quad_depth"])
        T._check_ref_is_a_tree(t, len(positions(name)))
        assert _limits(*numbers) == 0, name
        assert 3 * t["quad_depth"] + 2 > DRAIN_QUAD_STACK, name      # wf_drain<false> and the binary fallback of pt_query
        assert 3 * t["quad_depth"] + 2 <= TRACE_STACK, name          # wf_trace's stack holds
        assert D is None or (t["depth"] == D - 1 and t["n_large"] == 0 and t["n_flattened_tris"] > 0), name
    # the comb at 32 is the plain tree: no budget below 33 is needed, and (32, 0) would already cut it
    plain = yardstick("comb32")
    assert plain["n_flattened_tris"] == 0 and X.build(positions("comb32"), 32, 0.0)["depth"] == 31
    # on either side of the three: the last tree the 4-wide walks take, and the two that are refused
    t = X.build(X.chain_positions(), 27, 0.0)
    assert (t["depth"], t["quad_depth"]) == (26, 12) and 3 * 12 + 2 <= DRAIN_QUAD_STACK
    t = X.build(X.chain_positions(), 0, 0.0)
    assert (t["depth"], t["quad_depth"]) == (36, 17) and _limits(36, 17) == T.PT_ERR_UNSUPPORTED
    t = X.build(positions("comb33"), 0, 0.0)
    assert (t["depth"], t["quad_depth"]) == (33, 16)
    assert _limits(33, 16) == T.PT_ERR_UNSUPPORTED and "depth 33" in ptamd.lib().pt_last_error().decode()
    # the tree the comb started from: levels 2 .. 29 alone, the same with and without the largest budget
    for D in (0, 32):
        t = X.build(positions("comb29"), D, 0.0)
        assert (t["depth"], t["quad_depth"], t["n_flattened_tris"], Dp.both_interior_path(t["node_refs"])) == (29, 14, 0, 28), D


def test_binary_stack_of_every_tree():
    """trace_closest holds kStackDepth = 32 entries per lane and the limit check accepts depth 32.  Reading its loop: an entry is pushed
    only at a node whose two children are both interior, such nodes lie at depths 0 .. depth - 2, so a walk pushes at most depth - 1 = 31.
    The comb reaches that figure — on every ray that starts inside the region its boxes share — and nothing goes beyond it: the largest
    stack of the simulated walks (deep_tree_ref.binary_walks: an approximation of the kernel's arithmetic, as tools/stack_lab.cpp is)
    equals the structural bound, the number of nodes with two interior children on the tree's longest such path."""
    for name, (_, _, (depth, _), structural) in TREES.items():
        t, pos = yardstick(name), positions(name)
        assert Dp.both_interior_path(t["node_refs"]) == structural <= depth - 1 <= MAX_DEPTH - 1, name
        top, steps = Dp.binary_walks(t["node_refs"], Dp.child_boxes(t, pos, t["node_refs"]), query_rays(name))
        print(f"{name}: largest binary stack by ray {np.bincount(top).tolist()}, most node steps {steps.max()}")
        assert top.max() <= structural, name
        if name == "comb32":
            inside = top[:512 + LAST_ENTRY_RAYS]      # rays and segments from inside the common region, and the rays at code 0
            assert structural == depth - 1 == 31 and (inside == 31).all() and top.max() == 31
            # ... and what the 31st entry is good for: behind it lies the closest hit of every ray of comb_last_entry_rays
            O.set_libm(1)
            _, prim, _ = oracle_scene(name).raycast(query_rays(name)[512:512 + LAST_ENTRY_RAYS])
            assert (prim == Dp.COMB_LAST_ENTRY_PRIM).all(), prim
    # the refused sibling would need the 33rd entry
    t = X.build(positions("comb33"), 0, 0.0)
    assert Dp.both_interior_path(t["node_refs"]) == 32 > MAX_DEPTH - 1


def test_comb_camera_sees_the_comb_and_fills_the_wide_stack():
    """At least a tenth of the camera's pinhole rays hit (the oracle's ray cast), their binary walks fill the stack to 31 as well, and
    their 4-wide walks go far into wf_trace's global-memory overflow: the share that is the yardstick of the device's histogram."""
    O.set_libm(1)
    rays = pinhole_rays(camera_of("comb32"))
    _, prim, _ = oracle_scene("comb32").raycast(rays)
    print(f"comb scene: {np.mean(prim >= 0):.3f} of the pinhole rays hit, {len(np.unique(prim[prim >= 0]))} triangles seen")
    assert np.mean(prim >= 0) >= 0.10
    ref = oracle_frame("comb32")
    assert np.isfinite(ref).all() and (ref > 0).any(-1).mean() > 0.9      # the two lights reach the frame
    t, pos = yardstick("comb32"), positions("comb32")
    top, _ = Dp.binary_walks(t["node_refs"], Dp.child_boxes(t, pos, t["node_refs"]), rays[::4])
    assert top.max() == 31
    qboxes = Dp.child_boxes(t, pos, t["quad_refs"])
    hist, tops, steps = Dp.quad_walks(t, pos, qboxes, rays)
    inner = Dp.quad_walks(t, pos, qboxes, Dp.comb_query_rays(11, 256))
    share = hist[31] / hist.sum()
    print(f"comb scene, 4-wide walk of the pinhole rays: largest stack {tops.max()}, {hist.sum() / len(rays):.1f} node steps per ray, at most "
          f"{steps.max()} ({inner[2].max()} for rays from inside, {(steps > 32).mean():.3f} of the pinhole rays take more than 32), "
          f"share with 16 or more entries {hist[16:].sum() / hist.sum():.4f}, with 31 or more {share:.4f}")
    print("stack-depth histogram:", hist.tolist())
    # three pushes at each of the 16 levels 0 .. quad_depth: one more than 3 * quad_depth + 2, which counts the entries after the first
    # leaf of the deepest node is parked; 64 hold either figure up to quad_depth 20
    assert tops.max() == 3 * (t["quad_depth"] + 1) == 48 <= TRACE_STACK and 3 * (MAX_QUAD_DEPTH + 1) <= TRACE_STACK
    assert abs(share - CPU_DEEP_SHARE) < 0.005
    # what test_time_slicing_resumes_the_deepest_stacks rests on: rays long enough to be suspended, short enough for the iteration cap
    assert (steps > 32).mean() > 0.10 and max(steps.max(), inner[2].max()) < MAX_RAY_STEPS and inner[1].max() == 48


def test_chain_camera_sees_the_chain():
    """tests/test_rebuild_budget.py asks the same of the same camera: the deep trees are rendered through it."""
    O.set_libm(1)
    _, prim, _ = oracle_scene("chain32").raycast(pinhole_rays(camera_of("chain32")))
    assert np.mean(prim >= 0) >= 0.10


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    O.set_libm(1)            # the pinned contract: correctly rounded float transcendentals
    yield


def _assert_kept(now, was, what):
    for k in was:
        if was[k].dtype == np.float32:
            assert T._same_or_nan(now[k], was[k]), (what, k)
        else:
            assert np.array_equal(now[k], was[k]), (what, k)


def _assert_tree(sc, pos, what):
    a, info = T._arrays(sc), sc.tree_info()
    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 10000))
    try:
        T._assert_is_a_tree(a, info, pos, what)      # tree_info against walk_depths of the arrays; walk_nodes and walk_quad
    finally:
        sys.setrecursionlimit(limit)
    return a, info


def _nee_rows(hits_o, prim_o):
    pts = hits_o[prim_o >= 0][:512, 5:8]
    seeds = np.random.RandomState(12).randint(0, 2**32, (pts.shape[0], 2), dtype=np.uint64).astype(np.uint32)
    return np.concatenate([pts, seeds.view(np.float32)], 1)


def _everything(sc, cam, prm, rays, in5):
    out = T._everything(sc, cam, prm, rays)
    out["nee"] = sc.nee(in5)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TREES))
def test_bits_are_kept(_gpu, name):
    """Render, mode 0 with the counting build, AOV, pt_dbg_raycast, pt_trace_rays with surface records, any hit, pt_render_rays and
    pt_dbg_nee before the rebuild (the shallow host-built tree: 4-wide walks everywhere) and after it (the deep tree: trace_closest in
    wf_drain<false>, in pt_query's fallback and, as before, in mode 0, the AOV kernel and pt_dbg_raycast; wf_trace on the 4-wide tree)."""
    pos, t = positions(name), yardstick(name)
    sc = device_scene(name, rebuild=False)
    cam, prm, rays = camera_of(name), params(), query_rays(name)
    so = oracle_scene(name)
    hits_o, prim_o, _ = so.raycast(rays)
    in5 = _nee_rows(hits_o, prim_o)
    assert 3 * sc.tree_info()["quad_depth"] + 2 <= DRAIN_QUAD_STACK      # before: the 4-wide walks
    before, was = T._arrays(sc), _everything(sc, cam, prm, rays, in5)
    D = TREES[name][1]
    report = sc.rebuild_tree() if D is None else sc.rebuild_tree(depth_budget=D, large_fraction=0.0)
    if D is not None:
        assert report == {"n_large": 0, "n_flattened_tris": t["n_flattened_tris"]}
    a, info = _assert_tree(sc, pos, name)
    assert (info["n_wide"], info["n_quad"], info["depth"], info["quad_depth"], info["rebuilds"]) == (t["n_wide"], t["n_quad"], t["depth"], t["quad_depth"], 1)
    assert (info["depth"], info["quad_depth"]) == TREES[name][2] and 3 * info["quad_depth"] + 2 > DRAIN_QUAD_STACK      # after: the binary walks
    assert np.array_equal(a["tri"].reshape(-1, 12)[:, 3].view(np.int32), t["prim"]), f"{name}: tree order"
    assert np.array_equal(a["nodes"].reshape(-1, 16)[:, 12:14].view(np.int32), t["node_refs"]), f"{name}: refs of nodes"
    assert np.array_equal(a["quad"].reshape(-1, 16)[:, 4:8].view(np.int32), t["quad_refs"]), f"{name}: refs of quad"
    T._assert_arrays(a, before, f"{name}: arrays a rebuild does not touch", T.KEPT)
    assert sc.tree_inflation() == 1.0
    now = _everything(sc, cam, prm, rays, in5)
    _assert_kept(now, was, name)
    assert (now["any"] == (now["closest prim"] >= 0)).all() and np.isfinite(now["render"]).all()
    # ... and they are the oracle's: closest hits and NEE rows in every bit, the frame by the bar of the chain scene
    nee_o = so.nee(in5)
    lit = int((nee_o[:, 8:11].sum(1) > 0).sum())
    print(f"{name}: {info}; oracle hit share {np.mean(prim_o >= 0):.3f}, {len(in5)} NEE rows, {lit} lit")
    assert lit >= 20 or name != "comb32"      # lit and shadowed rows both (the chain scene's lights face away from what the rays hit)
    _assert_closest((now["closest t"], now["closest prim"], now["closest surface"]), hits_o, prim_o, f"{name}: trace_rays, binary fallback")
    at, aprim = sc.trace_rays(rays, any_hit=True)
    _assert_any(at, aprim, now["closest t"], now["closest prim"], rays, len(pos), f"{name}: any hit, binary fallback")
    assert np.array_equal(now["raycast prim"], prim_o) and same_bits_or_nan(now["raycast"], hits_o).all(), f"{name}: pt_dbg_raycast"
    assert T._same_or_nan(now["nee"], nee_o), f"{name}: pt_dbg_nee against the oracle"
    check_image(now["render"], oracle_frame(name), f"{name}: the deep tree against the oracle")


def _comb_frame():
    """The comb's frame at the default schedule on the deep tree, rendered once: (frame, iterations)."""
    def make():
        sc = device_scene("comb32")
        return sc.render(camera_of("comb32"), params()), sc.last_iterations()
    return _cached("comb frame", make)


@pytest.mark.gpu
def test_every_schedule_gives_the_same_bits(_gpu):
    """Drain thresholds 0, 1536 (a quarter of the streams) and 2^30, shade rounds, early shade and mode 0 on the comb.  The host polls
    the live count for the first time after 16 iterations, and at 2 spp every stream of this open scene has retired by then: whatever
    the threshold, last_iterations() is 16 and wf_trace has done the whole render, stack overflow and all.  The thresholds are kept here
    as the calls a host makes; the hand-over to wf_drain<false> is forced in test_the_binary_drain_does_the_whole_render."""
    want, _ = _comb_frame()
    cam, prm = camera_of("comb32"), params()
    sc = device_scene("comb32")
    assert sc.tree_info()["quad_depth"] >= 13
    its = {}
    for threshold in (0, 1536, 1 << 30):
        sc.set_drain_threshold(threshold)
        T._assert_same(sc.render(cam, prm), want, f"drain threshold {threshold}")
        its[threshold] = sc.last_iterations()
    print(f"iterations: drain threshold 2^30 {its[1 << 30]}, 1536 {its[1536]}, 0 {its[0]}")
    assert its[1 << 30] == 16 and its[1 << 30] <= its[1536] <= its[0]
    check_image(want, oracle_frame("comb32"), "comb32, default schedule")
    sc.set_drain_threshold(0)
    for rounds in (0, 1):
        sc.set_shade_rounds(rounds)
        T._assert_same(sc.render(cam, prm), want, f"shade rounds {rounds}")
    sc.set_shade_rounds(-1)
    sc.set_early_shade(STREAMS + 1)      # the PUBLISH build of wf_trace
    T._assert_same(sc.render(cam, prm), want, "early shade")
    sc.set_early_shade(0)
    sc.set_mode(0)                       # the one-kernel state machine: trace_closest for every ray
    T._assert_same(sc.render(cam, prm), want, "mode 0")


def short_rays(sc, cam):
    """The camera's rays of pass 0 with tmax = t / 2 on every other ray that hits: (rays, seeds, stride, which rays are cut)."""
    rays, seeds, stride = ptamd.camera_rays(cam, 0)
    t, prim = sc.trace_rays(rays)
    cut = (prim >= 0) & (np.arange(len(rays)) % 2 == 0)
    rays[cut, 7] = t[cut] * np.float32(0.5)
    return rays, seeds, stride, cut


@pytest.mark.gpu
def test_window_tile_list_views_and_rays(_gpu):
    """The entry points that size their own work buffer (and with it the stride of wf_trace's stack overflow)."""
    want, _ = _comb_frame()
    cam, prm = camera_of("comb32"), params()
    sc = device_scene("comb32")
    x0, y0 = W // 2 - 8, H // 2 - 8
    T._assert_same(sc.render_window(cam, prm, (x0, y0, x0 + 16, y0 + 16)), want[y0:y0 + 16, x0:x0 + 16], "16 x 16 window in the middle")
    tiles = [43, 0, 18, 29]                      # of the 8 x 6 tiles of the frame
    got = sc.render_tile_list(cam, prm, tiles)
    for i, tile in enumerate(tiles):
        ty, tx = divmod(tile, W // 8)
        T._assert_same(got[i], want[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8], f"tile {tile} of the list")
    cam2 = camera_of("comb32", pos=(-33.0, -13.0, 33.5))
    views = sc.render_views([cam, cam2], prm)
    T._assert_same(views[0], want, "view 0 of two")
    T._assert_same(views[1], sc.render(cam2, prm), "view 1 of two")
    assert not np.array_equal(T.bits(views[1]), T.bits(want))
    # the camera's own rays of pass 0, and a tmax that ends every other primary ray that hits
    one = params(passes=1)
    rays, seeds, stride = ptamd.camera_rays(cam, 0)
    pass0 = sc.render(cam, one).reshape(-1, 3)
    T._assert_same(sc.render_rays(rays, one, seeds, stride), pass0, "the camera's rays of pass 0")
    short, seeds, stride, cut = short_rays(sc, cam)
    assert cut.sum() > len(rays) // 8
    acc = np.float32(0)      # what a pixel that looks past the scene gets: spp times 0 + 1 * 0.1, then the mean (tests/test_rays.py)
    for _ in range(SPP):
        acc = np.float32(acc + np.float32(np.float32(1) * np.float32(0.1)))
    got = sc.render_rays(short, one, seeds, stride)
    T._assert_same(got[cut], np.full((int(cut.sum()), 3), np.float32(acc / np.float32(SPP)), np.float32), "tmax = t / 2: the ambient term")
    T._assert_same(got[~cut], pass0[~cut], "tmax = t / 2: the unchanged rays")


# ---------------------------------------------------------------------------------------------------------------------------------
# the overflow of wf_trace's stack, in processes of their own (the tuning knobs are read once per process)
# ---------------------------------------------------------------------------------------------------------------------------------
def _child(tmp_path, script, args, env):
    path = tmp_path / "child.py"
    path.write_text(script)
    r = subprocess.run([sys.executable, str(path), os.path.join(ROOT, "pathtrace-on-cuda_amd"), os.path.join(ROOT, "tests")] + [str(a) for a in args],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


_RENDER_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
from test_deep_tree import camera_of, device_scene, params
sc = device_scene("comb32")
sc.set_drain_threshold(0)
img = sc.render(camera_of("comb32"), params())
it = sc.last_iterations()
out = dict(img=img, iterations=it)
if int(sys.argv[4]):      # the counting build
    out.update(hist=sc.trace_depth_hist(), launch_rays=sc.trace_launch_rays(it))
np.savez(sys.argv[3], **out)
"""
SLICED = {"PTAMD_BS": "31", "PTAMD_LB": "0", "PTAMD_BM": "32"}


def _render_child(tmp_path, tag, env, counting=False):
    out = tmp_path / f"{tag}.npz"
    _child(tmp_path, _RENDER_CHILD, [out, int(counting)], dict(env, **({"PTAMD_TSTAT": "1"} if counting else {})))
    return np.load(out)


@pytest.mark.gpu
def test_the_top_of_the_stack_overflow_runs(_gpu, tmp_path):
    """The counting build of wf_trace (PTAMD_TSTAT=1) bins the stack depth after every node step; its last bin is 31 entries or more, of
    which 15 or more lie in global memory — entries the needle scene (24 or 25 at most) never reaches.  The share of the render's node
    steps in that bin must be half of what the CPU walker finds for the camera's pinhole rays (CPU_DEEP_SHARE = 0.2896, asserted by
    test_comb_camera_sees_the_comb_and_fills_the_wide_stack; the bar was set from that figure, before any run on a device).
    Measured on an MI355X: DESIGN.md section 27."""
    want, _ = _comb_frame()
    g = _render_child(tmp_path, "hist", {}, counting=True)
    hist = g["hist"].astype(np.int64)
    share = hist[31] / max(int(hist.sum()), 1)
    print(f"comb32: {int(hist.sum())} node steps in {int(g['iterations'])} iterations, share at stack depth >= 16: {hist[16:].sum() / max(int(hist.sum()), 1):.4f}, "
          f">= 31: {share:.4f}")
    print("stack-depth histogram:", hist.tolist())
    assert hist.sum() > 0 and hist[31] > 0
    assert share >= DEVICE_DEEP_SHARE_BAR
    T._assert_same(g["img"], want, "counting build of wf_trace")


@pytest.mark.gpu
def test_time_slicing_resumes_the_deepest_stacks(_gpu, tmp_path):
    """PTAMD_BS=31 makes the node budget PTAMD_BM steps per launch, PTAMD_LB=0 switches the late budget off: a ray is written to a
    suspend record (4 + 16 + 48 words) whenever its budget is spent and restored by another lane in the next launch.  The bits are
    those of the default budget.
    The CPU walk takes at most 33 node steps per ray (the tree has 33 4-wide nodes) and reaches the deepest node, with 45 entries on the
    stack, in 16.  A budget of 32 steps therefore suspends only the longest rays (more than a tenth of the camera's), once, near the end
    of their walk, and last_iterations() cannot show even that: the host counts iterations in polls of 16, and at 2 spp this open scene
    is done within the first poll either way.  So that run is held to the same bits and, in the counting build, to more rays handed to
    lanes than the default budget hands out — a suspended ray is queued once more.  A budget of 4 steps does what the test is after:
    every ray that goes down the chain is suspended with about 12, 24, 36 and 47 entries on its stack, and a stream whose rays take more
    than 64 steps together outlasts the first poll, so there are more iterations.
    The cap: a stream traces at most spp * (max_bounce + max_refract + 3) = 38 rays one after the other, a ray of S < 128 node steps
    (MAX_RAY_STEPS, asserted on the CPU) takes at most S / 4 + 1 = 33 launches: 1254 iterations, inside half of the pipeline's cap of
    (38 + 8) * 64 = 2944."""
    want, _ = _comb_frame()
    cam, prm = camera_of("comb32"), params()
    sc = device_scene("comb32")
    sc.set_drain_threshold(0)
    T._assert_same(sc.render(cam, prm), want, "default budget, pipeline to the end")
    it_parent = sc.last_iterations()
    rays_in_a_row = SPP * (prm.max_bounce + prm.max_refract + 3)
    hard_cap = (rays_in_a_row + 8) * 64
    assert rays_in_a_row * (MAX_RAY_STEPS // 4 + 1) < hard_cap // 2
    g = _render_child(tmp_path, "sliced32", SLICED)
    T._assert_same(g["img"], want, "node budget 32")
    counted, base = _render_child(tmp_path, "sliced32_counted", SLICED, counting=True), _render_child(tmp_path, "default_counted", {}, counting=True)
    T._assert_same(counted["img"], want, "node budget 32, counting build")
    handed, handed_base = int(counted["launch_rays"].sum()), int(base["launch_rays"].sum())
    g4 = _render_child(tmp_path, "sliced4", dict(SLICED, PTAMD_BM="4"))
    print(f"iterations: default budget {it_parent}, budget of 32 steps {int(g['iterations'])}, of 4 steps {int(g4['iterations'])} (cap {hard_cap}); "
          f"rays handed to lanes: default budget {handed_base}, budget of 32 steps {handed}")
    assert it_parent <= int(g["iterations"]) < hard_cap // 2 and handed > handed_base
    T._assert_same(g4["img"], want, "node budget 4")
    assert it_parent < int(g4["iterations"]) < hard_cap // 2


_DRAIN_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
from test_deep_tree import camera_of, device_scene, params, short_rays
name = sys.argv[3]
sc = device_scene(name)
cam, prm = camera_of(name), params()
short, seeds, stride, cut = short_rays(sc, cam)
out = {}
for what, threshold in (("pipeline", 0), ("drain", 1 << 30)):
    sc.set_drain_threshold(threshold)
    out[what] = sc.render(cam, prm)
    out["it_" + what] = sc.last_iterations()
out["short"] = sc.render_rays(short, params(passes=1), seeds, stride)
out["it_short"] = sc.last_iterations()
np.savez(sys.argv[4], **out)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TREES))
def test_the_binary_drain_does_the_whole_render(_gpu, tmp_path, name):
    """wf_drain<false, Cam>, the instantiation no knob selects: it runs when 3 * quad_depth + 2 > 40 and streams are alive at a poll.  A
    node budget of ONE step per launch (PTAMD_BS=31 PTAMD_BM=1 PTAMD_LB=0; tuning knobs, read once per process: a child) leaves every
    ray of more than 16 node steps pending at the first poll, after 16 iterations, where a drain threshold of 2^30 hands every live
    stream over: the drain traces those primary rays again from the root, with trace_closest, and everything after them.  That it had
    streams to take is read off the same child: with threshold 0 the same render needs more than 16 iterations, so streams were alive
    after 16.  Both frames are the parent's (default budget, wf_trace alone) bit for bit, and so is pt_render_rays with a tmax that
    ends every other primary ray, which the drain must honour when it traces them again."""
    sc = device_scene(name)
    cam = camera_of(name)
    assert sc.tree_info()["quad_depth"] >= 13
    want = _comb_frame()[0] if name == "comb32" else sc.render(cam, params())
    short, seeds, stride, cut = short_rays(sc, cam)
    want_short = sc.render_rays(short, params(passes=1), seeds, stride)
    out = tmp_path / "drain.npz"
    _child(tmp_path, _DRAIN_CHILD, [name, out], {"PTAMD_BS": "31", "PTAMD_LB": "0", "PTAMD_BM": "1"})
    g = np.load(out)
    print(f"{name}, one node step per launch: iterations {int(g['it_pipeline'])} without the drain, {int(g['it_drain'])} with it, "
          f"{int(g['it_short'])} for the shortened rays; {int(cut.sum())} rays cut")
    T._assert_same(g["pipeline"], want, f"{name}: one node step per launch, wf_trace to the end")
    T._assert_same(g["drain"], want, f"{name}: wf_drain<false> from the first poll")
    assert int(g["it_drain"]) == 16 < int(g["it_pipeline"])
    T._assert_same(g["short"], want_short, f"{name}: shortened rays, wf_drain<false> from the first poll")
    assert int(g["it_short"]) == 16 and cut.sum() > 64
    check_image(g["drain"], oracle_frame(name), f"{name}: wf_drain<false> against the oracle")


# ---------------------------------------------------------------------------------------------------------------------------------
# the boundary, and what comes after a rebuild
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_tree_33_deep_is_refused_and_nothing_changes(_gpu):
    """No refused tree is ever traversed: the scene keeps the host-built tree it had."""
    name = "comb33"
    sc = device_scene(name, rebuild=False)
    cam, prm = camera_of(name), params()
    rays = np.concatenate([Dp.comb_query_rays(11, 256), pinhole_rays(cam)[::3]]).astype(np.float32)
    before, was = T._arrays(sc), T._everything(sc, cam, prm, rays)
    info = sc.tree_info()
    TB._refused(sc.rebuild_tree)
    assert "depth 33" in ptamd.lib().pt_last_error().decode()
    T._assert_arrays(T._arrays(sc), before, "comb33: all nine arrays after the refused rebuild")
    assert sc.tree_info() == info and info["rebuilds"] == 0
    _assert_kept(T._everything(sc, cam, prm, rays), was, "comb33: after the refused rebuild")
    # the same scene is accepted with the largest budget
    sc.rebuild_tree(depth_budget=32, large_fraction=0.0)
    t = X.build(positions(name), 32, 0.0)
    assert (sc.tree_info()["depth"], sc.tree_info()["quad_depth"], sc.tree_info()["rebuilds"]) == (t["depth"], t["quad_depth"], 1) == (31, 15, 1)
    _assert_kept(T._everything(sc, cam, prm, rays), was, "comb33: under (32, 0)")


def _scale3(pos):
    """Every triangle three times its size about the centre of its own box (float32, rounded once per operation)."""
    c = B.centroids(pos).reshape(-1, 1, 3)
    return (c + np.float32(3) * (pos - c)).astype(np.float32)


def _rigid(pos):
    """A turn of 25 degrees about the y axis through the scene's middle and a shift, the same for every vertex."""
    mid = pos.reshape(-1, 3).astype(np.float64).mean(0)
    a = np.radians(25.0)
    rot = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    return ((pos.astype(np.float64) - mid) @ rot.T + mid + np.array([3.0, 1.5, -2.0])).astype(np.float32)


@pytest.mark.gpu
def test_vertex_updates_refit_the_32_deep_tree(_gpu):
    """pt_scene_update_vertices refits level by level: 32 levels here, 25 at most anywhere else in the suite."""
    name = "comb32"
    nodes, tris = host_tris(name)
    sc = device_scene(name)
    refs = T._refs_of(T._arrays(sc))
    cam, prm = camera_of(name), params()
    for move in (_scale3, _rigid):
        pos = move(positions(name))
        what = f"comb32, {move.__name__}"
        sc.update_vertices(pos.reshape(-1, 9))
        nodes2, tris2 = moved(name, pos)
        fresh = ptamd.Scene(nodes2, tris2)
        a = T._arrays(sc)
        T._assert_arrays(a, T._arrays(fresh), f"{what} against a fresh upload", ("surf", "lights", "leafbox", "spheres"))
        T._assert_is_a_tree(a, None, pos, what)      # every box of both trees is the padded exact bound of the new positions
        assert all(np.array_equal(x, y) for x, y in zip(T._refs_of(a), refs)), f"{what}: an update changed the refs of the rebuilt trees"
        assert sc.tree_info()["depth"] == 32 and sc.tree_inflation() != 1.0
        ref, _ = O.Scene(nodes2.tobytes(), tris2).render(camera_of(name, O), O.make_params(W, H, PASSES, SPP), 16)
        for mode in (1, 0):
            sc.set_mode(mode)
            fresh.set_mode(mode)
            got = sc.render(cam, prm)
            T._assert_same(got, fresh.render(cam, prm), f"{what}, mode {mode}, against a fresh upload")
            check_image(got, ref, f"{what}, mode {mode}, against the oracle")
        sc.set_mode(1)
        rays = query_rays(name)
        hits_o, prim_o, _ = O.Scene(nodes2.tobytes(), tris2).raycast(rays)
        _assert_closest(sc.trace_rays(rays, surface=True), hits_o, prim_o, f"{what}: trace_rays")


@pytest.mark.gpu
@pytest.mark.parametrize("D", (0, 32))
def test_treelet_passes_on_the_32_deep_tree(_gpu, D):
    """Two passes of pt_scene_rebuild_tree_opt.  Without a budget the limit of a pass is the depth of the tree it starts from, 32, and
    its launches cover every height up to it; under (32, 0) the tree it starts from is 31 deep."""
    name = "comb32"
    pos = positions(name)
    t = _cached(("opt", D), lambda: P.build(pos, D, 0.0, 2))
    assert t["depth"] <= (31 if D else 32) and t["n_restructured"] > 0
    sc = device_scene(name, rebuild=False)
    cam, prm, rays = camera_of(name), params(), query_rays(name)
    before, was = T._arrays(sc), T._everything(sc, cam, prm, rays)
    report = sc.rebuild_tree_optimized(passes=2, depth_budget=D, large_fraction=0.0)
    what = f"comb32 ({D}, 0) x 2"
    a, info = _assert_tree(sc, pos, what)
    print(f"{what}: {info} {report}")
    assert report == {k: t[k] for k in ("n_large", "n_flattened_tris", "n_roots", "n_restructured")}, what
    assert np.array_equal(a["tri"].reshape(-1, 12)[:, 3].view(np.int32), t["prim"]), f"{what}: tree order"
    assert np.array_equal(a["nodes"].reshape(-1, 16)[:, 12:14].view(np.int32), t["node_refs"]), f"{what}: refs of nodes"
    assert np.array_equal(a["quad"].reshape(-1, 16)[:, 4:8].view(np.int32), t["quad_refs"]), f"{what}: refs of quad"
    assert (info["n_wide"], info["n_quad"], info["depth"], info["quad_depth"], info["rebuilds"]) == (t["n_wide"], t["n_quad"], t["depth"], t["quad_depth"], 1)
    assert info["depth"] <= (31 if D else 32) and P.nodes_area(a["nodes"]) == t["nodes_area"], what
    T._assert_arrays(a, before, f"{what}: arrays a rebuild does not touch", T.KEPT)
    assert sc.tree_inflation() == 1.0
    _assert_kept(T._everything(sc, cam, prm, rays), was, what)
