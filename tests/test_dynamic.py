"""Moving the geometry of an uploaded scene (pt_scene_update_vertices, pt_scene_update_vertices_host, pt_scene_update_spheres,
pt_scene_tree_inflation, pt_dbg_scene_array): the C-ABI surface and the argument checks on the CPU, where the numpy yardstick
(tests/dynamic_ref.py) is also held against pt_bvh_build_sah and the arrays of pt_build_accel against their hashes before the refit
maps were added; on the GPU every array a render reads and every kind of render after an update, against a fresh upload of the moved
geometry, against numpy walks of the downloaded trees and against the CPU oracle.  Bits everywhere, no tolerances (the one
exception, stated where it is used: the float64 area sum of pt_scene_tree_inflation, whose summation order numpy does not follow).

How the hashes in ACCEL_SHA256 were taken: tools/dump_accel.cpp was linked against the host objects of the commit before this
feature and run as `dump_accel 1 16 <prefix>`; sha256 of the five files it wrote."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import dynamic_ref as R
import ptamd
from scenes_util import make_prims, scene_rays8
from scenes_util import test_spheres as make_test_spheres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pathtrace-on-cuda_amd")
NEW_SYMBOLS = ("pt_scene_update_vertices", "pt_scene_update_vertices_host", "pt_scene_update_spheres", "pt_scene_tree_inflation",
               "pt_dbg_scene_array")
CAMERAS = (((0.0, 20.0, 60.0), (0.0, 90.0, 0.0), 45.0), ((0.0, 20.0, 53.0), (0.0, 93.5, 0.0), 45.0), ((14.0, 23.5, 60.0), (0.0, 97.0, 0.0), 35.0))
FRAMES = ((64, 48), (100, 52))
PASSES, SPP = 3, 4
ARRAYS = ("nodes", "quad", "tri", "tripair", "leafbox", "surf", "lights", "spheres", "core")
ACCEL_SHA256 = {      # kind 1, lat_lon 16, at the parent commit
    "wide": "498772e0e74311379f1feb16f7c968a1ca534d5b6de45c7d436c3311e2f1bcfe",
    "quad": "4f2e3f37f0a28eb2e76460969c240f7ec3fa17eb48700e6d441a329b20acc85c",
    "tri": "03401434717a8bf88e9d5da5da518e382df60d29d1ff83646592b733f2e78050",
    "tripair": "27b393fd4b34d5524865d0ada88a2be17626da7d9db1f9a28876e1858fd4e31b",
    "leafbox": "fb126beb4095ff2d35016783fddf25db17d91af2e149c07288d993254ff56983",
}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def params(**kw):
    return ptamd.default_params(**{**dict(passes=PASSES, spp_per_pass=SPP), **kw})


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW_SYMBOLS:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    for name in ("update_vertices", "update_spheres", "tree_inflation", "dbg_array"):
        assert callable(getattr(ptamd.Scene, name))
    assert tuple(ptamd.SCENE_ARRAYS) == ARRAYS and [ptamd.SCENE_ARRAYS[a][0] for a in ARRAYS] == list(range(9))


def test_bad_arguments_are_rejected_before_any_device_call():
    """A fake scene and fake device addresses: never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    scene, d_pos = C.c_void_p(1 << 40), C.c_void_p((1 << 40) + (1 << 20))
    ratio = C.c_double(7.0)
    sph = make_test_spheres()
    buf = np.zeros(16, np.float32)
    cases = [
        ("update: NULL scene", lambda: l.pt_scene_update_vertices(None, d_pos, None, None)),
        ("update: NULL d_pos", lambda: l.pt_scene_update_vertices(scene, None, d_pos, None)),
        ("update_host: NULL scene", lambda: l.pt_scene_update_vertices_host(None, ptamd._ptr(buf), None)),
        ("update_host: NULL h_pos", lambda: l.pt_scene_update_vertices_host(scene, None, None)),
        ("spheres: NULL scene", lambda: l.pt_scene_update_spheres(None, ptamd._ptr(sph), 3)),
        ("spheres: NULL array", lambda: l.pt_scene_update_spheres(scene, None, 3)),
        ("inflation: NULL scene", lambda: l.pt_scene_tree_inflation(None, C.byref(ratio))),
        ("inflation: NULL ratio", lambda: l.pt_scene_tree_inflation(scene, None)),
        ("array: NULL scene", lambda: l.pt_dbg_scene_array(None, 0, ptamd._ptr(buf), 64)),
        ("array: which = 9", lambda: l.pt_dbg_scene_array(scene, 9, ptamd._ptr(buf), 64)),
        ("array: which = -1", lambda: l.pt_dbg_scene_array(scene, -1, ptamd._ptr(buf), 64)),
    ]
    for what, call in cases:
        assert call() == -1, what
        assert what.split(":")[0].split("_")[0] in l.pt_last_error().decode(), (what, l.pt_last_error())


class _FakeScene:
    n_tris, device, _h = 5, 0, C.c_void_p(1 << 40)


def test_wrapper_checks_shape_dtype_and_device_on_the_host():
    import torch
    fake = _FakeScene()
    up = ptamd.Scene.update_vertices
    for pos in (np.zeros((4, 9), np.float32), np.zeros((5, 8), np.float32), np.zeros(45, np.float32)):
        with pytest.raises(ptamd.PtError):
            up(fake, pos)
    with pytest.raises(ptamd.PtError):
        up(fake, np.zeros((5, 9), np.float32), frames=np.zeros((5, 26), np.float32))
    for pos in (torch.zeros((5, 9)), torch.zeros((5, 9), dtype=torch.float64), torch.zeros((4, 9)), torch.zeros((9, 5)).t(), [0.0] * 45):
        with pytest.raises(ptamd.PtError):      # a CPU tensor, a wrong dtype, a wrong size, not contiguous, not an array
            up(fake, pos)


@pytest.mark.parametrize("kind,lat_lon", [(0, 187), (1, 16), (1, 24)])
def test_yardstick_reproduces_the_host_build_on_unchanged_positions(kind, lat_lon):
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(kind, lat_lon))
    t2 = R.restate_tris(tris, R.positions(tris))
    assert np.array_equal(bits(t2), bits(tris))
    assert R.refit_nodes(nodes, t2).tobytes() == nodes.tobytes()
    # ... and a move changes them (lifting everything changes every box)
    moved = R.restate_tris(tris, R.move_translate(R.positions(tris), np.ones(len(tris), bool), np, (0.0, 2.5, 0.0)))
    n3 = R.refit_nodes(nodes, moved)
    assert not np.array_equal(bits(moved[:, :9]), bits(tris[:, :9]))
    assert (n3["bMin"][:, 1] > nodes["bMin"][:, 1]).all() and np.array_equal(n3["bMax"][:, 0], nodes["bMax"][:, 0])


def test_accel_arrays_are_those_of_the_build_before_the_maps(tmp_path):
    # the five host sources compiled into tmp_path with the Makefile's own g++ flags: nothing is written into the source tree
    objs = []
    for name in ("accel_build", "bvh_build", "scenes", "pt_host", "obj_loader"):
        objs.append(str(tmp_path / f"{name}.o"))
        subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-fvisibility=hidden", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                        "-c", os.path.join(PKG, "host", f"{name}.cpp"), "-o", objs[-1]], check=True)
    exe = str(tmp_path / "dump_accel")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "dump_accel.cpp")] + objs +
                   ["-pthread", "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("PTAMD_TREE", "PTAMD_LEAF", "PTAMD_BFS")}
    subprocess.run([exe, "1", "16", str(tmp_path / "a")], check=True, env=env)
    for name, want in ACCEL_SHA256.items():
        assert hashlib.sha256((tmp_path / f"a.{name}.bin").read_bytes()).hexdigest() == want, name


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
    """(nodes, tris, spheres) of a test scene, as tests/test_views.py builds them."""
    if name not in _BUILT:
        prims = ptamd.gen_scene(0, 187) if name == "cornell" else ptamd.gen_scene(1, 16)
        nodes, tris, _ = ptamd.build_bvh(prims)
        _BUILT[name] = (nodes, tris, make_test_spheres() if name == "standin_spheres" else None)
    return _BUILT[name]


MOVES = {"cornell": ("lights", "wall"), "standin": ("rigid", "lights", "scale3"), "standin_spheres": ("rigid", "lights", "scale3")}
CASES = [(n, m) for n in MOVES for m in MOVES[n]]


def _move(tris, move, device="cuda:0"):
    """The moved positions, made with torch on the device: (tensor (n, 9) on the device, the same as numpy)."""
    import torch
    pos = torch.from_numpy(R.positions(tris)).to(device)
    sel = lambda m: torch.from_numpy(m).to(device)      # noqa: E731
    if move == "rigid":
        pos = R.move_rigid_wobble(pos, sel(R.mesh_mask(tris)), torch)
        pos = R.move_translate(pos, sel(R.emissive(tris)), torch)
    elif move == "lights":
        pos = R.move_translate(pos, sel(R.emissive(tris)), torch)
    elif move == "scale3":
        pos = R.move_scale(pos, sel(R.mesh_mask(tris)), torch, 3.0)
    elif move == "wall":
        pos = R.move_wall_wobble(pos, sel(R.wall_mask(tris)), torch)
    elif move != "none":
        raise KeyError(move)
    pos = pos.reshape(-1, 9).contiguous()
    assert pos.dtype == torch.float32
    return pos, pos.cpu().numpy()


def _moved(name, move):
    """(updated scene, nodes', tris', spheres, positions (n, 3, 3))."""
    nodes, tris, sph = _build(name)
    sc = ptamd.Scene(nodes, tris, sph)
    d_pos, h_pos = _move(tris, move)
    sc.update_vertices(d_pos)
    tris2 = R.restate_tris(tris, h_pos)
    return sc, R.refit_nodes(nodes, tris2), tris2, sph, h_pos.reshape(-1, 3, 3)


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


def _oracle_render(so, W, H, prm, cam=CAMERAS[0], window=None):
    import oracle_lib as O
    pos, rot, fov = cam
    ref, _ = so.render(O.make_camera(W, H, pos=pos, rot=rot, fovy_deg=fov),
                       O.make_params(W, H, prm.passes, prm.spp_per_pass, first_pass=prm.first_pass, window=window), 16)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "standin", "standin_spheres"])
def test_identity_update_changes_nothing(_gpu, name):
    import torch
    nodes, tris, sph = _build(name)
    sc = ptamd.Scene(nodes, tris, sph)
    cam, prm = ptamd.make_camera(*FRAMES[1]), params()
    rays = scene_rays8(4000, np.random.RandomState(5))
    before = _arrays(sc)
    frame, (aov, aprim), (hits, hprim) = sc.render(cam, prm), sc.aov(cam, prm), sc.raycast(rays)
    sc.set_mode(0)
    sc.enable_counters(True)
    counted = sc.render(cam, prm)
    cnt = sc.counters()
    assert cnt[1] > 0 and sc.tree_inflation() == 1.0
    pos = torch.from_numpy(R.positions(tris).reshape(-1, 9)).cuda()
    sc.update_vertices(pos)
    # every array as it was.  Compared as bits: no zero changed its sign either (a padded traversal box cannot hold a zero, and the
    # records are the host's own expressions)
    _assert_arrays(_arrays(sc), before, f"{name}: arrays after an identity update")
    assert sc.tree_inflation() == 1.0
    _assert_same(sc.render(cam, prm), counted, "counting render")
    assert np.array_equal(sc.counters(), cnt), (sc.counters(), cnt)      # same tree, same node fetches
    sc.enable_counters(False)
    sc.set_mode(1)
    _assert_same(sc.render(cam, prm), frame, "render")
    aov2, aprim2 = sc.aov(cam, prm)
    assert np.array_equal(aprim2, aprim) and np.array_equal(bits(aov2), bits(aov))
    hits2, hprim2 = sc.raycast(rays)
    assert np.array_equal(hprim2, hprim) and ((bits(hits2) == bits(hits)) | (np.isnan(hits2) & np.isnan(hits))).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name,move", CASES)
def test_result_arrays_after_a_move(_gpu, name, move):
    sc, nodes2, tris2, sph, _ = _moved(name, move)
    got, fresh = _arrays(sc), _arrays(ptamd.Scene(nodes2, tris2, sph))
    _assert_arrays(got, fresh, f"{name} {move} against a fresh upload", ("surf", "lights", "leafbox", "spheres"))
    assert np.array_equal(bits(got["leafbox"].reshape(-1, 8)), bits(R.leaf_boxes(nodes2)))
    tri = got["tri"].reshape(-1, 12)
    prim, leaf = tri[:, 3].view(np.int32), tri[:, 7].view(np.int32)
    assert np.array_equal(np.sort(prim), np.arange(len(tris2)))
    want_tri, want_pair = R.tri_records(tris2, nodes2, prim, leaf)
    _assert_arrays(got, {"tri": want_tri.ravel(), "tripair": want_pair.ravel()}, f"{name} {move} records from numpy", ("tri", "tripair"))
    before = _arrays(ptamd.Scene(*_build(name)))
    assert not np.array_equal(bits(got["surf"]), bits(before["surf"]))
    # the core box (scheduling hint): the box of the triangles classified small AT UPLOAD, at their new positions, padded by the
    # upload's rule from the moved scene box.  A fresh upload may classify differently, so numpy is the yardstick here.
    assert before["core"].size == (0 if name == "cornell" else 6)
    if before["core"].size:
        h_pos = tris2[:, 0:9].reshape(-1, 3, 3)
        want = R.core_box(_build(name)[1], h_pos)
        assert np.array_equal(got["core"], want), (got["core"], want)
        if move != "lights":
            assert not np.array_equal(got["core"], before["core"])
        # ... and the rule itself is the upload's: on the uploaded positions it gives the uploaded box
        assert np.array_equal(R.core_box(_build(name)[1], R.positions(_build(name)[1])), before["core"])


def _check_trees(sc, pos, refs_before, what):
    a = _arrays(sc)
    bad, seen, boxes = R.walk_nodes(a["nodes"], a["tri"], pos)
    assert not bad, (what, "nodes: boxes that are not the padded exact bounds", bad[:5])
    assert (seen == 1).all(), (what, "nodes: triangles not reached exactly once")
    qbad, qseen, scales_ok = R.walk_quad(a["quad"], a["tri"], pos)
    assert not qbad, (what, "quad: boxes that do not contain the padded bounds", qbad[:5])
    assert (qseen == 1).all() and scales_ok, what
    if refs_before is not None:
        assert np.array_equal(a["nodes"].reshape(-1, 16)[:, 12:16].view(np.uint32), refs_before[0]), what
        assert np.array_equal(a["quad"].reshape(-1, 16)[:, 4:8], refs_before[1]), what
    return boxes


def _refs(sc):
    return sc.dbg_array("nodes").reshape(-1, 16)[:, 12:16].view(np.uint32).copy(), sc.dbg_array("quad").reshape(-1, 16)[:, 4:8].copy()


@pytest.mark.gpu
@pytest.mark.parametrize("name,move", CASES)
def test_traversal_trees_after_a_move(_gpu, name, move):
    nodes, tris, sph = _build(name)
    refs = _refs(ptamd.Scene(nodes, tris, sph))
    sc, _, _, _, pos = _moved(name, move)
    boxes = _check_trees(sc, pos, refs, f"{name} {move}")
    # pt_scene_tree_inflation against the same sum in numpy.  Its float64 summation order is the device reduction's, not numpy's:
    # fewer than 10^6 non-negative terms, each float64 addition within 2^-53 relative, so 1e-12 relative covers the difference.
    ref_boxes = R.walk_nodes(*[ptamd.Scene(nodes, tris, sph).dbg_array(a) for a in ("nodes", "tri")], R.positions(tris))[2]
    assert len(boxes) == len(ref_boxes)
    want = R.area_sum(boxes) / R.area_sum(ref_boxes)
    got = sc.tree_inflation()
    print(f"{name} {move}: tree inflation {got:.6f}")
    assert abs(got - want) <= 1e-12 * want, (got, want)
    if move == "scale3":
        assert got > 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("name,move", CASES)
def test_render_after_a_move_is_the_fresh_scenes_and_the_oracles(_gpu, name, move):
    sc, nodes2, tris2, sph, _ = _moved(name, move)
    fresh, so = ptamd.Scene(nodes2, tris2, sph), _oracle(nodes2, tris2, sph)
    still = ptamd.Scene(*_build(name))
    prm = params()
    for W, H in FRAMES:
        cam = ptamd.make_camera(W, H)
        ref = _oracle_render(so, W, H, prm)
        assert np.isfinite(ref).all()
        assert not np.array_equal(bits(ref), bits(still.render(cam, prm)))      # the move is visible
        for mode in (1, 0):
            sc.set_mode(mode)
            got = sc.render(cam, prm)
            _assert_same(got, fresh.render(cam, prm), f"{name} {move} {W}x{H} mode {mode} against a fresh upload")
            _assert_same(got, ref, f"{name} {move} {W}x{H} mode {mode} against the oracle")
        sc.set_mode(1)


@pytest.mark.gpu
def test_every_entry_point_after_a_move(_gpu):
    import denoise_ref as D
    import oracle_lib as O
    name, move = "standin_spheres", "rigid"
    sc, nodes2, tris2, sph, _ = _moved(name, move)
    so = _oracle(nodes2, tris2, sph)
    W, H = FRAMES[0]
    cam, prm = ptamd.make_camera(W, H), params()
    ref = _oracle_render(so, W, H, prm)
    streams = ((W + 7) // 8) * ((H + 7) // 8) * 64 * prm.passes
    for rounds in (0, 1):
        sc.set_shade_rounds(rounds)
        for drain in (0, 80000, streams + 1):      # never, the default, and above the stream count: all of it in wf_drain
            sc.set_drain_threshold(drain)
            _assert_same(sc.render(cam, prm), ref, f"shade rounds {rounds} drain {drain}")
    sc.set_drain_threshold(80000)
    sc.set_shade_rounds(1)
    cams = [ptamd.make_camera(W, H, pos=p, rot_deg=r, fovy_deg=f) for p, r, f in CAMERAS]
    views = sc.render_views(cams, prm)
    for v, c in enumerate(CAMERAS):
        _assert_same(views[v], _oracle_render(so, W, H, prm, cam=c), f"view {v}")
    win = (5, 3, 37, 29)
    _assert_same(sc.render_window(cam, prm, win), ref[win[1]:win[3], win[0]:win[2]], "window")
    aov, aprim = sc.aov(cam, params(first_pass=5))
    want, wprim = D.aov_from_oracle(so, O.make_camera(W, H), W, H, PASSES, 5)
    assert np.array_equal(aprim, wprim) and np.array_equal(bits(aov), bits(want))
    rs = np.random.RandomState(77)
    rays = scene_rays8(20000, rs)
    h_o, p_o, _ = so.raycast(rays)
    h_g, p_g = sc.raycast(rays)
    assert np.array_equal(p_g, p_o) and ((bits(h_g) == bits(h_o)) | (np.isnan(h_g) & np.isnan(h_o))).all()
    assert (p_o >= 0).mean() > 0.7
    pts = h_o[p_o >= 0][:4000, 5:8]
    seeds = rs.randint(0, 2**32, (pts.shape[0], 2), dtype=np.uint64).astype(np.uint32)
    in5 = np.concatenate([pts, seeds.view(np.float32)], 1)
    got, want = sc.nee(in5), so.nee(in5)
    assert (want[:, 8:11].sum(1) > 0).sum() > 300
    assert np.array_equal(bits(got), bits(want))
    unmoved = _oracle(*_build(name)).nee(in5)
    assert not np.array_equal(bits(unmoved[:, 1:4]), bits(want[:, 1:4]))      # the lights did move


@pytest.mark.gpu
def test_sequence_of_updates_does_not_drift(_gpu):
    nodes, tris, sph = _build("standin_spheres")
    sc = ptamd.Scene(nodes, tris, sph)
    cam, prm = ptamd.make_camera(*FRAMES[0]), params()
    start, frame = _arrays(sc), sc.render(cam, prm)
    keep = []
    for move in ("rigid", "scale3", "none"):
        d_pos, _ = _move(tris, move)
        keep.append(d_pos)
        sc.update_vertices(d_pos)
    _assert_arrays(_arrays(sc), start, "A -> B -> original positions")
    assert sc.tree_inflation() == 1.0
    _assert_same(sc.render(cam, prm), frame, "render after A -> B -> original positions")


@pytest.mark.gpu
def test_frames_are_stored_as_given_or_kept(_gpu):
    import torch
    nodes, tris, _ = _build("standin")
    d_pos, h_pos = _move(tris, "rigid")
    frames = R.rotate_frames(tris, 25.0)
    tris2 = R.restate_tris(tris, h_pos, frames)
    nodes2 = R.refit_nodes(nodes, tris2)
    sc = ptamd.Scene(nodes, tris)
    sc.update_vertices(d_pos, frames=torch.from_numpy(frames).cuda())
    surf = sc.dbg_array("surf").reshape(-1, 48)
    assert np.array_equal(bits(surf[:, 9:36]), bits(frames))
    assert np.array_equal(bits(surf), bits(ptamd.Scene(nodes2, tris2).dbg_array("surf").reshape(-1, 48)))
    W, H = FRAMES[0]
    prm = params()
    _assert_same(sc.render(ptamd.make_camera(W, H), prm), _oracle_render(_oracle(nodes2, tris2, None), W, H, prm), "render with the given frames")
    # frames=None: untouched
    sc.update_vertices(d_pos)
    assert np.array_equal(bits(sc.dbg_array("surf").reshape(-1, 48)[:, 9:]), bits(surf[:, 9:]))
    plain = ptamd.Scene(nodes, tris)
    plain.update_vertices(d_pos)
    kept = plain.dbg_array("surf").reshape(-1, 48)
    assert np.array_equal(bits(kept[:, 9:]), bits(ptamd.Scene(nodes, tris).dbg_array("surf").reshape(-1, 48)[:, 9:]))
    assert np.array_equal(bits(kept[:, :9]), bits(surf[:, :9]))


@pytest.mark.gpu
def test_update_and_render_in_stream_order(_gpu):
    """Update and render enqueued on a non-default stream with no synchronisation in between."""
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
        sc.render_tiles(cam, prm, tiles.data_ptr(), work.data_ptr(), st.cuda_stream)
        ptamd.untile(tiles.data_ptr(), cam, 1, frame.data_ptr(), st.cuda_stream)
        got = frame.cpu().numpy()
    st.synchronize()
    tris2 = R.restate_tris(tris, h_pos)
    _assert_same(got, ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph).render(cam, prm), "stream-ordered update + render")


@pytest.mark.gpu
def test_spheres_host_positions_and_device_bytes(_gpu):
    nodes, tris, sph = _build("standin_spheres")
    sc = ptamd.Scene(nodes, tris, sph)
    W, H = FRAMES[0]
    cam, prm = ptamd.make_camera(W, H), params()
    bytes0 = sc.device_bytes
    assert bytes0 == ptamd.Scene(nodes, tris, sph).device_bytes
    moved = sph.copy()
    moved[:, 0:3] += np.float32([[-3, 2, 4], [2, 3, -1], [4, -6, 5]])
    moved[1, 3] = 3.5
    sc.update_spheres(moved)
    assert sc.device_bytes == bytes0      # no update of the vertices yet: no maps on the device
    assert np.array_equal(bits(sc.dbg_array("spheres")), bits(moved.ravel()))
    _assert_same(sc.render(cam, prm), _oracle_render(_oracle(nodes, tris, moved), W, H, prm), "moved spheres")
    assert not np.array_equal(bits(sc.render(cam, prm)), bits(ptamd.Scene(nodes, tris, sph).render(cam, prm)))
    bad = moved.copy()
    bad[2, 9] = 0.5      # an albedo component
    with pytest.raises(ptamd.PtError, match="material"):
        sc.update_spheres(bad)
    with pytest.raises(ptamd.PtError):
        sc.update_spheres(moved[:2])
    with pytest.raises(ptamd.PtError):
        ptamd.Scene(nodes, tris).update_spheres(moved)      # a scene without spheres
    assert np.array_equal(bits(sc.dbg_array("spheres")), bits(moved.ravel()))
    # numpy positions go through pt_scene_update_vertices_host: the same bits as the tensor path
    d_pos, h_pos = _move(tris, "rigid")
    sc.update_vertices(h_pos)
    assert sc.device_bytes > bytes0
    bytes1 = sc.device_bytes
    other = ptamd.Scene(nodes, tris, moved)
    other.update_vertices(d_pos)
    _assert_arrays(_arrays(sc), _arrays(other), "numpy against tensor positions")
    _assert_same(sc.render(cam, prm), other.render(cam, prm), "numpy against tensor positions")
    sc.update_vertices(h_pos.reshape(-1, 3, 3))
    assert sc.device_bytes == bytes1      # nothing is allocated after the first update


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"PTAMD_TREE": "0"}, {"PTAMD_LEAF": "4"}])
def test_other_builds_refit_as_well(_gpu, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    nodes, tris, sph = _build("standin")
    refs = _refs(ptamd.Scene(nodes, tris, sph))
    sc, nodes2, tris2, _, pos = _moved("standin", "rigid")
    _check_trees(sc, pos, refs, str(env))
    W, H = FRAMES[0]
    prm = params()
    _assert_same(sc.render(ptamd.make_camera(W, H), prm), _oracle_render(_oracle(nodes2, tris2, None), W, H, prm), str(env))


@pytest.mark.gpu
def test_single_leaf_scene_refits_too(_gpu):
    """Two emissive triangles: the traversal tree is one leaf and takes the special-case records of the build."""
    import torch
    a = np.float32([[-6, 12, -3], [-6, 12, -3]])
    b = np.float32([[6, 12, -3], [6, 24, -3]])
    c = np.float32([[6, 24, -3], [-6, 24, -3]])
    nodes, tris, _ = ptamd.build_bvh(make_prims(a, b, c, emit=(5, 5, 5)))
    assert len(nodes) == 1 and len(tris) == 2
    sc = ptamd.Scene(nodes, tris)
    before = _arrays(sc)
    assert before["nodes"].size == 16 and before["quad"].size == 16
    pos = torch.from_numpy(R.positions(tris).reshape(-1, 9)).cuda()
    sc.update_vertices(pos)
    _assert_arrays(_arrays(sc), before, "single leaf, identity")
    moved = (pos.reshape(-1, 3, 3) * 1.25 + torch.tensor([2.0, -1.0, 3.0], device="cuda")).reshape(-1, 9).contiguous()
    sc.update_vertices(moved)
    tris2 = R.restate_tris(tris, moved.cpu().numpy())
    nodes2 = R.refit_nodes(nodes, tris2)
    _assert_arrays(_arrays(sc), _arrays(ptamd.Scene(nodes2, tris2)), "single leaf, moved, against a fresh upload")
    _check_trees(sc, moved.cpu().numpy().reshape(-1, 3, 3), None, "single leaf")
    W, H = FRAMES[0]
    prm = params()
    got = sc.render(ptamd.make_camera(W, H), prm)
    assert got.max() > 0
    _assert_same(got, _oracle_render(_oracle(nodes2, tris2, None), W, H, prm), "single leaf, moved")
