"""Ray queries on an uploaded scene (pt_trace_rays, pt_trace_rays_host, Scene.trace_rays): the C-ABI surface and the argument checks on
the CPU; on the GPU the closest hit against the CPU oracle (prim, t and the 29-float surface record) and, at the scale of a frame,
against pt_dbg_raycast (the existing kernel, itself pinned to the oracle), the any-hit contract, the device path on a non-default
stream, stream order behind a vertex update, the absence of side effects on renders, and termination on odd rays.  Bits everywhere
(NaN == NaN for the surface record); no tolerances.

What the oracle alone says about the ray sets, on the CPU (20,000 scene_rays8 rays per scene, seeds as below): hit share 0.758 in
the Cornell room, 0.796 with the lat_lon 24 stand-in and the test spheres (1,911 sphere hits), 0.783 with kind 1 and kind 2 at
lat_lon 187; of 20,000 set-C segments the oracle lets 23.2 %, 8.4 % and 7.6 % hit in the three scenes with a mesh (fewer than there
are: LONG_DIRECTIONS below; the Cornell room is empty, no segment between two points inside it hits, so set C is not run there)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dynamic_ref as R
import ptamd
import query_ref as Q
from scenes_util import scene_rays8
from scenes_util import test_spheres as make_test_spheres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pathtrace-on-cuda_amd")
SCENES = {      # name: (kind, lat_lon, spheres?, seed of its scene_rays8 set)
    "cornell": (0, 187, False, 11),
    "standin24_spheres": (1, 24, True, 12),
    "kind1_187": (1, 187, False, 13),
    "kind2_187": (2, 187, False, 14),
}
N_RAYS = 20000
# LONG_DIRECTIONS.  Set C's directions are whole segments (|dir| ~ 30).  The reference's box test compares an entry distance measured with
# the NORMALISED inverse direction against the un-scaled closest t (CudaUtil.cuh:65-88), which is harmless while |(1/dx, 1/dy, 1/dz)| >= 1
# (every direction with components in [-1, 1]: the scaled distance is then the smaller one) but, for longer directions, drops hits inside
# [0, tmax] depending on the order of its own traversal: on the lat_lon 24 scene the oracle answers 2,454 of 20,000 set-C segments differently
# from its own answer for the same segment with the direction normalised (2,253 hits dropped, 201 a farther primitive; every one of them
# has |1/dir| < 1, checked on the CPU).
# The device keeps the order-independent answer, as pt_dbg_raycast always has (include/pt_api.h), so set C is compared with
# pt_dbg_raycast and between the query kernels, and the oracle judges the rays with |1/dir| >= 1.
FRAME = (1920, 1080)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits_or_nan(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound():
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in ("pt_trace_rays", "pt_trace_rays_host"):
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    assert callable(ptamd.Scene.trace_rays)
    assert "#define PT_QUERY_CLOSEST 0" in hdr and "#define PT_QUERY_ANY     1" in hdr
    assert (ptamd.QUERY_CLOSEST, ptamd.QUERY_ANY) == (0, 1)


def test_ray_hit_is_eight_bytes_in_c_and_in_python(tmp_path):
    assert C.sizeof(ptamd.PtRayHit) == 8 and ptamd.HIT_DTYPE.itemsize == 8
    assert ptamd.PtRayHit.t.offset == 0 and ptamd.PtRayHit.prim.offset == 4
    src = tmp_path / "hit.c"
    src.write_text('#include "pt_api.h"\n_Static_assert(sizeof(PtRayHit) == 8, "PtRayHit");\n'
                   '_Static_assert(PT_QUERY_CLOSEST == 0 && PT_QUERY_ANY == 1, "modes");\n')
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)


def test_bad_arguments_are_rejected_before_any_device_call():
    """A fake scene and fake device addresses: never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    base = 1 << 40
    scene, rays, hits, surf = (C.c_void_p(base + (i << 20)) for i in range(4))
    off = lambda p, k: C.c_void_p(p.value + k)      # noqa: E731
    dev = [
        ("NULL scene", (None, rays, 64, 0, hits, None)),
        ("NULL rays", (scene, None, 64, 0, hits, None)),
        ("NULL hits", (scene, rays, 64, 0, None, None)),
        ("n < 0", (scene, rays, -1, 0, hits, None)),
        ("mode 2", (scene, rays, 64, 2, hits, None)),
        ("mode -1", (scene, rays, 64, -1, hits, None)),
        ("rays + 4", (scene, off(rays, 4), 64, 0, hits, None)),
        ("rays + 8", (scene, off(rays, 8), 64, 0, hits, None)),
        ("hits + 4", (scene, rays, 64, 0, off(hits, 4), None)),
        ("surface + 2", (scene, rays, 64, 0, hits, off(surf, 2))),
        ("surface with any-hit", (scene, rays, 64, 1, hits, surf)),
        ("n = 0 does not excuse a NULL", (scene, None, 0, 0, hits, None)),
    ]
    for what, a in dev:
        assert l.pt_trace_rays(*a, None) == -1, what
        assert b"pt_trace_rays:" in l.pt_last_error(), (what, l.pt_last_error())
    h_rays, h_hits, h_surf = np.zeros((64, 8), np.float32), np.zeros(64, ptamd.HIT_DTYPE), np.zeros((64, 29), np.float32)
    P = ptamd._ptr
    host = [
        ("NULL scene", (None, P(h_rays), 64, 0, P(h_hits), None)),
        ("NULL rays", (scene, None, 64, 0, P(h_hits), None)),
        ("NULL hits", (scene, P(h_rays), 64, 0, None, None)),
        ("n < 0", (scene, P(h_rays), -5, 0, P(h_hits), None)),
        ("mode 7", (scene, P(h_rays), 64, 7, P(h_hits), None)),
        ("surface with any-hit", (scene, P(h_rays), 64, 1, P(h_hits), P(h_surf))),
    ]
    for what, a in host:
        assert l.pt_trace_rays_host(*a) == -1, what
        assert b"pt_trace_rays_host:" in l.pt_last_error(), (what, l.pt_last_error())
    # nothing to do: PT_OK, still without touching the scene or the device
    assert l.pt_trace_rays(scene, rays, 0, 0, hits, None, None) == 0
    assert l.pt_trace_rays(scene, rays, 0, 1, hits, None, None) == 0
    assert l.pt_trace_rays(scene, rays, 0, 0, hits, surf, None) == 0
    assert l.pt_trace_rays_host(scene, P(h_rays), 0, 0, P(h_hits), None) == 0


class _FakeScene:
    n_tris, device, _h = 5, 0, C.c_void_p(1 << 40)


def test_wrapper_checks_shape_dtype_and_device_on_the_host():
    import torch
    fake = _FakeScene()
    tr = ptamd.Scene.trace_rays
    for rays in (np.zeros((4, 7), np.float32), np.zeros(32, np.float32), np.zeros((2, 4, 8), np.float32)):
        with pytest.raises(ptamd.PtError):
            tr(fake, rays)
    for rays in (torch.zeros((5, 8)), torch.zeros((5, 8), dtype=torch.float64), torch.zeros((5, 7)), torch.zeros((8, 5)).t(), [[0.0] * 8]):
        with pytest.raises(ptamd.PtError):      # a CPU tensor, a wrong dtype, a wrong shape, not contiguous, not an array
            tr(fake, rays)
    with pytest.raises(ptamd.PtError):
        tr(fake, np.zeros((4, 8), np.float32), any_hit=True, surface=True)
    t, prim = tr(fake, np.zeros((0, 8), np.float32))      # n = 0: PT_OK without a device
    assert t.shape == (0,) and prim.shape == (0,) and t.dtype == np.float32 and prim.dtype == np.int32


def test_ray_sets_are_seeded_and_well_formed():
    c1, c2 = Q.set_c(1000, np.random.RandomState(5)), Q.set_c(1000, np.random.RandomState(5))
    assert np.array_equal(bits(c1), bits(c2)) and c1.shape == (1000, 8) and (c1[:, 6] == 0).all() and (c1[:, 7] == 1).all()
    px = Q.pixel_list(7, 3)
    assert px.shape == (21, 3) and tuple(px[8]) == (1, 1, 0)
    for r in (Q.sphere_only_rays(), Q.odd_rays()):
        assert r.dtype == np.float32 and r.shape[1] == 8 and (r[:, 6] == 0).all()


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
    """(nodes, tris, spheres) of a test scene."""
    if name not in _BUILT:
        kind, lat_lon, with_spheres, _ = SCENES[name]
        nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(kind, lat_lon))
        _BUILT[name] = (nodes, tris, make_test_spheres() if with_spheres else None)
    return _BUILT[name]


def _n_prims(name):
    _, tris, sph = _build(name)
    return len(tris) + (0 if sph is None else len(sph))


def _scene(name):
    return ptamd.Scene(*_build(name))


def _rays(name):
    return scene_rays8(N_RAYS, np.random.RandomState(SCENES[name][3]))


def _oracle(name, rays):
    import oracle_lib as O
    nodes, tris, sph = _build(name)
    hits, prim, _ = O.Scene(nodes.tobytes(), tris, sph).raycast(rays)
    return hits, prim


def _assert_closest(got, hits_o, prim_o, what):
    """(t, prim, surface) of a closest-hit query against the oracle's HIT records."""
    t, prim, surf = got
    assert np.array_equal(prim, prim_o), f"{what}: {(prim != prim_o).sum()} prims differ, first at {np.nonzero(prim != prim_o)[0][:5]}"
    assert np.array_equal(bits(t), bits(hits_o[:, 1])), f"{what}: t differs at {np.nonzero(bits(t) != bits(hits_o[:, 1]))[0][:5]}"
    assert (t[prim_o < 0] == 0).all() and (prim[prim_o < 0] == -1).all(), what
    ok = same_bits_or_nan(surf, hits_o).all(1)
    assert ok.all(), f"{what}: {(~ok).sum()} surface records differ, first at {np.nonzero(~ok)[0][:5]}"
    assert (surf[prim_o < 0] == 0).all(), what


def _assert_any(any_t, any_prim, closest_t, closest_prim, rays, n_prims, what):
    hit = closest_prim >= 0
    assert np.array_equal(any_prim >= 0, hit), f"{what}: {((any_prim >= 0) != hit).sum()} rays decide differently from the closest-hit query"
    assert (any_prim[~hit] == -1).all() and (any_t[~hit] == 0).all(), what
    assert (any_prim < n_prims).all(), what
    assert (any_t[hit] <= rays[hit, 7]).all() and (any_t[hit] >= 0).all(), what
    assert (any_t[hit] >= closest_t[hit]).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_closest_hit_is_the_oracles(_gpu, name):
    rays = _rays(name)
    hits_o, prim_o = _oracle(name, rays)
    share = (prim_o >= 0).mean()
    print(f"{name}: oracle hit share {share:.4f}")
    assert 0.7 < share < 0.99      # hits and misses both
    sc = _scene(name)
    _assert_closest(sc.trace_rays(rays, surface=True), hits_o, prim_o, name)
    t, prim = sc.trace_rays(rays)      # without the surface pass: the same 8 bytes
    assert np.array_equal(prim, prim_o) and np.array_equal(bits(t), bits(hits_o[:, 1]))
    if SCENES[name][2]:
        assert (prim_o >= len(_build(name)[1])).sum() > 1000      # spheres are hit


CHILD = r"""
import sys
import numpy as np
import ptamd
import query_ref as Q
from scenes_util import scene_rays8, test_spheres
kind, lat_lon, seed, out = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(kind, lat_lon))
sc = ptamd.Scene(nodes, tris, test_spheres())
rays = np.concatenate([scene_rays8(20000, np.random.RandomState(seed)), Q.set_c(20000, np.random.RandomState(seed + 100)), Q.sphere_only_rays()])
t, prim, surf = sc.trace_rays(rays, surface=True)
at, aprim = sc.trace_rays(rays, any_hit=True)
np.savez(out, rays=rays, t=t, prim=prim, surf=surf, at=at, aprim=aprim)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("knob", ["PTAMD_QUERY_QUAD=0"])
def test_binary_tree_fallback_gives_the_oracles_bits(_gpu, tmp_path, knob):
    """The binary-tree fallback (taken by itself only when the 4-wide walk does not fit the kernel's stack), forced by its knob in a fresh
    process (the knob is read when a scene is created)."""
    name = "standin24_spheres"
    kind, lat_lon, _, seed = SCENES[name]
    out = str(tmp_path / "child.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]))
    env[knob.split("=")[0]] = knob.split("=")[1]
    subprocess.run([sys.executable, "-c", CHILD, str(kind), str(lat_lon), str(seed), out], check=True, env=env, timeout=600)
    g = np.load(out)
    rays = g["rays"]
    assert np.array_equal(bits(rays[:N_RAYS]), bits(_rays(name)))
    got = (g["t"], g["prim"], g["surf"])
    unit = np.r_[0:N_RAYS, 2 * N_RAYS:len(rays)]      # scene_rays8 and the sphere rays against the oracle
    hits_o, prim_o = _oracle(name, rays[unit])
    _assert_closest(tuple(x[unit] for x in got), hits_o, prim_o, knob)
    # the long directions of set C (LONG_DIRECTIONS above) against the parity hook and against this process's default kernel
    hits_d, prim_d = _scene(name).raycast(rays)
    _assert_closest(got, hits_d, prim_d, knob + " against pt_dbg_raycast")
    for x, y in zip(got, _scene(name).trace_rays(rays, surface=True)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    _assert_any(g["at"], g["aprim"], g["t"], g["prim"], rays, _n_prims(name), knob)


_FRAME_SETS = {}


def _frame_sets():
    """Sets A and B of a 1920 x 1080 frame on kind 1, lat_lon 187, and what pt_dbg_raycast says about them: {set: (rays, hits29, prim)}."""
    if not _FRAME_SETS:
        W, H = FRAME
        sc = _scene("kind1_187")
        a = Q.set_a(ptamd.dbg_pixel_dir(ptamd.make_camera(W, H), Q.pixel_list(W, H)))
        hits_a, prim_a = sc.raycast(a)
        b = Q.set_b(prim_a, hits_a, np.random.RandomState(21))
        _FRAME_SETS["A"] = (a, hits_a, prim_a)
        _FRAME_SETS["B"] = (b,) + sc.raycast(b)
    return _FRAME_SETS


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["A", "B"])
def test_closest_hit_at_frame_scale_is_pt_dbg_raycasts(_gpu, which):
    rays, hits_d, prim_d = _frame_sets()[which]
    n = len(rays) - 7                      # 2,073,593: not a multiple of 64
    assert n % 64 != 0 and n > 2_000_000
    share = (prim_d >= 0).mean()
    print(f"set {which}: {len(rays)} rays, hit share {share:.4f}")
    assert share > 0.05
    sc = _scene("kind1_187")
    got = sc.trace_rays(rays[:n], surface=True)
    _assert_closest(got, hits_d[:n], prim_d[:n], f"set {which}")
    again = sc.trace_rays(rays[:n], surface=True)
    for x, y in zip(got, again):           # two calls, the same bits
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    for lo, m in ((0, 1), (1000, 63), (77, 65), (500000, 64 * 1000 + 1)):
        _assert_closest(sc.trace_rays(rays[lo:lo + m], surface=True), hits_d[lo:lo + m], prim_d[lo:lo + m], f"set {which}, n = {m}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_any_hit_decides_as_the_closest_hit_does(_gpu, name):
    sc = _scene(name)
    sets = [("scene_rays8", _rays(name))]
    if name != "cornell":                  # the Cornell room is empty: no segment inside it hits anything (module docstring)
        sets.append(("set C", Q.set_c(200000 if name == "kind1_187" else N_RAYS, np.random.RandomState(SCENES[name][3] + 100))))
    for what, rays in sets:
        t, prim = sc.trace_rays(rays)
        hits_d, prim_d = sc.raycast(rays)      # set C's long directions: the closest hit is the parity hook's (LONG_DIRECTIONS)
        assert np.array_equal(prim, prim_d) and np.array_equal(bits(t), bits(hits_d[:, 1]))
        at, aprim = sc.trace_rays(rays, any_hit=True)
        share = (prim >= 0).mean()
        print(f"{name} {what}: hit share {share:.4f}, any-hit returned the closest in {(aprim == prim)[prim >= 0].mean():.4f} of the hits")
        assert 0.02 < share < 0.99
        _assert_any(at, aprim, t, prim, rays, _n_prims(name), f"{name} {what}")


@pytest.mark.gpu
def test_any_hit_sees_a_sphere_that_alone_blocks_the_ray(_gpu):
    name = "standin24_spheres"
    n_tris = len(_build(name)[1])
    rays = Q.sphere_only_rays()
    _, prim_o = _oracle(name, rays)
    assert list(prim_o) == [n_tris + 2, n_tris + 2, -1, -1]      # the oracle: the metal sphere and nothing else; short of it, nothing
    sc = _scene(name)
    t, prim = sc.trace_rays(rays)
    at, aprim = sc.trace_rays(rays, any_hit=True)
    assert np.array_equal(prim, prim_o)
    assert list(aprim) == [n_tris + 2, n_tris + 2, -1, -1] and np.array_equal(bits(at), bits(t))


@pytest.mark.gpu
def test_device_path_on_a_stream_equals_the_host_path(_gpu):
    import torch
    name = "standin24_spheres"
    rays = np.concatenate([_rays(name), Q.set_c(N_RAYS + 5, np.random.RandomState(3))])
    sc = _scene(name)
    want = sc.trace_rays(rays, surface=True)
    want_any = sc.trace_rays(rays, any_hit=True)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    bytes0 = sc.device_bytes
    with torch.cuda.stream(st):
        d_rays = torch.from_numpy(rays).to(dev)
        got = sc.trace_rays(d_rays, surface=True, stream_ptr=st.cuda_stream)
        got_any = sc.trace_rays(d_rays, any_hit=True, stream_ptr=st.cuda_stream)
        assert sc.device_bytes == bytes0       # a query allocates nothing
        for x in got + got_any:
            assert x.device == dev and x.shape[0] == len(rays)
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].shape == (len(rays), 29)
        host = [x.cpu().numpy() for x in got + got_any]
    st.synchronize()
    for x, y in zip(host[:3], want):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), y.view(np.uint32))
    # any-hit: which hit is unspecified in general, but one build answers one batch the same way on either path
    assert np.array_equal(host[4] >= 0, want_any[1] >= 0)
    _assert_any(host[3], host[4], want[0], want[1], rays, _n_prims(name), "device path")


@pytest.mark.gpu
def test_query_after_an_update_on_the_same_stream_sees_the_moved_geometry(_gpu):
    import torch
    nodes, tris, sph = _build("standin24_spheres")
    rays = np.concatenate([_rays("standin24_spheres"), Q.set_c(N_RAYS, np.random.RandomState(4))])
    sc = ptamd.Scene(nodes, tris, sph)
    before = sc.trace_rays(rays)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        pos = torch.from_numpy(R.positions(tris)).to(dev)
        sel = torch.from_numpy(R.mesh_mask(tris)).to(dev)
        d_pos = R.move_rigid_wobble(pos, sel, torch).reshape(-1, 9).contiguous()
        d_rays = torch.from_numpy(rays).to(dev)
        sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
        got = sc.trace_rays(d_rays, surface=True, stream_ptr=st.cuda_stream)
        got_any = sc.trace_rays(d_rays, any_hit=True, stream_ptr=st.cuda_stream)
        host = [x.cpu().numpy() for x in got + got_any]
        h_pos = d_pos.cpu().numpy()
    st.synchronize()
    tris2 = R.restate_tris(tris, h_pos)
    fresh = ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph)
    want = fresh.trace_rays(rays, surface=True)
    for x, y in zip(host[:3], want):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint32), y.view(np.uint32))
    _assert_any(host[3], host[4], want[0], want[1], rays, len(tris) + len(sph), "after the update")
    moved = (want[1] != before[1]) | (bits(want[0]) != bits(before[0]))
    print(f"the move changed {moved.mean():.4f} of the results")
    assert moved.mean() > 0.02      # the move is seen at all


@pytest.mark.gpu
def test_queries_leave_renders_and_the_parity_hook_alone(_gpu):
    import torch
    name = "standin24_spheres"
    rays = _rays(name)
    W, H = 100, 52
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=3, spp_per_pass=4)
    img_q = _scene(name).render(cam, prm)               # a scene that never sees a query
    sc = _scene(name)
    sc.trace_rays(rays)                                   # before the first render, too
    sc.enable_counters(True)
    img = sc.render(cam, prm)
    state = (sc.last_iterations(), sc.counters().copy(), sc.last_render_ms())
    ray0 = sc.raycast(rays)
    d_rays = torch.from_numpy(rays).cuda()
    for _ in range(2):
        sc.trace_rays(rays, surface=True)
        sc.trace_rays(rays, any_hit=True)
        sc.trace_rays(d_rays, surface=True)
        sc.trace_rays(d_rays, any_hit=True)
    torch.cuda.synchronize()
    assert sc.last_iterations() == state[0] and np.array_equal(sc.counters(), state[1]) and sc.last_render_ms() == state[2]
    ray1 = sc.raycast(rays)
    assert np.array_equal(ray0[1], ray1[1]) and same_bits_or_nan(ray0[0], ray1[0]).all()
    img2 = sc.render(cam, prm)
    assert same_bits_or_nan(img, img2).all() and same_bits_or_nan(img, img_q).all()
    assert sc.last_iterations() == state[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["standin24_spheres", "kind1_187"])
def test_odd_rays_end_and_leave_their_neighbours_alone(_gpu, name):
    """Zero directions, NaN and inf components mixed into a batch: the call returns (the walk is a depth-first search over a finite tree,
    whatever the floats are), every prim is in range and the other rays' results are those of the batch without them."""
    good = _rays(name)[:4096]
    odd = Q.odd_rays()
    rs = np.random.RandomState(9)
    at = np.sort(rs.choice(len(good), 40 * len(odd), replace=False))      # every odd ray forty times, scattered over the waves
    mixed = good.copy()
    mixed[at] = np.tile(odd, (40, 1))
    keep = np.ones(len(good), bool)
    keep[at] = False
    sc = _scene(name)
    n_prims = _n_prims(name)
    want = sc.trace_rays(good, surface=True)
    got = sc.trace_rays(mixed, surface=True)
    assert ((got[1] >= -1) & (got[1] < n_prims)).all()
    for x, y in zip(got, want):
        assert np.array_equal(x[keep].view(np.uint32), y[keep].view(np.uint32))
    want_any = sc.trace_rays(good, any_hit=True)
    got_any = sc.trace_rays(mixed, any_hit=True)
    assert ((got_any[1] >= -1) & (got_any[1] < n_prims)).all()
    assert np.array_equal(got_any[1][keep] >= 0, want_any[1][keep] >= 0)
