"""The NEE verdict formed where the shadow ray ends (pt_shade.h: nee_verdict).

A shadow ray's hit record carries (t, the primitive if the hit is the sampled light point, else -1): wf_trace's epilogue forms it from the
ray it still holds and the light point it fetches there, wf_drain / the one-kernel mode / the pt_dbg_nee hook form it right after their
own trace, and the shade step reads neither the shadow ray nor the light point.  No floating-point operation changes, so every frame
here must be the oracle's bit for bit, on every path a shadow ray can take: each shade schedule, early shade, wf_drain, suspended and
resumed traversals, a batch of views and the caller's own rays, and light tables of 1, 32 and 40 records (a copy of the first 32 in
LDS was measured beside this change and not kept, DESIGN.md 5.6: the cases stay, as a table that small and one that large).
"""
import numpy as np
import pytest

import oracle_lib as O
import ptamd
from scenes_util import V_EMIT, make_prims, scene_rays8
from scenes_util import test_spheres as make_test_spheres

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(got, want, what):
    same = bits(got) == bits(want)
    print(f"{what}: bit-identical floats {same.mean():.6f}")
    assert got.shape == want.shape and same.all(), what


@pytest.fixture(scope="module", autouse=True)
def _contract():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    O.set_libm(1)            # the pinned contract: correctly rounded float transcendentals
    yield


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. lit, shadowed and grazing NEE terms on the stand-in scene, every way a step can be scheduled
# ---------------------------------------------------------------------------------------------------------------------------------
W1, H1, PASSES1, SPP1 = 64, 64, 2, 8
STREAMS1 = W1 * H1 * PASSES1


@pytest.fixture(scope="module")
def standin():
    """Stand-in scene of 3,120 triangles + the room: (GPU scene, oracle frame), the reference computed once."""
    prims = ptamd.gen_scene(1, 40)
    nodes, tris, _ = ptamd.build_bvh(prims)
    assert 2000 < tris.shape[0] < 8000
    ref, _ = O.Scene(nodes.tobytes(), tris).render(O.make_camera(W1, H1), O.make_params(W1, H1, PASSES1, SPP1), 16)
    assert np.isfinite(ref).all() and ref.mean() > 0.05
    ref.setflags(write=False)
    return ptamd.Scene(nodes, tris), ref


@pytest.mark.parametrize("drain", [0, 1 << 30], ids=["pipeline_to_the_end", "every_verdict_in_wf_drain"])
@pytest.mark.parametrize("early", [False, True], ids=["one_launch_step", "early_shade"])
@pytest.mark.parametrize("rounds", [0, 1], ids=["one_round", "two_rounds"])
def test_frame_is_the_oracles_on_every_schedule(standin, rounds, early, drain):
    sc, ref = standin
    sc.set_mode(1)
    sc.set_shade_rounds(rounds)
    sc.set_early_shade(STREAMS1 if early else 0)      # on: the limit is the render's own stream count
    sc.set_drain_threshold(drain)                      # above the stream count: wf_drain takes every stream at the first poll
    img = sc.render(ptamd.make_camera(W1, H1), ptamd.default_params(passes=PASSES1, spp_per_pass=SPP1))
    _assert_same(img, ref, f"shade rounds {rounds}, early shade {early}, drain threshold {drain}")


def test_one_kernel_mode_is_the_oracles(standin):
    sc, ref = standin
    sc.set_mode(0)
    img = sc.render(ptamd.make_camera(W1, H1), ptamd.default_params(passes=PASSES1, spp_per_pass=SPP1))
    sc.set_mode(1)
    _assert_same(img, ref, "one-kernel mode")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. light tables of 1, 32 and 40 records
# ---------------------------------------------------------------------------------------------------------------------------------
def cornell_with_lights(n):
    """The Cornell room of pt_scene_gen(0) with its ceiling light (a 10 x 10 square) cut into n triangles: n / 2 strips of two, or, for
    n = 1, its first triangle alone."""
    room = ptamd.gen_scene(0)
    lit = room.reshape(-1, 3, 28)[:, 0, V_EMIT] > 0
    assert lit.sum() == 2
    emit = tuple(float(x) for x in room.reshape(-1, 3, 28)[lit][0, 0, V_EMIT:V_EMIT + 3])
    y = 39.98
    if n == 1:
        a, b, c = [(-5, y, -5)], [(5, y, -5)], [(5, y, 5)]
    else:
        assert n % 2 == 0
        xs = np.linspace(-5.0, 5.0, n // 2 + 1)
        a, b, c = [], [], []
        for x0, x1 in zip(xs[:-1], xs[1:]):
            a += [(x0, y, -5), (x0, y, -5)]; b += [(x1, y, -5), (x1, y, 5)]; c += [(x1, y, 5), (x0, y, 5)]
    lights = make_prims(np.float32(a), np.float32(b), np.float32(c), albedo=(0, 0, 0), emit=emit)
    assert (lights.reshape(-1, 3, 28)[:, 0, 4] < 0).all()      # flat normals point down, like the room's own light
    return np.ascontiguousarray(np.concatenate([room[~lit], lights]), np.float32)


@pytest.mark.parametrize("n_lights", [1, 32, 40])
def test_light_counts(n_lights):
    """The Cornell room with its light cut into 40, 32 and 1 triangles: a wave's lanes draw many different lights, or all the same one."""
    nodes, tris, _ = ptamd.build_bvh(cornell_with_lights(n_lights))
    sc = ptamd.Scene(nodes, tris)
    assert sc.num_lights == n_lights
    W, H = 64, 64
    ref, _ = O.Scene(nodes.tobytes(), tris).render(O.make_camera(W, H), O.make_params(W, H, 1, 8), 16)
    assert np.isfinite(ref).all() and ref.mean() > 0.05
    for drain in (0, 1 << 30):      # wf_shade to the end / wf_drain from the first poll
        sc.set_drain_threshold(drain)
        _assert_same(sc.render(ptamd.make_camera(W, H), ptamd.default_params(passes=1, spp_per_pass=8)), ref, f"{n_lights} lights, drain threshold {drain}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. shadow rays that are suspended and resumed: the verdict belongs to the launch that finishes the ray
# ---------------------------------------------------------------------------------------------------------------------------------
_SLICED_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
from test_needle_scene import SLICED, SLICED_H, SLICED_W, camera, params, scene
sc = scene()
n = SLICED_W * SLICED_H * SLICED["passes"]
out = {}
for name, drain in (("pipeline", 0), ("half", n // 2), ("first_poll", 1 << 30)):
    sc.set_drain_threshold(drain)
    out[name] = sc.render(camera(SLICED_W, SLICED_H), params(**SLICED))
    out["it_" + name] = sc.last_iterations()
np.savez(sys.argv[3], **out)
"""


def test_suspended_shadow_rays(tmp_path):
    """The needle scene at the node budget of test_needle_scene's time-slicing test (32 steps per launch, a child process: the knobs are
    read once): every ray is suspended and resumed some thirty times, shadow rays included.  To the end in the pipeline, and handed to
    wf_drain at the first poll (every primary ray still suspended) and once half the streams have retired (what is in flight then is
    suspended path and shadow rays: wf_drain retraces them and forms their verdicts)."""
    from test_needle_scene import SLICED, SLICED_BM, SLICED_H, SLICED_W, _child, build
    from scenes_util import NEEDLE_CAMERA_POS
    _, nodes, tris, _ = build()
    ref, _ = O.Scene(nodes.tobytes(), tris).render(O.make_camera(SLICED_W, SLICED_H, pos=NEEDLE_CAMERA_POS),
                                                   O.make_params(SLICED_W, SLICED_H, SLICED["passes"], SLICED["spp_per_pass"], max_bounce=SLICED["max_bounce"]), 16)
    assert np.isfinite(ref).all() and (ref > 0).all(-1).mean() > 0.5
    out = tmp_path / "sliced.npz"
    _child(tmp_path, _SLICED_CHILD, [out], {"PTAMD_BS": "31", "PTAMD_LB": "0", "PTAMD_BM": str(SLICED_BM)})
    g = np.load(out)
    print("iterations: pipeline to the end %d, wf_drain from half the streams %d, from the first poll %d" % (g["it_pipeline"], g["it_half"], g["it_first_poll"]))
    assert int(g["it_first_poll"]) == 16 < int(g["it_half"]) < int(g["it_pipeline"])
    for name in ("pipeline", "half", "first_poll"):
        _assert_same(g[name], ref, f"node budget {SLICED_BM}, {name}")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the other pixel sources: the ViewTable and RayTable instantiations of the same step
# ---------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_two_views():
    from test_views import CAMERAS, _build, _singles, cams, params
    nodes, tris, _ = _build("standin")
    sc = ptamd.Scene(nodes, tris)
    W, H = 64, 36
    cs, prm = cams(W, H, (0, 1)), params()
    got = sc.render_views(cs, prm)
    _assert_same(got, _singles(sc, cs, prm), "two views against one pt_render each")
    so = O.Scene(nodes.tobytes(), tris)
    for v in (0, 1):
        pos, rot, fov = CAMERAS[v]
        ref, _ = so.render(O.make_camera(W, H, pos=pos, rot=rot, fovy_deg=fov), O.make_params(W, H, prm.passes, prm.spp_per_pass), 16)
        _assert_same(got[v], ref, f"view {v} against the oracle")


def test_rays_with_finite_tmax():
    """4,096 rays, every one with a finite tmax: 1.5 t for a ray that hits (nothing changes: the camera's frame, and the oracle's), 0.5 t for
    every fourth of them (the ambient term), 500 for one that misses."""
    from test_rays import SPP, cam_rays, params
    from test_views import CAMERAS, _build
    nodes, tris, _ = _build("standin")
    sc = ptamd.Scene(nodes, tris)
    W, H = 64, 64
    rays, seeds, stride = cam_rays(W, H, 0, 0)
    assert rays.shape == (4096, 8)
    t, prim = sc.trace_rays(np.array(rays))
    hit = prim >= 0
    cut = hit & (np.arange(len(rays)) % 4 == 0)
    mine = np.array(rays)
    mine[hit, 7] = t[hit] * np.float32(1.5)
    mine[cut, 7] = t[cut] * np.float32(0.5)
    mine[~hit, 7] = 500.0
    assert hit.sum() > 2048 and np.isfinite(mine[:, 7]).all() and (mine[:, 7] < 999999.0).all()
    got = sc.render_rays(mine, params(), seeds, stride)
    pos, rot, fov = CAMERAS[0]
    ref, _ = O.Scene(nodes.tobytes(), tris).render(O.make_camera(W, H, pos=pos, rot=rot, fovy_deg=fov), O.make_params(W, H, 1, SPP), 16)
    _assert_same(got[~cut], ref.reshape(-1, 3)[~cut], "rays that end behind their hit: the oracle's frame")
    acc = np.float32(0)
    for _ in range(SPP):
        acc = np.float32(acc + np.float32(np.float32(1) * np.float32(0.1)))
    _assert_same(got[cut], np.full((int(cut.sum()), 3), np.float32(acc / np.float32(SPP)), np.float32), "rays cut short: the ambient term")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the verdict's arithmetic, row by row
# ---------------------------------------------------------------------------------------------------------------------------------
def test_nee_table_through_the_shared_verdict():
    """pt_dbg_nee (one NEE sample and its visibility per row, through nee_sample and nee_verdict) against the oracle on about
    6,000 surface points: hit points of rays cast into the stand-in scene with the test spheres, points just under the light, points
    just under the ceiling beside it."""
    prims = ptamd.gen_scene(1, 24)
    nodes, tris, _ = ptamd.build_bvh(prims)
    sph = make_test_spheres()
    sg, so = ptamd.Scene(nodes, tris, sph), O.Scene(nodes.tobytes(), tris, sph)
    rs = np.random.RandomState(23)
    hits, prim, _ = so.raycast(scene_rays8(6200, rs))
    pts = hits[prim >= 0][:, 5:8]
    pts = np.concatenate([pts, np.stack([rs.uniform(-5, 5, 300), np.full(300, 39.98), rs.uniform(-5, 5, 300)], 1),
                          np.stack([rs.uniform(-20, 20, 300), np.full(300, 39.999), rs.uniform(-20, 20, 300)], 1)]).astype(np.float32)
    assert 5000 < len(pts) < 7000
    seeds = rs.randint(0, 2**32, (pts.shape[0], 2), dtype=np.uint64).astype(np.uint32)
    in5 = np.concatenate([pts, seeds.view(np.float32)], 1)
    got, want = sg.nee(in5), so.nee(in5)
    lit = want[:, 8:11].sum(1) > 0
    assert lit.sum() > 1000 and (~lit).sum() > 1000      # lit and shadowed rows both present
    _assert_same(got, want, "NEE table")
