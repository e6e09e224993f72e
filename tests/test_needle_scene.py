"""Parity on scenes_util.needle_scene: 16384 long thin triangles whose boxes all overlap.  The tree is shallow (4-wide depth 8), so
wf_drain and pt_query take their 4-wide walks, but a ray pushes three entries per level: its traversal stack leaves the 16 LDS entries of
wf_trace for the global-memory overflow, it is suspended at the node budget with that stack and resumed by another lane, and a
6144-stream render has more such rays than its pool of suspend records holds.  None of this happens on the config scenes (Cornell, the
stand-in, its instances, the attribute scene).  tests/test_stack_depth.py checks the premise on the CPU; the evidence test below reads
the device's own stack-depth histogram.

One oracle scene and one oracle frame (64 x 48, 2 passes, 2 spp, default bounce limits: 3 s on 16 CPU threads) serve every test.
The bar against the oracle is the project's (scenes_util.check_image); every other comparison is bit for bit.

Time slicing (test_time_slicing_...): PTAMD_BS=31 makes the node budget PTAMD_BM = 32 steps per launch, PTAMD_LB=0 switches the late
budget off.  Iterations, worked out before any run: max_bounce = 3 lets a stream trace at most 4 rays one after the other (the camera ray
and three bounces; the shadow rays travel beside them), and a ray of S node steps takes at most S / 32 + 1 launches.  With S < 4096
(asserted by tests/test_stack_depth.py; its CPU walk finds at most 2765) that is at most 4 * 129 + 2 = 518 iterations, with S = 2765
350; the pipeline gives up after hardCap = (spp * (max_bounce + max_refract + 3) + 8) * 64 = 1408, half of which is 704."""
import os
import subprocess
import sys
import time
import types

import numpy as np
import pytest

import denoise_ref as D
import dynamic_ref as R
import oracle_lib as O
import ptamd
from scenes_util import NEEDLE_CAMERA_POS, NEEDLE_N, NEEDLE_SEED, check_image, needle_inner_rays, needle_positions, needle_scene
from test_query import _assert_any, _assert_closest, bits, same_bits_or_nan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, PASSES, SPP = 64, 48, 2, 2
STREAMS = W * H * PASSES                                   # 6144: its pool holds 6144 / 4 + 1024 = 2560 suspend records
SLICED = dict(passes=1, spp_per_pass=1, max_bounce=3)      # the time-slicing test's render, on a 32 x 24 frame
SLICED_W, SLICED_H, SLICED_BM = 32, 24, 32

_BUILT = {}


def build():
    """(prims, nodes, tris, needle centres) of the needle scene."""
    if not _BUILT:
        prims, _, centres = needle_scene(NEEDLE_SEED)
        nodes, tris, _ = ptamd.build_bvh(prims)
        _BUILT["scene"] = (prims, nodes, tris, centres)
    return _BUILT["scene"]


def scene():
    _, nodes, tris, _ = build()
    return ptamd.Scene(nodes, tris)


def camera(w=W, h=H, **kw):
    return ptamd.make_camera(w, h, **{**dict(pos=NEEDLE_CAMERA_POS), **kw})


def params(**kw):
    return ptamd.default_params(**{**dict(passes=PASSES, spp_per_pass=SPP), **kw})


def query_rays():
    """4096 rays: the camera's jittered rays of pass 0, 512 rays from points inside the cube, 512 segments between two such points."""
    cam_rays, _, _ = ptamd.camera_rays(camera(), 0)
    return np.concatenate([cam_rays, needle_inner_rays(np.random.RandomState(NEEDLE_SEED + 2), 512)]).astype(np.float32)


def frame():
    """The production frame at the default schedule, rendered once."""
    if "frame" not in _BUILT:
        sc = scene()
        _BUILT["frame"] = sc.render(camera(), params())
        _BUILT["frame_iterations"] = sc.last_iterations()
    return _BUILT["frame"]


def _assert_same(got, want, what):
    same = bits(got) == bits(want)
    print(f"{what}: bit-identical floats {same.mean():.6f}")
    assert got.shape == want.shape and same.all(), what


@pytest.fixture(scope="module")
def needle():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    O.set_libm(1)            # the pinned contract: correctly rounded float transcendentals
    prims, nodes, tris, centres = build()
    so = O.Scene(nodes.tobytes(), tris)
    t0 = time.time()
    img_o, _ = so.render(O.make_camera(W, H, pos=NEEDLE_CAMERA_POS), O.make_params(W, H, PASSES, SPP), 16)
    print(f"oracle frame of the needle scene: {time.time() - t0:.1f} s")
    assert np.isfinite(img_o).all() and (img_o > 0).all(-1).mean() > 0.9
    yield types.SimpleNamespace(prims=prims, nodes=nodes, tris=tris, centres=centres, oscene=so, img_o=img_o)


def _child(tmp_path, script, args, env=None):
    """Runs a script in a fresh process (the tuning knobs are read once per process); args follow the package and test directories."""
    path = tmp_path / "child.py"
    path.write_text(script)
    r = subprocess.run([sys.executable, str(path), os.path.join(ROOT, "pathtrace-on-cuda_amd"), os.path.join(ROOT, "tests")] + [str(a) for a in args],
                       env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------
# closest hits: the binary walk of pt_dbg_raycast, the 4-wide walk of pt_query with its 40-entry stack, its binary fallback
# ---------------------------------------------------------------------------------------------------------------------------------
_QUERY_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
from test_needle_scene import scene
rays = np.load(sys.argv[3])
sc = scene()
t, prim, surf = sc.trace_rays(rays, surface=True)
at, aprim = sc.trace_rays(rays, any_hit=True)
np.savez(sys.argv[4], t=t, prim=prim, surf=surf, at=at, aprim=aprim)
"""


def test_closest_hits_are_the_oracles(needle, tmp_path):
    rays = query_rays()
    n_cam = W * H
    hits_o, prim_o, _ = needle.oscene.raycast(rays)
    hit = prim_o >= 0
    print(f"oracle hit share: camera rays {hit[:n_cam].mean():.3f}, inside the cube {hit[n_cam:n_cam + 512].mean():.3f}, segments {hit[n_cam + 512:].mean():.3f}")
    assert hit[:n_cam].mean() > 0.5 and 0.05 < hit[n_cam + 512:].mean() < 0.95      # needles are one-sided; segments end before and behind their first one
    n_prims = len(needle.tris)
    sc = scene()
    h_g, p_g = sc.raycast(rays)                                        # the binary walk (trace_closest)
    assert np.array_equal(p_g, prim_o), f"pt_dbg_raycast: {(p_g != prim_o).sum()} prims differ, first at {np.nonzero(p_g != prim_o)[0][:5]}"
    assert same_bits_or_nan(h_g, hits_o).all()
    got = sc.trace_rays(rays, surface=True)                            # the 4-wide walk
    _assert_closest(got, hits_o, prim_o, "trace_rays, 4-wide walk")
    at, aprim = sc.trace_rays(rays, any_hit=True)
    _assert_any(at, aprim, got[0], got[1], rays, n_prims, "any hit, 4-wide walk")
    # the binary fallback of pt_query, in a process of its own (the knob is read when a scene is created)
    ray_file, out = tmp_path / "rays.npy", tmp_path / "query.npz"
    np.save(ray_file, rays)
    _child(tmp_path, _QUERY_CHILD, [ray_file, out], {"PTAMD_QUERY_QUAD": "0"})
    g = np.load(out)
    _assert_closest((g["t"], g["prim"], g["surf"]), hits_o, prim_o, "trace_rays, PTAMD_QUERY_QUAD=0")
    _assert_any(g["at"], g["aprim"], g["t"], g["prim"], rays, n_prims, "any hit, PTAMD_QUERY_QUAD=0")


# ---------------------------------------------------------------------------------------------------------------------------------
# the frame: against the oracle, and every schedule against the other
# ---------------------------------------------------------------------------------------------------------------------------------
def test_frame_is_the_oracles(needle):
    check_image(frame(), needle.img_o, "needle scene, default schedule (tail in wf_drain)")
    sc = scene()
    sc.set_drain_threshold(0)
    check_image(sc.render(camera(), params()), needle.img_o, "needle scene, pipeline to the end")


def test_every_schedule_gives_the_same_bits(needle):
    want = frame()
    cam, prm = camera(), params()
    sc = scene()
    sc.set_drain_threshold(0)
    _assert_same(sc.render(cam, prm), want, "drain threshold 0")
    it_pipeline = sc.last_iterations()
    sc.set_drain_threshold(1 << 30)
    _assert_same(sc.render(cam, prm), want, "drain threshold 2^30")
    it_drain = sc.last_iterations()
    sc.set_drain_threshold(STREAMS // 4)
    _assert_same(sc.render(cam, prm), want, f"drain threshold {STREAMS // 4}")
    it_between = sc.last_iterations()
    print(f"iterations: wf_drain from the first poll {it_drain}, from {STREAMS // 4} live streams {it_between}, never {it_pipeline}")
    assert it_drain < it_between < it_pipeline
    sc.set_drain_threshold(0)
    for rounds in (0, 1):
        sc.set_shade_rounds(rounds)
        _assert_same(sc.render(cam, prm), want, f"shade rounds {rounds}")
    sc.set_shade_rounds(-1)
    sc.set_early_shade(STREAMS + 1)      # the PUBLISH build of wf_trace: hits and suspend marks are stored device-coherently
    _assert_same(sc.render(cam, prm), want, "early shade")
    sc.set_early_shade(0)
    sc.set_mode(0)                       # the one-kernel state machine: trace_closest on the binary tree
    _assert_same(sc.render(cam, prm), want, "mode 0")


# ---------------------------------------------------------------------------------------------------------------------------------
# evidence that the overflow path ran: the device's own histogram of stack depths
# ---------------------------------------------------------------------------------------------------------------------------------
_HIST_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
from test_needle_scene import camera, params, scene
sc = scene()
sc.set_drain_threshold(0)
img = sc.render(camera(), params())
it = sc.last_iterations()
np.savez(sys.argv[3], img=img, hist=sc.trace_depth_hist(), iterations=it, counters=sc.counters(), launch_rays=sc.trace_launch_rays(it),
         step_hist=sc.trace_step_hist())
"""


def test_the_stack_overflow_path_runs(needle, tmp_path):
    """The counting build of wf_trace (PTAMD_TSTAT=1) bins the stack depth after every node step.  At least 1 % of the node steps of the
    frame's render must leave the stack at 16 entries or more (the CPU walk of tools/stack_lab.cpp gives 2.9 % for the camera rays;
    the margin is for the kernel's cull, which parked leaves delay), and some step at 20 or more.
    Measured on an MI355X: see DESIGN.md, "The needle scene".
    What the counting build's own counters must satisfy, by construction (pt_trace_probe.h): every queue index of a launch is handed to
    exactly one lane, so counters()[5], the lanes refilled, is the sum of the launches' ray counts; a node trip (counters()[0]) serves
    at most 64 lanes (counters()[1]), and so does a triangle trip ([2], [3]); every finished ray adds one to the histogram of node steps
    per ray and one to counters()[7].  The stack-depth histogram gets one count from every lane of every node trip; counters()[0..3]
    are lane 0's accumulators, and lane 0 counts a trip only while it holds a ray itself, so they are a part of the trips: the
    histogram's sum is an upper bound of counters()[1], not equal to it (MI355X, this render: 32.7 M steps in the histogram, 26.3 M
    lanes in counters()[1], 35,870 finished rays)."""
    out = tmp_path / "hist.npz"
    _child(tmp_path, _HIST_CHILD, [out], {"PTAMD_TSTAT": "1"})
    g = np.load(out)
    hist = g["hist"].astype(np.int64)
    share = hist[16:].sum() / max(int(hist.sum()), 1)
    print(f"needle scene: {int(hist.sum())} node steps in {int(g['iterations'])} iterations, share at stack depth >= 16: {share:.4f}, "
          f"deepest bin {int(np.nonzero(hist)[0].max())}")
    print("stack-depth histogram:", hist.tolist())
    assert hist.sum() > 0
    assert share >= 0.01
    assert hist[20:].any()
    counters, launch_rays, iterations = g["counters"].astype(np.int64), g["launch_rays"].astype(np.int64), int(g["iterations"])
    print(f"counters {counters.tolist()}, rays of {iterations} launches {int(launch_rays.sum())}")
    assert 0 < iterations < ptamd.TRACE_STAT_LAUNCHES and launch_rays.shape == (iterations,)
    assert (counters > 0).all()
    assert int(counters[5]) == int(launch_rays.sum())
    assert int(counters[1]) <= 64 * int(counters[0]) and int(counters[3]) <= 64 * int(counters[2])
    assert int(counters[1]) <= int(hist.sum())
    assert int(g["step_hist"].sum()) == int(counters[7])
    _assert_same(g["img"], frame(), "counting build of wf_trace")


# ---------------------------------------------------------------------------------------------------------------------------------
# time slicing with deep stacks: every ray suspended many times, each time with its overflowed stack
# ---------------------------------------------------------------------------------------------------------------------------------
_SLICED_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import numpy as np
from test_needle_scene import SLICED, SLICED_H, SLICED_W, camera, params, scene
sc = scene()
sc.set_drain_threshold(0)
img = sc.render(camera(SLICED_W, SLICED_H), params(**SLICED))
np.savez(sys.argv[3], img=img, iterations=sc.last_iterations())
"""


def test_time_slicing_resumes_overflowed_stacks(needle, tmp_path):
    """A node budget of 32 steps per launch: a ray of ~1000 steps is written to a suspend record and restored by another lane some thirty
    times, most of them with more than 16 stack entries.  The iteration bound is worked out in the module docstring."""
    hard_cap = (SLICED["spp_per_pass"] * (SLICED["max_bounce"] + 8 + 3) + 8) * 64
    assert 4 * (4096 // SLICED_BM + 1) + 2 < hard_cap // 2
    cam, prm = camera(SLICED_W, SLICED_H), params(**SLICED)
    sc = scene()
    want = sc.render(cam, prm)                   # the default schedule
    sc.set_drain_threshold(0)
    _assert_same(sc.render(cam, prm), want, "default budget, pipeline to the end")
    it_parent = sc.last_iterations()
    out = tmp_path / "sliced.npz"
    _child(tmp_path, _SLICED_CHILD, [out], {"PTAMD_BS": "31", "PTAMD_LB": "0", "PTAMD_BM": str(SLICED_BM)})
    g = np.load(out)
    print(f"iterations: default budget {it_parent}, budget of {SLICED_BM} steps {int(g['iterations'])} (cap {hard_cap})")
    _assert_same(g["img"], want, f"node budget {SLICED_BM}")
    assert it_parent < int(g["iterations"]) < hard_cap // 2
    check_image(want, needle.oscene.render(O.make_camera(SLICED_W, SLICED_H, pos=NEEDLE_CAMERA_POS),
                                           O.make_params(SLICED_W, SLICED_H, 1, 1, max_bounce=3), 16)[0], "32 x 24, max_bounce 3")


# ---------------------------------------------------------------------------------------------------------------------------------
# entry points that size their own work buffer (and with it the stride of the stack overflow)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_window_tile_list_views_rays_and_aov(needle):
    want = frame()
    cam, prm = camera(), params()
    sc = scene()
    x0, y0 = W // 2 - 8, H // 2 - 8
    _assert_same(sc.render_window(cam, prm, (x0, y0, x0 + 16, y0 + 16)), want[y0:y0 + 16, x0:x0 + 16], "16 x 16 window in the middle")
    tiles = [43, 0, 18, 29]                      # of the 8 x 6 tiles of the frame
    got = sc.render_tile_list(cam, prm, tiles)
    for i, t in enumerate(tiles):
        ty, tx = divmod(t, W // 8)
        _assert_same(got[i], want[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8], f"tile {t} of the list")
    cam2 = camera(pos=(7.0, 24.0, 42.0), rot_deg=(0.0, 98.0, 0.0))
    views = sc.render_views([cam, cam2], prm)
    _assert_same(views[0], want, "view 0 of two")
    _assert_same(views[1], sc.render(cam2, prm), "view 1 of two")
    assert not np.array_equal(bits(views[1]), bits(want))
    rays, seeds, stride = ptamd.camera_rays(cam, 0)
    pass0 = sc.render(cam, params(passes=1))
    _assert_same(sc.render_rays(rays, params(passes=1), seeds, stride).reshape(H, W, 3), pass0, "the camera's rays of pass 0")
    check_image(pass0, needle.oscene.render(O.make_camera(W, H, pos=NEEDLE_CAMERA_POS), O.make_params(W, H, 1, SPP), 16)[0], "pass 0")
    aov, prim = sc.aov(cam, prm)
    aov_o, prim_o = D.aov_from_oracle(needle.oscene, O.make_camera(W, H, pos=NEEDLE_CAMERA_POS), W, H, PASSES, 0)
    assert np.array_equal(prim, prim_o), f"{(prim != prim_o).sum()} first hits differ"
    assert np.array_equal(bits(aov), bits(aov_o))
    assert (prim_o >= 0).mean() > 0.5 and (prim_o < NEEDLE_N).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# refit of a tree whose boxes all overlap
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refit_to_new_needle_directions(needle):
    """Every needle gets a new random direction about its centre.  The topology stays, so a walk still pushes at most three entries per
    level; every box of the tree changes."""
    tris, nodes = needle.tris, needle.nodes
    key = {p[[0, 1, 2, 28, 29, 30, 56, 57, 58]].tobytes(): i for i, p in enumerate(needle.prims)}
    src = np.array([key[t[0:9].tobytes()] for t in tris])                      # input index of every triangle of the tree order
    assert len(key) == len(tris) and sorted(src) == list(range(len(tris)))
    moved, _ = needle_positions(np.random.RandomState(NEEDLE_SEED + 3), NEEDLE_N, centres=needle.centres)
    is_needle = src < NEEDLE_N
    pos = R.positions(tris).reshape(-1, 9)
    pos[is_needle] = moved[src[is_needle]]
    sc = scene()
    sc.update_vertices(pos)
    tris2 = R.restate_tris(tris, pos)
    nodes2 = R.refit_nodes(nodes, tris2)
    fresh = ptamd.Scene(nodes2, tris2)
    inflation = sc.tree_inflation()
    print(f"tree inflation after the refit: {inflation:.4f}")
    assert inflation > 1.0 and fresh.tree_inflation() == 1.0
    rays = query_rays()
    hits_o, prim_o, _ = O.Scene(nodes2.tobytes(), tris2).raycast(rays)
    assert not np.array_equal(prim_o, needle.oscene.raycast(rays)[1])
    got = sc.trace_rays(rays, surface=True)
    _assert_closest(got, hits_o, prim_o, "trace_rays after the refit")
    for x, y in zip(got, fresh.trace_rays(rays, surface=True)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    h_g, p_g = sc.raycast(rays)
    assert np.array_equal(p_g, prim_o) and same_bits_or_nan(h_g, hits_o).all()
    cam, prm = camera(), params()
    want = fresh.render(cam, prm)
    assert not np.array_equal(bits(want), bits(frame()))
    _assert_same(sc.render(cam, prm), want, "render after the refit, default schedule")
    sc.set_drain_threshold(0)
    _assert_same(sc.render(cam, prm), want, "render after the refit, pipeline to the end")
