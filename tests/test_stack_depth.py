"""Host-only premise check of tests/test_needle_scene.py, measured by tools/stack_lab.cpp: on scenes_util.needle_scene the 4-wide tree is
shallow enough for wf_drain's and pt_query's 4-wide walks (depth <= 12), yet most camera rays fill their traversal stack beyond the 16
entries wf_trace keeps in LDS, take more node steps than the default budget of 256, and are more than a 6144-stream render's pool of
suspend records can hold; no ray needs more than 36 stack entries (wf_drain's and pt_query's stacks hold 40) or more than 4096 node steps
(what the pipeline's iteration cap assumes: 64 launches per bounce at the late budget of 64 steps).

Figures of the scene as built (seed 5, 16384 needles of length 0.8 side in a cube of side 30, and the two light triangles), from the CPU
walk of stack_lab (an approximation of the kernel's arithmetic), for the 64 x 48 pinhole rays from (0, 20, 40) and, second, for 1536 rays
and 1536 segments that start inside the cube:
                               binary / 4-wide depth  stack > 16   > 256 steps  max stack  max node steps  node steps at depth >= 16
  size-aware tree (default)    18 / 8                 0.91 / 0.82  1.00 / 1.00  21 / 24    2030 / 2765     0.029 / 0.031
  centroid-SAH (PTAMD_TREE=0)  19 / 8                 0.99 / 0.85  1.00 / 1.00  24 / 25    2266 / 3130     0.037 / 0.034
With 8192 needles every condition below but the last holds as well (stack > 16 for 0.76 of the camera rays, max node steps 1054), but
only 0.013 of the node steps are taken at depth >= 16: too close to the 0.01 the GPU test asks of the device, hence 16384."""
import os
import re
import subprocess

import numpy as np
import pytest

import ptamd
from scenes_util import NEEDLE_CAMERA_POS, NEEDLE_SEED, V_POS, needle_inner_rays, needle_scene, pinhole_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pathtrace-on-cuda_amd")
OBJS = ["accel_build.o", "bvh_build.o", "scenes.o", "pt_host.o", "obj_loader.o"]
W, H = 64, 48
STREAMS = 6144      # the render of tests/test_needle_scene.py: 64 x 48 pixels, 2 passes


def build_stack_lab(directory):
    objs = [os.path.join(PKG, "build", o) for o in OBJS]
    if not all(os.path.exists(o) for o in objs):
        subprocess.run(["make", "-s", "-C", PKG], check=True)
    exe = os.path.join(str(directory), "stack_lab")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "stack_lab.cpp")] + objs +
                   ["-pthread", "-o", exe], check=True)
    return exe


def run_stack_lab(exe, directory, positions, rays, tree=None):
    """stack_lab's figures for (n, 9) positions and (m, 8) rays; tree: None = the upload's default, 0 = PTAMD_TREE=0."""
    pos_file, ray_file = os.path.join(str(directory), "positions.bin"), os.path.join(str(directory), "rays.bin")
    np.ascontiguousarray(positions, np.float32).tofile(pos_file)
    np.ascontiguousarray(rays, np.float32).tofile(ray_file)
    env = {k: v for k, v in os.environ.items() if k != "PTAMD_TREE"}
    if tree is not None:
        env["PTAMD_TREE"] = str(tree)
    r = subprocess.run([exe, pos_file, ray_file], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"^STACK tris (\d+) rays (\d+) bdepth (\d+) depth (\d+) over_lds (\S+) over_budget (\S+) n_over_budget (\d+) max_stack (\d+) "
                  r"max_steps (\d+) deep_share (\S+)$", r.stdout, re.M)
    assert m, r.stdout
    g = m.groups()
    return dict(tris=int(g[0]), rays=int(g[1]), bdepth=int(g[2]), depth=int(g[3]), over_lds=float(g[4]), over_budget=float(g[5]),
                n_over_budget=int(g[6]), max_stack=int(g[7]), max_steps=int(g[8]), deep_share=float(g[9]))


def scene_positions(prims):
    return np.ascontiguousarray(prims.reshape(-1, 3, 28)[:, :, V_POS:V_POS + 3].reshape(-1, 9), np.float32)


@pytest.fixture(scope="module")
def stack_lab(tmp_path_factory):
    return build_stack_lab(tmp_path_factory.mktemp("stack"))


@pytest.mark.parametrize("tree", [None, 0], ids=["default_tree", "PTAMD_TREE=0"])
def test_needle_scene_fills_the_stack_of_a_shallow_tree(stack_lab, tmp_path, tree):
    prims, _, _ = needle_scene(NEEDLE_SEED)
    pos = scene_positions(prims)
    s = run_stack_lab(stack_lab, tmp_path, pos, pinhole_rays(ptamd.make_camera(W, H, pos=NEEDLE_CAMERA_POS)), tree)
    print(f"needle scene, tree {tree}, camera rays: {s}")
    assert s["tris"] == len(prims) and s["rays"] == W * H
    assert s["depth"] <= 12, s                  # wf_drain and pt_query walk the 4-wide tree
    assert s["bdepth"] <= 32, s                 # kAccelMaxDepth
    assert s["over_lds"] >= 0.5, s              # most rays leave the 16 LDS entries of wf_trace's stack
    assert s["over_budget"] >= 0.5, s           # most rays are suspended at the default budget of 256 steps, with that stack
    assert s["n_over_budget"] * STREAMS / s["rays"] > STREAMS / 4 + 1024, s      # more of them than the pool of suspend records holds
    assert s["max_stack"] <= 36, s              # inside the 40 entries of wf_drain and pt_query
    assert s["max_steps"] < 4096, s             # inside the pipeline's iteration cap: 64 launches per bounce at the late budget of 64
    assert s["deep_share"] >= 0.02, s           # twice what tests/test_needle_scene.py asks of the device's own histogram
    # the rays a path goes on with, from inside the cube: the two bounds that must hold for every ray of a render
    t = run_stack_lab(stack_lab, tmp_path, pos, needle_inner_rays(np.random.RandomState(NEEDLE_SEED + 1), 1536), tree)
    print(f"needle scene, tree {tree}, rays and segments inside the cube: {t}")
    assert t["max_stack"] <= 36 and t["max_steps"] < 4096, t
