"""Host-only quality checks of the size-aware traversal tree (host/accel_build.cpp) against the centroid-SAH tree (PTAMD_TREE=0),
measured by tools/tree_lab.cpp on one ray set: the 4-wide tree of the config scenes stays within wf_drain's depth (12), and on the
bunny-in-the-room scene the weighted traversal cost per ray (node steps + 3.1 x leaf visits) drops by at least 15 %."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pathtrace-on-cuda_amd")
OBJS = ["accel_build.o", "bvh_build.o", "scenes.o", "pt_host.o", "obj_loader.o"]


@pytest.fixture(scope="module")
def tree_lab(tmp_path_factory):
    objs = [os.path.join(PKG, "build", o) for o in OBJS]
    if not all(os.path.exists(o) for o in objs):
        subprocess.run(["make", "-s", "-C", PKG], check=True)
    exe = str(tmp_path_factory.mktemp("tree") / "tree_lab")
    subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "tree_lab.cpp")] + objs +
                   ["-pthread", "-o", exe], check=True)
    return exe


def run_lab(exe, kind, pixels):
    r = subprocess.run([exe, str(kind), "187", str(pixels)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    trees = {}
    for m in re.finditer(r"^TREE (\d) kind \d+ nodes (\d+) children (\S+) depth (\d+) bdepth (\d+) steps (\S+) leaves (\S+) weighted (\S+)$",
                         r.stdout, re.M):
        trees[int(m.group(1))] = dict(nodes=int(m.group(2)), depth=int(m.group(4)), bdepth=int(m.group(5)), weighted=float(m.group(8)))
    assert set(trees) == {0, 1}, r.stdout
    return trees


@pytest.mark.parametrize("kind", [1, 2])
def test_quad_depth_within_drain_stack(tree_lab, kind):
    t = run_lab(tree_lab, kind, 2000)[1]
    assert t["depth"] <= 12, t          # wf_drain walks the 4-wide tree only while 3 * quad_depth + 2 <= 40
    assert t["bdepth"] <= 32, t         # kAccelMaxDepth


def test_bunny_room_weighted_cost(tree_lab):
    t = run_lab(tree_lab, 1, 20000)
    assert t[1]["weighted"] <= 0.85 * t[0]["weighted"], t
