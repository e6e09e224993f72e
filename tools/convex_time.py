"""Time the convex-region queries (pt_convex_count, pt_convex_any, pt_convex_list) on the GPU.

  python tools/convex_time.py [--reps 20] [--parent-lib build/libptamd_parent.so] [--out profiles/convex_time_mi355x.json]

Scene: the Cornell room + one stand-in mesh (kind 1) at lat_lon 187 (69,576 triangles).  Three region sets, six planes each:
  tiles      the 32,400 frusta of the 8 x 8-pixel tiles of a 1920 x 1080 camera (ptamd.frustum_planes, no near or far plane)
  voxels     the 2,097,152 voxels of the 128^3 grid over the scene's bounds as aabb_planes — beside pt_box_count of the same boxes, on
             this tree and, with --parent-lib, on a build of the parent commit (tools/build_variant.sh; used through PTAMD_LIB)
  obb        2,097,152 voxel-sized boxes, turned at random, centred on fixed-seed points on random triangles
each with count, any and count + offsets + fill (pt_convex_count, pt_list_offsets, pt_convex_list into a buffer allocated beforehand
from the warm-up's total: no read-back inside the timed region), for PT_CONVEX_TOUCHING and PT_CONVEX_INSIDE.

Call time = the median over --reps calls, after WARM calls, of the time between two device events around the call(s) on device tensors.
Each library's measurements run in one child process under its own `timeout`; if one fails nothing more is started on the GPU.
Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 2
GRID = 128
NEW = ("pt_convex_", "pt_camera_frustum")


def step(a):
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import ptamd
    if a.box_only:      # a library of the parent commit has no convex entry points to bind
        ptamd.API = [e for e in ptamd.API if not e[0].startswith(NEW)]
    import convex_ref as V
    import dynamic_ref as R
    import nearest_ref as N
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, a.lat_lon))
    pos = R.positions(tris)
    v = pos.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    assert torch.cuda.is_available(), "convex_time.py needs a GPU"
    sc = ptamd.Scene(nodes, tris)
    voxels = ptamd.grid_boxes(lo, hi, (a.grid,) * 3)
    n = voxels.shape[0]

    def turns(rs, m):
        """m random rotations, (m, 3, 3) float64, from unit quaternions"""
        q = rs.standard_normal((m, 4))
        w, x, y, z = (q / np.sqrt((q * q).sum(1, keepdims=True))).T
        return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                         np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                         np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)

    def timed(call):
        ms = []
        for k in range(WARM + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            torch.cuda.synchronize()
            if k >= WARM:
                ms.append(e0.elapsed_time(e1))
        return out, {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    def stats(cnt):
        return dict(mean=float(cnt.float().mean().item()), max=int(cnt.max().item()), nonempty_share=float((cnt > 0).float().mean().item()))

    res = {"triangles": int(len(tris)), "tree": sc.tree_info(), "grid": a.grid, "sets": {}}
    box = {}
    for inside in (False, True):
        cnt, row = timed(lambda: sc.box_count(voxels, inside=inside))
        row.update(stats(cnt))
        box["inside" if inside else "touching"] = row
    res["pt_box_count on the voxels"] = box
    if a.box_only:
        print(json.dumps(res))
        return
    half = ((hi - lo) / np.float32(2 * a.grid)).astype(np.float64)
    vb = voxels.cpu().numpy()
    cam = ptamd.make_camera(1920, 1080)
    tiles = [(x, y, x + 8, y + 8) for y in range(0, 1080, 8) for x in range(0, 1920, 8)]
    rs = np.random.RandomState(77)
    p = N.surface_points(rs, n, pos).astype(np.float64)
    sets = {"tiles": ptamd.frustum_planes(cam, tiles), "voxels": V.aabb_many(vb[:, 0:3], vb[:, 4:7]),
            "obb": V.obb_many(p, turns(rs, n), np.broadcast_to(half, (n, 3)))}
    for name, planes in sets.items():
        d = torch.from_numpy(np.ascontiguousarray(planes)).cuda()
        m, k = d.shape[0], d.shape[1]
        res["sets"][name] = {"regions": int(m), "n_planes": int(k)}
        for inside in (False, True):
            row = {}
            cnt, row["count"] = timed(lambda: sc.convex_count(d, inside=inside))
            row["count"].update(stats(cnt))
            _, row["any"] = timed(lambda: sc.convex_any(d, inside=inside))
            total = int(cnt.sum().item())
            rec = torch.empty((max(total, 1), 2), dtype=torch.int32, device="cuda")

            def csr():
                off = ptamd.list_offsets(sc.convex_count(d, inside=inside))
                ptamd._check(ptamd.lib().pt_convex_list(sc._h, C.c_void_p(d.data_ptr()), m, k, int(inside), C.c_void_p(off.data_ptr()), total, None,
                                                        C.c_void_p(rec.data_ptr()), None), "pt_convex_list")
                return off
            off, row["count_offsets_fill"] = timed(csr)
            assert int(off[-1].item()) == total and (total == 0 or int((rec[:total, 1] >= 0).all().item()) == 1)
            row["count_offsets_fill"]["records"] = total
            res["sets"][name]["inside" if inside else "touching"] = row
            sys.stderr.write(f"{name}, inside={inside}: {json.dumps(row)}\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--grid", type=int, default=GRID, help="voxels per axis")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds one library's measurements may take")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit: pt_box_count on the voxels is timed on it, too")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--box-only", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return step(a)
    res = {"lat_lon": a.lat_lon, "warm_up_calls": WARM, "timed_calls": a.reps, "timing": "device events around the call(s) on device tensors"}
    for what, lib in (("this tree", None), ("parent", a.parent_lib)):
        if what == "parent" and not lib:
            continue
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--lat-lon", str(a.lat_lon),
               "--grid", str(a.grid)] + (["--box-only"] if lib else [])
        env = dict(os.environ)
        env.pop("PTAMD_LIB", None)
        if lib:
            env["PTAMD_LIB"] = os.path.abspath(lib)
        r = subprocess.run(cmd, capture_output=True, text=True, env=env)
        sys.stderr.write(r.stderr[-8000:])
        if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
            sys.stderr.write(r.stdout[-2000:])
            sys.exit(f"convex_time.py: the measurements on {what} ended with status {r.returncode}")
        out = json.loads(r.stdout.strip().splitlines()[-1])
        if lib:
            res["parent build: pt_box_count on the voxels"] = out["pt_box_count on the voxels"]
        else:
            res.update(out)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
