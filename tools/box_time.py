"""Time the box queries (pt_box_count, pt_box_any, pt_box_list) on the GPU.  The parent of these calls had nothing to compare with; for
orientation the same run records pt_count_within on the voxel centres with the voxel's half-diagonal as radius, what a caller had to
use before (it over-reports by the ball's corners).

  python tools/box_time.py [--reps 7] [--out profiles/box_time_mi355x.json]

Scene: the Cornell room + one stand-in mesh (kind 1) at lat_lon 187.  Two box sets of 2,097,152 boxes each:
  voxels     the 128^3 grid over the scene's bounds (ptamd.grid_boxes): most voxels are empty, the rest hold a few triangles
  surface    voxel-sized boxes centred on fixed-seed points on random triangles (tests/nearest_ref.py): every box holds something
each with count, any and count + offsets + fill (pt_box_count, pt_list_offsets, pt_box_list into a buffer allocated beforehand from
the warm-up's total: no read-back inside the timed region), for PT_BOX_TOUCHING and PT_BOX_INSIDE, unfiltered and with every second
primitive masked out.

Call time = the median over --reps calls, after WARM calls, of the time between two device events around the call(s) on device tensors.
The measurements run in one child process under its own `timeout`; if it fails nothing more is started on the GPU.  Prints one JSON line.
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


def step(a):
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import dynamic_ref as R
    import nearest_ref as N
    import ptamd
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, a.lat_lon))
    pos = R.positions(tris)
    v = pos.reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    assert torch.cuda.is_available(), "box_time.py needs a GPU"
    sc = ptamd.Scene(nodes, tris)
    voxels = ptamd.grid_boxes(lo, hi, (a.grid,) * 3)
    n = voxels.shape[0]
    half = ((hi - lo) / np.float32(2 * a.grid)).astype(np.float32)
    p = N.surface_points(np.random.RandomState(77), n, pos)
    surf = np.zeros((n, 8), np.float32)
    surf[:, 0:3], surf[:, 4:7] = p - half, p + half
    sets = {"voxels": voxels, "surface": torch.from_numpy(surf).cuda()}
    mask = ptamd.QueryFilter(prim_bits=(np.arange(len(tris)) % 2).astype(np.uint32), bits=1)

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

    res = {"triangles": int(len(tris)), "tree": sc.tree_info(), "boxes_per_set": int(n), "grid": a.grid, "voxel_half_size": half.tolist(), "sets": {}}
    for name, d_boxes in sets.items():
        res["sets"][name] = {}
        for flt_name, flt in (("unfiltered", None), ("half masked", mask)):
            for inside in (False, True):
                row = {}
                cnt, row["count"] = timed(lambda: sc.box_count(d_boxes, inside=inside, filter=flt))
                row["count"].update(mean=float(cnt.float().mean().item()), max=int(cnt.max().item()), nonempty_share=float((cnt > 0).float().mean().item()))
                _, row["any"] = timed(lambda: sc.box_any(d_boxes, inside=inside, filter=flt))
                total = int(cnt.sum().item())
                rec = torch.empty((max(total, 1), 2), dtype=torch.int32, device="cuda")
                fs = C.byref(flt.struct(sc, n)) if flt is not None else None

                def csr():
                    off = ptamd.list_offsets(sc.box_count(d_boxes, inside=inside, filter=flt))
                    ptamd._check(ptamd.lib().pt_box_list(sc._h, C.c_void_p(d_boxes.data_ptr()), n, int(inside), C.c_void_p(off.data_ptr()), total, fs,
                                                         C.c_void_p(rec.data_ptr()), None), "pt_box_list")
                    return off
                off, row["count_offsets_fill"] = timed(csr)
                assert int(off[-1].item()) == total and (total == 0 or int((rec[:total, 1] >= 0).all().item()) == 1)
                row["count_offsets_fill"]["records"] = total
                res["sets"][name][f"{flt_name}, {'inside' if inside else 'touching'}"] = row
                sys.stderr.write(f"{name}, {flt_name}, inside={inside}: {json.dumps(row)}\n")
    # orientation: the bounding ball of every voxel through pt_count_within
    ctr = ((voxels[:, 0:3] + voxels[:, 4:7]) * 0.5)
    balls = torch.cat([ctr, torch.full((n, 1), float(np.sqrt((half.astype(np.float64) ** 2).sum())), device="cuda")], 1).contiguous()
    cnt, row = timed(lambda: sc.count_within(balls))
    row.update(mean=float(cnt.float().mean().item()), max=int(cnt.max().item()), nonempty_share=float((cnt > 0).float().mean().item()))
    res["count_within on the voxels' bounding balls"] = row
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--grid", type=int, default=GRID, help="voxels per axis")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds the measurements may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return step(a)
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--lat-lon", str(a.lat_lon),
           "--grid", str(a.grid)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(r.stderr[-8000:])
    if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
        sys.stderr.write(r.stdout[-2000:])
        sys.exit(f"box_time.py: the measurements ended with status {r.returncode}")
    res = {"lat_lon": a.lat_lon, "warm_up_calls": WARM, "timed_calls": a.reps, "timing": "device events around the call(s) on device tensors"}
    res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
