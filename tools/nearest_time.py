"""Time the closest-point queries (pt_closest_points) on the GPU, with pt_trace_rays on camera rays from the same run as orientation.

  python tools/nearest_time.py [--reps 7] [--out profiles/nearest_time_mi355x.json]

Scenes: the Cornell room + one stand-in mesh (kind 1) and + four (kind 2) at lat_lon 187.  Three fixed-seed point sets of a
1920 x 1080 frame's size (2,073,600 points each; tests/nearest_ref.py):
  surface   on random triangles, every third point moved by a normal draw of 1e-3
  room      uniform in the room
  far       the room points 300 times farther out
each with an infinite radius and with a radius of 1, closest with and without the detail records, and any-within.
Orientation: Scene.trace_rays, closest hit, on the camera rays of the frame (as many rays as there are points).

Call time = the median over --reps calls, after WARM calls, of the time between two device events around one call on a device tensor
(one kernel; two with the detail records).  Nothing here is compared with a parent: the parent commit has no such query.
Every scene is measured in a process of its own under its own `timeout`, one after the other; the first one that fails ends the run
(nothing more is started on the GPU).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 2
W, H = 1920, 1080
KINDS = (1, 2)


def step_scene(a):
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import dynamic_ref as R
    import nearest_ref as N
    import ptamd
    import query_ref as Q
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(a.kind, a.lat_lon))
    n = W * H
    rs = np.random.RandomState(77)
    room = N.room_points(rs, n)
    sets = {"surface": N.surface_points(rs, n, R.positions(tris)), "room": room, "far": room * np.float32(300)}
    assert torch.cuda.is_available(), "nearest_time.py needs a GPU"
    sc = ptamd.Scene(nodes, tris)

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

    res = {"kind": a.kind, "triangles": int(len(tris)), "tree": sc.tree_info(), "points_per_set": n, "sets": {}}
    for name, p in sets.items():
        for radius in (float("inf"), 1.0):
            d_pts = torch.from_numpy(N.with_radius(p, radius)).cuda()
            row = {}
            for what, kw in (("closest", {}), ("closest_detail", {"detail": True}), ("any", {"any_within": True})):
                out, t = timed(lambda: sc.closest_points(d_pts, **kw))
                row[what] = dict(t, points_per_s=n / (t["ms_median"] * 1e-3))
                row.setdefault("found_share", float((out[1] >= 0).float().mean().item()))
            res["sets"][f"{name}, radius {radius}"] = row
            sys.stderr.write(f"kind {a.kind} {name} radius {radius}: {json.dumps(row)}\n")
    rays = torch.from_numpy(Q.set_a(ptamd.dbg_pixel_dir(ptamd.make_camera(W, H), Q.pixel_list(W, H)))).cuda()
    out, t = timed(lambda: sc.trace_rays(rays))
    res["trace_rays_camera_closest"] = dict(t, rays=int(rays.shape[0]), rays_per_s=rays.shape[0] / (t["ms_median"] * 1e-3),
                                            hit_share=float((out[1] >= 0).float().mean().item()))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds the measurements of one scene may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kind", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kind is not None:
        return step_scene(a)
    res = {"lat_lon": a.lat_lon, "warm_up_calls": WARM, "timed_calls": a.reps, "timing": "device events around one call on a device tensor", "scenes": {}}
    for kind in KINDS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--kind", str(kind), "--reps", str(a.reps),
               "--lat-lon", str(a.lat_lon)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-6000:])
        if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
            sys.stderr.write(r.stdout[-2000:])
            sys.exit(f"nearest_time.py: kind {kind} ended with status {r.returncode}; stopping")
        res["scenes"][f"kind {kind}"] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
