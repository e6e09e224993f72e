"""Time the K-nearest and count-within queries (pt_nearest_k, pt_count_within) on the GPU, with pt_closest_points from the same run as
the reference: its kernel is the closest query's own, so k = 1 against it is the price of keeping a list.

  python tools/nearest_k_time.py [--reps 7] [--out profiles/nearest_k_time_mi355x.json]

Scenes: the Cornell room + one stand-in mesh (kind 1) and + four (kind 2) at lat_lon 187.  Three fixed-seed point sets of a
1920 x 1080 frame's size (2,073,600 points each; tests/nearest_ref.py):
  surface, radius 1     on random triangles, every third point moved by a normal draw of 1e-3
  room, radius 1        uniform in the room
  room, radius inf      the same points: every list fills, and the count walks the whole tree
each with closest_points, nearest_k for k = 1, 4, 8, 16, 32 (one capacity class each but the first two), nearest_k with the detail
records at k = 8, and count_within.

Call time = the median over --reps calls, after WARM calls, of the time between two device events around one call on a device tensor
(one kernel; two with the detail records).  Every scene is measured in a process of its own under its own `timeout`, one after the
other; the first one that fails ends the run (nothing more is started on the GPU).  Prints one JSON line.
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
KS = (1, 4, 8, 16, 32)


def step_scene(a):
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import dynamic_ref as R
    import nearest_ref as N
    import ptamd
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(a.kind, a.lat_lon))
    n = a.points
    rs = np.random.RandomState(77)
    surface, room = N.surface_points(rs, n, R.positions(tris)), N.room_points(rs, n)
    sets = {"surface, radius 1": (surface, 1.0), "room, radius 1": (room, 1.0), "room, radius inf": (room, float("inf"))}
    assert torch.cuda.is_available(), "nearest_k_time.py needs a GPU"
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
    for name, (p, radius) in sets.items():
        d_pts = torch.from_numpy(N.with_radius(p, radius)).cuda()
        row = {}
        out, row["closest"] = timed(lambda: sc.closest_points(d_pts))
        row["found_share"] = float((out[1] >= 0).float().mean().item())
        for k in KS:
            out, row[f"k{k}"] = timed(lambda: sc.nearest_k(d_pts, k))
            row[f"k{k}"]["slots_filled"] = float((out[1] >= 0).float().mean().item())
        out, row["k8_detail"] = timed(lambda: sc.nearest_k(d_pts, 8, detail=True))
        out, row["count"] = timed(lambda: sc.count_within(d_pts))
        row["count"]["mean"] = float(out.float().mean().item())
        row["count"]["max"] = int(out.max().item())
        res["sets"][name] = row
        sys.stderr.write(f"kind {a.kind} {name}: {json.dumps(row)}\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--points", type=int, default=W * H, help="points per set")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds the measurements of one scene may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kind", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.kind is not None:
        return step_scene(a)
    res = {"lat_lon": a.lat_lon, "warm_up_calls": WARM, "timed_calls": a.reps, "timing": "device events around one call on a device tensor", "scenes": {}}
    for kind in KINDS:
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--kind", str(kind), "--reps", str(a.reps),
               "--lat-lon", str(a.lat_lon), "--points", str(a.points)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stderr.write(r.stderr[-8000:])
        if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
            sys.stderr.write(r.stdout[-2000:])
            sys.exit(f"nearest_k_time.py: kind {kind} ended with status {r.returncode}; stopping")
        res["scenes"][f"kind {kind}"] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
