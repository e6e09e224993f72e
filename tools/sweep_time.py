"""Time the sphere casts (pt_sweep_spheres) on the GPU, each figure beside pt_trace_rays(PT_QUERY_CLOSEST) of the same segments in the
same run: the yardstick.

  python tools/sweep_time.py [--reps 20] [--n 1048576] [--out profiles/sweep_time_mi355x.json]

Scene: the Cornell room + one stand-in mesh (kind 1) at lat_lon 187 (69,576 triangles).  Two sets of segments, unit directions (so that
a ray's t and a sweep's t are the same parameter), fixed seeds:
  long     free flight: from uniform points in the room in uniform directions, tmax 100 (the room is 40 wide: every segment ends on a wall
           or the mesh)
  short    starts near the surface: from a point on a random triangle moved off it by the radius plus 0.05 .. 0.5 mesh edges along its
           normal, in a uniform direction, tmax two mesh edges
each with the radii 0, one mesh edge (the median edge length of the scene's triangles) and 10 mesh edges, closest and any.

Call time = the median over --reps calls, after WARM calls, of the time between two device events around the call on device tensors.
The measurements run in one child process under its own `timeout`.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 2


def step(a):
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import ptamd
    import dynamic_ref as R
    import nearest_ref as N
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, a.lat_lon))
    pos = R.positions(tris)
    assert torch.cuda.is_available(), "sweep_time.py needs a GPU"
    sc = ptamd.Scene(nodes, tris)
    n = a.n
    e = (pos[:, 1] - pos[:, 0]).astype(np.float64)
    edge = float(np.median(np.sqrt((e * e).sum(1))))

    def unit(rs, m):
        u = rs.standard_normal((m, 3))
        return u / np.sqrt((u * u).sum(1, keepdims=True))

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

    def segments(kind, radius):
        rs = np.random.RandomState(7 if kind == "long" else 8)
        if kind == "long":
            return N.room_points(rs, n).astype(np.float64), unit(rs, n), np.full(n, 100.0)
        k = rs.randint(0, len(pos), n)
        p = pos[k].astype(np.float64)
        u = rs.uniform(0, 1, (n, 2))
        flip = u.sum(1) > 1
        u[flip] = 1 - u[flip]
        on = p[:, 0] + u[:, :1] * (p[:, 1] - p[:, 0]) + u[:, 1:] * (p[:, 2] - p[:, 0])
        nrm = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        with np.errstate(invalid="ignore", divide="ignore"):
            nrm /= np.sqrt((nrm * nrm).sum(1, keepdims=True))
        nrm = np.where(np.isfinite(nrm).all(1, keepdims=True), nrm, unit(rs, n))
        return on + nrm * (radius + edge * rs.uniform(0.05, 0.5, n))[:, None], unit(rs, n), np.full(n, 2.0 * edge)

    res = {"triangles": int(len(tris)), "tree": sc.tree_info(), "segments": n, "mesh_edge": edge, "sets": {}}
    for kind in ("long", "short"):
        res["sets"][kind] = {}
        for label, radius in (("radius 0", 0.0), ("radius 1 edge", edge), ("radius 10 edges", 10.0 * edge)):
            org, d, tmax = segments(kind, radius)
            sw = torch.from_numpy(ptamd.sweep_records(org, d, radius, tmax)).cuda()
            rays = np.zeros((n, 8), np.float32)
            rays[:, 0:3], rays[:, 3:6], rays[:, 7] = org, d, tmax
            rays = torch.from_numpy(rays).cuda()
            row = {}
            (t, prim), row["pt_trace_rays closest"] = timed(lambda: sc.trace_rays(rays))
            row["pt_trace_rays closest"]["hit_share"] = float((prim >= 0).float().mean().item())
            (t, prim), row["sweep closest"] = timed(lambda: sc.sweep_spheres(sw))
            row["sweep closest"].update(hit_share=float((prim >= 0).float().mean().item()), starts_in_contact_share=float(((prim >= 0) & (t == 0)).float().mean().item()))
            _, row["sweep closest with detail"] = timed(lambda: sc.sweep_spheres(sw, detail=True))
            (_, aprim), row["sweep any"] = timed(lambda: sc.sweep_spheres(sw, any_hit=True))
            assert bool(((aprim >= 0) == (prim >= 0)).all().item())
            for k in ("sweep closest", "sweep closest with detail", "sweep any"):
                row[k]["times_the_ray_query"] = row[k]["ms_median"] / row["pt_trace_rays closest"]["ms_median"]
            res["sets"][kind][label] = row
            sys.stderr.write(f"{kind}, {label}: {json.dumps(row)}\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 20, help="segments per set")
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds the measurements may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return step(a)
    res = {"lat_lon": a.lat_lon, "warm_up_calls": WARM, "timed_calls": a.reps, "timing": "device events around the call on device tensors"}
    cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--n", str(a.n),
           "--lat-lon", str(a.lat_lon)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stderr.write(r.stderr[-8000:])
    if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
        sys.stderr.write(r.stdout[-2000:])
        sys.exit(f"sweep_time.py: the measurements ended with status {r.returncode}")
    res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
