"""Time the triangle queries (pt_tri_count, pt_tri_any, pt_tri_list) on the GPU, each set beside pt_convex_count on the five-plane
stand-in of the same triangles (the two sides of the triangle's plane and its three edge planes) in the same run: its time and its
member count, to show how much the conservative class over-reports.

  python tools/tri_time.py [--reps 20] [--n 1048576] [--out profiles/tri_time_mi355x.json]

Scene: the Cornell room + one stand-in mesh (kind 1) at lat_lon 187 (69,576 triangles).  Query sets, fixed seeds:
  surface 1 edge     n triangles of one mesh edge (the median edge length of the scene's triangles) placed on the surface
  surface 10 edges   the same, ten mesh edges
  stack, tiled       a 1,024-layer slicing stack over the scene's height, every layer a square larger than the scene cut into 16 x 32
                     tiles of two triangles: 1,048,576 queries
  stack, whole       the same 1,024 layers as one quad each: 2,048 queries, every one a lone large query that holds its wave
Per set: count, any, count + offsets + fill without and with the segments.

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
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, a.lat_lon))
    pos = R.positions(tris)
    assert torch.cuda.is_available(), "tri_time.py needs a GPU"
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

    def surface(size, seed):
        rs = np.random.RandomState(seed)
        p = pos[rs.randint(0, len(pos), n)].astype(np.float64)
        w = rs.dirichlet([1, 1, 1], n)
        at = (p * w[:, :, None]).sum(1)
        u = unit(rs, n)
        v = np.cross(u, unit(rs, n))
        v /= np.sqrt((v * v).sum(1, keepdims=True))
        th = rs.uniform(0, 2 * np.pi, (n, 1)) + np.array([0.0, 2 * np.pi / 3, 4 * np.pi / 3])
        r = size / np.sqrt(3.0)      # an equilateral triangle of that edge
        T = at[:, None, :] + r * (np.cos(th)[:, :, None] * u[:, None, :] + np.sin(th)[:, :, None] * v[:, None, :])
        return ptamd.tri_records(T[:, 0], T[:, 1], T[:, 2])

    def stack(tiles_x, tiles_z, layers=1024):
        v = pos.reshape(-1, 3).astype(np.float64)
        lo, hi = v.min(0), v.max(0)
        ys = lo[1] + (hi[1] - lo[1]) * (np.arange(layers) + 0.5) / layers
        xs = np.linspace(lo[0] - 1.0, hi[0] + 1.0, tiles_x + 1)
        zs = np.linspace(lo[2] - 1.0, hi[2] + 1.0, tiles_z + 1)
        y, ix, iz = np.meshgrid(ys, np.arange(tiles_x), np.arange(tiles_z), indexing="ij")
        y, ix, iz = y.reshape(-1), ix.reshape(-1), iz.reshape(-1)
        p00 = np.stack([xs[ix], y, zs[iz]], 1)
        p10 = np.stack([xs[ix + 1], y, zs[iz]], 1)
        p11 = np.stack([xs[ix + 1], y, zs[iz + 1]], 1)
        p01 = np.stack([xs[ix], y, zs[iz + 1]], 1)
        return np.concatenate([ptamd.tri_records(p00, p10, p11), ptamd.tri_records(p00, p11, p01)])

    def five_planes(rec):
        """(n, 5, 4) PLANE4 records n.xyz | d, inside where dot(n, x) <= d: both sides of the triangle's plane, then its three edges"""
        qa, qb, qc = (rec[:, 0:3].astype(np.float64), rec[:, 4:7].astype(np.float64), rec[:, 8:11].astype(np.float64))
        nrm = np.cross(qb - qa, qc - qa)
        out = np.zeros((len(rec), 5, 4))
        out[:, 0, 0:3], out[:, 0, 3] = nrm, (nrm * qa).sum(1)
        out[:, 1, 0:3], out[:, 1, 3] = -nrm, -(nrm * qa).sum(1)
        for j, (v0, v1) in enumerate(((qa, qb), (qb, qc), (qc, qa))):
            m = -np.cross(nrm, v1 - v0)      # outward
            out[:, 2 + j, 0:3], out[:, 2 + j, 3] = m, (m * v0).sum(1)
        return out.astype(np.float32)

    res = {"triangles": int(len(tris)), "tree": sc.tree_info(), "mesh_edge": edge, "sets": {}}
    sets = (("surface 1 edge", lambda: surface(edge, 7)), ("surface 10 edges", lambda: surface(10 * edge, 8)), ("stack, tiled", lambda: stack(16, 32)),
            ("stack, whole", lambda: stack(1, 1)))
    for label, make in sets:
        rec = make()
        d_q = torch.from_numpy(rec).cuda()
        d_planes = torch.from_numpy(five_planes(rec)).cuda()
        row = {"queries": int(len(rec))}
        cnt, row["count"] = timed(lambda: sc.tri_count(d_q))
        total = int(cnt.sum().item())
        row["count"].update(members=total, queries_with_a_member=float((cnt > 0).float().mean().item()), most_members=int(cnt.max().item()))
        (_, aprim), row["any"] = timed(lambda: sc.tri_any(d_q))
        assert bool(((aprim >= 0) == (cnt > 0)).all().item())
        _, row["count + offsets + fill"] = timed(lambda: sc.cut_by_triangles(d_q))
        (off, _, _, det), row["count + offsets + fill with segments"] = timed(lambda: sc.cut_by_triangles(d_q, segments=True))
        assert int(off[-1].item()) == total and tuple(det.shape) == (total, 8)
        ccnt, row["pt_convex_count, five planes"] = timed(lambda: sc.convex_count(d_planes))
        row["pt_convex_count, five planes"].update(members=int(ccnt.sum().item()), times_the_members=float(ccnt.sum().item()) / max(total, 1))
        res["sets"][label] = row
        sys.stderr.write(f"{label}: {json.dumps(row)}\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 20, help="queries per surface set")
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
        sys.exit(f"tri_time.py: the measurements ended with status {r.returncode}")
    res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
