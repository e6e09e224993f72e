"""Time the first-K-hits and hit-count queries (pt_trace_rays_k, pt_count_hits) on the GPU against the closest-hit query
(pt_trace_rays, PT_QUERY_CLOSEST) of a library built from the parent commit: k = 1 against it is the price of keeping a list and of a
walk that cannot stop at the first hit.

  tools/build_variant.sh parent ""        # on a checkout of the parent commit; gives build/libptamd_parent.so
  python tools/ray_hits_time.py --parent-lib pathtrace-on-cuda_amd/build/libptamd_parent.so [--reps 7] [--out profiles/ray_hits_time_mi355x.json]

Scene: the Cornell room + one stand-in mesh (kind 1, lat_lon 187: 69,576 triangles).  The three fixed-seed ray sets of
tools/query_time.py, of a 1920 x 1080 frame's size (2,073,600 rays each; tests/query_ref.py):
  A   the camera rays of the frame (pt_dbg_pixel_dir)
  B   incoherent bounce rays from A's hit points, random directions in the hemisphere about the normal
  C   segments between random pairs of points in the room, dir = b - a, tmax = 1
each with trace_rays (closest hit), trace_rays_k for k = 1, 4, 8, 32 with front faces and with both sides, with and without the detail
records, and count_hits with front faces and with both sides.

Call time = the median over --reps calls, after WARM calls, of the time between two device events around one call on a device tensor
(one kernel; two with the detail records).  The parent's library and this one are measured in processes of their own, alternating
(parent, this, parent, this), each under its own `timeout`; the first one that fails ends the run (nothing more is started on the
GPU).  Without --parent-lib the closest-hit query of this library stands in and the result says so.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 2
W, H = 1920, 1080
SETS = ("A", "B", "C")
KS = (1, 4, 8, 32)


def _imports():
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes as C
    import ptamd
    have = C.CDLL(ptamd.LIB_PATH)      # a build of the parent commit lacks the new calls: bind what the library exports
    ptamd.API[:] = [e for e in ptamd.API if hasattr(have, e[0])]
    return ptamd


def _scene(ptamd, a):
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, a.lat_lon))
    return ptamd.Scene(nodes, tris), len(tris)


def step_rays(a):
    """Writes the three ray sets to --work and prints what the queries say about them."""
    import numpy as np
    ptamd = _imports()
    import query_ref as Q
    sc, n_tris = _scene(ptamd, a)
    n = a.rays
    ra = Q.set_a(ptamd.dbg_pixel_dir(ptamd.make_camera(W, H), Q.pixel_list(W, H)))[:n]
    _, pa, sa = sc.trace_rays(ra, surface=True)
    rb = Q.set_b(pa, sa, np.random.RandomState(21))
    rc = Q.set_c(len(ra), np.random.RandomState(22))
    out = {"step": "rays", "triangles": n_tris, "rays_per_set": len(ra), "tree": sc.tree_info(), "sets": {}}
    for name, r in zip(SETS, (ra, rb, rc)):
        np.save(os.path.join(a.work, f"rays_{name}.npy"), r)
        _, p = sc.trace_rays(r)
        cf, cb = sc.count_hits(r), sc.count_hits(r, both_sides=True)
        assert np.array_equal(cf > 0, p >= 0)
        out["sets"][name] = {"hit_share": float((p >= 0).mean()), "hits_front_mean": float(cf.mean()), "hits_front_max": int(cf.max()),
                             "hits_both_mean": float(cb.mean()), "hits_both_max": int(cb.max())}
    print(json.dumps(out))


def step_time(a):
    """The timed calls of one library: the closest-hit query, and the new queries where the library has them."""
    import numpy as np
    import torch
    ptamd = _imports()
    assert torch.cuda.is_available(), "ray_hits_time.py needs a GPU"
    sc, _ = _scene(ptamd, a)
    new = any(e[0] == "pt_trace_rays_k" for e in ptamd.API) and not a.closest_only

    def timed(call):
        ms = []
        for k in range(WARM + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if k >= WARM:
                ms.append(e0.elapsed_time(e1))
        return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    res = {}
    for name in SETS:
        rays = torch.from_numpy(np.load(os.path.join(a.work, f"rays_{name}.npy"))).cuda()
        row = {"closest": timed(lambda: sc.trace_rays(rays))}
        if new:
            for both in (False, True):
                side = "both" if both else "front"
                for k in KS:
                    row[f"k{k}_{side}"] = timed(lambda: sc.trace_rays_k(rays, k, both_sides=both))
                    row[f"k{k}_{side}_detail"] = timed(lambda: sc.trace_rays_k(rays, k, both_sides=both, detail=True))
                row[f"count_{side}"] = timed(lambda: sc.count_hits(rays, both_sides=both))
        res[name] = row
        sys.stderr.write(f"{'this' if new else 'closest only'} {name}: {json.dumps(row)}\n")
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libptamd.so built from the parent commit (its closest-hit query is the yardstick)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=2, help="how often the pair (parent, this) is measured")
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--rays", type=int, default=W * H, help="rays per set")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a measurement may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("rays", "time"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--closest-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--work", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return {"rays": step_rays, "time": step_time}[a.step](a)

    with tempfile.TemporaryDirectory() as work:
        base = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--lat-lon", str(a.lat_lon), "--rays", str(a.rays), "--work", work]

        def run(args, lib=None):
            env = dict(os.environ)
            for k in ("PTAMD_LIB", "PTAMD_QUERY_QUAD"):
                env.pop(k, None)
            if lib:
                env["PTAMD_LIB"] = os.path.abspath(lib)
            r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + args, env=env, capture_output=True, text=True)
            sys.stderr.write(r.stderr[-6000:])
            if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
                sys.stderr.write(r.stdout[-2000:])
                sys.exit(f"ray_hits_time.py: step {args} ended with status {r.returncode}; stopping")
            sys.stderr.flush()
            return json.loads(r.stdout.strip().splitlines()[-1])

        rays = run(["--step", "rays"])
        res = {"scene": f"kind 1, lat_lon {a.lat_lon}", "triangles": rays["triangles"], "tree": rays["tree"], "rays_per_set": rays["rays_per_set"],
               "ray_sets": rays["sets"], "warm_up_calls": WARM, "timed_calls": a.reps, "rounds": a.rounds,
               "timing": "device events around one call on a device tensor; medians of the rounds' medians",
               "yardstick": "pt_trace_rays of the parent's library" if a.parent_lib else "pt_trace_rays of THIS library (no parent library given)", "sets": {}}
        parent, this = [], []
        for _ in range(a.rounds):
            parent.append(run(["--step", "time", "--closest-only"], lib=a.parent_lib))
            this.append(run(["--step", "time"]))
        for s in SETS:
            row = {key: {"ms_median": statistics.median(r[s][key]["ms_median"] for r in this), "ms_min": min(r[s][key]["ms_min"] for r in this),
                         "ms_max": max(r[s][key]["ms_max"] for r in this)} for key in this[0][s]}
            row["parent_closest"] = {"ms_median": statistics.median(r[s]["closest"]["ms_median"] for r in parent), "ms_min": min(r[s]["closest"]["ms_min"] for r in parent),
                                     "ms_max": max(r[s]["closest"]["ms_max"] for r in parent), "ms_medians": [r[s]["closest"]["ms_median"] for r in parent]}
            for key in list(row):
                row[key]["mrays_per_s"] = rays["rays_per_set"] / row[key]["ms_median"] / 1e3
            row["k1_front_over_parent_closest"] = row["k1_front"]["ms_median"] / row["parent_closest"]["ms_median"]
            row["closest_over_parent_closest"] = row["closest"]["ms_median"] / row["parent_closest"]["ms_median"]
            res["sets"][s] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
