"""Time the ray-query kernels (pt_trace_rays) on the GPU against the parity hook they replace and against the render's own traversal.

  python tools/query_time.py --parent-lib pathtrace-on-cuda_amd/build/libptamd_parent.so [--reps 10] [--out profiles/query_time_mi355x.json]

Scene: the Cornell room + one stand-in mesh (kind 1, lat_lon 187: the geometry of configs[2]).  Three fixed-seed ray sets of a
1920 x 1080 frame's size (2,073,600 rays each; tests/query_ref.py):
  A   the camera rays of the frame (pt_dbg_pixel_dir)
  B   incoherent bounce rays from A's hit points, random directions in the hemisphere about the normal
  C   segments between random pairs of points in the room, dir = b - a, tmax = 1

  query      per set, closest hit then any hit: WARM + --reps calls of Scene.trace_rays on a device tensor, in one process under
             `rocprofv3 --kernel-trace`; kernel time = the median duration of the timed dispatches of the query kernel, taken from the
             trace in dispatch order.
  dbg        the same three sets through pt_dbg_raycast of the library given by --parent-lib (a build of the parent commit, used through
             PTAMD_LIB), traced the same way: the duration of its dbg_raycast kernel.
  wf_trace   one configs[2] pass (1920 x 1080, 256 spp) rendered twice under the trace: the summed duration of wf_trace per render, over
             the rays of that render (pt_last_counters[0], counted by a third render in a process of its own).

Every measurement is a process of its own under its own `timeout`, one after the other; the first one that fails ends the run
(nothing more is started on the GPU).  Prints one JSON line.
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 3
SETS = ("A", "B", "C")
W, H = 1920, 1080


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
    return ptamd.Scene(nodes, tris)


def step_rays(a):
    """Writes the three ray sets to --work and prints what the closest-hit query says about them."""
    import numpy as np
    ptamd = _imports()
    import query_ref as Q
    sc = _scene(ptamd, a)
    ra = Q.set_a(ptamd.dbg_pixel_dir(ptamd.make_camera(W, H), Q.pixel_list(W, H)))
    ta, pa, sa = sc.trace_rays(ra, surface=True)
    rb = Q.set_b(pa, sa, np.random.RandomState(21))
    rc = Q.set_c(len(ra), np.random.RandomState(22))
    out = {"step": "rays", "rays_per_set": len(ra), "hit_share": {}}
    for name, r in zip(SETS, (ra, rb, rc)):
        np.save(os.path.join(a.work, f"rays_{name}.npy"), r)
        _, p = sc.trace_rays(r)
        _, q = sc.trace_rays(r, any_hit=True)
        assert np.array_equal(p >= 0, q >= 0)
        out["hit_share"][name] = float((p >= 0).mean())
    print(json.dumps(out))


def step_query(a):
    """The timed calls, nothing else on the device in between: per set, WARM + reps closest-hit calls, then as many any-hit calls."""
    import numpy as np
    import torch
    ptamd = _imports()
    sc = _scene(ptamd, a)
    for name in SETS:
        rays = torch.from_numpy(np.load(os.path.join(a.work, f"rays_{name}.npy"))).cuda()
        for any_hit in (False, True):
            for _ in range(WARM + a.reps):
                sc.trace_rays(rays, any_hit=any_hit)
                torch.cuda.synchronize()


def step_dbg(a):
    import numpy as np
    ptamd = _imports()
    sc = _scene(ptamd, a)
    for name in SETS:
        rays = np.load(os.path.join(a.work, f"rays_{name}.npy"))
        for _ in range(1 + a.dbg_reps):
            sc.raycast(rays)


def _render_args(ptamd, torch):
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=1, spp_per_pass=256, rank=0, world=1)
    tiles = torch.empty(ptamd.tiles_floats(cam, prm), dtype=torch.float32, device="cuda:0")
    work = torch.empty(ptamd.work_bytes(cam, prm), dtype=torch.uint8, device="cuda:0")
    return cam, prm, tiles, work


def step_render(a):
    import torch
    ptamd = _imports()
    sc = _scene(ptamd, a)
    cam, prm, tiles, work = _render_args(ptamd, torch)
    for _ in range(2):
        sc.render_tiles(cam, prm, tiles.data_ptr(), work.data_ptr(), 0)
        torch.cuda.synchronize()


def step_count(a):
    import torch
    ptamd = _imports()
    sc = _scene(ptamd, a)
    cam, prm, tiles, work = _render_args(ptamd, torch)
    sc.enable_counters(True)
    sc.render_tiles(cam, prm, tiles.data_ptr(), work.data_ptr(), 0)
    torch.cuda.synchronize()
    print(json.dumps({"step": "count", "rays": int(sc.counters()[0])}))


def _col(row, *want):
    for k in row:
        if k.replace("_", "").lower() in want:
            return k
    raise KeyError(f"no column {want} in {list(row)}")


def step_trace(a):
    """Runs one of the plain steps under rocprofv3 and prints the durations (ns) of the kernels whose name contains --kernel, in dispatch order."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(max(a.step_timeout - 20, 30)), "/opt/rocm/bin/rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--step", a.inner, "--work", a.work, "--lat-lon", str(a.lat_lon), "--reps", str(a.reps), "--dbg-reps", str(a.dbg_reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(r.returncode)
        rows = []
        for root, _, files in os.walk(d):
            for f in files:
                if f.endswith("kernel_trace.csv"):
                    rows += list(csv.DictReader(open(os.path.join(root, f))))
    if not rows:
        sys.exit("query_time.py: the profiler wrote no kernel trace")
    kn, ks, ke = _col(rows[0], "kernelname"), _col(rows[0], "starttimestamp"), _col(rows[0], "endtimestamp")
    rows.sort(key=lambda row: int(row[ks]))
    out = {}
    for key in a.kernel.split(","):
        out[key] = [int(row[ke]) - int(row[ks]) for row in rows if key in row[kn]]
    print(json.dumps({"step": "trace", "inner": a.inner, "ns": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libptamd.so built from the parent commit (its dbg_raycast is the yardstick)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dbg-reps", type=int, default=5)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a measurement may take")
    ap.add_argument("--skip", default="", help="comma-separated steps to leave out (dbg, wf_trace)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("rays", "query", "dbg", "render", "count", "trace"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--inner", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--kernel", default="", help=argparse.SUPPRESS)
    ap.add_argument("--work", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return {"rays": step_rays, "query": step_query, "dbg": step_dbg, "render": step_render, "count": step_count, "trace": step_trace}[a.step](a)

    skip = set(a.skip.split(","))
    with tempfile.TemporaryDirectory() as work:
        base = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--dbg-reps", str(a.dbg_reps), "--lat-lon", str(a.lat_lon), "--work", work,
                "--step-timeout", str(a.step_timeout)]

        def run(args, env_extra=None, lib=None):
            env = dict(os.environ)
            for k in ("PTAMD_LIB", "PTAMD_QUERY_QUAD"):
                env.pop(k, None)
            env.update(env_extra or {})
            if lib:
                env["PTAMD_LIB"] = os.path.abspath(lib)
            r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + args, env=env, capture_output=True, text=True)
            if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(f"query_time.py: step {args} ended with status {r.returncode}; stopping")
            sys.stderr.write(f"done: {' '.join(args)} {env_extra or ''}\n")
            sys.stderr.flush()
            return json.loads(r.stdout.strip().splitlines()[-1])

        def per_set(ns, warm, reps):
            """ns: durations in dispatch order, warm + reps dispatches per set (and mode) -> per set (and mode) the median of the timed ones."""
            per = warm + reps
            assert len(ns) % per == 0 and len(ns) // per in (len(SETS), 2 * len(SETS)), (len(ns), per)
            chunks = [ns[i:i + per][warm:] for i in range(0, len(ns), per)]
            return [{"us_median": statistics.median(c) / 1e3, "us_min": min(c) / 1e3, "us_max": max(c) / 1e3} for c in chunks]

        rays = run(["--step", "rays"])
        n = rays["rays_per_set"]
        res = {"scene": f"kind 1, lat_lon {a.lat_lon} (configs[2] geometry)", "rays_per_set": n, "hit_share": rays["hit_share"], "warm_up_calls": WARM,
               "timed_calls": a.reps, "dbg_yardstick": "parent" if a.parent_lib else "this tree's own library (NOT the parent)", "sets": {}}
        t = run(["--step", "trace", "--inner", "query", "--kernel", "query_rays"])
        sched = {"query": per_set(t["ns"]["query_rays"], WARM, a.reps)}
        dbg = None
        if "dbg" not in skip:
            t = run(["--step", "trace", "--inner", "dbg", "--kernel", "dbg_raycast"], lib=a.parent_lib)
            dbg = per_set(t["ns"]["dbg_raycast"], 1, a.dbg_reps)
        for i, s in enumerate(SETS):
            row = {}
            for name, rows in sched.items():
                for j, mode in enumerate(("closest", "any")):
                    m = rows[2 * i + j]
                    row[f"{name}_{mode}"] = dict(m, rays_per_s=n / (m["us_median"] * 1e-6))
            if dbg:
                row["parent_dbg_raycast"] = dict(dbg[i], rays_per_s=n / (dbg[i]["us_median"] * 1e-6))
                for name in sched:
                    row[f"{name}_closest_over_dbg"] = row[f"{name}_closest"]["us_median"] / dbg[i]["us_median"]
                    row[f"{name}_any_over_dbg"] = row[f"{name}_any"]["us_median"] / dbg[i]["us_median"]
            res["sets"][s] = row
        if "wf_trace" not in skip:
            cnt = run(["--step", "count"])
            t = run(["--step", "trace", "--inner", "render", "--kernel", "wf_trace"])
            total_us = sum(t["ns"]["wf_trace"]) / 2 / 1e3      # two renders under the trace
            res["wf_trace"] = {"workload": "one configs[2] pass, 1920x1080, 256 spp", "rays": cnt["rays"], "launches_per_render": len(t["ns"]["wf_trace"]) / 2,
                               "kernel_us_per_render": total_us, "ns_per_ray": total_us * 1e3 / cnt["rays"], "rays_per_s": cnt["rays"] / (total_us * 1e-6)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
