"""Measure the tree rebuild with treelet restructuring (pt_scene_rebuild_tree_opt): what the passes do to the area sum (CPU, the numpy
yardstick), what the call costs against pt_scene_rebuild_tree_ex of the parent commit, and how the tree it builds renders.

  python tools/rebuild_opt_time.py --parent-lib build/libptamd_parent.so [--kinds 1,2] [--reps 20] [--out profiles/rebuild_opt_mi355x.json]

Scenes and move as tools/rebuild_budget_time.py: the Cornell room + one stand-in mesh (kind 1, configs[2]) and + four (kind 2),
lat_lon 187; the mesh turned about y with a sine wobble and a translation, the two light triangles translated.

  area      no GPU: tests/rebuild_opt_ref.py with (26, 1/16) on the stand-in scene of the tests (kind 1, lat_lon 16) and on kind 1 at
            --area-lat-lon, the sum of the interior boxes' areas after 1 .. 4 passes as a fraction of the unoptimised tree's, and the
            smallest pass count after which one more pass gains less than 1 % of the area sum.
  call      per kind, at the uploaded pose (0 degrees) and the 25 degree pose: HIP events around the call on its stream, median of --reps
            after warm-up (the first call, which allocates, apart); tree_info and the report afterwards.  Each a process of its own: the
            new call with (26, 1/16) and 0, 1, 2 passes in this tree's library (the split: the build pt_scene_rebuild_tree_ex does, the
            first pass, the second), and pt_scene_rebuild_tree_ex with its defaults in the library given by --parent-lib (a build of
            the parent commit, used through PTAMD_LIB).  Kind 1 also without a budget, (0, 1/16) with 0 and 2 passes: every pass then
            launches heights 1 .. 63.
  trees     kind 1: one pass of configs[2] (1920 x 1080, 256 spp) and the closest-hit query along the frame's 2.07 M pinhole rays on
            trees of the same moved geometry, alternating in one process, for turns of 10 / 25 / 90 degrees: refit (update only), ex
            (update + pt_scene_rebuild_tree_ex with its defaults — this tree's, which tests/test_rebuild_opt.py pins to passes = 0 and
            the existing tests to the parent's), opt (update + the new call with its defaults), fresh (host build + upload).  Medians of
            --render-reps, whether all frames are bit-identical, tree_info, the report, and the mode-0 counters (node records
            fetched, triangle tests) of a 480 x 270, 16 spp frame.

Every GPU measurement is a process of its own under its own `timeout`, one after the other; the first one that fails ends the run
(nothing more is started on the GPU).  Prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import update_time as U      # noqa: E402  (the scenes and the move are its own)

WARM = 3


def step_area(a):
    ptamd = U._imports()
    import dynamic_ref as R
    import rebuild_opt_ref as P
    rows = []
    for what, lat_lon in (("standin (kind 1, lat_lon 16)", 16), (f"kind 1, lat_lon {a.area_lat_lon}", a.area_lat_lon)):
        _, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, lat_lon))
        trace = []
        t = P.build(R.positions(tris), passes=4, trace=trace)
        frac = [x / t["area_before"] for x in trace]
        gain = [1.0 - frac[0]] + [frac[k - 1] - frac[k] for k in range(1, len(frac))]      # of the unoptimised sum, per pass
        enough = next((k for k in range(1, len(frac)) if gain[k] < 0.01), len(frac))
        rows.append({"scene": what, "tris": len(tris), "params": [26, 0.0625], "area_over_unoptimised_after_pass": frac, "gain_of_pass": gain,
                     "smallest_count_after_which_a_pass_gains_less_than_1_percent": enough, "n_roots": t["n_roots"], "n_restructured": t["n_restructured"],
                     "depth_before": P.build(R.positions(tris), passes=0)["depth"], "depth_after": t["depth"]})
    print(json.dumps({"step": "area", "rows": rows}))


def step_call(a):
    import numpy as np
    import torch
    ptamd = U._imports()
    dev = torch.device("cuda:0")
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(a.kind, a.lat_lon))
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d_pos = U._moved_positions(tris, 25.0, torch, dev)
    st.synchronize()
    res = {"step": "call", "kind": a.kind, "tris": len(tris),
           "call": "pt_scene_rebuild_tree_ex, defaults" if a.passes < 0 else f"pt_scene_rebuild_tree_opt, ({a.budget}, 1/16), {a.passes} passes",
           "library": "the one given by --parent-lib" if os.environ.get("PTAMD_LIB") else "this tree's", "poses": []}
    for deg in (0.0, 25.0):
        sc = ptamd.Scene(nodes, tris)
        if deg:
            sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
            st.synchronize()
        ms, report = [], None
        for _ in range(1 + WARM + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            if a.passes < 0:
                report = sc.rebuild_tree(stream_ptr=st.cuda_stream, depth_budget=26)
            else:
                report = sc.rebuild_tree_optimized(passes=a.passes, depth_budget=a.budget, stream_ptr=st.cuda_stream)
            e1.record(st)
            st.synchronize()
            ms.append(e0.elapsed_time(e1))
        first, ms = ms[0], ms[1 + WARM:]
        res["poses"].append({"degrees": deg, "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms": ms, "first_ms": first,
                             "tree_info": sc.tree_info(), "report": report, "device_bytes": sc.device_bytes})
    print(json.dumps(res))


def step_trees(a):
    import numpy as np
    import torch
    ptamd = U._imports()
    import dynamic_ref as R
    dev = torch.device("cuda:0")
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, a.lat_lon))
    W, H = 1920, 1080
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=1, spp_per_pass=256, rank=0, world=1)
    tiles = torch.empty(ptamd.tiles_floats(cam, prm), dtype=torch.float32, device=dev)
    work = torch.empty(ptamd.work_bytes(cam, prm), dtype=torch.uint8, device=dev)
    ccam, cprm = ptamd.make_camera(480, 270), ptamd.default_params(passes=1, spp_per_pass=16)
    d_rays = torch.from_numpy(ptamd.camera_rays(cam, 0)[0]).to(dev)
    rows = []
    for deg in (10.0, 25.0, 90.0):
        d_pos = U._moved_positions(tris, deg, torch, dev)
        torch.cuda.synchronize()
        row = {"degrees": deg}
        trees = []
        for name in ("refit", "ex", "opt"):
            sc = ptamd.Scene(nodes, tris)
            sc.update_vertices(d_pos)
            if name == "refit":
                row["tree_inflation_refit"] = sc.tree_inflation()
            elif name == "ex":
                row["ex_report"] = sc.rebuild_tree(depth_budget=26)
            else:
                row["opt_report"] = sc.rebuild_tree_optimized()
            trees.append((name, sc))
        tris2 = R.restate_tris(tris, d_pos.cpu().numpy())
        trees.append(("fresh", ptamd.Scene(R.refit_nodes(nodes, tris2), tris2)))
        t, q, frames = {n: [] for n, _ in trees}, {n: [] for n, _ in trees}, {}
        for i in range(1 + a.render_reps):
            for name, sc in trees:
                t0 = time.perf_counter()
                sc.render_tiles(cam, prm, tiles.data_ptr(), work.data_ptr(), 0)
                torch.cuda.synchronize()
                if i:
                    t[name].append(time.perf_counter() - t0)
                else:
                    frames[name] = tiles.cpu().numpy()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sc.trace_rays(d_rays)
                e1.record()
                torch.cuda.synchronize()
                if i:
                    q[name].append(e0.elapsed_time(e1))
        row["bit_identical"] = bool(all(np.array_equal(frames[n].view(np.uint32), frames["fresh"].view(np.uint32)) for n in frames))
        row["spread"] = max((np.median(x) - np.min(x)) / np.median(x) for x in t.values())
        for name, sc in trees:
            row[name + "_s_median"] = float(np.median(t[name]))
            row[name + "_s"] = t[name]
            row[name + "_query_ms_median"] = float(np.median(q[name]))
            row[name + "_tree_info"] = sc.tree_info()
            sc.set_mode(0)
            sc.enable_counters(True)
            sc.render(ccam, cprm)
            row[name + "_mode0_counters"] = [int(c) for c in sc.counters()]
            sc.enable_counters(False)
            sc.set_mode(1)
        for name in ("ex", "opt", "fresh"):
            row[name + "_over_refit"] = row[name + "_s_median"] / row["refit_s_median"]
        row["opt_over_fresh"] = row["opt_s_median"] / row["fresh_s_median"]
        row["opt_over_ex"] = row["opt_s_median"] / row["ex_s_median"]
        rows.append(row)
    print(json.dumps({"step": "trees", "workload": "configs[2] geometry, 1920x1080, 1 pass x 256 spp per call; pt_trace_rays closest hit, 2,073,600 rays",
                      "counters": "pt_last_counters of a 480x270, 16 spp frame in mode 0", "turns": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libptamd.so built from the parent commit (the yardstick of the call's cost)")
    ap.add_argument("--kinds", default="1,2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--render-reps", type=int, default=5)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--area-lat-lon", type=int, default=96)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a measurement may take")
    ap.add_argument("--skip", default="", help="comma-separated steps to leave out (area, call, trees)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("area", "call", "trees"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--kind", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--passes", type=int, default=-1, help=argparse.SUPPRESS)
    ap.add_argument("--budget", type=int, default=26, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return {"area": step_area, "call": step_call, "trees": step_trees}[a.step](a)

    base = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--lat-lon", str(a.lat_lon), "--render-reps", str(a.render_reps),
            "--area-lat-lon", str(a.area_lat_lon)]
    skip = set(a.skip.split(","))

    def run(args, lib=None):
        env = dict(os.environ)
        env.pop("PTAMD_LIB", None)
        if lib:
            env["PTAMD_LIB"] = os.path.abspath(lib)
        r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + args, env=env, capture_output=True, text=True)
        if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"rebuild_opt_time.py: step {args} ended with status {r.returncode}; stopping")
        sys.stderr.write(f"done: {' '.join(args)}\n")
        sys.stderr.flush()
        return json.loads(r.stdout.strip().splitlines()[-1])

    def save(res):
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")

    res = {"move": "mesh turned about y + sine wobble + translation, lights translated", "reps": a.reps,
           "yardstick": "pt_scene_rebuild_tree_ex of the parent commit's library" if a.parent_lib else "pt_scene_rebuild_tree_ex of this tree's own library (NOT the parent)",
           "scenes": []}
    if "area" not in skip:
        res["area"] = run(["--step", "area"])
        save(res)
    if "call" not in skip:
        for kind in (int(k) for k in a.kinds.split(",")):
            row = {"kind": kind, "parent": run(["--step", "call", "--kind", str(kind)], a.parent_lib)}
            for passes in (0, 1, 2):
                row[f"passes_{passes}"] = run(["--step", "call", "--kind", str(kind), "--passes", str(passes)])
            row["new_over_parent"] = [n["ms_median"] / p["ms_median"] for n, p in zip(row["passes_2"]["poses"], row["parent"]["poses"])]
            row["split_ms"] = [{"build_as_ex": z["ms_median"], "pass_1": o["ms_median"] - z["ms_median"], "pass_2": t["ms_median"] - o["ms_median"]}
                               for z, o, t in zip(row["passes_0"]["poses"], row["passes_1"]["poses"], row["passes_2"]["poses"])]
            if kind == 1:
                row["no_budget"] = {f"passes_{passes}": run(["--step", "call", "--kind", "1", "--passes", str(passes), "--budget", "0"]) for passes in (0, 2)}
            res["scenes"].append(row)
            save(res)
    if "trees" not in skip:
        res["trees"] = run(["--step", "trees"])
    print(json.dumps(res))
    save(res)


if __name__ == "__main__":
    main()
