"""Time the tree rebuild on the GPU (pt_scene_rebuild_tree) against the host rebuild it replaces, and measure the tree it builds.

  python tools/rebuild_time.py --parent-lib build/libptamd_parent.so [--kinds 1,2] [--reps 20] [--out profiles/rebuild_time_mi355x.json]

Scenes and move as tools/update_time.py: the Cornell room + one stand-in mesh (kind 1, configs[2]) and + four (kind 2), lat_lon 187;
the mesh triangles turned about y through their centroid with a sine wobble and a translation, the two light triangles translated.

  rebuild   update to the 25 degree pose once, then pt_scene_rebuild_tree: HIP events on its stream, median of --reps after warm-up
            (the first call, which allocates, is timed apart); tree_info() before and after; device bytes.  A rebuild the library
            refuses (PT_ERR_UNSUPPORTED: the new tree is too deep for the kernels' stacks) is recorded as refused, its calls timed as
            they are (the whole build and the read-back, no commit), and the uploaded pose is measured as well.
  groups    the same calls under `rocprofv3 --kernel-trace --stats`, kernel time per rebuild summed per group: keys (rb_box_*,
            rb_keys, rb_tmap), sorts and scans (rocPRIM), topology (rb_karras, rb_depth, rb_height), numbering (rb_*_keys,
            rb_level_start, rb_qidx, rb_emit, rb_refs), refit (the dyn_* kernels), area (dyn_area).
  host      pt_bvh_build_sah + pt_scene_create of the moved geometry on the host clock (tools/update_time.py: step_rebuild), with the
            library given by --parent-lib (a build of the parent commit, used through PTAMD_LIB).
  render    kind 1 only: one pass of configs[2] (1920 x 1080, 256 spp) on three trees of the same moved geometry — refit (update
            only), rebuilt (update + rebuild), fresh (host build + upload) — alternating in one process, median of --render-reps,
            for turns of 10 / 25 / 90 degrees; whether the three frames are bit-identical; tree_inflation of the refit tree;
            tree_info of each; and the mode-0 counters (node records fetched, triangle tests) of a 480 x 270, 16 spp frame.

Every measurement is a process of its own under its own `timeout`, one after the other; the first one that fails ends the run
(nothing more is started on the GPU).  Prints one JSON line.
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import update_time as U      # noqa: E402  (the scenes, the move and the host rebuild are its own)

GROUPS = (("keys", ("rb_prim_leaf", "rb_box_partial", "rb_box_final", "rb_keys", "rb_tmap")), ("sorts_and_scans", ("rocprim",)),
          ("topology", ("rb_karras", "rb_depth", "rb_height", "rb_single")),
          ("numbering", ("rb_height_keys", "rb_level_keys", "rb_level_start", "rb_qidx", "rb_emit", "rb_refs")),
          ("refit", ("dyn_tri", "dyn_refit_level", "dyn_nodes", "dyn_quad")), ("area", ("dyn_area",)))
WARM = 3


def step_rebuild(a):
    import numpy as np
    import torch
    ptamd = U._imports()
    dev = torch.device("cuda:0")
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(a.kind, a.lat_lon))
    sc = ptamd.Scene(nodes, tris)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d_pos = U._moved_positions(tris, 25.0, torch, dev)
    st.synchronize()
    info0, bytes0 = sc.tree_info(), sc.device_bytes

    def timed(n_calls):
        """(ms of every call, error text of a refused rebuild or None): a rebuild whose tree is too deep for the kernels' stacks returns
        PT_ERR_UNSUPPORTED after the whole build and the read-back, with the scene as it was — the refused calls are timed as they are."""
        ms, refused = [], None
        for _ in range(n_calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            try:
                sc.rebuild_tree(stream_ptr=st.cuda_stream)
            except ptamd.PtError as e:
                refused = str(e)
            e1.record(st)
            st.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms, refused

    res = {"step": "rebuild", "kind": a.kind, "tris": len(tris), "tree_info_upload": info0, "poses": []}
    for deg in (25.0, 0.0):      # the moved pose; the uploaded pose as well when the moved one is refused
        if deg:
            sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
            st.synchronize()
        else:
            sc = ptamd.Scene(nodes, tris)
        inflation, bytes1 = sc.tree_inflation(), sc.device_bytes
        ms, refused = timed(1 + WARM + a.reps)
        first, ms = ms[0], ms[1 + WARM:]
        res["poses"].append({"degrees": deg, "refused": refused, "rebuild_ms_median": float(np.median(ms)), "rebuild_ms_min": float(np.min(ms)), "rebuild_ms": ms,
                             "first_rebuild_ms": first, "tree_inflation_before": inflation, "tree_inflation_after": sc.tree_inflation(),
                             "tree_info_after": sc.tree_info(), "device_bytes": {"upload": bytes0, "before": bytes1, "after": sc.device_bytes}})
        if a.plain or not refused:
            break
    if a.plain:
        return
    res["rebuild_ms_median"] = res["poses"][0]["rebuild_ms_median"]
    res["refused"] = res["poses"][0]["refused"]
    print(json.dumps(res))


def step_groups(a):
    """Runs `--step rebuild --plain` under rocprofv3 and sums its kernel statistics per group (no GPU work in this process)."""
    prof = "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--step", "rebuild",
               "--plain", "--kind", str(a.kind), "--lat-lon", str(a.lat_lon), "--reps", str(a.reps)]
        r = subprocess.run(["timeout", "-k", "10", str(max(60, a.step_timeout - 30))] + cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(r.returncode)
        rows = []
        for root, _, files in os.walk(d):
            for f in files:
                if f.endswith("kernel_stats.csv"):
                    rows += list(csv.DictReader(open(os.path.join(root, f))))
    calls = 1 + WARM + a.reps
    out = {"step": "groups", "kind": a.kind, "calls": calls, "us_per_rebuild": {}, "launches_per_rebuild": {}}
    taken = set()
    for group, names in GROUPS:      # the one vertex update of the run adds its dyn_* launches to "refit": 1 / calls of that group
        rs = [row for row in rows if row["Name"] not in taken and any((nm + "(") in row["Name"] or (nm + "<") in row["Name"] or (nm == "rocprim" and "rocprim" in row["Name"])
                                                                       for nm in names)]
        taken |= {row["Name"] for row in rs}
        out["us_per_rebuild"][group] = sum(float(row["TotalDurationNs"]) for row in rs) / calls / 1e3
        out["launches_per_rebuild"][group] = sum(int(row["Calls"]) for row in rs) / calls
    out["us_per_rebuild"]["all_kernels"] = sum(out["us_per_rebuild"].values())
    # a refused rebuild runs the whole build and the read-back but no commit: no rb_refs, no refit and no area launch of its own
    out["refused"] = not any("rb_refs(" in row["Name"] for row in rows)
    print(json.dumps(out))


def step_render(a):
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
        refit = ptamd.Scene(nodes, tris)
        refit.update_vertices(d_pos)
        rebuilt = ptamd.Scene(nodes, tris)
        rebuilt.update_vertices(d_pos)
        refused = None
        try:
            rebuilt.rebuild_tree()
        except ptamd.PtError as e:      # too deep for the kernels' stacks: the scene stays the refit one, the row says so
            refused = str(e)
        tris2 = R.restate_tris(tris, d_pos.cpu().numpy())
        fresh = ptamd.Scene(R.refit_nodes(nodes, tris2), tris2)
        trees = (("refit", refit),) + ((("rebuilt", rebuilt),) if refused is None else ()) + (("fresh", fresh),)
        t = {name: [] for name, _ in trees}
        frames = {}
        for i in range(1 + a.render_reps):
            for name, sc in trees:
                t0 = time.perf_counter()
                sc.render_tiles(cam, prm, tiles.data_ptr(), work.data_ptr(), 0)
                torch.cuda.synchronize()
                if i:
                    t[name].append(time.perf_counter() - t0)
                else:
                    frames[name] = tiles.cpu().numpy()
        row = {"degrees": deg, "tree_inflation_refit": refit.tree_inflation(), "rebuild_refused": refused,
               "bit_identical": bool(all(np.array_equal(frames[n].view(np.uint32), frames["fresh"].view(np.uint32)) for n in frames)),
               "spread": max((np.median(x) - np.min(x)) / np.median(x) for x in t.values())}
        for name, sc in trees:
            row[name + "_s_median"] = float(np.median(t[name]))
            row[name + "_tree_info"] = sc.tree_info()
            sc.set_mode(0)
            sc.enable_counters(True)
            sc.render(ccam, cprm)
            cnt = sc.counters()
            sc.enable_counters(False)
            sc.set_mode(1)
            row[name + "_mode0_counters"] = [int(c) for c in cnt]
            # closest-hit query along the frame's 2 M pinhole rays: pt_trace_rays (and wf_drain) walk the 4-wide tree only while
            # 3 * quad_depth + 2 fits their 40-entry stacks, i.e. up to level 12, and the binary tree otherwise
            q_ms = []
            for i in range(1 + a.render_reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sc.trace_rays(d_rays)
                e1.record()
                torch.cuda.synchronize()
                if i:
                    q_ms.append(e0.elapsed_time(e1))
            row[name + "_query_ms_median"] = float(np.median(q_ms))
            row[name + "_query_walks_quad"] = bool(3 * sc.tree_info()["quad_depth"] + 2 <= 40)
        if refused is None:
            row["rebuilt_over_refit"] = row["rebuilt_s_median"] / row["refit_s_median"]
            row["rebuilt_over_fresh"] = row["rebuilt_s_median"] / row["fresh_s_median"]
        row["refit_over_fresh"] = row["refit_s_median"] / row["fresh_s_median"]
        rows.append(row)
    print(json.dumps({"step": "render", "workload": "configs[2] geometry, 1920x1080, 1 pass x 256 spp per call",
                      "counters": "pt_last_counters of a 480x270, 16 spp frame in mode 0", "turns": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libptamd.so built from the parent commit (the yardstick: the host rebuild)")
    ap.add_argument("--kinds", default="1,2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rebuild-reps", type=int, default=3)
    ap.add_argument("--render-reps", type=int, default=5)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a measurement may take")
    ap.add_argument("--skip", default="", help="comma-separated steps to leave out (rebuild, groups, host, render)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("rebuild", "groups", "host", "render"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--kind", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--plain", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return {"rebuild": step_rebuild, "groups": step_groups, "host": U.step_rebuild, "render": step_render}[a.step](a)

    base = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--lat-lon", str(a.lat_lon), "--rebuild-reps", str(a.rebuild_reps),
            "--render-reps", str(a.render_reps)]
    skip = set(a.skip.split(","))

    def run(args, lib=None):
        env = dict(os.environ)
        env.pop("PTAMD_LIB", None)
        if lib:
            env["PTAMD_LIB"] = os.path.abspath(lib)
        r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + args, env=env, capture_output=True, text=True)
        if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"rebuild_time.py: step {args} ended with status {r.returncode}; stopping")
        sys.stderr.write(f"done: {' '.join(args)}\n")
        sys.stderr.flush()
        return json.loads(r.stdout.strip().splitlines()[-1])

    res = {"move": "mesh turned 25 degrees about y + sine wobble + translation, lights translated", "reps": a.reps,
           "host_yardstick": "parent" if a.parent_lib else "this tree's own library (NOT the parent)", "scenes": []}
    for kind in (int(k) for k in a.kinds.split(",")):
        row = {"kind": kind}
        if "rebuild" not in skip:
            row["rebuild"] = run(["--step", "rebuild", "--kind", str(kind)])
        if "groups" not in skip:
            row["groups"] = run(["--step", "groups", "--kind", str(kind)])
        if "host" not in skip:
            row["host"] = run(["--step", "host", "--kind", str(kind)], a.parent_lib)
        if "rebuild" in row and "host" in row:
            row["host_over_gpu"] = row["host"]["rebuild_ms_median"] / row["rebuild"]["rebuild_ms_median"]
        res["scenes"].append(row)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")
    if "render" not in skip:
        res["render"] = run(["--step", "render"])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
