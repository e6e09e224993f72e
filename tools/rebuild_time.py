"""Time and compare the tree rebuild on the GPU: the three entry points (pt_scene_rebuild_tree, _ex, _opt) against each other, against
the host rebuild they replace and against another build of the library, and measure the trees they build.

  python tools/rebuild_time.py --run host|budget|opt|ab --parent-lib build/libptamd_parent.so [--kinds 1,2] [--reps 20] [--out FILE.json]

Scenes and move as tools/update_time.py: the Cornell room + one stand-in mesh (kind 1, configs[2]) and + four (kind 2), lat_lon 187;
the mesh triangles turned about y through their centroid with a sine wobble and a translation, the two light triangles translated.
A step is one measurement in a process of its own; the library it loads is this tree's, or the one PTAMD_LIB names.

  rebuild   update to the 25 degree pose once, then pt_scene_rebuild_tree: HIP events on its stream, median of --reps after warm-up
            (the first call, which allocates, is timed apart); tree_info() before and after; device bytes.  A rebuild the library
            refuses (PT_ERR_UNSUPPORTED: the new tree is too deep for the kernels' stacks) is recorded as refused, its calls timed as
            they are (the whole build and the read-back, no commit), and the uploaded pose is measured as well.
  groups    the same calls under `rocprofv3 --kernel-trace --stats`, kernel time per rebuild summed per group: keys (rb_box_*,
            rb_keys, rb_tmap), sorts and scans (rocPRIM), topology (rb_karras, rb_depth, rb_height), numbering (rb_*_keys,
            rb_level_start, rb_qidx, rb_emit, rb_refs), refit (the dyn_* kernels), area (dyn_area).
  host      pt_bvh_build_sah + pt_scene_create of the moved geometry on the host clock (tools/update_time.py: step_rebuild).
  render    kind 1 only: one pass of configs[2] (1920 x 1080, 256 spp) on three trees of the same moved geometry — refit (update
            only), rebuilt (update + rebuild), fresh (host build + upload) — alternating in one process, median of --render-reps,
            for turns of 10 / 25 / 90 degrees; whether the three frames are bit-identical; tree_inflation of the refit tree;
            tree_info of each; and the mode-0 counters (node records fetched, triangle tests) of a 480 x 270, 16 spp frame.
  area      no GPU: tests/rebuild_opt_ref.py with (26, 1/16) on the stand-in scene of the tests (kind 1, lat_lon 16) and on kind 1 at
            --area-lat-lon, the sum of the interior boxes' areas after 1 .. 4 passes as a fraction of the unoptimised tree's, and the
            smallest pass count after which one more pass gains less than 1 % of the area sum.
  call      one call, --call plain|ex|opt with --budget, --fraction, --passes, at the uploaded pose (0 degrees) and the 25 degree pose:
            HIP events around the call on its stream, median of --reps after warm-up (the first call, which allocates, apart);
            tree_info, the report and the device bytes afterwards; whether it was refused.
  trees     kind 1: one pass of configs[2] and the closest-hit query along the frame's 2.07 M pinhole rays on trees of the same moved
            geometry, alternating in one process, for turns of 10 / 25 / 90 degrees.  --variants names the trees (VARIANTS): refit
            (update only), fresh (host build + upload), and update + a rebuild: plain, ex, budget_only (26, 0), classes_only
            (0, 1/16), opt.  Medians of --render-reps, whether all frames are bit-identical, tree_info, the report, the mode-0 counters.
  arrays    one JSON line per case — the sha256 of nodes, quad, tri and tripair, tree_info, the report and the device bytes after one
            call on a fresh scene: kinds 1 and 2 at 0 and 25 degrees under ARRAY_CALLS.  A refused call is recorded as refused.

A run (--run) is a sequence of steps, one after the other, each under its own `timeout`; the first one that fails ends the run
(nothing more is started on the GPU).  Prints one JSON line.
  host      rebuild, groups, host per kind, render: the GPU rebuild against the host rebuild (profiles/rebuild_time_mi355x.json)
  budget    call ex with its defaults against call plain of --parent-lib, trees refit,plain,ex,budget_only,classes_only,fresh
            (profiles/rebuild_budget_mi355x.json, once tools/rebuild_budget_time.py)
  opt       area; call opt with (26, 1/16) and 0, 1, 2 passes against call ex of --parent-lib, kind 1 also with (0, 1/16) and 0, 2 passes;
            trees refit,ex,opt,fresh (profiles/rebuild_opt_mi355x.json, once tools/rebuild_opt_time.py)
  ab        this tree's library against --parent-lib where both must compute the same: arrays once per library, compared case by
            case (everything equal; the device bytes are listed side by side); then AB_CALLS per kind, --ab-rounds rounds of three
            processes — the parent's, this tree's, the parent's again.  The spread of the parent's medians over its processes is
            the margin the difference of new and parent must lie inside (profiles/rebuild_refactor_mi355x.json)
"""
import argparse
import csv
import hashlib
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

DEFAULTS = (26, 0.0625)      # pt_rebuild_params_default
# the trees of the `trees` step: None = no rebuild, else (call, depth_budget, large_fraction, passes)
VARIANTS = {"refit": None, "fresh": None, "plain": ("plain", 0, 0.0, 0), "ex": ("ex",) + DEFAULTS + (0,), "budget_only": ("ex", 26, 0.0, 0),
            "classes_only": ("ex", 0, 0.0625, 0), "opt": ("opt",) + DEFAULTS + (2,)}
ARRAY_CALLS = (("plain", 0, 0.0, 0), ("ex", 26, 0.0625, 0), ("ex", 0, 0.0, 0), ("ex", 26, 0.0, 0), ("ex", 0, 0.0625, 0), ("opt", 26, 0.0625, 0),
               ("opt", 26, 0.0625, 1), ("opt", 26, 0.0625, 2), ("opt", 0, 0.0625, 2))
AB_CALLS = (("plain", 0, 0.0, 0), ("ex",) + DEFAULTS + (0,), ("opt", 26, 0.0625, 2), ("opt", 0, 0.0625, 2))


def _rebuild(sc, call, budget, fraction, passes, stream_ptr=0):
    """The call by name; the report of ex and opt as a dict, None for plain."""
    if call == "plain":
        return sc.rebuild_tree(stream_ptr=stream_ptr)
    if call == "ex":
        return sc.rebuild_tree(stream_ptr=stream_ptr, depth_budget=budget, large_fraction=fraction)
    return sc.rebuild_tree_optimized(passes=passes, depth_budget=budget, large_fraction=fraction, stream_ptr=stream_ptr)


def _library():
    return "the one PTAMD_LIB names" if os.environ.get("PTAMD_LIB") else "this tree's"


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
    res = {"step": "call", "kind": a.kind, "tris": len(tris), "call": [a.call, a.budget, a.fraction, a.passes], "library": _library(), "poses": []}
    for deg in (0.0, 25.0):
        sc = ptamd.Scene(nodes, tris)
        if deg:
            sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
            st.synchronize()
        ms, refused, report = [], None, None
        for _ in range(1 + WARM + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            try:
                report = _rebuild(sc, a.call, a.budget, a.fraction, a.passes, st.cuda_stream)
            except ptamd.PtError as e:      # too deep for the kernels' stacks: the whole build and the read-back ran, no commit
                refused = str(e)
            e1.record(st)
            st.synchronize()
            ms.append(e0.elapsed_time(e1))
        first, ms = ms[0], ms[1 + WARM:]
        res["poses"].append({"degrees": deg, "refused": refused, "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms": ms, "first_ms": first,
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
        for name in a.variants.split(","):
            if name == "fresh":
                tris2 = R.restate_tris(tris, d_pos.cpu().numpy())
                trees.append((name, ptamd.Scene(R.refit_nodes(nodes, tris2), tris2)))
                continue
            sc = ptamd.Scene(nodes, tris)
            sc.update_vertices(d_pos)
            if name == "refit":
                row["tree_inflation_refit"] = sc.tree_inflation()
            else:
                try:
                    row[name + "_report"] = _rebuild(sc, *VARIANTS[name])
                except ptamd.PtError as e:      # the scene stays the refit one; the row says so and the tree is left out
                    row[name + "_refused"] = str(e)
                    continue
            trees.append((name, sc))
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
        first = next(iter(frames.values())).view(np.uint32)
        row["bit_identical"] = bool(all(np.array_equal(f.view(np.uint32), first) for f in frames.values()))
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
            row[name + "_over_" + trees[0][0]] = row[name + "_s_median"] / row[trees[0][0] + "_s_median"]
        rows.append(row)
    print(json.dumps({"step": "trees", "workload": "configs[2] geometry, 1920x1080, 1 pass x 256 spp per call; pt_trace_rays closest hit, 2,073,600 rays",
                      "counters": "pt_last_counters of a 480x270, 16 spp frame in mode 0", "variants": a.variants, "turns": rows}))


def step_arrays(a):
    import torch
    ptamd = U._imports()
    dev = torch.device("cuda:0")

    def hashes(sc):
        return {name: hashlib.sha256(sc.dbg_array(name).tobytes()).hexdigest() for name in ("nodes", "quad", "tri", "tripair")}

    for kind in (1, 2):
        nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(kind, a.lat_lon))
        d_pos = U._moved_positions(tris, 25.0, torch, dev)
        torch.cuda.synchronize()
        for deg in (0.0, 25.0):
            for call in ARRAY_CALLS:
                sc = ptamd.Scene(nodes, tris)
                if deg:
                    sc.update_vertices(d_pos)
                before, refused, report = hashes(sc), None, None
                try:
                    report = _rebuild(sc, *call)
                except ptamd.PtError as e:
                    refused = str(e)
                after = hashes(sc)
                print(json.dumps({"step": "arrays", "library": _library(), "kind": kind, "tris": len(tris), "degrees": deg, "call": list(call), "refused": refused,
                                  "unchanged": after == before, "sha256": after, "tree_info": sc.tree_info(), "report": report, "device_bytes": sc.device_bytes}))


STEPS = {"rebuild": step_rebuild, "groups": step_groups, "host": U.step_rebuild, "render": step_render, "area": step_area, "call": step_call,
         "trees": step_trees, "arrays": step_arrays}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", choices=("host", "budget", "opt", "ab"), default="host")
    ap.add_argument("--parent-lib", default=None, help="libptamd.so built from the parent commit (the yardstick)")
    ap.add_argument("--kinds", default="1,2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rebuild-reps", type=int, default=3)
    ap.add_argument("--render-reps", type=int, default=5)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--area-lat-lon", type=int, default=96)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a step may take")
    ap.add_argument("--skip", default="", help="comma-separated steps to leave out of the run")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=tuple(STEPS), default=None, help="run this one step in this process")
    ap.add_argument("--kind", type=int, default=1)
    ap.add_argument("--plain", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--call", choices=("plain", "ex", "opt"), default="plain")
    ap.add_argument("--budget", type=int, default=DEFAULTS[0])
    ap.add_argument("--fraction", type=float, default=DEFAULTS[1])
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--variants", default="refit,plain,ex,opt,fresh")
    ap.add_argument("--ab-rounds", type=int, default=3, help="run ab: rounds of (parent, new, parent) per call")
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a)

    base = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--lat-lon", str(a.lat_lon), "--rebuild-reps", str(a.rebuild_reps),
            "--render-reps", str(a.render_reps), "--area-lat-lon", str(a.area_lat_lon)]
    skip = set(a.skip.split(","))
    kinds = [int(k) for k in a.kinds.split(",")]
    res = {"run": a.run, "move": "mesh turned 25 degrees about y + sine wobble + translation, lights translated", "reps": a.reps,
           "yardstick": "the parent commit's library" if a.parent_lib else "this tree's own library (NOT the parent)"}

    def run(step, *args, lib=None, lines=False):
        """One step as a process of its own; None where the step is skipped.  lib: the library it loads instead of this tree's."""
        if step in skip:
            return None
        env = dict(os.environ)
        env.pop("PTAMD_LIB", None)
        if lib:
            env["PTAMD_LIB"] = os.path.abspath(lib)
        args = ["--step", step] + [str(x) for x in args]
        r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + args, env=env, capture_output=True, text=True)
        if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"rebuild_time.py: step {args} ended with status {r.returncode}; stopping")
        sys.stderr.write(f"done: {' '.join(args)}{' (parent library)' if lib else ''}\n")
        sys.stderr.flush()
        out = [json.loads(x) for x in r.stdout.strip().splitlines() if x.startswith("{")]
        save()
        return out if lines else out[-1]

    def save():
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res) + "\n")

    def call(kind, c, lib=None):
        return run("call", "--kind", kind, "--call", c[0], "--budget", c[1], "--fraction", c[2], "--passes", c[3], lib=lib)

    def medians(row):
        return [p["ms_median"] for p in row["poses"]]

    scenes = res.setdefault("scenes", [])
    if a.run == "host":
        for kind in kinds:
            row = {"kind": kind, "rebuild": run("rebuild", "--kind", kind), "groups": run("groups", "--kind", kind), "host": run("host", "--kind", kind, lib=a.parent_lib)}
            if row["rebuild"] and row["host"]:
                row["host_over_gpu"] = row["host"]["rebuild_ms_median"] / row["rebuild"]["rebuild_ms_median"]
            scenes.append(row)
        res["render"] = run("render")
    elif a.run == "budget":
        for kind in kinds:
            row = {"kind": kind, "new": call(kind, VARIANTS["ex"]), "parent": call(kind, VARIANTS["plain"], a.parent_lib)}
            if row["new"] and row["parent"]:
                row["new_over_parent"] = [n / p for n, p in zip(medians(row["new"]), medians(row["parent"]))]
            scenes.append(row)
        res["trees"] = run("trees", "--variants", "refit,plain,ex,budget_only,classes_only,fresh")
    elif a.run == "opt":
        res["area"] = run("area")
        for kind in kinds:
            row = {"kind": kind, "parent": call(kind, VARIANTS["ex"], a.parent_lib)}
            for passes in (0, 1, 2):
                row[f"passes_{passes}"] = call(kind, ("opt",) + DEFAULTS + (passes,))
            if row["parent"]:
                row["new_over_parent"] = [n / p for n, p in zip(medians(row["passes_2"]), medians(row["parent"]))]
                row["split_ms"] = [{"build_as_ex": z, "pass_1": o - z, "pass_2": t - o} for z, o, t in zip(*(medians(row[f"passes_{k}"]) for k in (0, 1, 2)))]
            if kind == 1:
                row["no_budget"] = {f"passes_{passes}": call(1, ("opt", 0, DEFAULTS[1], passes)) for passes in (0, 2)}
            scenes.append(row)
        res["trees"] = run("trees", "--variants", "refit,ex,opt,fresh")
    else:
        new, old = run("arrays", lines=True), run("arrays", lib=a.parent_lib, lines=True)
        if new and old:
            same = ("kind", "tris", "degrees", "call", "refused", "unchanged", "sha256", "tree_info", "report")
            res["arrays"] = [{**{k: n[k] for k in same}, "equal": all(n[k] == o[k] for k in same), "device_bytes": n["device_bytes"], "device_bytes_parent": o["device_bytes"]}
                             for n, o in zip(new, old)]
            res["arrays_equal"] = len(new) == len(old) == 4 * len(ARRAY_CALLS) and all(r["equal"] for r in res["arrays"])
        res["calls"] = []
        for kind in kinds:
            for c in AB_CALLS:      # per round three processes next to each other in time: the parent's library, this tree's, the parent's again
                runs = {"parent": [], "new": []}
                for _ in range(a.ab_rounds):
                    for who in ("parent", "new", "parent"):
                        runs[who].append(call(kind, c, a.parent_lib if who == "parent" else None))
                row = {"kind": kind, "call": list(c)}
                if all(r for rs in runs.values() for r in rs):
                    for who, rs in runs.items():      # per pose (0 and 25 degrees), the median of every process
                        row[who + "_ms_median"] = [list(x) for x in zip(*(medians(r) for r in rs))]
                    mid = lambda xs: sorted(xs)[len(xs) // 2] if len(xs) % 2 else (sorted(xs)[len(xs) // 2 - 1] + sorted(xs)[len(xs) // 2]) / 2
                    row["new_minus_parent"] = [mid(n) - mid(p) for n, p in zip(row["new_ms_median"], row["parent_ms_median"])]
                    row["parent_spread"] = [max(p) - min(p) for p in row["parent_ms_median"]]
                    row["inside"] = all(d <= sp for d, sp in zip(row["new_minus_parent"], row["parent_spread"]))
                res["calls"].append(row)
        # the margin nobody can fix in advance: per row, the parent-against-parent difference of medians seen in this run
        if all("inside" in r for r in res["calls"]):
            res["every_row_inside_its_parent_spread"] = all(r["inside"] for r in res["calls"])
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
