"""Time the vertex update (pt_scene_update_vertices) on the GPU against what it replaces, and the render cost of a refit tree.

  python tools/update_time.py --parent-lib build/libptamd_parent.so [--kinds 1,2] [--reps 20] [--out profiles/update_time.json]

Scenes: the Cornell room + one stand-in mesh (kind 1, configs[2]) and + four (kind 2), lat_lon 187.  The move: the mesh triangles
turned 25 degrees about y through their centroid with a sine wobble and a translation, the two light triangles translated
(tests/dynamic_ref.py).

  update    one pt_scene_update_vertices, HIP events on its stream, median of --reps after warm-up; the bytes it moves; the
            pt_dbg_triad rate of this GPU for comparison.
  groups    the same calls under `rocprofv3 --kernel-trace --stats`, kernel time per call summed per group: records (dyn_leafbox,
            dyn_surf, dyn_tri, dyn_lights), binary refit (dyn_refit_level), nodes (dyn_nodes), quad (dyn_quad), core (dyn_core_*).
  rebuild   pt_bvh_build_sah + pt_scene_create of the moved geometry on the host clock, with the library given by --parent-lib
            (a build of the parent commit, tools/build_variant.sh, used through PTAMD_LIB): the yardstick is never the build under
            test.  Without --parent-lib this tree's library does it and the result says so.
  render    kind 1 only: one pass of configs[2] (1920 x 1080, 256 spp) on the refit scene and on a fresh upload of the same moved
            geometry, alternating in one process, with pt_scene_tree_inflation, for turns of 10 / 25 / 90 degrees.

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
GROUPS = (("records", ("dyn_leafbox", "dyn_surf", "dyn_tri", "dyn_lights")), ("binary_refit", ("dyn_refit_level",)), ("nodes", ("dyn_nodes",)),
          ("quad", ("dyn_quad",)), ("core", ("dyn_core_partial", "dyn_core_final")))
WARM = 3


def _imports():
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes as C
    import ptamd
    have = C.CDLL(ptamd.LIB_PATH)      # a build of the parent commit lacks the new calls: bind what the library exports
    ptamd.API[:] = [e for e in ptamd.API if hasattr(have, e[0])]
    return ptamd


def _moved_positions(tris, deg, torch, dev):
    import dynamic_ref as R
    pos = torch.from_numpy(R.positions(tris)).to(dev)
    pos = R.move_rigid_wobble(pos, torch.from_numpy(R.mesh_mask(tris)).to(dev), torch, deg=deg)
    pos = R.move_translate(pos, torch.from_numpy(R.emissive(tris)).to(dev), torch)
    return pos.reshape(-1, 9).contiguous()


def step_update(a):
    import numpy as np
    import torch
    ptamd = _imports()
    dev = torch.device("cuda:0")
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(a.kind, a.lat_lon))
    sc = ptamd.Scene(nodes, tris)
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d_pos = _moved_positions(tris, 25.0, torch, dev)
    st.synchronize()
    ms = []
    for i in range(WARM + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
        e1.record(st)
        st.synchronize()
        if i >= WARM:
            ms.append(e0.elapsed_time(e1))
    if a.plain:
        return
    n = len(tris)
    sizes = {k: sc.dbg_array(k).nbytes for k in ("nodes", "quad", "tri", "tripair", "leafbox", "surf", "lights")}
    # bytes of the record kernels: positions read by dyn_leafbox, dyn_surf and (two triangles each) dyn_tri; surf floats 0..11 written and
    # 8..11 read; tri, tripair, leafbox written; the leaf boxes read back per pair record; the maps
    rec_bytes = n * 36 * 4 + n * 48 + n * 16 + sizes["tri"] + sizes["tripair"] + sizes["leafbox"] + n * 2 * 32 + n * 16
    res = {"step": "update", "kind": a.kind, "tris": n, "update_ms_median": float(np.median(ms)), "update_ms_min": float(np.min(ms)), "update_ms": ms,
           "tree_inflation": sc.tree_inflation(), "array_bytes": sizes, "record_bytes": rec_bytes, "device_bytes": sc.device_bytes,
           "triad_gb_per_s": ptamd.triad_gbps(1 << 28, 5)}
    print(json.dumps(res))


def step_groups(a):
    """Runs `--step update --plain` under rocprofv3 and sums its kernel statistics per group (no GPU work in this process)."""
    prof = "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--step", "update",
               "--plain", "--kind", str(a.kind), "--lat-lon", str(a.lat_lon), "--reps", str(a.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(r.returncode)
        rows = []
        for root, _, files in os.walk(d):
            for f in files:
                if f.endswith("kernel_stats.csv"):
                    rows += list(csv.DictReader(open(os.path.join(root, f))))
    calls = WARM + a.reps
    out = {"step": "groups", "kind": a.kind, "calls": calls, "us_per_update": {}, "launches_per_update": {}}
    for group, names in GROUPS:
        rs = [row for row in rows if any(f"::{nm}(" in row["Name"] or f" {nm}(" in row["Name"] for nm in names)]
        out["us_per_update"][group] = sum(float(row["TotalDurationNs"]) for row in rs) / calls / 1e3
        out["launches_per_update"][group] = sum(int(row["Calls"]) for row in rs) / calls
    out["us_per_update"]["all_kernels"] = sum(out["us_per_update"].values())
    print(json.dumps(out))


def step_rebuild(a):
    import numpy as np
    ptamd = _imports()
    import dynamic_ref as R
    prims = ptamd.gen_scene(a.kind, a.lat_lon)
    # the moved primitives: the same move applied to the vertex positions of the input records (3 x 28 floats, position first)
    v = prims.reshape(-1, 3, 28)
    p = np.ascontiguousarray(v[:, :, 0:3])
    diag = np.sqrt(((p.max(1) - p.min(1)).astype(np.float64) ** 2).sum(1))
    emit = (np.abs(v[:, :, 14:17]).sum((1, 2)) > 0)
    p = R.move_rigid_wobble(p, (~emit) & (diag < 10.0), np)
    v[:, :, 0:3] = R.move_translate(p, emit, np)
    secs = []
    for _ in range(a.rebuild_reps):
        t0 = time.perf_counter()
        nodes, tris, _ = ptamd.build_bvh(prims)
        t1 = time.perf_counter()
        sc = ptamd.Scene(nodes, tris)
        t2 = time.perf_counter()
        sc.close()
        secs.append((t2 - t0, t1 - t0, t2 - t1))
    secs.sort()
    mid = secs[len(secs) // 2]
    print(json.dumps({"step": "rebuild", "kind": a.kind, "lib": os.path.basename(ptamd.LIB_PATH), "rebuild_ms_median": mid[0] * 1e3,
                      "bvh_build_sah_ms": mid[1] * 1e3, "scene_create_ms": mid[2] * 1e3, "all": secs}))


def step_render(a):
    import numpy as np
    import torch
    ptamd = _imports()
    import dynamic_ref as R
    dev = torch.device("cuda:0")
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, a.lat_lon))
    W, H = 1920, 1080
    cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=1, spp_per_pass=256, rank=0, world=1)
    tiles = torch.empty(ptamd.tiles_floats(cam, prm), dtype=torch.float32, device=dev)
    work = torch.empty(ptamd.work_bytes(cam, prm), dtype=torch.uint8, device=dev)
    rows = []
    for deg in (10.0, 25.0, 90.0):
        d_pos = _moved_positions(tris, deg, torch, dev)
        torch.cuda.synchronize()
        refit = ptamd.Scene(nodes, tris)
        refit.update_vertices(d_pos)
        tris2 = R.restate_tris(tris, d_pos.cpu().numpy())
        fresh = ptamd.Scene(R.refit_nodes(nodes, tris2), tris2)
        t = {"refit": [], "fresh": []}
        frames = {}
        for i in range(1 + a.render_reps):
            for name, sc in (("refit", refit), ("fresh", fresh)):
                t0 = time.perf_counter()
                sc.render_tiles(cam, prm, tiles.data_ptr(), work.data_ptr(), 0)
                torch.cuda.synchronize()
                if i:
                    t[name].append(time.perf_counter() - t0)
                else:
                    frames[name] = tiles.cpu().numpy()
        rows.append({"degrees": deg, "tree_inflation": refit.tree_inflation(), "refit_s_median": float(np.median(t["refit"])),
                     "fresh_s_median": float(np.median(t["fresh"])), "refit_over_fresh": float(np.median(t["refit"]) / np.median(t["fresh"])),
                     "spread": max((np.median(x) - np.min(x)) / np.median(x) for x in t.values()),
                     "bit_identical": bool(np.array_equal(frames["refit"].view(np.uint32), frames["fresh"].view(np.uint32)))})
    print(json.dumps({"step": "render", "workload": "configs[2] geometry, 1920x1080, 1 pass x 256 spp per call", "turns": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libptamd.so built from the parent commit (the yardstick of the rebuild)")
    ap.add_argument("--kinds", default="1,2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rebuild-reps", type=int, default=3)
    ap.add_argument("--render-reps", type=int, default=5)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a measurement may take")
    ap.add_argument("--skip", default="", help="comma-separated steps to leave out (update, groups, rebuild, render)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("update", "groups", "rebuild", "render"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--kind", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--plain", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return {"update": step_update, "groups": step_groups, "rebuild": step_rebuild, "render": step_render}[a.step](a)

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
            sys.exit(f"update_time.py: step {args} ended with status {r.returncode}; stopping")
        sys.stderr.write(f"done: {' '.join(args)}\n")
        sys.stderr.flush()
        return json.loads(r.stdout.strip().splitlines()[-1])

    res = {"move": "mesh turned 25 degrees about y + sine wobble + translation, lights translated", "reps": a.reps,
           "rebuild_yardstick": "parent" if a.parent_lib else "this tree's own library (NOT the parent)", "scenes": []}
    for kind in (int(k) for k in a.kinds.split(",")):
        row = {"kind": kind}
        if "update" not in skip:
            row["update"] = run(["--step", "update", "--kind", str(kind)])
        if "groups" not in skip:
            row["groups"] = run(["--step", "groups", "--kind", str(kind)])
        if "rebuild" not in skip:
            row["rebuild"] = run(["--step", "rebuild", "--kind", str(kind)], a.parent_lib)
        if "update" in row and "rebuild" in row:
            row["rebuild_over_update"] = row["rebuild"]["rebuild_ms_median"] / row["update"]["update_ms_median"]
        if "update" in row and "groups" in row:
            rec_s = row["groups"]["us_per_update"]["records"] * 1e-6
            row["records_gb_per_s"] = row["update"]["record_bytes"] / rec_s / 1e9
            row["records_fraction_of_triad"] = row["records_gb_per_s"] / row["update"]["triad_gb_per_s"]
        res["scenes"].append(row)
    if "render" not in skip:
        res["render"] = run(["--step", "render"])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
