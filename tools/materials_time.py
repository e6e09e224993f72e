"""Time the material update (pt_scene_update_materials) on the GPU against what it replaces.

  python tools/materials_time.py --parent-lib build/libptamd_parent.so [--kinds 1,2] [--reps 20] [--out profiles/materials_time.json]

Scenes: the Cornell room + one stand-in mesh (kind 1, configs[2]) and + four (kind 2), lat_lon 187.  Material sets of
tests/materials_ref.py: (a) every triangle a new albedo / specular / opacity / roughness / metallic, the two lights kept; (b) the
uploaded lights off and a seeded 30 % of all triangles emitting.

  update    one pt_scene_update_materials of a device tensor, host clock (the call waits for the stream once; the clock stops after a
            synchronise that also covers the light records, which are written after that wait), median of --reps after warm-up, the two
            sets applied in turn so that every call changes the set of lights; the bytes the kernels move; the pt_dbg_triad rate of this GPU.
  groups    the same calls under `rocprofv3 --kernel-trace --stats`: kernel time per call of mat_apply (phase A), mat_scan, mat_lights
            (phase B).
  create    pt_scene_create of the same triangles with the new materials on the host clock, with the library given by --parent-lib
            (a build of the parent commit, used through PTAMD_LIB): the yardstick is never the build under test.  Without --parent-lib
            this tree's library does it and the result says so.

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
KERNELS = ("mat_apply", "mat_scan", "mat_lights")
WARM = 3
SEED = 20


def _imports():
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ctypes as C
    import ptamd
    have = C.CDLL(ptamd.LIB_PATH)      # a build of the parent commit lacks the new calls: bind what the library exports
    ptamd.API[:] = [e for e in ptamd.API if hasattr(have, e[0])]
    return ptamd


def step_update(a):
    import numpy as np
    import torch
    ptamd = _imports()
    import materials_ref as M
    dev = torch.device("cuda:0")
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(a.kind, a.lat_lon))
    sets = {"a": M.set_a(tris, SEED), "b": M.set_b(tris, SEED)}
    d_mat = {k: torch.from_numpy(v).to(dev) for k, v in sets.items()}
    torch.cuda.synchronize()
    sc = ptamd.Scene(nodes, tris)
    ms = {"a": [], "b": []}
    call_ms = {"a": [], "b": []}
    for i in range(WARM + a.reps):
        for k in ("a", "b"):
            t0 = time.perf_counter()
            sc.update_materials(d_mat[k])
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i >= WARM:
                ms[k].append((t2 - t0) * 1e3)
                call_ms[k].append((t1 - t0) * 1e3)
    if a.plain:
        return
    n = len(tris)
    blocks = (n + 255) // 256
    res = {"step": "update", "kind": a.kind, "tris": n, "device_bytes": sc.device_bytes, "triad_gb_per_s": ptamd.triad_gbps(1 << 28, 5), "sets": {}}
    for k in ("a", "b"):
        nl = int(M.is_light(sets[k]).sum())
        res["sets"][k] = {"lights": nl, "update_ms_median": float(np.median(ms[k])), "update_ms_min": float(np.min(ms[k])),
                          "call_ms_median": float(np.median(call_ms[k])), "update_ms": ms[k],
                          # phase A: 48 bytes read and 48 written per triangle, one pair per block; phase B: the emittance quad of every
                          # surface record and the block offsets read, per light 36 bytes of positions read, 64 + 4 written
                          "phase_a_bytes": n * 96 + blocks * 8, "phase_b_bytes": n * 16 + blocks * 8 + nl * 104}
    print(json.dumps(res))


def step_groups(a):
    """Runs `--step update --plain` under rocprofv3 and sums its kernel statistics per kernel (no GPU work in this process)."""
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
    calls = 2 * (WARM + a.reps)      # both sets per repetition
    out = {"step": "groups", "kind": a.kind, "calls": calls, "us_per_update": {}, "launches_per_update": {}}
    for nm in KERNELS:
        rs = [row for row in rows if f"::{nm}(" in row["Name"] or f" {nm}(" in row["Name"]]
        out["us_per_update"][nm] = sum(float(row["TotalDurationNs"]) for row in rs) / calls / 1e3
        out["launches_per_update"][nm] = sum(int(row["Calls"]) for row in rs) / calls
    out["us_per_update"]["all_kernels"] = sum(out["us_per_update"].values())
    print(json.dumps(out))


def step_create(a):
    ptamd = _imports()
    import dynamic_ref as R
    import materials_ref as M
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(a.kind, a.lat_lon))
    out = {"step": "create", "kind": a.kind, "lib": os.path.basename(ptamd.LIB_PATH), "sets": {}}
    ptamd.Scene(nodes, tris).close()      # the first call of a process pays for the device and the code objects
    for k, mat in (("a", M.set_a(tris, SEED)), ("b", M.set_b(tris, SEED))):
        tris2 = R.restate_tris(M.apply_materials(tris, mat), R.positions(tris))
        secs = []
        for _ in range(a.create_reps):
            t0 = time.perf_counter()
            sc = ptamd.Scene(nodes, tris2)
            secs.append(time.perf_counter() - t0)
            sc.close()
        secs.sort()
        out["sets"][k] = {"scene_create_ms_median": secs[len(secs) // 2] * 1e3, "all_ms": [s * 1e3 for s in secs]}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libptamd.so built from the parent commit (the yardstick)")
    ap.add_argument("--kinds", default="1,2")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--create-reps", type=int, default=5)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a measurement may take")
    ap.add_argument("--skip", default="", help="comma-separated steps to leave out (update, groups, create)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=("update", "groups", "create"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--kind", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--plain", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return {"update": step_update, "groups": step_groups, "create": step_create}[a.step](a)

    base = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--lat-lon", str(a.lat_lon), "--create-reps", str(a.create_reps)]
    skip = set(a.skip.split(","))

    def run(args, lib=None):
        env = dict(os.environ)
        env.pop("PTAMD_LIB", None)
        if lib:
            env["PTAMD_LIB"] = os.path.abspath(lib)
        r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + args, env=env, capture_output=True, text=True)
        if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit(f"materials_time.py: step {args} ended with status {r.returncode}; stopping")
        sys.stderr.write(f"done: {' '.join(args)}\n")
        sys.stderr.flush()
        return json.loads(r.stdout.strip().splitlines()[-1])

    res = {"sets": "(a) new albedo, specular, opacity, roughness, metallic, the lights kept; (b) the lights off, a seeded 30 % of all triangles emitting",
           "reps": a.reps, "create_yardstick": "parent" if a.parent_lib else "this tree's own library (NOT the parent)", "scenes": []}
    for kind in (int(k) for k in a.kinds.split(",")):
        row = {"kind": kind}
        if "update" not in skip:
            row["update"] = run(["--step", "update", "--kind", str(kind)])
        if "groups" not in skip:
            row["groups"] = run(["--step", "groups", "--kind", str(kind)])
        if "create" not in skip:
            row["create"] = run(["--step", "create", "--kind", str(kind)], a.parent_lib)
        if "update" in row and "create" in row:
            row["create_over_update"] = {k: row["create"]["sets"][k]["scene_create_ms_median"] / row["update"]["sets"][k]["update_ms_median"] for k in ("a", "b")}
        if "update" in row and "groups" in row:
            # both sets alternate under the profiler: the rate of phase A, whose bytes are the same for either set
            a_s = row["groups"]["us_per_update"]["mat_apply"] * 1e-6
            row["phase_a_gb_per_s"] = row["update"]["sets"]["a"]["phase_a_bytes"] / a_s / 1e9
            row["phase_a_fraction_of_triad"] = row["phase_a_gb_per_s"] / row["update"]["triad_gb_per_s"]
        res["scenes"].append(row)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
