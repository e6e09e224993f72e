"""Time a batch of camera views (pt_render_views) against the same views rendered one after the other, on the GPU.

  python tools/views_time.py --parent-lib build/libptamd_parent.so [--reps 5] [--out FILE.json]

Workload: BASELINE.json configs[2]'s scene (Cornell room + one stand-in mesh, lat_lon 187), 8 passes x 256 spp in one call.
Views: V in {1, 4, 16, 64} of 240 x 136 pixels and V in {1, 4} of 960 x 544, cameras on an arc round the mesh (60 units from the
room's axis at the reference camera's height, -30 ... +30 degrees about the reference camera, each looking at the axis).
  t_batch(V)  one pt_render_views call of this tree + the V pt_untile calls that assemble the frames.
  t_seq(V)    V pt_render_tiles calls + pt_untile, one per camera, of the library given with --parent-lib (a build of the parent
              commit: tools/build_variant.sh or a plain build of that tree, used through PTAMD_LIB) — the only way a library
              without the batch call can produce those frames.  The yardstick is the parent, never this tree's own single path;
              without --parent-lib this tree's library renders it and the result says so.

Every measurement is a process of its own, started under its own `timeout`, one after the other; the first one that fails ends the
run (nothing more is started on the GPU).  A measurement: device buffers allocated once and reused by every render, one warm-up
of the same shape, then --reps timed repetitions (host clock around the blocking render calls, the scatters and a stream
synchronisation); median and minimum.  The batch's frames are compared bit for bit with the sequence's.

Reported per (size, V): t_batch, t_seq, their ratio, the run-to-run spread (the largest gap between minimum and median of the two,
relative), the bounce iterations and the work-buffer size.  Prints one JSON line.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = 8
CASES = ((240, 136, 1), (240, 136, 4), (240, 136, 16), (240, 136, 64), (960, 544, 1), (960, 544, 4))


def orbit(ptamd, W, H, V):
    """V cameras on the arc, in order."""
    cams = []
    for i in range(V):
        a = 0.0 if V == 1 else -30.0 + 60.0 * i / (V - 1)
        pos = (60.0 * math.sin(math.radians(a)), 20.0, 60.0 * math.cos(math.radians(a)))
        cams.append(ptamd.make_camera(W, H, pos=pos, rot_deg=(0.0, 90.0, a)))
    return cams


# ---------------------------------------------------------------------------------------------------------------------------------
# one measurement (child process)
# ---------------------------------------------------------------------------------------------------------------------------------
def measure(a):
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    import ctypes as C
    import numpy as np
    import torch
    import ptamd
    assert torch.cuda.is_available(), "views_time.py measures on the GPU"
    # a build of the parent commit has no batch call: bind what the library exports
    have = C.CDLL(ptamd.LIB_PATH)
    ptamd.API[:] = [e for e in ptamd.API if hasattr(have, e[0])]
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    sc = ptamd.Scene.from_prims(ptamd.gen_scene(1, a.lat_lon))
    W, H, V = a.width, a.height, a.views
    cams = orbit(ptamd, W, H, V)
    prm = ptamd.default_params(passes=PASSES, spp_per_pass=a.spp)
    out = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev)
    iters = []
    if a.step == "batch":
        per = ptamd.views_floats(cams[0], 1)
        tiles = torch.empty(ptamd.views_floats(cams[0], V), dtype=torch.float32, device=dev)
        work = torch.empty(ptamd.views_work_bytes(cams[0], prm, V), dtype=torch.uint8, device=dev)

        def render():
            sc.render_views_device(cams, prm, tiles.data_ptr(), work.data_ptr(), s)
            iters[:] = [sc.last_iterations()]
            for v in range(V):
                ptamd.untile(tiles.data_ptr() + 4 * per * v, cams[v], 1, out[v].data_ptr(), s)
    else:
        tiles = torch.empty(ptamd.tiles_floats(cams[0], prm), dtype=torch.float32, device=dev)
        work = torch.empty(ptamd.work_bytes(cams[0], prm), dtype=torch.uint8, device=dev)

        def render():
            iters.clear()
            for v in range(V):
                sc.render_tiles(cams[v], prm, tiles.data_ptr(), work.data_ptr(), s)
                iters.append(sc.last_iterations())
                ptamd.untile(tiles.data_ptr(), cams[v], 1, out[v].data_ptr(), s)
    render()                                                  # warm-up: code objects, clocks, the same shape as the timed calls
    stream.synchronize()
    secs = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        render()
        stream.synchronize()
        secs.append(time.perf_counter() - t0)
    with torch.cuda.stream(stream):
        img = out.cpu().numpy()
    stream.synchronize()
    res = {"step": a.step, "lib": os.path.basename(ptamd.LIB_PATH), "size": [W, H], "views": V, "streams": V * ((W + 7) // 8) * ((H + 7) // 8) * 64 * PASSES,
           "seconds_median": float(np.median(secs)), "seconds_min": float(np.min(secs)), "seconds": secs,
           "iterations": int(iters[0]) if a.step == "batch" else [int(i) for i in iters], "work_bytes": int(work.numel())}
    if a.frames:
        if a.step == "seq":
            np.save(a.frames, img)
        else:
            res["bit_identical_to_sequence"] = bool(np.array_equal(np.load(a.frames).view(np.uint32), img.view(np.uint32)))
    print(json.dumps(res))


# ---------------------------------------------------------------------------------------------------------------------------------
# the sequence of measurements (no GPU work in this process)
# ---------------------------------------------------------------------------------------------------------------------------------
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libptamd.so built from the parent commit (the yardstick); default: this tree's library")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a measurement may take")
    ap.add_argument("--out", default=None)
    # child
    ap.add_argument("--step", choices=("batch", "seq"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--width", type=int, default=240, help=argparse.SUPPRESS)
    ap.add_argument("--height", type=int, default=136, help=argparse.SUPPRESS)
    ap.add_argument("--views", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--frames", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return measure(a)

    with tempfile.TemporaryDirectory() as tmp:
        base = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--spp", str(a.spp), "--lat-lon", str(a.lat_lon)]

        def run(args, lib=None):
            env = dict(os.environ)
            env.pop("PTAMD_LIB", None)
            if lib:
                env["PTAMD_LIB"] = os.path.abspath(lib)
            r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + args, env=env, capture_output=True, text=True)
            if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(f"views_time.py: step {args} ended with status {r.returncode}; stopping")
            out = json.loads(r.stdout.strip().splitlines()[-1])
            sys.stderr.write(f"{out['step']} {out['size'][0]}x{out['size'][1]} x {out['views']}: median {out['seconds_median']:.4f} s\n")      # progress
            sys.stderr.flush()
            return out

        res = {"workload": f"configs[2]'s scene (kind 1, lat_lon {a.lat_lon}), {PASSES} passes x {a.spp} spp, cameras on an arc of 60 degrees",
               "reps": a.reps, "yardstick": "parent" if a.parent_lib else "this tree's own single-camera path (NOT the parent)", "cases": []}
        for W, H, V in CASES:
            frames = os.path.join(tmp, f"seq_{W}x{H}_{V}.npy")
            shape = ["--width", str(W), "--height", str(H), "--views", str(V), "--frames", frames]
            seq = run(["--step", "seq"] + shape, a.parent_lib)
            bat = run(["--step", "batch"] + shape)
            spread = max((r["seconds_median"] - r["seconds_min"]) / r["seconds_median"] for r in (seq, bat))
            res["cases"].append({"size": [W, H], "views": V, "t_batch": bat["seconds_median"], "t_seq": seq["seconds_median"],
                                 "ratio": seq["seconds_median"] / bat["seconds_median"], "spread": spread,
                                 "iterations_batch": bat["iterations"], "iterations_seq_max": max(seq["iterations"]),
                                 "work_bytes_batch": bat["work_bytes"], "work_bytes_seq": seq["work_bytes"],
                                 "bit_identical": bat["bit_identical_to_sequence"], "batch": bat, "seq": seq})
            os.remove(frames)
        res["spread_max"] = max(c["spread"] for c in res["cases"])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
