"""Time pt_render_tile_list on centred windows of the configs[2] frame against the full frame, on the GPU.

  python tools/region_time.py [--parent-lib build/libptamd_parent.so] [--reps 5] [--leads] [--out FILE.json]

Workload: BASELINE.json configs[2] (Cornell room + one stand-in mesh, lat_lon 187), 1920 x 1080, 8 passes x 256 spp in one call.
Windows: tile-aligned, centred on the frame, covering about 1/4, 1/16 and 1/64 of it (960 x 544, 480 x 272, 240 x 136 pixels).
Yardstick: the full frame rendered by pt_render_tiles (world 1) + pt_untile — the only way a library without the list calls can
produce those pixels.  With --parent-lib (a build of the parent commit: tools/build_variant.sh or a plain build of that tree, used
through PTAMD_LIB) that library renders the yardstick; this tree's own full frame is timed too, and must agree with it bit for bit.

Every measurement is a process of its own, started under its own `timeout`, one after the other; the first one that fails ends the
run (nothing more is started on the GPU).  A measurement: device buffers allocated once, one warm-up render of the same shape, then
--reps timed renders (host clock around the blocking render call, the scatter and a stream synchronisation); median and minimum.
Each window is compared bit for bit with the crop of the full frame.

Reported per window: t_window, t_full_parent, area share, efficiency = t_full_parent x share / t_window, and the pipeline's bounce
iterations.  --leads repeats the smallest window with other settings of pt_set_drain_threshold and pt_set_early_shade.
Prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, PASSES = 1920, 1080, 8


def centred_window(frac):
    """Tile-aligned window of about 1/frac of the frame (1/sqrt(frac) of each side, rounded up to whole tiles), centred."""
    side = int(round(frac ** 0.5))
    w, h = -(-(W // side) // 8) * 8, -(-(H // side) // 8) * 8
    x0, y0 = (W - w) // 2 // 8 * 8, (H - h) // 2 // 8 * 8
    return x0, y0, x0 + w, y0 + h


# ---------------------------------------------------------------------------------------------------------------------------------
# one measurement (child process)
# ---------------------------------------------------------------------------------------------------------------------------------
def measure(a):
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    import ctypes as C
    import numpy as np
    import torch
    import ptamd
    assert torch.cuda.is_available(), "region_time.py measures on the GPU"
    # a build of the parent commit has no list calls: bind what the library exports
    have = C.CDLL(ptamd.LIB_PATH)
    ptamd.API[:] = [e for e in ptamd.API if hasattr(have, e[0])]
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    sc = ptamd.Scene.from_prims(ptamd.gen_scene(1, a.lat_lon))
    if a.drain is not None:
        sc.set_drain_threshold(a.drain)
    if a.early is not None:
        sc.set_early_shade(a.early)
    cam = ptamd.make_camera(W, H)
    prm = ptamd.default_params(passes=PASSES, spp_per_pass=a.spp)
    if a.step == "full":
        win = (0, 0, W, H)
        tiles = torch.empty(ptamd.tiles_floats(cam, prm), dtype=torch.float32, device=dev)
        work = torch.empty(ptamd.work_bytes(cam, prm), dtype=torch.uint8, device=dev)
        out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)

        def render(p):
            sc.render_tiles(cam, p, tiles.data_ptr(), work.data_ptr(), s)
            ptamd.untile(tiles.data_ptr(), cam, 1, out.data_ptr(), s)
    else:
        win = centred_window(a.frac)
        lst = ptamd.tiles_of_window(cam, win)
        tiles = torch.empty(ptamd.tile_list_floats(lst.size), dtype=torch.float32, device=dev)
        work = torch.empty(ptamd.tile_list_work_bytes(cam, prm, lst.size), dtype=torch.uint8, device=dev)
        out = torch.empty((win[3] - win[1], win[2] - win[0], 3), dtype=torch.float32, device=dev)

        def render(p):
            sc.render_tile_list_device(cam, p, lst, tiles.data_ptr(), work.data_ptr(), s)
            ptamd.untile_list(tiles.data_ptr(), lst, cam, win, out.data_ptr(), s)
    render(prm)                                               # warm-up: code objects, clocks, the same shape as the timed calls
    stream.synchronize()
    secs = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        render(prm)
        stream.synchronize()
        secs.append(time.perf_counter() - t0)
    with torch.cuda.stream(stream):
        img = out.cpu().numpy()
    stream.synchronize()
    res = {"step": a.step, "lib": os.path.basename(ptamd.LIB_PATH), "window": list(win), "pixels": (win[2] - win[0]) * (win[3] - win[1]),
           "seconds_median": float(np.median(secs)), "seconds_min": float(np.min(secs)), "seconds": secs, "iterations": sc.last_iterations(),
           "work_bytes": int(work.numel()), "drain": a.drain, "early": a.early}
    if a.frame:
        if a.step == "full" and not os.path.exists(a.frame):
            np.save(a.frame, img)
        else:
            ref = np.load(a.frame)[win[1]:win[3], win[0]:win[2]]
            res["bit_identical_to_full_frame"] = bool(np.array_equal(ref.view(np.uint32), img.view(np.uint32)))
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
    ap.add_argument("--leads", action="store_true", help="the smallest window again with other drain / early-shade settings")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a measurement may take")
    ap.add_argument("--out", default=None)
    # child
    ap.add_argument("--step", choices=("full", "window"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--frac", type=int, default=4, help=argparse.SUPPRESS)
    ap.add_argument("--drain", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--early", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--frame", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return measure(a)

    with tempfile.TemporaryDirectory() as tmp:
        frame = os.path.join(tmp, "full.npy")
        base = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--spp", str(a.spp), "--lat-lon", str(a.lat_lon), "--frame", frame]

        def run(args, lib=None):
            env = dict(os.environ)
            env.pop("PTAMD_LIB", None)
            if lib:
                env["PTAMD_LIB"] = os.path.abspath(lib)
            r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + args, env=env, capture_output=True, text=True)
            if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(f"region_time.py: step {args} ended with status {r.returncode}; stopping")
            return json.loads(r.stdout.strip().splitlines()[-1])

        res = {"workload": f"configs[2] (kind 1, lat_lon {a.lat_lon}), {W}x{H}, {PASSES} passes x {a.spp} spp", "reps": a.reps}
        res["full"] = run(["--step", "full"])                                        # this tree; writes the frame the windows are compared with
        if a.parent_lib:
            res["full_parent"] = run(["--step", "full"], a.parent_lib)               # compared with that frame
        yard = res.get("full_parent", res["full"])
        res["yardstick"] = "full_parent" if a.parent_lib else "full"
        res["windows"] = {}
        for frac in (4, 16, 64):
            w = run(["--step", "window", "--frac", str(frac)])
            share = w["pixels"] / (W * H)
            w.update(area_share=share, t_window=w["seconds_median"], t_full_parent=yard["seconds_median"],
                     efficiency=yard["seconds_median"] * share / w["seconds_median"])
            res["windows"][f"1/{frac}"] = w
        if a.leads:
            res["leads_1/64"] = []
            for drain, early in ((0, None), (20000, None), (320000, None), (None, 0), (None, 1000000)):
                extra = (["--drain", str(drain)] if drain is not None else []) + (["--early", str(early)] if early is not None else [])
                res["leads_1/64"].append(run(["--step", "window", "--frac", "64"] + extra))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
