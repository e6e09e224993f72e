"""Time adaptive sampling (pt_render_adaptive) against a fixed number of passes rendered by a parent build, on the GPU.

  python tools/adaptive_time.py --parent-lib pathtrace-on-cuda_amd/build/libptamd_parent.so [--reps 2] [--out profiles/adaptive_time_mi355x.json]

Workload: BASELINE.json configs[2] (Cornell room + one stand-in mesh, lat_lon 187) at 1920x1080 with that config's 256 spp per pass,
batches of 8 passes, a cap of 64.  Every step is a process of its own (a library is chosen when ptamd is imported):
  first     render_adaptive with the cap at one batch: the tile errors after the first batch.  The targets are the 0.25 / 0.5 / 0.75
            quantiles of the positive ones.
  adaptive  per target: wall time of render_adaptive (host clock around the synchronous call, allocation and read-backs included,
            median of --reps after a warm-up render), the rounds, the mean passes per tile, the tiles active in each round, and — per
            round, for that round's number of tiles — the duration of pt_accumulate_tile_list and pt_tile_errors, and of pt_finish_tiles
            once, taken with device events around --kernel-reps launches after a warm-up (a work buffer filled by a real 8-pass render).
  parent    pt_render of all 64 passes in one call by the library given with --parent-lib (a build of the parent commit: a plain
            build of that tree, used through PTAMD_LIB) — the yardstick is the parent, never this tree's own render; without
            --parent-lib this tree's library renders it and the result says so.
  bar       sanity: render_adaptive with min_passes == max_passes == 16 (no tile ever stops) against pt_render_converge of the parent
            for the same 16 passes in batches of 8 (unreachable target).  The parent is measured before and after this tree; its
            spread is the largest gap between any two of its timings.  Frames are compared bit for bit.
Reported per target: time saved = 1 - t_adaptive / t_parent against tile-passes saved = 1 - mean passes / 64.
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
W, H, BATCH, CAP, BAR_PASSES = 1920, 1080, 8, 64, 16
QUANTILES = (0.25, 0.5, 0.75)


# ---------------------------------------------------------------------------------------------------------------------------------
# one measurement (child process)
# ---------------------------------------------------------------------------------------------------------------------------------
def measure(a):
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    import ctypes as C
    import numpy as np
    import torch
    import ptamd
    assert torch.cuda.is_available(), "adaptive_time.py measures on the GPU"
    # a build of the parent commit has no adaptive calls: bind what the library exports
    have = C.CDLL(ptamd.LIB_PATH)
    ptamd.API[:] = [e for e in ptamd.API if hasattr(have, e[0])]
    sc = ptamd.Scene.from_prims(ptamd.gen_scene(1, a.lat_lon))
    cam = ptamd.make_camera(W, H)
    prm = ptamd.default_params(passes=BATCH, spp_per_pass=a.spp)
    sc.render(cam, ptamd.default_params(passes=1, spp_per_pass=4))      # warm-up: code objects, clocks
    res = {"step": a.step, "lib": os.path.basename(ptamd.LIB_PATH)}

    def wall(fn, reps):
        secs, out = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            secs.append(time.perf_counter() - t0)
        return dict(seconds_median=float(np.median(secs)), seconds_min=float(np.min(secs)), seconds=secs), out

    if a.step == "first":
        got = sc.render_adaptive(cam, prm, 0.0, BATCH)
        err = got["tile_err"].ravel()
        pos = np.sort(err[err > 0])
        res.update(tiles=int(err.size), positive=int(pos.size), targets=[float(np.quantile(pos, q)) for q in QUANTILES], quantiles=list(QUANTILES))
    elif a.step == "adaptive":
        t, got = wall(lambda: sc.render_adaptive(cam, prm, a.target, CAP), a.reps)
        tp = got["tile_passes"].ravel()
        active = [int((tp > BATCH * r).sum()) for r in range(got["report"]["rounds"])]
        res.update(t, target=a.target, report=got["report"], mean_passes_per_tile=float(tp.mean()), active_tiles_per_round=active,
                   tiles_per_pass_count={int(k): int(v) for k, v in zip(*np.unique(tp, return_counts=True))})
        # the three new kernels at each round's size
        dev = torch.device("cuda:0")
        stream = torch.cuda.Stream(dev)
        s = stream.cuda_stream
        total = tp.size
        one = ptamd.default_params(passes=BATCH, spp_per_pass=1)
        everything = np.arange(total, dtype=np.int32)
        n = total * 192
        out, S, M2, mean, var = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(5))
        work = torch.empty(ptamd.tile_list_work_bytes(cam, one, total), dtype=torch.uint8, device=dev)
        d_err = torch.empty(total * 16, dtype=torch.uint8, device=dev)
        d_np = torch.empty(total, dtype=torch.int32, device=dev)
        d_list = torch.from_numpy(everything).to(dev)
        torch.cuda.synchronize()
        sc.render_tile_list_device(cam, one, everything, out.data_ptr(), work.data_ptr(), s)
        ptamd.accumulate_tile_list(work.data_ptr(), cam, one, d_list.data_ptr(), total, 0, S.data_ptr(), M2.data_ptr(), d_np.data_ptr(), s)
        stream.synchronize()

        def timed(fn):
            for _ in range(3):
                fn()
            stream.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.kernel_reps)]
            for e0, e1 in ev:
                e0.record(stream)
                fn()
                e1.record(stream)
            stream.synchronize()
            ms = [e0.elapsed_time(e1) for e0, e1 in ev]
            return dict(ms_median=float(np.median(ms)), ms_min=float(np.min(ms)))

        # the staging slab of a round of k tiles is k x 192 floats per pass: the first k tiles' worth of the buffer stands in for it
        rounds = []
        for r, k in enumerate(active):
            rounds.append({"round": r + 1, "tiles": k,
                           "fold_list": timed(lambda: ptamd.accumulate_tile_list(work.data_ptr(), cam, one, d_list.data_ptr(), k, BATCH * r, S.data_ptr(),
                                                                                 M2.data_ptr(), d_np.data_ptr(), s)),
                           "tile_errors": timed(lambda: ptamd.tile_errors(S.data_ptr(), M2.data_ptr(), cam, d_list.data_ptr(), k, BATCH * (r + 1),
                                                                          d_err.data_ptr(), s))})
        res["kernels_per_round"] = rounds
        res["finish_tiles"] = timed(lambda: ptamd.finish_tiles(S.data_ptr(), M2.data_ptr(), d_np.data_ptr(), cam, mean.data_ptr(), var.data_ptr(), s))
    elif a.step == "parent":
        full = ptamd.default_params(passes=CAP, spp_per_pass=a.spp)
        t, _ = wall(lambda: sc.render(cam, full), a.reps)
        res.update(t, passes=CAP)
    elif a.step in ("bar_parent", "bar_adaptive"):
        if a.step == "bar_parent":
            t, got = wall(lambda: sc.render_converge(cam, prm, 1e-12, BAR_PASSES), a.bar_reps)
            frame, done = got[0], got[2]
        else:
            t, got = wall(lambda: sc.render_adaptive(cam, prm, 1e-12, BAR_PASSES, min_passes=BAR_PASSES), a.bar_reps)
            frame, done = got["rgb"], int(got["tile_passes"].max())
            assert (got["tile_passes"] == BAR_PASSES).all()
        assert done == BAR_PASSES
        res.update(t, passes=BAR_PASSES, batch=BATCH)
        if os.path.exists(a.frame):
            res["bit_identical_to_first_frame"] = bool(np.array_equal(np.load(a.frame).view(np.uint32), frame.view(np.uint32)))
        else:
            np.save(a.frame, frame)
    print(json.dumps(res))


# ---------------------------------------------------------------------------------------------------------------------------------
# the sequence of measurements (no GPU work in this process)
# ---------------------------------------------------------------------------------------------------------------------------------
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libptamd.so built from the parent commit (the yardstick); default: this tree's library")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--bar-reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds a measurement may take")
    ap.add_argument("--out", default=None)
    # child
    ap.add_argument("--step", choices=("first", "adaptive", "parent", "bar_parent", "bar_adaptive"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--target", type=float, default=0.0, help=argparse.SUPPRESS)
    ap.add_argument("--frame", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return measure(a)

    with tempfile.TemporaryDirectory() as tmp:
        base = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--bar-reps", str(a.bar_reps), "--kernel-reps", str(a.kernel_reps),
                "--spp", str(a.spp), "--lat-lon", str(a.lat_lon), "--frame", os.path.join(tmp, "bar.npy")]

        def run(args, lib=None):
            env = dict(os.environ)
            env.pop("PTAMD_LIB", None)
            if lib:
                env["PTAMD_LIB"] = os.path.abspath(lib)
            sys.stderr.write(f"adaptive_time.py: {' '.join(args)}\n")
            r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + args, env=env, capture_output=True, text=True)
            if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(f"adaptive_time.py: step {args} ended with status {r.returncode}; stopping")
            return json.loads(r.stdout.strip().splitlines()[-1])

        res = {"workload": f"configs[2] (kind 1, lat_lon {a.lat_lon}), {W}x{H}, {a.spp} spp per pass, batches of {BATCH}, cap {CAP}",
               "reps": a.reps, "yardstick": "parent" if a.parent_lib else "this tree's own pt_render (NOT the parent)"}
        res["first"] = run(["--step", "first"])
        res["parent"] = run(["--step", "parent"], a.parent_lib)
        t_parent = res["parent"]["seconds_median"]
        res["targets"] = []
        for q, target in zip(QUANTILES, res["first"]["targets"]):
            row = run(["--step", "adaptive", "--target", repr(target)])
            row.update(quantile=q, t_adaptive=row["seconds_median"], t_parent=t_parent, time_saved=1.0 - row["seconds_median"] / t_parent,
                       tile_passes_saved=1.0 - row["mean_passes_per_tile"] / CAP)
            res["targets"].append(row)
        before = run(["--step", "bar_parent"], a.parent_lib)
        ours = run(["--step", "bar_adaptive"])
        after = run(["--step", "bar_parent"], a.parent_lib)
        par = before["seconds"] + after["seconds"]
        par_median = sorted(par)[len(par) // 2] if len(par) % 2 else 0.5 * (sorted(par)[len(par) // 2 - 1] + sorted(par)[len(par) // 2])
        res["bar"] = {"passes": BAR_PASSES, "batch": BATCH, "t_parent_converge": par_median, "parent_spread": max(par) - min(par),
                      "t_adaptive": ours["seconds_median"], "difference": ours["seconds_median"] - par_median,
                      "within_parent_spread": abs(ours["seconds_median"] - par_median) <= max(par) - min(par),
                      "bit_identical": ours.get("bit_identical_to_first_frame"), "parent_before": before, "adaptive": ours, "parent_after": after}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
