"""Time the moments calls (pt_accumulate_passes, pt_variance, pt_error_estimate) and pt_render_converge on the GPU.

  python tools/stats_time.py [--passes 8] [--reps 20] [--spp 256] [--no-converge] [--out FILE.json]

Scene: BASELINE.json configs[2] (Cornell room + one stand-in mesh, lat_lon 187).
Part 1, at 1080p and 4K: one render of `--passes` passes x 1 spp leaves its per-pass means in the work buffer; the fold of those
passes, the variance and the estimate (which ends with a 40 KB read-back and a stream synchronisation) are then timed with torch
events on the launch stream: median and minimum ms over --reps repetitions after 0.3 s of warm-up.  The sum_passes launch the fold
sits beside has no entry point of its own; its duration comes from a kernel trace of this script (rocprofv3 --kernel-trace --stats).
Part 2, at 1080p with --spp samples per pass: wall time of pt_render of `--passes` passes in one call against pt_render_converge
reaching the same number of passes (unreachable target) in batches of 1, 4 and 8 passes; frames compared bit for bit.
Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ptamd  # noqa: E402


def timed(fn, stream, reps, warm_s=0.3):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    t0 = time.time()
    while time.time() - t0 < warm_s:                          # warm-up: code object load, and clocks up to speed
        fn()
        stream.synchronize()
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    stream.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--no-converge", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "stats_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    sc = ptamd.Scene.from_prims(ptamd.gen_scene(1, a.lat_lon))
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    res = {"scene": f"configs[2] (kind 1, lat_lon {a.lat_lon})", "passes": a.passes, "sizes": {}}
    for W, H in ((1920, 1080), (3840, 2160)):
        cam = ptamd.make_camera(W, H)
        prm = ptamd.default_params(passes=a.passes, spp_per_pass=1)
        n = ptamd.tiles_floats(cam, prm)
        tiles, S, M2, var = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(4))
        work = torch.empty(ptamd.work_bytes(cam, prm), dtype=torch.uint8, device=dev)
        scratch = torch.empty(ptamd.error_scratch_bytes(n), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        sc.render_tiles(cam, prm, tiles.data_ptr(), work.data_ptr(), s)
        stream.synchronize()
        est = {}

        def fold():
            ptamd.accumulate_passes(work.data_ptr(), cam, prm, 0, S.data_ptr(), M2.data_ptr(), s)

        def fold_more():      # the same means as passes 9 .. 16: state read as well as written
            ptamd.accumulate_passes(work.data_ptr(), cam, prm, a.passes, S.data_ptr(), M2.data_ptr(), s)

        def variance():
            ptamd.variance(M2.data_ptr(), n, a.passes, var.data_ptr(), s)

        def estimate():
            est.update(ptamd.error_estimate(S.data_ptr(), M2.data_ptr(), cam, prm, a.passes, scratch.data_ptr(), s))

        def all_three():
            fold(), variance(), estimate()

        t = {k: timed(f, stream, a.reps) for k, f in (("fold", fold), ("fold_with_state", fold_more), ("variance", variance))}
        fold()
        t["estimate"] = timed(estimate, stream, a.reps)
        t["fold_variance_estimate"] = timed(all_three, stream, a.reps)
        assert torch.equal(S.view(torch.int32), tiles.view(torch.int32))      # S is the frame
        gb = n * 4 * (a.passes + 2) / 1e9
        res["sizes"][f"{W}x{H}"] = {**{f"{k}_ms_median": v[0] for k, v in t.items()}, **{f"{k}_ms_min": v[1] for k, v in t.items()},
                                   "fold_GBps": gb / (t["fold"][0] * 1e-3), "estimate": dict(est)}
        del tiles, S, M2, var, work, scratch
    if not a.no_converge:
        W, H = 1920, 1080
        cam = ptamd.make_camera(W, H)
        one = ptamd.default_params(passes=a.passes, spp_per_pass=a.spp)
        sc.render(cam, ptamd.default_params(passes=1, spp_per_pass=4))      # warm-up
        t0 = time.time()
        frame = sc.render(cam, one)
        t_render = time.time() - t0
        conv = {"pt_render_s": t_render, "spp_per_pass": a.spp}
        for batch in (1, 4, 8):
            if batch > a.passes:
                continue
            t0 = time.time()
            rgb, _, done, est = sc.render_converge(cam, ptamd.default_params(passes=batch, spp_per_pass=a.spp), 1e-12, a.passes)
            dt = time.time() - t0
            assert done == a.passes and np.array_equal(rgb.view(np.uint32), frame.view(np.uint32))
            conv[f"batch_{batch}"] = {"seconds": dt, "ratio_to_pt_render": dt / t_render, "rel_rms": est["rel_rms"], "mean_rel_se": est["mean_rel_se"]}
        res["converge_1080p"] = conv
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
