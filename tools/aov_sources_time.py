"""Time the feature buffers and the denoiser of windows and view batches on the GPU against a build of the parent commit.

  python tools/aov_sources_time.py --parent-lib pathtrace-on-cuda_amd/build/libptamd_parent.so [--reps 20] [--rounds 2] [--out profiles/aov_sources_time_mi355x.json]

Scene: BASELINE.json configs[2] (Cornell room + one stand-in mesh, lat_lon 187).  Torch events on the launch stream, medians of --reps
timed repetitions after 0.3 s of warm-up per shape.  Three measurements:

  a  full-frame feature buffers, 8 passes, at 1920 x 1080 and 3840 x 2160: the parent's pt_render_aov (aov_kernel) against this tree's
     aov_source instantiated for the whole frame (pt_render_aov_window with the frame as its window), and this tree's own pt_render_aov.
  b  16 views of 240 x 136 after one render_views_device: per view pt_untile + pt_render_aov + pt_denoise (144 launches) on the parent
     against pt_untile_views + pt_render_aov_views + pt_denoise_batch (9 launches and one table copy); this tree's per-view path as well.
  c  a 256 x 256 window of the 1080p frame, 4 passes x 1 spp: Scene.render_window_denoised at margin M = 62 and at margin 0 against
     full-frame render + feature buffers + denoise (host clock around the synchronous calls; this tree only).

The two libraries ALTERNATE as processes of their own within one run (parent, this tree, parent, this tree, ... --rounds times), each
under its own `timeout`; the spread of a repeated identical leg is reported beside every difference.  The first leg that fails ends the
run: nothing more is started on the GPU.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS, VW, VH = 16, 240, 136
WIN = (800, 400, 1056, 656)


def _imports():
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    import ctypes as C
    import ptamd
    have = C.CDLL(ptamd.LIB_PATH)      # a build of the parent commit lacks the new calls: bind what the library exports
    ptamd.API[:] = [e for e in ptamd.API if hasattr(have, e[0])]
    return ptamd, hasattr(have, "pt_render_aov_window")


def timed(fn, stream, reps, torch, warm_s=0.3):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    t0 = time.time()
    while time.time() - t0 < warm_s:
        fn()
        stream.synchronize()
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    stream.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def leg(a):
    """One process: every measurement this library can make."""
    import numpy as np
    import torch
    ptamd, new = _imports()
    assert torch.cuda.is_available(), "aov_sources_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    sc = ptamd.Scene.from_prims(ptamd.gen_scene(1, a.lat_lon))
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    out = {"new_calls": new, "a": {}, "b": {}, "c": {}}
    # ---- a
    for W, H in ((1920, 1080), (3840, 2160)):
        cam, prm = ptamd.make_camera(W, H), ptamd.default_params(passes=8)
        aov = torch.empty((H, W, 8), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        row = {"render_aov": timed(lambda: sc.render_aov(cam, prm, aov.data_ptr(), 0, s), stream, a.reps, torch)}
        if new:
            keep = aov.clone()
            row["aov_source_full_frame"] = timed(lambda: sc.render_aov_window(cam, prm, (0, 0, W, H), aov.data_ptr(), 0, s), stream, a.reps, torch)
            assert torch.equal(keep.view(torch.int32), aov.view(torch.int32))      # the same bits at the size that is timed
        out["a"][f"{W}x{H}"] = row
        del aov
    # ---- b
    cams = [ptamd.make_camera(VW, VH, pos=(8.0 * np.sin(0.39 * v), 20.0, 60.0 - 4.0 * abs(np.sin(0.39 * v))), rot_deg=(0.0, 90.0 + 1.5 * v - 12.0, 0.0))
            for v in range(VIEWS)]
    prm = ptamd.default_params(passes=4, spp_per_pass=1)
    tiles = torch.empty(ptamd.views_floats(cams[0], VIEWS), dtype=torch.float32, device=dev)
    work = torch.empty(max(ptamd.views_work_bytes(cams[0], prm, VIEWS), 48 * VW * VH * VIEWS), dtype=torch.uint8, device=dev)
    frames = torch.empty((VIEWS, VH, VW, 3), dtype=torch.float32, device=dev)
    aov = torch.empty((VIEWS, VH, VW, 8), dtype=torch.float32, device=dev)
    den = torch.empty_like(frames)
    sc.render_views_device(cams, prm, tiles.data_ptr(), work.data_ptr(), s)
    stream.synchronize()
    T = tiles.numel() // VIEWS
    one = ptamd.denoise_work_bytes(VW, VH)

    def per_view():
        for v in range(VIEWS):
            ptamd.untile(tiles[v * T:].data_ptr(), cams[v], 1, frames[v].data_ptr(), s)
            sc.render_aov(cams[v], prm, aov[v].data_ptr(), 0, s)
            ptamd.denoise_device(frames[v].data_ptr(), aov[v].data_ptr(), VW, VH, prm.passes, den[v].data_ptr(), work.data_ptr(), s)
    assert one <= work.numel()
    out["b"]["per_view"] = dict(timed(per_view, stream, a.reps, torch), launches=VIEWS * (1 + 1 + 7))
    if new:
        keep = den.clone()

        def batched():
            ptamd.untile_views(tiles.data_ptr(), cams[0], VIEWS, frames.data_ptr(), s)
            sc.render_aov_views(cams, prm, aov.data_ptr(), 0, s)
            ptamd.denoise_batch_device(frames.data_ptr(), aov.data_ptr(), VW, VH, VIEWS, prm.passes, den.data_ptr(), work.data_ptr(), s)
        out["b"]["batched"] = dict(timed(batched, stream, a.reps, torch), launches=1 + 1 + 7, copies=1)
        assert torch.equal(keep.view(torch.int32), den.view(torch.int32))
        # ---- c
        W, H = 1920, 1080
        cam = ptamd.make_camera(W, H)
        M = ptamd.denoise_margin()

        def wall(fn, reps=7):
            fn()
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            return {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}
        out["c"] = {"window": WIN, "params": "4 passes x 1 spp, default denoiser (5 iterations)", "clock": "host, around synchronous calls (allocation and transfers included)",
                    "margin_M": dict(wall(lambda: sc.render_window_denoised(cam, prm, WIN)), margin=M, expanded=ptamd.expand_window(cam, WIN, M)),
                    "margin_0": dict(wall(lambda: sc.render_window_denoised(cam, prm, WIN, margin=0)), margin=0),
                    "full_frame": wall(lambda: ptamd.denoise(sc.render(cam, prm), sc.aov(cam, prm)[0], prm.passes))}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libptamd.so built from the parent commit (the yardstick)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="how often each library's leg is repeated (>= 2: the spread of an identical leg)")
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    if not a.parent_lib:
        sys.exit("aov_sources_time.py: --parent-lib is the yardstick (a build of the parent commit); the code under test is never its own")
    runs = {"parent": [], "new": []}
    for r in range(a.rounds):
        for side in ("parent", "new"):
            env = dict(os.environ)
            env.pop("PTAMD_LIB", None)
            if side == "parent":
                env["PTAMD_LIB"] = os.path.abspath(a.parent_lib)
            cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--leg", "--reps", str(a.reps), "--lat-lon", str(a.lat_lon)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True)
            if p.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                sys.exit(f"aov_sources_time.py: the {side} leg of round {r} ended with status {p.returncode}; stopping")
            runs[side].append(json.loads(p.stdout.strip().splitlines()[-1]))
            sys.stderr.write(f"done: {side} leg, round {r}\n")
            sys.stderr.flush()
    assert not runs["parent"][0]["new_calls"] and runs["new"][0]["new_calls"], "--parent-lib must be the parent's build, the tree's library the new one"

    def med(side, *path):
        vals = []
        for run in runs[side]:
            x = run
            for k in path:
                x = x[k]
            vals.append(x["ms_median"])
        return {"ms": statistics.median(vals), "legs": vals, "spread_ms": max(vals) - min(vals)}

    res = {"scene": f"configs[2] (kind 1, lat_lon {a.lat_lon})", "reps": a.reps, "rounds": a.rounds, "method": "torch events on the launch stream, median of reps after warm-up; "
           "parent and new legs alternate as processes; spread_ms = max - min over the repeated identical legs", "a": {}, "b": {}, "c": runs["new"][-1]["c"]}
    for size in ("1920x1080", "3840x2160"):
        p, n, own = med("parent", "a", size, "render_aov"), med("new", "a", size, "aov_source_full_frame"), med("new", "a", size, "render_aov")
        spread = max(p["spread_ms"], n["spread_ms"])
        res["a"][size] = {"parent_render_aov": p, "aov_source_full_frame": n, "new_render_aov": own, "difference_ms": n["ms"] - p["ms"], "spread_ms": spread,
                          "not_slower": n["ms"] - p["ms"] <= spread}
    res["a"]["not_slower_at_both_sizes"] = all(res["a"][s]["not_slower"] for s in ("1920x1080", "3840x2160"))
    p, n, own = med("parent", "b", "per_view"), med("new", "b", "batched"), med("new", "b", "per_view")
    res["b"] = {"views": VIEWS, "size": f"{VW}x{VH}", "parent_per_view": dict(p, launches=runs["parent"][0]["b"]["per_view"]["launches"]),
                "new_per_view": own, "batched": dict(n, launches=runs["new"][0]["b"]["batched"]["launches"], copies=1),
                "difference_ms": n["ms"] - p["ms"], "spread_ms": max(p["spread_ms"], n["spread_ms"]), "speedup": p["ms"] / n["ms"]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
