"""Time the ray render (pt_render_rays) on a camera's own rays against that camera's frame rendered by a parent build, on the GPU.

  python tools/rays_time.py --parent-lib build/libptamd_parent.so [--reps 5] [--out FILE.json]

Workload: BASELINE.json configs[2]'s scene (Cornell room + one stand-in mesh, lat_lon 187) at 1920 x 1080, one pass x 256 spp.
  parent  pt_render_tiles + pt_untile of the library given with --parent-lib (a build of the parent commit: tools/build_variant.sh or
          a plain build of that tree, used through PTAMD_LIB) — the yardstick is the parent, never this tree's own camera path;
          without --parent-lib this tree's library renders it and the result says so.
  rays    pt_render_rays of this tree on ptamd.camera_rays(cam, 0): the same 2,073,600 streams, each of which reads 32 bytes of ray
          at init and 16 bytes of origin where a sample restarts.  Its output must be the parent's frame bit for bit.
  pano    pt_render_rays on ptamd.equirect_rays(camera position, 1920, 1080): 2,073,600 rays of a 360 x 180 degree panorama.  Recorded
          (time, bounce iterations, work bytes); it has no yardstick.

Every measurement is a process of its own, started under its own `timeout`, one after the other; the first one that fails ends the
run (nothing more is started on the GPU).  A measurement: device buffers allocated once and reused by every render, one warm-up of
the same shape, then --reps timed repetitions (host clock around the blocking render call, the scatter where there is one, and a
stream synchronisation); median and minimum.

Condition: the ray render's median is not above the parent's by more than twice the session's own spread, the largest gap between the
minimum and the median of the timed steps.  Prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 1920, 1080


def measure(a):
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    import ctypes as C
    import numpy as np
    import torch
    import ptamd
    assert torch.cuda.is_available(), "rays_time.py measures on the GPU"
    # a build of the parent commit has no ray render: bind what the library exports
    have = C.CDLL(ptamd.LIB_PATH)
    ptamd.API[:] = [e for e in ptamd.API if hasattr(have, e[0])]
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(dev)
    s = stream.cuda_stream
    sc = ptamd.Scene.from_prims(ptamd.gen_scene(1, a.lat_lon))
    cam = ptamd.make_camera(W, H)
    prm = ptamd.default_params(passes=1, spp_per_pass=a.spp, first_pass=0, rank=0, world=1)
    n = W * H
    if a.step == "parent":
        out = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
        tiles = torch.empty(ptamd.tiles_floats(cam, prm), dtype=torch.float32, device=dev)
        work = torch.empty(ptamd.work_bytes(cam, prm), dtype=torch.uint8, device=dev)

        def render():
            sc.render_tiles(cam, prm, tiles.data_ptr(), work.data_ptr(), s)
            ptamd.untile(tiles.data_ptr(), cam, 1, out.data_ptr(), s)
    else:
        if a.step == "rays":
            rays, seeds, stride = ptamd.camera_rays(cam, 0)
        else:
            rays, seeds, stride = ptamd.equirect_rays(cam.pos[:], W, H), np.arange(n, dtype=np.int32), n
        d_rays, d_seeds = torch.from_numpy(rays).to(dev), torch.from_numpy(seeds).to(dev)
        rgb = torch.empty(ptamd.rays_floats(n), dtype=torch.float32, device=dev)
        work = torch.empty(ptamd.rays_work_bytes(prm, n), dtype=torch.uint8, device=dev)
        out = rgb[:3 * n].view(H, W, 3)
        torch.cuda.synchronize(dev)

        def render():
            sc.render_rays_device(d_rays.data_ptr(), n, prm, rgb.data_ptr(), work.data_ptr(), d_seeds.data_ptr(), stride, s)
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
    res = {"step": a.step, "lib": os.path.basename(os.path.dirname(ptamd.LIB_PATH)) + "/" + os.path.basename(ptamd.LIB_PATH), "streams": 64 * ((n + 63) // 64),
           "seconds_median": float(np.median(secs)), "seconds_min": float(np.min(secs)), "seconds": secs, "render_ms_last": float(sc.last_render_ms()),
           "iterations": int(sc.last_iterations()), "work_bytes": int(work.numel()), "finite": bool(np.isfinite(img).all()), "mean": float(img.mean())}
    if a.step == "parent":
        np.save(a.frames, img)
    elif a.step == "rays":
        res["bit_identical_to_parent"] = bool(np.array_equal(np.load(a.frames).view(np.uint32), img.view(np.uint32)))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="libptamd.so built from the parent commit (the yardstick); default: this tree's library")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--step-timeout", type=int, default=180, help="seconds a measurement may take")
    ap.add_argument("--out", default=None)
    # child
    ap.add_argument("--step", choices=("parent", "rays", "pano"), default=None, help=argparse.SUPPRESS)
    ap.add_argument("--frames", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return measure(a)

    with tempfile.TemporaryDirectory() as tmp:
        frames = os.path.join(tmp, "parent.npy")
        base = [sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--spp", str(a.spp), "--lat-lon", str(a.lat_lon), "--frames", frames]

        def run(step, lib=None):
            env = dict(os.environ)
            env.pop("PTAMD_LIB", None)
            if lib:
                env["PTAMD_LIB"] = os.path.abspath(lib)
            r = subprocess.run(["timeout", "-k", "10", str(a.step_timeout)] + base + ["--step", step], env=env, capture_output=True, text=True)
            if r.returncode != 0:      # a fault, an abort or a time limit: stop here, start nothing more
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(f"rays_time.py: step {step} ended with status {r.returncode}; stopping")
            out = json.loads(r.stdout.strip().splitlines()[-1])
            sys.stderr.write(f"{step}: median {out['seconds_median']:.4f} s, minimum {out['seconds_min']:.4f} s, {out['iterations']} iterations\n")      # progress
            sys.stderr.flush()
            return out

        par, ray, pano = run("parent", a.parent_lib), run("rays"), run("pano")
    spread = max(r["seconds_median"] - r["seconds_min"] for r in (par, ray))      # seconds: the largest min-to-median gap of the two timed steps that are compared
    res = {"workload": f"configs[2]'s scene (kind 1, lat_lon {a.lat_lon}), {W}x{H}, 1 pass x {a.spp} spp", "reps": a.reps,
           "yardstick": "parent" if a.parent_lib else "this tree's own camera path (NOT the parent)",
           "t_parent": par["seconds_median"], "t_rays": ray["seconds_median"], "ratio": ray["seconds_median"] / par["seconds_median"],
           "spread_seconds": spread, "within_twice_the_spread": bool(ray["seconds_median"] <= par["seconds_median"] + 2.0 * spread),
           "bit_identical": ray["bit_identical_to_parent"], "t_pano": pano["seconds_median"], "parent": par, "rays": ray, "pano": pano}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
