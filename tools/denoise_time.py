"""Time pt_render_aov and pt_denoise on the GPU (torch events on the launch stream), at 1080p and 4K.

  python tools/denoise_time.py [--passes 8] [--reps 20] [--out FILE.json]

Scene: BASELINE.json configs[2] (Cornell room + one stand-in mesh, lat_lon 187).  The AOV call takes the first-hit buffers of
`--passes` passes (one primary ray per pixel and pass); the denoiser runs the default parameters (5 iterations).  Prints one JSON
line: per frame size the median and minimum ms of each call over --reps timed repetitions after 0.3 s of warm-up.
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
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "denoise_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    sc = ptamd.Scene.from_prims(ptamd.gen_scene(1, a.lat_lon))
    stream = torch.cuda.Stream(dev)
    res = {"scene": f"configs[2] (kind 1, lat_lon {a.lat_lon})", "aov_passes": a.passes, "denoise": "defaults (5 iterations)", "sizes": {}}
    for W, H in ((1920, 1080), (3840, 2160)):
        cam = ptamd.make_camera(W, H)
        prm = ptamd.default_params(passes=a.passes)
        aov = torch.empty((H, W, 8), dtype=torch.float32, device=dev)
        rgb = torch.rand((H, W, 3), dtype=torch.float32, device=dev)
        out = torch.empty_like(rgb)
        work = torch.empty(ptamd.denoise_work_bytes(W, H), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        s = stream.cuda_stream
        aov_ms = timed(lambda: sc.render_aov(cam, prm, aov.data_ptr(), 0, s), stream, a.reps)
        den_ms = timed(lambda: ptamd.denoise_device(rgb.data_ptr(), aov.data_ptr(), W, H, a.passes, out.data_ptr(), work.data_ptr(), s),
                       stream, a.reps)
        it1 = timed(lambda: ptamd.denoise_device(rgb.data_ptr(), aov.data_ptr(), W, H, a.passes, out.data_ptr(), work.data_ptr(), s,
                                                 iterations=1), stream, a.reps)
        assert torch.isfinite(out).all()
        res["sizes"][f"{W}x{H}"] = {"aov_ms_median": aov_ms[0], "aov_ms_min": aov_ms[1], "primary_rays_per_s": W * H * a.passes / (aov_ms[0] * 1e-3),
                                   "denoise_ms_median": den_ms[0], "denoise_ms_min": den_ms[1],
                                   "denoise_1iter_ms_median": it1[0]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
