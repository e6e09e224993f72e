"""Time the variable-length query lists (pt_list_offsets, pt_trace_rays_list, pt_within_radius_list) on the GPU.

  python tools/lists_time.py [--reps 7] [--out profiles/lists_time_mi355x.json]

Scene: the Cornell room + one stand-in mesh (kind 1, lat_lon 187: 69,576 triangles).  Rays: tools/query_time.py's three fixed-seed sets
of a 1920 x 1080 frame's size (2,073,600 rays each; tests/query_ref.py): A camera rays, B bounce rays from A's hits, C segments, front
faces.  Points: 2,073,600 on random triangles (every third moved off by 1e-3) at the radius whose median count is 8 (found by bisection on
the counts), and 4,096 points in the room at radius inf (every list is the whole scene: the sort's global steps).

Per set, in one process, alternating call by call after WARM calls of each, the time between two device events around:
  count        pt_count_hits / pt_count_within alone
  list         count + pt_list_offsets + the fill into records allocated beforehand for the known total: the three device calls, no read-back
  list_detail  the same with the detail records
  count_k32    count + pt_trace_rays_k / pt_nearest_k with k = 32 (what a caller of the K calls would pay for lists of up to 32)
  wrapper      Scene.trace_rays_all / within_radius on a device tensor: the same with the 8-byte read-back and torch's allocations
Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM = 2
W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--rays", type=int, default=W * H, help="rays (and points) per set")
    ap.add_argument("--long-points", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "pathtrace-on-cuda_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import dynamic_ref as R
    import nearest_ref as N
    import ptamd
    import query_ref as Q
    assert torch.cuda.is_available(), "lists_time.py needs a GPU"
    l = ptamd.lib()
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, a.lat_lon))
    sc = ptamd.Scene(nodes, tris)
    dev = torch.device("cuda:0")

    def bench(calls):
        """{name: call}: every call WARM times, then reps rounds of one call each, in turn."""
        for f in calls.values():
            for _ in range(WARM):
                f()
        ms = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in ms.items()}

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    def lists(kind, q, extra):
        """The calls of one set; q a device tensor.  extra: bytes of detail per record."""
        n = q.shape[0]
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        scr = torch.empty(l.pt_list_offsets_scratch_bytes(n), dtype=torch.uint8, device=dev)
        count = (lambda: l.pt_count_hits(sc._h, ptr(q), n, 0, ptr(cnt), None)) if kind == "rays" else (lambda: l.pt_count_within(sc._h, ptr(q), n, ptr(cnt), None))
        assert count() == 0 and l.pt_list_offsets(ptr(cnt), n, ptr(off), ptr(scr), None) == 0
        total = int(off[-1].item())
        c = cnt.cpu().numpy()
        rec = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
        det = torch.empty((max(total, 1), extra // 4), dtype=torch.float32, device=dev) if total * extra < (40 << 30) else None
        k32 = torch.empty((n, 32, 2), dtype=torch.int32, device=dev) if n * 256 < (40 << 30) else None

        def fill(d):
            if kind == "rays":
                return l.pt_trace_rays_list(sc._h, ptr(q), n, 0, ptr(off), total, ptr(rec), ptr(d) if d is not None else None, None)
            return l.pt_within_radius_list(sc._h, ptr(q), n, ptr(off), total, ptr(rec), ptr(d) if d is not None else None, None)

        def seq(d=None):
            assert count() == 0 and l.pt_list_offsets(ptr(cnt), n, ptr(off), ptr(scr), None) == 0 and fill(d) == 0

        def count_k32():
            assert count() == 0
            if kind == "rays":
                assert l.pt_trace_rays_k(sc._h, ptr(q), n, 32, 0, ptr(k32), None, None) == 0
            else:
                assert l.pt_nearest_k(sc._h, ptr(q), n, 32, ptr(k32), None, None) == 0
        calls = {"count": lambda: count(), "list": seq}
        if det is not None:
            calls["list_detail"] = lambda: seq(det)
        if k32 is not None:
            calls["count_k32"] = count_k32
        calls["wrapper"] = (lambda: sc.trace_rays_all(q)) if kind == "rays" else (lambda: sc.within_radius(q))
        row = bench(calls)
        row["queries"], row["records"] = n, total
        row["count_mean"], row["count_median"], row["count_max"] = float(c.mean()), float(np.median(c)), int(c.max())
        row["list_over_count"] = row["list"]["ms_median"] / row["count"]["ms_median"]
        if "count_k32" in row:
            row["list_over_count_k32"] = row["list"]["ms_median"] / row["count_k32"]["ms_median"]
        sys.stderr.write(f"{kind}: {json.dumps(row)}\n")
        return row

    res = {"scene": f"kind 1, lat_lon {a.lat_lon}", "triangles": len(tris), "tree": sc.tree_info(), "warm_up_calls": WARM, "timed_calls": a.reps,
           "timing": "device events around the calls; each call's median over the reps, the calls of a set alternating", "sets": {}}
    ra = Q.set_a(ptamd.dbg_pixel_dir(ptamd.make_camera(W, H), Q.pixel_list(W, H)))[:a.rays]
    _, pa, sa = sc.trace_rays(ra, surface=True)
    rsets = {"A camera": ra, "B bounce": Q.set_b(pa, sa, np.random.RandomState(21)), "C segments": Q.set_c(len(ra), np.random.RandomState(22))}
    for name, r in rsets.items():
        res["sets"]["rays " + name] = lists("rays", torch.from_numpy(np.ascontiguousarray(r, np.float32)).to(dev), 16)
    p = N.surface_points(np.random.RandomState(31), a.rays, R.positions(tris))
    d_p = torch.from_numpy(N.with_radius(p, 1.0)).to(dev)
    lo, hi = 0.0, 4.0      # bisection of the radius on the median count: at most 8 at lo, above 8 at hi
    for _ in range(14):
        mid = 0.5 * (lo + hi)
        d_p[:, 3] = mid
        med = float(sc.count_within(d_p).float().median().item())
        lo, hi = (mid, hi) if med <= 8 else (lo, mid)
    d_p[:, 3] = lo
    res["median8_radius"] = lo
    res["sets"]["points median 8"] = lists("points", d_p, 32)
    room = N.room_points(np.random.RandomState(32), a.long_points)
    res["sets"]["points radius inf"] = lists("points", torch.from_numpy(N.with_radius(room, float("inf"))).to(dev), 32)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
