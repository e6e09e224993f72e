"""Time the filtered queries (the eight pt_*_f entry points) against their unfiltered twins on the GPU.

  python tools/filter_time.py [--reps 7] [--out profiles/filter_time_mi355x.json]

Scene: the Cornell room + one stand-in mesh (kind 1, lat_lon 187: 69,576 triangles).  Rays: tools/ray_hits_time.py's three fixed-seed sets
of a 1920 x 1080 frame's size (2,073,600 rays each; tests/query_ref.py): A camera rays, B bounce rays from A's hits, C segments.
Points: tools/nearest_time.py's surface and room points (2,073,600 each), the surface points at the radius whose median count is 8
(bisection on the counts, as tools/lists_time.py finds it) for every point call, the room points at radius inf for the closest call.

Per set and call, in one process, alternating variant by variant after WARM calls of each, the time between two device events around
  twin       the unfiltered entry point
  neutral    the _f entry point with filter = NULL (it enqueues the twin's own kernels)
  all_pass   the _f entry point with a d_prim_bits array whose every word is 0xFFFFFFFF: the filtered kernels, nothing filtered out
  half       the _f entry point with a seeded d_prim_bits of 0 / 1 words, bits = 1: half of the primitives are members
Calls: closest, any, k = 8, count, and list = count + pt_list_offsets + fill (the three device calls, records allocated beforehand for
that variant's total).  Prints one JSON line.
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
VARIANTS = ("twin", "neutral", "all_pass", "half")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--lat-lon", type=int, default=187)
    ap.add_argument("--rays", type=int, default=W * H, help="rays (and points) per set")
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
    assert torch.cuda.is_available(), "filter_time.py needs a GPU"
    l = ptamd.lib()
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, a.lat_lon))
    sc = ptamd.Scene(nodes, tris)
    dev = torch.device("cuda:0")
    n_prims = len(tris)
    all_bits = torch.full((n_prims,), -1, dtype=torch.int32, device=dev)
    half_bits = torch.from_numpy(np.random.RandomState(40).randint(0, 2, n_prims).astype(np.int32)).to(dev)
    filters = {"neutral": None,
               "all_pass": C.byref(ptamd.PtQueryFilter(all_bits.data_ptr(), None, None, 0xFFFFFFFF, 0)),
               "half": C.byref(ptamd.PtQueryFilter(half_bits.data_ptr(), None, None, 1, 0))}

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    def bench(calls):
        """{name: call}: every call WARM times, then reps rounds of one call each, in turn."""
        for f in calls.values():
            for _ in range(WARM):
                assert f() == 0, l.pt_last_error()
        ms = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        row = {k: {"ms_median": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in ms.items()}
        for k in row:
            if k != "twin":
                row[k]["over_twin"] = row[k]["ms_median"] / row["twin"]["ms_median"]
        return row

    def one_set(kind, q, calls_wanted):
        n = q.shape[0]
        ray = kind == "rays"
        one = torch.empty((n, 2), dtype=torch.int32, device=dev)
        k8 = torch.empty((n, 8, 2), dtype=torch.int32, device=dev)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        off = torch.empty(n + 1, dtype=torch.int64, device=dev)
        scr = torch.empty(l.pt_list_offsets_scratch_bytes(n), dtype=torch.uint8, device=dev)
        S, Q_ = sc._h, ptr(q)

        def call(what, v):
            f = filters.get(v)
            if ray:
                if what in ("closest", "any"):
                    mode = int(what == "any")
                    return (lambda: l.pt_trace_rays(S, Q_, n, mode, ptr(one), None, None)) if v == "twin" else (lambda: l.pt_trace_rays_f(S, Q_, n, mode, f, ptr(one), None, None))
                if what == "k8":
                    return (lambda: l.pt_trace_rays_k(S, Q_, n, 8, 0, ptr(k8), None, None)) if v == "twin" else (lambda: l.pt_trace_rays_k_f(S, Q_, n, 8, 0, f, ptr(k8), None, None))
                return (lambda: l.pt_count_hits(S, Q_, n, 0, ptr(cnt), None)) if v == "twin" else (lambda: l.pt_count_hits_f(S, Q_, n, 0, f, ptr(cnt), None))
            if what in ("closest", "any"):
                mode = int(what == "any")
                return (lambda: l.pt_closest_points(S, Q_, n, mode, ptr(one), None, None)) if v == "twin" else (lambda: l.pt_closest_points_f(S, Q_, n, mode, f, ptr(one), None, None))
            if what == "k8":
                return (lambda: l.pt_nearest_k(S, Q_, n, 8, ptr(k8), None, None)) if v == "twin" else (lambda: l.pt_nearest_k_f(S, Q_, n, 8, f, ptr(k8), None, None))
            return (lambda: l.pt_count_within(S, Q_, n, ptr(cnt), None)) if v == "twin" else (lambda: l.pt_count_within_f(S, Q_, n, f, ptr(cnt), None))

        def list_call(v):
            count = call("count", v)
            assert count() == 0 and l.pt_list_offsets(ptr(cnt), n, ptr(off), ptr(scr), None) == 0
            total = int(off[-1].item())
            rec = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
            f = filters.get(v)

            def fill():
                if ray:
                    return l.pt_trace_rays_list(S, Q_, n, 0, ptr(off), total, ptr(rec), None, None) if v == "twin" else \
                        l.pt_trace_rays_list_f(S, Q_, n, 0, ptr(off), total, f, ptr(rec), None, None)
                return l.pt_within_radius_list(S, Q_, n, ptr(off), total, ptr(rec), None, None) if v == "twin" else \
                    l.pt_within_radius_list_f(S, Q_, n, ptr(off), total, f, ptr(rec), None, None)
            return (lambda: count() or l.pt_list_offsets(ptr(cnt), n, ptr(off), ptr(scr), None) or fill()), total

        out = {"queries": n}
        for what in calls_wanted:
            if what == "list":
                made = {v: list_call(v) for v in VARIANTS}
                row = bench({v: m[0] for v, m in made.items()})
                row["records"] = {v: m[1] for v, m in made.items()}
            else:
                row = bench({v: call(what, v) for v in VARIANTS})
            out[what] = row
            sys.stderr.write(f"{kind} {what}: {json.dumps(row)}\n")
        return out

    res = {"scene": f"kind 1, lat_lon {a.lat_lon}", "triangles": len(tris), "tree": sc.tree_info(), "warm_up_calls": WARM, "timed_calls": a.reps,
           "timing": "device events around the calls; each variant's median over the reps, the variants of a call alternating", "sets": {}}
    ra = Q.set_a(ptamd.dbg_pixel_dir(ptamd.make_camera(W, H), Q.pixel_list(W, H)))[:a.rays]
    _, pa, sa = sc.trace_rays(ra, surface=True)
    rsets = {"A camera": ra, "B bounce": Q.set_b(pa, sa, np.random.RandomState(21)), "C segments": Q.set_c(len(ra), np.random.RandomState(22))}
    every = ("closest", "any", "k8", "count", "list")
    for name, r in rsets.items():
        res["sets"]["rays " + name] = one_set("rays", torch.from_numpy(np.ascontiguousarray(r, np.float32)).to(dev), every)
    rs = np.random.RandomState(77)
    room = N.room_points(rs, a.rays)
    surface = N.surface_points(rs, a.rays, R.positions(tris))
    d_p = torch.from_numpy(N.with_radius(surface, 1.0)).to(dev)
    lo, hi = 0.0, 4.0      # bisection of the radius on the median count: at most 8 at lo, above 8 at hi
    for _ in range(14):
        mid = 0.5 * (lo + hi)
        d_p[:, 3] = mid
        med = float(sc.count_within(d_p).float().median().item())
        lo, hi = (mid, hi) if med <= 8 else (lo, mid)
    d_p[:, 3] = lo
    res["median8_radius"] = lo
    res["sets"]["points surface, median 8"] = one_set("points", d_p, every)
    res["sets"]["points room, radius inf"] = one_set("points", torch.from_numpy(N.with_radius(room, float("inf"))).to(dev), ("closest", "any"))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
