"""Query filters: primitive masks, a skipped primitive per query and a near bound on every query (the eight pt_*_f entry points,
ptamd.QueryFilter and the filter= keyword of the Scene's query methods; include/pt_api.h "Query filters").

A filtered query answers over a subset H' of the set H its unfiltered twin is defined over, so the yardstick is a numpy selection
(tests/filters_ref.py: select) from the brute-force lists that exist: ray_hits_ref.brute for rays, nearest_k_ref / lists_ref for points,
both in CSR form as tests/test_lists.py keeps them.

On the CPU: the C-ABI surface and the place of the section, every argument check with a fake scene and fake device addresses, the
wrappers' own checks, the yardstick's identities, and the conditions on the inputs (CONDITIONS below: what the seeded filters must hit,
asserted on the reference before any comparison).

On the GPU: bits only, no tolerance, no query left out.  Every slot, count, offset, record and detail record of all eight calls against
the selection of brute force and against the selection of the product's own unfiltered lists, for K in (1, 2, 5, 8, 9, 32), both flag
values and every filter of the recipe; the any forms; the neutral filter against each twin; partial waves and per-query arrays at an
odd word offset, between sentinels; the binary walk forced by its knob in a fresh process; the same bits whatever tree the scene
holds; an update, a count, the scan and a fill on one stream; no side effect on a render; a batch with odd rays."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import dynamic_ref as R
import filters_ref as FR
import lists_ref as L
import ptamd
import query_ref as Q
import test_lists as TL
import test_nearest as T
import test_nearest_k as TK
import test_ray_hits as TH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pathtrace-on-cuda_amd")
F = np.float32
bits = TH.bits
KS = FR.KS
RAY_SCENES = TH.SCENES                  # the four ray scenes and ray sets of tests/test_ray_hits.py, <= 4,096 rays each
POINT_SCENES = T.SCENES                 # nearest_k_ref.PointSets on the scenes of tests/test_nearest.py, as tests/test_lists.py draws them
SEEDS = {name: 300 + i for i, name in enumerate(RAY_SCENES + POINT_SCENES)}
SENT = 0x5A5A5A5A
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ray_H(name, both):
    """(offsets, t, prim, detail): every H of the scene's ray set."""
    return TL.ray_want(name, both)


def point_H(name):
    """(points, (offsets, dist2, prim, detail))"""
    pts, want, _ = TL.point_case(name)
    return pts, want


def ray_recipe(name):
    c = TH.case(name)
    return _cached(("rr", name), lambda: FR.Recipe(ray_H(name, True), c.n_prims, c.n_tris, SEEDS[name], True))


def point_recipe(name):
    n_tris = len(T._positions(name))
    return _cached(("pr", name), lambda: FR.Recipe(point_H(name)[1], T._n_prims(name), n_tris, SEEDS[name], False))


def qfilter(flt):
    """ptamd.QueryFilter of a recipe's (name, prim_bits, m, skip, tmin)."""
    _, pb, m, skip, tmin = flt
    per_query = np.ndim(m) > 0
    return ptamd.QueryFilter(prim_bits=pb, bits=0xFFFFFFFF if per_query else int(m), query_bits=m if per_query else None, skip=skip, tmin=tmin is not None)


def with_tmin(rays, tmin):
    """The rays with their 7th float set (0 where the filter has no near bound: the field every other call ignores)."""
    r = np.array(rays, F, copy=True)
    if tmin is not None:
        r[:, 6] = tmin
    return np.ascontiguousarray(r)


def selected(H, flt):
    return FR.select(H, flt[1], flt[2], flt[3], flt[4])


# ---------------------------------------------------------------------------------------------------------------------------------
# the conditions on the inputs: existence conditions, each met by at least 5 queries over the sets (counts of queries)
# ---------------------------------------------------------------------------------------------------------------------------------
CONDITIONS = ("emptied", "first_removed", "long_to_short", "still_long", "tie_split", "kept_at_tmin", "dropped_below_tmin", "sphere_by_bits",
              "between_roots", "nearest_is_sphere")


def _tie_split(H, Hs):
    """Queries with two adjacent members of H of equal key (compared as floats) of which exactly one is in H'."""
    off, key, prim = H[0], H[1], H[2]
    own = FR.owners(off)
    in_s = np.isin(own.astype(np.int64) * (1 << 32) + prim, FR.owners(Hs[0]).astype(np.int64) * (1 << 32) + Hs[2])      # (query, prim): a sphere's two roots never tie
    if len(key) < 2:
        return 0
    pair = (own[1:] == own[:-1]) & (key[1:] == key[:-1]) & (in_s[1:] != in_s[:-1])
    return len(np.unique(own[1:][pair]))


def ray_condition_counts(name):
    def make():
        c, rec = TH.case(name), ray_recipe(name)
        out = dict.fromkeys(CONDITIONS, 0)
        for both in (False, True):
            H = ray_H(name, both)
            cnt = np.diff(H[0])
            for flt in rec.filters():
                Hs = selected(H, flt)
                cs = np.diff(Hs[0])
                out["emptied"] += int(((cnt > 0) & (cs == 0)).sum())
                ne = (cnt > 0) & (cs > 0)
                out["first_removed"] += int((H[2][H[0][:-1][ne]] != Hs[2][Hs[0][:-1][ne]]).sum())
                out["long_to_short"] += int(((cnt > 32) & (cs <= 32) & (cs >= 1)).sum())
                out["still_long"] += int((cs > 32).sum())
                out["tie_split"] += _tie_split(H, Hs)
                if flt[1] is not None and flt[3] is None and flt[4] is None:
                    sph = H[2] >= c.n_tris
                    gone = ~np.isin(FR.owners(H[0])[sph].astype(np.int64) * (1 << 32) + H[2][sph], FR.owners(Hs[0]).astype(np.int64) * (1 << 32) + Hs[2])
                    out["sphere_by_bits"] += len(np.unique(FR.owners(H[0])[sph][gone]))
            own = FR.owners(H[0])
            tm = rec.tmin[own]
            only = selected(H, ("", None, np.uint32(0xFFFFFFFF), None, rec.tmin))
            at = (H[1] == tm) & (tm > 0)
            out["kept_at_tmin"] += len(np.unique(own[at]))
            assert np.isin(own[at].astype(np.int64) * (1 << 32) + H[2][at], FR.owners(only[0]).astype(np.int64) * (1 << 32) + only[2]).all()
            below = (np.nextafter(H[1], F(np.inf)) == tm) & (tm > 0)
            out["dropped_below_tmin"] += len(np.unique(own[below]))
            if both:
                for q in np.nonzero(rec.tmin > 0)[0]:
                    row, t = H[2][H[0][q]:H[0][q + 1]], H[1][H[0][q]:H[0][q + 1]]
                    for p in np.unique(row[row >= c.n_tris]):
                        r = t[row == p]
                        if len(r) == 2 and r[0] < rec.tmin[q] < r[1]:
                            out["between_roots"] += 1
        return out
    return _cached(("rc", name), make)


def point_condition_counts(name):
    def make():
        n_tris = len(T._positions(name))
        _, H = point_H(name)
        cnt = np.diff(H[0])
        out = dict.fromkeys(CONDITIONS, 0)
        for flt in point_recipe(name).filters():
            Hs = selected(H, flt)
            cs = np.diff(Hs[0])
            out["emptied"] += int(((cnt > 0) & (cs == 0)).sum())
            ne = (cnt > 0) & (cs > 0)
            out["first_removed"] += int((H[2][H[0][:-1][ne]] != Hs[2][Hs[0][:-1][ne]]).sum())
            out["long_to_short"] += int(((cnt > 32) & (cs <= 32) & (cs >= 1)).sum())
            out["still_long"] += int((cs > 32).sum())
            out["tie_split"] += _tie_split(H, Hs)
            out["nearest_is_sphere"] += int((Hs[2][Hs[0][:-1][cs > 0]] >= n_tris).sum())
            if flt[1] is not None and flt[3] is None:
                own, sph = FR.owners(H[0]), H[2] >= n_tris
                gone = ~np.isin(own[sph].astype(np.int64) * (1 << 32) + H[2][sph], FR.owners(Hs[0]).astype(np.int64) * (1 << 32) + Hs[2])
                out["sphere_by_bits"] += len(np.unique(own[sph][gone]))
        return out
    return _cached(("pc", name), make)


def assert_conditions():
    rays, points = dict.fromkeys(CONDITIONS, 0), dict.fromkeys(CONDITIONS, 0)
    for name in RAY_SCENES:
        for k, v in ray_condition_counts(name).items():
            rays[k] += v
    for name in POINT_SCENES:
        for k, v in point_condition_counts(name).items():
            points[k] += v
    print(f"ray sets: {rays}\npoint sets: {points}")
    for key in ("emptied", "first_removed", "long_to_short", "still_long", "tie_split", "sphere_by_bits"):      # per kind
        assert rays[key] >= 5 and points[key] >= 5, (key, rays[key], points[key])
    for key in ("kept_at_tmin", "dropped_below_tmin", "between_roots"):
        assert rays[key] >= 5, (key, rays[key])
    assert points["nearest_is_sphere"] >= 5, points["nearest_is_sphere"]


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
NEW = ("pt_query_filter_default", "pt_trace_rays_f", "pt_trace_rays_k_f", "pt_count_hits_f", "pt_trace_rays_list_f", "pt_closest_points_f",
       "pt_nearest_k_f", "pt_count_within_f", "pt_within_radius_list_f")
METHODS = ("trace_rays", "trace_rays_k", "count_hits", "trace_rays_all", "closest_points", "nearest_k", "count_within", "within_radius")


def test_new_symbols_are_exported_declared_and_bound(tmp_path):
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    for name in METHODS:
        assert inspect.signature(getattr(ptamd.Scene, name)).parameters["filter"].default is None, name
    assert ptamd.FILTER_TMIN == 1 and C.sizeof(ptamd.PtQueryFilter) == 32
    src = tmp_path / "filter.c"
    src.write_text('#include <stddef.h>\n#include "pt_api.h"\n_Static_assert(PT_FILTER_TMIN == 1u, "PT_FILTER_TMIN");\n'
                   '_Static_assert(sizeof(PtQueryFilter) == 32 && offsetof(PtQueryFilter, bits) == 24 && offsetof(PtQueryFilter, flags) == 28, "PtQueryFilter");\n')
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    at = hdr.index("Query filters (new")
    assert hdr.index("Variable-length query results") < at < hdr.index("Radiance along the caller's own rays")
    assert hdr.index(" pt_within_radius_list_host(") < at < hdr.index(" pt_query_filter_default(")      # directly after that section
    assert all(at < hdr.index(f" {name}(") < hdr.index("Radiance along the caller's own rays") for name in NEW)
    f = ptamd.PtQueryFilter(1, 2, 3, 4, 5)
    ptamd.lib().pt_query_filter_default(C.byref(f))
    assert (f.d_prim_bits, f.d_query_bits, f.d_skip_prim, f.bits, f.flags) == (None, None, None, 0xFFFFFFFF, 0)
    ptamd.lib().pt_query_filter_default(None)


# how each call takes (scene, queries, n, filter, out, detail, offsets); its k / mode / flags are valid ones
CALLS = {
    "pt_trace_rays_f": (True, lambda s, q, n, f, o, d, off: (s, q, n, 0, f, o, d, None)),
    "pt_trace_rays_k_f": (True, lambda s, q, n, f, o, d, off: (s, q, n, 8, 1, f, o, d, None)),
    "pt_count_hits_f": (True, lambda s, q, n, f, o, d, off: (s, q, n, 0, f, o, None)),
    "pt_trace_rays_list_f": (True, lambda s, q, n, f, o, d, off: (s, q, n, 1, off, 100, f, o, d, None)),
    "pt_closest_points_f": (False, lambda s, q, n, f, o, d, off: (s, q, n, 0, f, o, d, None)),
    "pt_nearest_k_f": (False, lambda s, q, n, f, o, d, off: (s, q, n, 8, f, o, d, None)),
    "pt_count_within_f": (False, lambda s, q, n, f, o, d, off: (s, q, n, f, o, None)),
    "pt_within_radius_list_f": (False, lambda s, q, n, f, o, d, off: (s, q, n, off, 100, f, o, d, None)),
}


def test_bad_arguments_are_rejected_before_any_device_call():
    """A fake scene and fake device addresses: never dereferenced, and no HIP call is made, when an argument is bad.  The twin's checks
    come first, in the twin's order; then unknown filter flags, PT_FILTER_TMIN on a point query, a misaligned filter array."""
    l = ptamd.lib()
    base = 1 << 40
    scene, q, out, det, offs, pb, qb, sk = (base + (i << 20) for i in range(8))
    P = C.c_void_p
    flt = lambda pb_=pb, qb_=qb, sk_=sk, bits_=5, flags=0: C.byref(ptamd.PtQueryFilter(pb_, qb_, sk_, bits_, flags))      # noqa: E731
    for name, (rays, args) in CALLS.items():
        fn = getattr(l, name)
        err = lambda: l.pt_last_error().decode()      # noqa: E731
        tag = name + ":"
        a = lambda **kw: args(*(kw.get(k, v) for k, v in (("s", P(scene)), ("q", P(q)), ("n", 64), ("f", flt()), ("o", P(out)), ("d", None), ("off", P(offs)))))      # noqa: E731
        # the twin's checks, with a good filter
        for what, kw, msg in (("NULL scene", {"s": None}, "NULL scene"), ("NULL queries", {"q": None}, "NULL"), ("NULL output", {"o": None}, "NULL"),
                              ("n < 0", {"n": -1}, "n < 0"), ("queries + 4", {"q": P(q + 4)}, "16-byte aligned"), ("output + 2", {"o": P(out + 2)}, "aligned")):
            assert fn(*a(**kw)) == -1, (name, what)
            assert err().startswith(tag) and msg in err(), (name, what, err())
        # the filter's checks
        bad = [("flags 2", flt(flags=2), "unknown filter flags"), ("flags 3", flt(flags=3), "unknown filter flags"), ("flags 1 << 31", flt(flags=1 << 31), "unknown filter flags"),
               ("prim_bits + 2", flt(pb_=pb + 2), "d_prim_bits must be 4-byte aligned"), ("query_bits + 1", flt(qb_=qb + 1), "d_query_bits must be 4-byte aligned"),
               ("skip + 3", flt(sk_=sk + 3), "d_skip_prim must be 4-byte aligned")]
        if not rays:
            bad.append(("tmin on points", flt(flags=1), "PT_FILTER_TMIN applies to ray queries only"))
        for what, f, msg in bad:
            assert fn(*a(f=f)) == -1, (name, what)
            assert err().startswith(tag) and msg in err(), (name, what, err())
            assert fn(*a(f=f, n=0)) == -1, (name, what, "n = 0 does not excuse it")
        # the twin's come first
        assert fn(*a(q=P(q + 8), f=flt(flags=2))) == -1 and "16-byte aligned" in err(), (name, err())
        assert fn(*a(n=-2, f=flt(pb_=pb + 1))) == -1 and "n < 0" in err(), (name, err())
        if name not in ("pt_count_hits_f", "pt_count_within_f"):
            assert fn(*a(d=P(det + 2), f=flt(flags=2))) == -1 and "4-byte aligned" in err() and "filter" not in err(), (name, err())
        # nothing to do: PT_OK, still without touching the scene, the filter's arrays or the device
        for f in (None, flt(), flt(None, None, None, 0xFFFFFFFF, 0), flt(pb + 4, qb + 8, sk + 12, 0, 0)) + ((flt(flags=1),) if rays else ()):
            assert fn(*a(n=0, f=f)) == 0, (name, err())
    # the queries' own parameters, before the filter's
    assert l.pt_trace_rays_k_f(P(scene), P(q), 64, 33, 0, flt(flags=2), P(out), None, None) == -1 and "PT_RAY_HITS_KMAX" in l.pt_last_error().decode()
    assert l.pt_trace_rays_k_f(P(scene), P(q), 64, 8, 2, flt(flags=2), P(out), None, None) == -1 and "PT_HITS_FRONT" in l.pt_last_error().decode()
    assert l.pt_count_hits_f(P(scene), P(q), 64, 7, flt(flags=2), P(out), None) == -1 and "PT_HITS_FRONT" in l.pt_last_error().decode()
    assert l.pt_trace_rays_list_f(P(scene), P(q), 64, 0, P(offs), -1, flt(flags=2), P(out), None, None) == -1 and "cap < 0" in l.pt_last_error().decode()
    assert l.pt_trace_rays_list_f(P(scene), P(q), 64, 0, None, 10, flt(), P(out), None, None) == -1 and "NULL offsets" in l.pt_last_error().decode()
    assert l.pt_within_radius_list_f(P(scene), P(q), 64, P(offs + 4), 10, flt(), P(out), None, None) == -1 and "8-byte aligned" in l.pt_last_error().decode()
    assert l.pt_trace_rays_f(P(scene), P(q), 64, 2, flt(flags=2), P(out), None, None) == -1 and "mode must be" in l.pt_last_error().decode()
    assert l.pt_trace_rays_f(P(scene), P(q), 64, 1, flt(), P(out), P(det), None) == -1 and "no surface record" in l.pt_last_error().decode()
    assert l.pt_closest_points_f(P(scene), P(q), 64, 1, flt(), P(out), P(det), None) == -1 and "no detail record" in l.pt_last_error().decode()
    assert l.pt_nearest_k_f(P(scene), P(q), 64, 0, flt(flags=2), P(out), None, None) == -1 and "PT_NEAREST_KMAX" in l.pt_last_error().decode()


class _FakeScene:
    n_tris, n_spheres, device, _h = 5, 1, 0, C.c_void_p(1 << 40)
    _filtered = ptamd.Scene._filtered
    trace_rays, trace_rays_k, count_hits, trace_rays_all = (getattr(ptamd.Scene, m) for m in ("trace_rays", "trace_rays_k", "count_hits", "trace_rays_all"))
    closest_points, nearest_k, count_within, within_radius = (getattr(ptamd.Scene, m) for m in ("closest_points", "nearest_k", "count_within", "within_radius"))


def test_wrapper_checks_the_filter_on_the_host():
    import torch
    QF = ptamd.QueryFilter
    for kw in ({"bits": -1}, {"bits": 1 << 32}, {"prim_bits": np.zeros(6, np.float32)}, {"prim_bits": np.zeros((6, 1), np.uint32)}, {"query_bits": np.zeros(4, np.int64)},
               {"skip": np.zeros(4, np.uint32)}, {"skip": [0, 1, 2, 3]}, {"prim_bits": torch.zeros(6, dtype=torch.float32)}, {"skip": torch.zeros((4, 1), dtype=torch.int32)},
               {"query_bits": torch.zeros(8, dtype=torch.int32)[::2]}):
        with pytest.raises(ptamd.PtError):
            QF(**kw)
    fake = _FakeScene()
    rays, pts = np.zeros((4, 8), F), np.zeros((4, 4), F)
    S = ptamd.Scene
    ray_calls = (lambda f: S.trace_rays(fake, rays, filter=f), lambda f: S.trace_rays_k(fake, rays, 4, filter=f), lambda f: S.count_hits(fake, rays, filter=f),
                 lambda f: S.trace_rays_all(fake, rays, filter=f))
    point_calls = (lambda f: S.closest_points(fake, pts, filter=f), lambda f: S.nearest_k(fake, pts, 4, filter=f), lambda f: S.count_within(fake, pts, filter=f),
                   lambda f: S.within_radius(fake, pts, filter=f))
    wrong = (QF(prim_bits=np.zeros(5, np.uint32)), QF(query_bits=np.zeros(3, np.uint32)), QF(skip=np.zeros(5, np.int32)), QF(prim_bits=torch.zeros(6, dtype=torch.int32)),
             "a filter", {"bits": 1})      # 6 primitives, 4 queries; a CPU tensor; not a QueryFilter
    for call in ray_calls + point_calls:
        for f in wrong:
            with pytest.raises(ptamd.PtError):
                call(f)
    for call in point_calls:
        with pytest.raises(ptamd.PtError, match="ray queries only"):
            call(QF(tmin=True))
    for bad in (np.zeros((4, 7), F), torch.zeros((4, 8)), [[0.0] * 8]):      # the twin's checks of the queries hold with a filter
        with pytest.raises(ptamd.PtError):
            S.trace_rays_k(fake, bad, 4, filter=QF())
    with pytest.raises(ptamd.PtError):
        S.trace_rays_k(fake, rays, 33, filter=QF())
    with pytest.raises(ptamd.PtError):
        S.trace_rays(fake, rays, any_hit=True, surface=True, filter=QF())
    f = QF(prim_bits=np.arange(6, dtype=np.uint32), bits=3, skip=np.arange(4, dtype=np.int32), tmin=True)
    assert f.bits == 3 and f.tmin
    # n = 0 on the numpy path: the empty arrays of the unfiltered call, without a device — after the filter's own checks
    e8, e4 = np.zeros((0, 8), F), np.zeros((0, 4), F)
    fr, fp = QF(prim_bits=np.zeros(6, np.uint32), skip=np.zeros(0, np.int32), tmin=True), QF(prim_bits=np.zeros(6, np.uint32), query_bits=np.zeros(0, np.uint32))
    t, prim, det = S.trace_rays_k(fake, e8, 7, both_sides=True, detail=True, filter=fr)
    assert t.shape == (0, 7) and prim.shape == (0, 7) and det.shape == (0, 7, 4) and t.dtype == F and prim.dtype == np.int32
    t, prim, surf = S.trace_rays(fake, e8, surface=True, filter=fr)
    assert t.shape == (0,) and prim.dtype == np.int32 and surf.shape == (0, 29)
    assert S.count_hits(fake, e8, filter=fr).shape == (0,) and S.count_within(fake, e4, filter=fp).shape == (0,)
    d2, prim, det = S.nearest_k(fake, e4, 5, detail=True, filter=fp)
    assert d2.shape == (0, 5) and det.shape == (0, 5, 8)
    d2, prim = S.closest_points(fake, e4, any_within=True, filter=fp)
    assert d2.shape == (0,) and prim.shape == (0,)
    off, t, prim, det = S.trace_rays_all(fake, e8, detail=True, filter=fr)
    assert np.array_equal(off, [0]) and t.shape == (0,) and det.shape == (0, 4)
    off, d2, prim = S.within_radius(fake, e4, filter=fp)
    assert np.array_equal(off, [0]) and d2.shape == (0,)
    for call, q in ((S.trace_rays_k, e8), (S.nearest_k, e4)):
        with pytest.raises(ptamd.PtError):
            call(fake, q, 4, filter=QF(skip=np.zeros(3, np.int32)))      # three entries for no query


@pytest.mark.parametrize("name", RAY_SCENES)
def test_yardstick_identities_on_rays(name):
    """The neutral filter returns H; the selection keeps H's order, so it commutes with cutting at k: the survivors of the first k
    members of H are the first survivors of H — select(cut_k(H)) is a prefix of select(H), and all of it where |H| <= k."""
    rec = ray_recipe(name)
    for both in (False, True):
        H = ray_H(name, both)
        n = len(H[0]) - 1
        assert FR.same(FR.select(H, None, np.uint32(0xFFFFFFFF), None, None), H)
        assert FR.same(FR.select(H, rec.all_set, np.full(n, 0xFFFFFFFF, np.uint32), np.full(n, -1), np.zeros(n, F)), H)
        assert np.diff(FR.select(H, rec.prim_bits, np.uint32(0), None, None)[0]).sum() == 0
        for k in (1, 8, 32):
            key, prim = FR.cut(H, k)[:2]
            Hk = FR.uncut(key, prim, k)
            for flt in rec.filters():
                a, b = selected(Hk, flt), selected(H[:3], flt)
                ca, cb = np.diff(a[0]), np.diff(b[0])
                assert (ca <= cb).all() and (ca[np.diff(H[0]) <= k] == cb[np.diff(H[0]) <= k]).all()
                assert FR.same(FR.cut(a, k), tuple(np.where((np.arange(k)[None, :] < ca[:, None]), x, fill) for x, fill in zip(FR.cut(b, k), (F(0), np.int32(-1))))), (name, k, flt[0])


@pytest.mark.parametrize("name", ["standin24_spheres", "attribute"])
def test_yardstick_identities_on_points(name):
    _, H = point_H(name)
    rec = point_recipe(name)
    assert FR.same(FR.select(H, None, np.uint32(0xFFFFFFFF), None, None), H)
    for k in (1, 8, 32):
        key, prim = FR.cut(H, k)[:2]
        Hk = FR.uncut(key, prim, k)
        for flt in rec.filters():
            a, b = selected(Hk, flt), selected(H[:3], flt)
            ca = np.diff(a[0])
            assert FR.same(FR.cut(a, k), tuple(np.where((np.arange(k)[None, :] < ca[:, None]), x, fill) for x, fill in zip(FR.cut(b, k), (F(0), np.int32(-1))))), (name, k, flt[0])


def test_filters_hit_what_they_should():
    assert_conditions()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


def _combo(own, keybits, prim):
    return set(zip(own.tolist(), keybits.tolist(), prim.tolist()))


def assert_any(got, Hs, what):
    """An any form: prim >= 0 exactly when H' is not empty, and then (key, prim) is a member of H', bit for bit; else the miss record."""
    key, prim = np.asarray(got[0]), np.asarray(got[1])
    cs = np.diff(Hs[0])
    assert np.array_equal(prim >= 0, cs > 0), f"{what}: {((prim >= 0) != (cs > 0)).sum()} queries disagree with 'H' is not empty'"
    assert (bits(key[prim < 0]) == 0).all() and (prim >= -1).all(), what
    members = _combo(FR.owners(Hs[0]), bits(Hs[1]), Hs[2])
    hit = np.nonzero(prim >= 0)[0]
    missing = [i for i in hit.tolist() if (i, int(bits(key[i:i + 1])[0]), int(prim[i])) not in members]
    assert not missing, f"{what}: {len(missing)} answers are no member of H', first at {missing[:5]}"


def _check_ray_scene(sc, name, rays, H_of, filters, what, ks=KS, product=True):
    """Every filtered ray call of `sc` on `rays` against the selection of H_of[both], and of the product's own unfiltered lists."""
    for both in (False, True):
        H = H_of[both]
        mine = sc.trace_rays_all(rays, both_sides=both, detail=True) if product else None
        for flt in filters:
            w = f"{what}, both = {both}, {flt[0]}"
            r, f = with_tmin(rays, flt[4]), qfilter(flt)
            Hs = selected(H, flt)
            cnt = sc.count_hits(r, both_sides=both, filter=f)
            assert cnt.dtype == np.int32 and np.array_equal(cnt, np.diff(Hs[0])), f"{w}: {(cnt != np.diff(Hs[0])).sum()} counts differ"
            got = sc.trace_rays_all(r, both_sides=both, detail=True, filter=f)
            TL.assert_csr(got, Hs, w + ", the list")
            if product:
                TL.assert_csr(got, selected(tuple(np.asarray(x) for x in mine), flt), w + ", the list against the selection of trace_rays_all")
            for k in ks:
                TH.assert_lists(sc.trace_rays_k(r, k, both_sides=both, detail=True, filter=f), FR.cut(Hs, k), f"{w}, K = {k}")
            if not both:
                assert_any(sc.trace_rays(r, any_hit=True, filter=f), Hs, w + ", any hit")
                t, prim = sc.trace_rays(r, filter=f)
                want = FR.cut(Hs, 1)
                assert np.array_equal(prim, want[1][:, 0]) and np.array_equal(bits(t), bits(want[0][:, 0])), f"{w}: the closest form"
                t1, p1 = sc.trace_rays_k(r, 1, filter=f)
                assert np.array_equal(bits(t1[:, 0]), bits(t)) and np.array_equal(p1[:, 0], prim), f"{w}: column 0 of the K call is not the closest call"


@pytest.mark.gpu
@pytest.mark.parametrize("name", RAY_SCENES)
def test_filtered_ray_calls_are_the_selection_of_brute_force(_gpu, name):
    assert_conditions()
    c, sc = TH.case(name), TL.ray_scene(name)
    TH.assert_inputs(name, sc)
    _check_ray_scene(sc, name, c.rays, {b: ray_H(name, b) for b in (False, True)}, ray_recipe(name).filters(), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sheet", "standin24_spheres"])
def test_filtered_surface_records_and_device_tensors(_gpu, name):
    """d_surface29 through the existing surface kernel: with the filter that keeps everything (arrays given, so the filtered kernels run)
    the twin's records, bit for bit; with a selective one the record of the hit the filtered query returns — the twin's record for a ray
    that stops just behind that hit —, zeros for a miss.  And torch tensors in, torch tensors out, the same bits as the numpy path."""
    import torch
    c, sc = TH.case(name), TL.ray_scene(name)
    rec = ray_recipe(name)
    keep_all = [f for f in rec.filters() if f[0].startswith("every word set")][0]
    t0, p0, s0 = sc.trace_rays(c.rays, surface=True)
    t1, p1, s1 = sc.trace_rays(c.rays, surface=True, filter=qfilter(keep_all))
    assert np.array_equal(bits(t0), bits(t1)) and np.array_equal(p0, p1) and np.array_equal(bits(s0), bits(s1))
    flt = [f for f in rec.filters() if f[0] == "all four fields"][0]
    r, f = with_tmin(c.rays, flt[4]), qfilter(flt)
    t, prim, surf = sc.trace_rays(r, surface=True, filter=f)
    assert (surf[prim < 0] == 0).all() and (surf[prim >= 0, 0] == 1).all() and np.array_equal(bits(surf[prim >= 0, 1]), bits(t[prim >= 0]))
    d = torch.from_numpy(r).cuda()
    fd = ptamd.QueryFilter(prim_bits=torch.from_numpy(flt[1].view(np.int32)).cuda(), query_bits=torch.from_numpy(flt[2].view(np.int32)).cuda(),
                           skip=torch.from_numpy(flt[3]).cuda(), tmin=True)
    td, pd, sd = sc.trace_rays(d, surface=True, filter=fd)
    assert td.dtype == torch.float32 and pd.dtype == torch.int32 and td.device == d.device
    torch.cuda.synchronize()
    assert np.array_equal(bits(td.cpu().numpy()), bits(t)) and np.array_equal(pd.cpu().numpy(), prim) and np.array_equal(bits(sd.cpu().numpy()), bits(surf))
    got = sc.trace_rays_all(d, both_sides=True, detail=True, filter=fd)
    TL.assert_csr(got, selected(ray_H(name, True), flt), f"{name}: device tensors, the list")
    cd = sc.count_hits(d, both_sides=True, filter=fd)
    assert np.array_equal(cd.cpu().numpy(), np.diff(got[0].cpu().numpy()))


def _check_point_scene(sc, pts, H, filters, what, ks=KS, product=True):
    mine = sc.within_radius(pts, detail=True) if product else None
    for flt in filters:
        w = f"{what}, {flt[0]}"
        f = qfilter(flt)
        Hs = selected(H, flt)
        cnt = sc.count_within(pts, filter=f)
        assert cnt.dtype == np.int32 and np.array_equal(cnt, np.diff(Hs[0])), f"{w}: {(cnt != np.diff(Hs[0])).sum()} counts differ"
        got = sc.within_radius(pts, detail=True, filter=f)
        TL.assert_csr(got, Hs, w + ", the list")
        if product:
            TL.assert_csr(got, selected(tuple(np.asarray(x) for x in mine), flt), w + ", the list against the selection of within_radius")
        for k in ks:
            TK.assert_lists(sc.nearest_k(pts, k, detail=True, filter=f), FR.cut(Hs, k), f"{w}, K = {k}")
        assert_any(sc.closest_points(pts, any_within=True, filter=f), Hs, w + ", any within")
        d2, prim, det = sc.closest_points(pts, detail=True, filter=f)
        want = FR.cut(Hs, 1)
        assert np.array_equal(prim, want[1][:, 0]) and np.array_equal(bits(d2), bits(want[0][:, 0])), f"{w}: the closest form"
        assert np.array_equal(bits(det), bits(want[2][:, 0])), f"{w}: the closest form's detail records"
        d1, p1 = sc.nearest_k(pts, 1, filter=f)
        assert np.array_equal(bits(d1[:, 0]), bits(d2)) and np.array_equal(p1[:, 0], prim), f"{w}: column 0 of the K call is not the closest call"


@pytest.mark.gpu
@pytest.mark.parametrize("name", POINT_SCENES)
def test_filtered_point_calls_are_the_selection_of_brute_force(_gpu, name):
    assert_conditions()
    pts, H = point_H(name)
    sc = TL.point_scene(name)
    TK._assert_walk(sc, name)
    _check_point_scene(sc, pts, H, point_recipe(name).filters(), name)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded(n_words, pad=256):
    import torch
    return torch.full((n_words + 2 * pad,), SENT, dtype=torch.int32, device="cuda:0"), pad


def _inside(buf, pad, what):
    b = buf.cpu().numpy()
    assert (b[:pad] == SENT).all() and (b[-pad:] == SENT).all(), what + ": written outside the records"
    return b[pad:-pad]


def _odd(a):
    """A device copy of the int32 / uint32 array one word into a larger allocation: (tensor kept alive, address)."""
    import torch
    big = torch.full((len(a) + 3,), 0x7F7F7F7F, dtype=torch.int32, device="cuda:0")
    big[1:1 + len(a)] = torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()
    return big, big.data_ptr() + 4


def _c_filter(flt, lo, m, keep):
    """PtQueryFilter of a recipe's filter for the queries lo .. lo + m - 1, its per-query arrays at an odd word offset."""
    _, pb, mk, skip, tmin = flt
    s = ptamd.PtQueryFilter(None, None, None, 0xFFFFFFFF, ptamd.FILTER_TMIN if tmin is not None else 0)
    if pb is not None:
        t = _dev(pb.view(np.int32))
        keep.append(t)
        s.d_prim_bits = t.data_ptr()
    if np.ndim(mk) > 0:
        t, s.d_query_bits = _odd(mk[lo:lo + m])
        keep.append(t)
    else:
        s.bits = int(mk)
    if skip is not None:
        t, s.d_skip_prim = _odd(skip[lo:lo + m])
        keep.append(t)
    return s


def _run_c(l, sc, kind, d_q, m, k, flags, fptr, detw):
    """One count, scan, fill and K call through the C-ABI with every output between sentinels: (count, CSR list, K list)."""
    import torch
    P = C.c_void_p
    ray = kind == "rays"
    cnt, pad = _padded(m)
    rc = (l.pt_count_hits_f(sc._h, P(d_q.data_ptr()), m, flags, fptr, P(cnt.data_ptr() + 4 * pad), None) if ray else
          l.pt_count_within_f(sc._h, P(d_q.data_ptr()), m, fptr, P(cnt.data_ptr() + 4 * pad), None))
    assert rc == 0, l.pt_last_error()
    torch.cuda.synchronize()
    count = _inside(cnt, pad, "count").copy()
    off = ptamd.list_offsets(cnt[pad:pad + m].contiguous())
    total = int(off[-1].item())
    rec, _ = _padded(2 * total)
    det, _ = _padded(detw * total)
    if ray:
        rc = l.pt_trace_rays_list_f(sc._h, P(d_q.data_ptr()), m, flags, P(off.data_ptr()), total, fptr, P(rec.data_ptr() + 4 * pad), P(det.data_ptr() + 4 * pad), None)
    else:
        rc = l.pt_within_radius_list_f(sc._h, P(d_q.data_ptr()), m, P(off.data_ptr()), total, fptr, P(rec.data_ptr() + 4 * pad), P(det.data_ptr() + 4 * pad), None)
    assert rc == 0, l.pt_last_error()
    krec, _ = _padded(2 * m * k)
    kdet, _ = _padded(detw * m * k)
    if ray:
        rc = l.pt_trace_rays_k_f(sc._h, P(d_q.data_ptr()), m, k, flags, fptr, P(krec.data_ptr() + 4 * pad), P(kdet.data_ptr() + 4 * pad), None)
    else:
        rc = l.pt_nearest_k_f(sc._h, P(d_q.data_ptr()), m, k, fptr, P(krec.data_ptr() + 4 * pad), P(kdet.data_ptr() + 4 * pad), None)
    assert rc == 0, l.pt_last_error()
    one, _ = _padded(2 * m)
    mode0 = l.pt_trace_rays_f(sc._h, P(d_q.data_ptr()), m, 0, fptr, P(one.data_ptr() + 4 * pad), None, None) if ray else \
        l.pt_closest_points_f(sc._h, P(d_q.data_ptr()), m, 0, fptr, P(one.data_ptr() + 4 * pad), None, None)
    assert mode0 == 0, l.pt_last_error()
    torch.cuda.synchronize()
    r = _inside(rec, pad, "records").reshape(total, 2)
    kr = _inside(krec, pad, "K records").reshape(m, k, 2)
    o = _inside(one, pad, "closest records").reshape(m, 2)
    csr = (off.cpu().numpy(), np.ascontiguousarray(r[:, 0]).view(F), np.ascontiguousarray(r[:, 1]), _inside(det, pad, "detail").view(F).reshape(total, detw))
    klist = (np.ascontiguousarray(kr[:, :, 0]).view(F), np.ascontiguousarray(kr[:, :, 1]), _inside(kdet, pad, "K detail").view(F).reshape(m, k, detw))
    return count, csr, klist, (np.ascontiguousarray(o[:, 0]).view(F), np.ascontiguousarray(o[:, 1]))


@pytest.mark.gpu
def test_partial_waves_and_odd_offsets_between_sentinels(_gpu):
    """n = 1, 63, 64, 65 and 130 through the C-ABI, every output inside a larger sentinel-filled buffer, d_query_bits and d_skip_prim one
    word into a larger allocation: the records are the selection of brute force and nothing before or past them is written."""
    l = ptamd.lib()
    name = "sheet"
    c, sc, rec = TH.case(name), TL.ray_scene(name), ray_recipe(name)
    flt = [f for f in rec.filters() if f[0] == "all four fields"][0]
    rays = with_tmin(c.rays, flt[4])
    for both in (0, 1):
        Hs = selected(ray_H(name, bool(both)), flt)
        for k in (5, 32):
            for lo, m in TK.SLICES:
                keep = []
                s = _c_filter(flt, lo, m, keep)
                count, csr, klist, one = _run_c(l, sc, "rays", _dev(rays[lo:lo + m]), m, k, both, C.byref(s), 4)
                want = FR.rows(Hs, lo, m)
                w = f"{name}, both = {both}, K = {k}, n = {m}"
                assert np.array_equal(count, np.diff(want[0])), w
                TL.assert_csr(csr, want, w)
                TH.assert_lists(klist, FR.cut(want, k), w)
                if not both:
                    assert np.array_equal(bits(one[0]), bits(FR.cut(want, 1)[0][:, 0])) and np.array_equal(one[1], FR.cut(want, 1)[1][:, 0]), w
    name = "standin24_spheres"
    pts, H = point_H(name)
    sc, rec = TL.point_scene(name), point_recipe(name)
    flt = [f for f in rec.filters() if f[0] == "all three fields"][0]
    Hs = selected(H, flt)
    for k in (8, 32):
        for lo, m in TK.SLICES:
            keep = []
            s = _c_filter(flt, lo, m, keep)
            count, csr, klist, one = _run_c(l, sc, "points", _dev(pts[lo:lo + m]), m, k, 0, C.byref(s), 8)
            want = FR.rows(Hs, lo, m)
            w = f"{name}, K = {k}, n = {m}"
            assert np.array_equal(count, np.diff(want[0])), w
            TL.assert_csr(csr, want, w)
            TK.assert_lists(klist, FR.cut(want, k), w)
            assert np.array_equal(bits(one[0]), bits(FR.cut(want, 1)[0][:, 0])) and np.array_equal(one[1], FR.cut(want, 1)[1][:, 0]), w


@pytest.mark.gpu
def test_the_neutral_filter_is_the_twin(_gpu):
    """NULL and the explicit neutral filter: each twin's output bit for bit, between sentinels (the any forms included: the twin's own
    kernels run)."""
    import torch
    l = ptamd.lib()
    P = C.c_void_p
    neutral = ptamd.PtQueryFilter(1, 2, 3, 4, 5)
    l.pt_query_filter_default(C.byref(neutral))
    c, sc = TH.case("sheet"), TL.ray_scene("sheet")
    pts, _ = point_H("standin24_spheres")
    psc = TL.point_scene("standin24_spheres")
    m = 130
    d_rays, d_pts = _dev(c.rays[33:33 + m]), _dev(pts[33:33 + m])
    k = 9

    def outputs(call, words):
        bufs = [_padded(w) for w in words]
        assert call(*(P(b.data_ptr() + 4 * pad) for b, pad in bufs)) == 0, l.pt_last_error()
        torch.cuda.synchronize()
        return [_inside(b, pad, "neutral") for b, pad in bufs]

    for fptr in (None, C.byref(neutral)):
        for mode in (0, 1):
            a = outputs(lambda o, s: l.pt_trace_rays(sc._h, P(d_rays.data_ptr()), m, mode, o, s if mode == 0 else None, None), (2 * m, 29 * m))
            b = outputs(lambda o, s: l.pt_trace_rays_f(sc._h, P(d_rays.data_ptr()), m, mode, fptr, o, s if mode == 0 else None, None), (2 * m, 29 * m))
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), ("pt_trace_rays_f", mode)
            a = outputs(lambda o, s: l.pt_closest_points(psc._h, P(d_pts.data_ptr()), m, mode, o, s if mode == 0 else None, None), (2 * m, 8 * m))
            b = outputs(lambda o, s: l.pt_closest_points_f(psc._h, P(d_pts.data_ptr()), m, mode, fptr, o, s if mode == 0 else None, None), (2 * m, 8 * m))
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), ("pt_closest_points_f", mode)
        for flags in (0, 1):
            a = outputs(lambda o, d: l.pt_trace_rays_k(sc._h, P(d_rays.data_ptr()), m, k, flags, o, d, None), (2 * m * k, 4 * m * k))
            b = outputs(lambda o, d: l.pt_trace_rays_k_f(sc._h, P(d_rays.data_ptr()), m, k, flags, fptr, o, d, None), (2 * m * k, 4 * m * k))
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), ("pt_trace_rays_k_f", flags)
            a = outputs(lambda o: l.pt_count_hits(sc._h, P(d_rays.data_ptr()), m, flags, o, None), (m,))
            b = outputs(lambda o: l.pt_count_hits_f(sc._h, P(d_rays.data_ptr()), m, flags, fptr, o, None), (m,))
            assert np.array_equal(a[0], b[0]), ("pt_count_hits_f", flags)
            off = ptamd.list_offsets(_dev(a[0]))
            total = int(off[-1].item())
            a = outputs(lambda o, d: l.pt_trace_rays_list(sc._h, P(d_rays.data_ptr()), m, flags, P(off.data_ptr()), total, o, d, None), (2 * total, 4 * total))
            b = outputs(lambda o, d: l.pt_trace_rays_list_f(sc._h, P(d_rays.data_ptr()), m, flags, P(off.data_ptr()), total, fptr, o, d, None), (2 * total, 4 * total))
            assert total > 32 * m // 4 and all(np.array_equal(x, y) for x, y in zip(a, b)), ("pt_trace_rays_list_f", flags)
        a = outputs(lambda o, d: l.pt_nearest_k(psc._h, P(d_pts.data_ptr()), m, k, o, d, None), (2 * m * k, 8 * m * k))
        b = outputs(lambda o, d: l.pt_nearest_k_f(psc._h, P(d_pts.data_ptr()), m, k, fptr, o, d, None), (2 * m * k, 8 * m * k))
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "pt_nearest_k_f"
        a = outputs(lambda o: l.pt_count_within(psc._h, P(d_pts.data_ptr()), m, o, None), (m,))
        b = outputs(lambda o: l.pt_count_within_f(psc._h, P(d_pts.data_ptr()), m, fptr, o, None), (m,))
        assert np.array_equal(a[0], b[0]), "pt_count_within_f"
        off = ptamd.list_offsets(_dev(a[0]))
        total = int(off[-1].item())
        a = outputs(lambda o, d: l.pt_within_radius_list(psc._h, P(d_pts.data_ptr()), m, P(off.data_ptr()), total, o, d, None), (2 * total, 8 * total))
        b = outputs(lambda o, d: l.pt_within_radius_list_f(psc._h, P(d_pts.data_ptr()), m, P(off.data_ptr()), total, fptr, o, d, None), (2 * total, 8 * total))
        assert total > m and all(np.array_equal(x, y) for x, y in zip(a, b)), "pt_within_radius_list_f"


CHILD = r"""
import sys
import numpy as np
assert "torch" not in sys.modules      # the numpy-only caller: the library is loaded, and a scene made, before anything here names torch
import ptamd
res = {}
with np.load(sys.argv[1], allow_pickle=False) as g:
    sc = ptamd.Scene(g["nodes"].view(ptamd.NODE_DTYPE).reshape(-1), g["tris"], g["spheres"])
    assert not (3 * sc.tree_info()["quad_depth"] + 2 > 40)      # the 4-wide walk would fit: the knob alone forces the binary one
    rays, pts = g["rays"], g["pts"]
    fr = ptamd.QueryFilter(prim_bits=g["r_pb"], query_bits=g["r_qb"], skip=g["r_skip"], tmin=True)
    fp = ptamd.QueryFilter(prim_bits=g["p_pb"], query_bits=g["p_qb"], skip=g["p_skip"])
    for both in (0, 1):
        off, t, prim, det = sc.trace_rays_all(rays, both_sides=bool(both), detail=True, filter=fr)
        res.update({f"off_{both}": off, f"t_{both}": t, f"prim_{both}": prim, f"det_{both}": det, f"cnt_{both}": sc.count_hits(rays, both_sides=bool(both), filter=fr)})
        for k in (1, 2, 5, 8, 9, 32):
            t, prim, det = sc.trace_rays_k(rays, k, both_sides=bool(both), detail=True, filter=fr)
            res.update({f"t_{both}_{k}": t, f"prim_{both}_{k}": prim, f"det_{both}_{k}": det})
    res["ct"], res["cprim"] = sc.trace_rays(rays, filter=fr)
    res["at"], res["aprim"] = sc.trace_rays(rays, any_hit=True, filter=fr)
    off, d2, prim, det = sc.within_radius(pts, detail=True, filter=fp)
    res.update({"p_off": off, "p_d2": d2, "p_prim": prim, "p_det": det, "p_cnt": sc.count_within(pts, filter=fp)})
    for k in (1, 2, 5, 8, 9, 32):
        d2, prim, det = sc.nearest_k(pts, k, detail=True, filter=fp)
        res.update({f"p_d2_{k}": d2, f"p_prim_{k}": prim, f"p_det_{k}": det})
    res["p_cd2"], res["p_cprim"], res["p_cdet"] = sc.closest_points(pts, detail=True, filter=fp)
    res["p_ad2"], res["p_aprim"] = sc.closest_points(pts, any_within=True, filter=fp)
np.savez(sys.argv[2], **res)
"""


@pytest.mark.gpu
def test_binary_walk_forced_by_its_knob_gives_the_same_bits(_gpu, tmp_path):
    """PTAMD_QUERY_QUAD=0 in a fresh process (the knob is read when a scene is created): all eight calls with every field of the filter
    in use, on the scene with spheres.  The child is the numpy-only caller: it imports ptamd and makes its scene before torch is named
    anywhere in the process, and the filters' numpy arrays and the queries then go through torch (ptamd.lib() sees to the order in
    which the two meet the HIP runtime)."""
    name = "standin24_spheres"
    c = TH.case(name)
    pts, PH = point_H(name)
    assert np.array_equal(bits(T._spheres(name)), bits(c.spheres)) and len(T._positions(name)) == c.n_tris      # one scene serves both
    fr = [f for f in ray_recipe(name).filters() if f[0] == "all four fields"][0]
    fp = [f for f in point_recipe(name).filters() if f[0] == "all three fields"][0]
    rays = with_tmin(c.rays, fr[4])
    scene_file, out = str(tmp_path / "scene.npz"), str(tmp_path / "child.npz")
    np.savez(scene_file, nodes=np.frombuffer(c.nodes.tobytes(), np.uint8), tris=c.tris, spheres=c.spheres, rays=rays, pts=pts,
             r_pb=fr[1], r_qb=fr[2], r_skip=fr[3], p_pb=fp[1], p_qb=fp[2], p_skip=fp[3])
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]), PTAMD_QUERY_QUAD="0")
    subprocess.run([sys.executable, "-c", CHILD, scene_file, out], check=True, env=env, timeout=600)
    g = np.load(out)
    for both in (0, 1):
        Hs = selected(ray_H(name, bool(both)), fr)
        w = f"PTAMD_QUERY_QUAD=0, rays, both = {both}"
        TL.assert_csr((g[f"off_{both}"], g[f"t_{both}"], g[f"prim_{both}"], g[f"det_{both}"]), Hs, w)
        assert np.array_equal(g[f"cnt_{both}"], np.diff(Hs[0])), w
        for k in KS:
            TH.assert_lists((g[f"t_{both}_{k}"], g[f"prim_{both}_{k}"], g[f"det_{both}_{k}"]), FR.cut(Hs, k), f"{w}, K = {k}")
    Hf = selected(ray_H(name, False), fr)
    assert np.array_equal(bits(g["ct"]), bits(FR.cut(Hf, 1)[0][:, 0])) and np.array_equal(g["cprim"], FR.cut(Hf, 1)[1][:, 0])
    assert_any((g["at"], g["aprim"]), Hf, "PTAMD_QUERY_QUAD=0, any hit")
    Hs = selected(PH, fp)
    TL.assert_csr((g["p_off"], g["p_d2"], g["p_prim"], g["p_det"]), Hs, "PTAMD_QUERY_QUAD=0, points")
    assert np.array_equal(g["p_cnt"], np.diff(Hs[0]))
    for k in KS:
        TK.assert_lists((g[f"p_d2_{k}"], g[f"p_prim_{k}"], g[f"p_det_{k}"]), FR.cut(Hs, k), f"PTAMD_QUERY_QUAD=0, points, K = {k}")
    one = FR.cut(Hs, 1)
    assert np.array_equal(bits(g["p_cd2"]), bits(one[0][:, 0])) and np.array_equal(g["p_cprim"], one[1][:, 0]) and np.array_equal(bits(g["p_cdet"]), bits(one[2][:, 0]))
    assert_any((g["p_ad2"], g["p_aprim"]), Hs, "PTAMD_QUERY_QUAD=0, any within")


@pytest.mark.gpu
def test_the_same_bits_before_and_after_the_rebuilds(_gpu):
    """comb32 (the binary walk by itself): the scene's tree from its first rebuild, then rebuild_tree(26, 1/16) and
    rebuild_tree_optimized — primitive numbers survive them, the filter is untouched, the results are the same bits."""
    name = "comb32"
    c = TH.case(name)
    sc = c.scene()
    fr = [f for f in ray_recipe(name).filters() if f[0] in ("all four fields", "prim_bits, bits 0x1")]
    H_of = {b: ray_H(name, b) for b in (False, True)}
    pts, PH = point_H(name)
    psc = T._scene(name)
    fp = [f for f in point_recipe(name).filters() if f[0] in ("all three fields", "skip alone")]
    for what, rebuild in (("as built", lambda s: None), ("after rebuild_tree", lambda s: s.rebuild_tree(depth_budget=26, large_fraction=1 / 16)),
                          ("after rebuild_tree_optimized", lambda s: s.rebuild_tree_optimized())):
        rebuild(sc)
        rebuild(psc)
        _check_ray_scene(sc, name, c.rays, H_of, fr, f"{name} {what}", ks=(1, 8, 32), product=False)
        _check_point_scene(psc, pts, PH, fp, f"{name} {what}", ks=(1, 8, 32), product=False)
    assert sc.tree_info()["rebuilds"] == 3


@pytest.mark.gpu
def test_update_count_scan_and_fill_on_one_stream_without_a_host_wait(_gpu):
    """Behind a vertex update on a non-default stream, with no host wait in between: the filtered count, pt_list_offsets and the filtered
    fill (the caller provides the room: the reference's total), then the K call — the selection of brute force on the MOVED positions."""
    import torch
    name = "standin24_spheres"
    c = TH.case(name)
    pos2, _, _, hs = TH._moved(name)
    flt = [f for f in ray_recipe(name).filters() if f[0] == "all four fields"][0]
    both = True
    Hs = selected(L.ray_lists(hs[both]), flt)
    total = int(Hs[0][-1])
    sc = ptamd.Scene(c.nodes, c.tris, c.spheres)
    sc.update_vertices(R.positions(c.tris).reshape(-1, 9))      # the first update allocates the scene's maps
    l, P = ptamd.lib(), C.c_void_p
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    n = len(c.rays)
    bytes0 = sc.device_bytes
    with torch.cuda.stream(st):
        d_pos, d_rays = torch.from_numpy(pos2).to(dev), torch.from_numpy(with_tmin(c.rays, flt[4])).to(dev)
        keep = []
        s = _c_filter(flt, 0, n, keep)
        cnt = torch.empty(n, dtype=torch.int32, device=dev)
        rec = torch.empty((total, 2), dtype=torch.int32, device=dev)
        det = torch.empty((total, 4), dtype=torch.float32, device=dev)
        krec = torch.empty((n, 8, 2), dtype=torch.int32, device=dev)
        torch.cuda.current_stream().synchronize()      # the uploads; nothing below waits
        sp = P(st.cuda_stream)
        sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
        assert l.pt_count_hits_f(sc._h, P(d_rays.data_ptr()), n, 1, C.byref(s), P(cnt.data_ptr()), sp) == 0, l.pt_last_error()
        off = ptamd.list_offsets(cnt, stream_ptr=st.cuda_stream)
        assert l.pt_trace_rays_list_f(sc._h, P(d_rays.data_ptr()), n, 1, P(off.data_ptr()), total, C.byref(s), P(rec.data_ptr()), P(det.data_ptr()), sp) == 0, l.pt_last_error()
        assert l.pt_trace_rays_k_f(sc._h, P(d_rays.data_ptr()), n, 8, 1, C.byref(s), P(krec.data_ptr()), None, sp) == 0, l.pt_last_error()
        assert sc.device_bytes == bytes0      # a filtered query allocates nothing
    st.synchronize()
    r = rec.cpu().numpy()
    TL.assert_csr((off.cpu().numpy(), np.ascontiguousarray(r[:, 0]).view(F), np.ascontiguousarray(r[:, 1]), det.cpu().numpy()), Hs, "behind an update on one stream")
    assert np.array_equal(cnt.cpu().numpy(), np.diff(Hs[0]))
    kr = krec.cpu().numpy()
    TH.assert_lists((np.ascontiguousarray(kr[:, :, 0]).view(F), np.ascontiguousarray(kr[:, :, 1])), FR.cut(Hs, 8)[:2], "the K call behind them")
    moved = FR.same(Hs[:3], selected(ray_H(name, both), flt)[:3])
    assert not moved, "the move changed nothing: the test would pass without stream order"


@pytest.mark.gpu
def test_filtered_queries_leave_renders_alone(_gpu):
    import torch
    name = "standin24_spheres"
    c = TH.case(name)
    pts, _ = point_H(name)
    cam, prm = ptamd.make_camera(100, 52), ptamd.default_params(passes=3, spp_per_pass=4)
    sc = ptamd.Scene(c.nodes, c.tris, c.spheres)
    fr = [f for f in ray_recipe(name).filters() if f[0] == "all four fields"][0]
    fp = [f for f in point_recipe(name).filters() if f[0] == "all three fields"][0]
    f, g = qfilter(fr), qfilter(fp)
    r = with_tmin(c.rays, fr[4])
    sc.trace_rays_k(r, 8, filter=f)      # before the first render, too
    sc.enable_counters(True)
    img = sc.render(cam, prm)
    state = (sc.last_iterations(), sc.device_bytes)
    counters = sc.counters()
    sc.trace_rays(r, surface=True, filter=f)
    sc.trace_rays(r, any_hit=True, filter=f)
    sc.trace_rays_k(r, 32, both_sides=True, detail=True, filter=f)
    sc.count_hits(r, both_sides=True, filter=f)
    sc.trace_rays_all(r, both_sides=True, detail=True, filter=f)
    sc.closest_points(pts, detail=True, filter=g)
    sc.closest_points(pts, any_within=True, filter=g)
    sc.nearest_k(pts, 9, detail=True, filter=g)
    sc.count_within(pts, filter=g)
    sc.within_radius(pts, detail=True, filter=g)
    torch.cuda.synchronize()
    assert (sc.last_iterations(), sc.device_bytes) == state
    assert np.array_equal(counters, sc.counters())
    img2 = sc.render(cam, prm)
    assert np.array_equal(bits(img), bits(img2)) and np.array_equal(bits(img), bits(ptamd.Scene(c.nodes, c.tris, c.spheres).render(cam, prm)))
    assert (sc.last_iterations(), sc.device_bytes) == state


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["standin24_spheres", "comb32"])
def test_odd_rays_end_and_leave_their_neighbours_alone(_gpu, name):
    """query_ref.odd_rays (zero directions, NaN and inf components, a NaN, infinite and negative tmax) spread over a batch of 200, under a
    filter with every field in use: the calls return, those rows keep every prim and count in range, every other row is the selection
    of brute force."""
    c, sc = TH.case(name), TL.ray_scene(name)
    flt = [f for f in ray_recipe(name).filters() if f[0] == "all four fields"][0]
    odd = Q.odd_rays()
    rays = with_tmin(c.rays, flt[4])[:200]
    at = 3 + 16 * np.arange(len(odd))      # in every wave
    rays[at] = odd
    keep = np.ones(len(rays), bool)
    keep[at] = False
    sub = (flt[0], flt[1], flt[2][:200], flt[3][:200], flt[4][:200])
    f = qfilter(sub)
    n_sph = c.n_prims - c.n_tris
    for both in (False, True):
        Hs = FR.rows(selected(ray_H(name, both), flt), 0, 200)
        for k in (1, 8, 32):
            got = sc.trace_rays_k(rays, k, both_sides=both, detail=True, filter=f)
            assert ((got[1] >= -1) & (got[1] < c.n_prims)).all()
            TH.assert_lists(tuple(x[keep] for x in got), tuple(x[keep] for x in FR.cut(Hs, k)), f"{name}, K = {k}, both = {both}, the rows beside the odd ones")
        cnt = sc.count_hits(rays, both_sides=both, filter=f)
        assert ((cnt >= 0) & (cnt <= c.n_tris + 2 * n_sph)).all() and np.array_equal(cnt[keep], np.diff(Hs[0])[keep])
        off, t, prim = sc.trace_rays_all(rays, both_sides=both, filter=f)
        assert ((prim >= -1) & (prim < c.n_prims)).all() and np.array_equal(np.diff(off)[keep], np.diff(Hs[0])[keep])
        t1, p1 = sc.trace_rays(rays, filter=f)
        a1, q1 = sc.trace_rays(rays, any_hit=True, filter=f)
        assert ((p1 >= -1) & (p1 < c.n_prims)).all() and ((q1 >= -1) & (q1 < c.n_prims)).all()
        if not both:
            assert np.array_equal(p1[keep], FR.cut(Hs, 1)[1][keep, 0]) and np.array_equal(bits(t1[keep]), bits(FR.cut(Hs, 1)[0][keep, 0]))
            assert np.array_equal(q1[keep] >= 0, np.diff(Hs[0])[keep] > 0)
