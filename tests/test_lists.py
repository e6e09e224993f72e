"""Variable-length query results: every hit along a ray and every primitive within a radius, in CSR form (pt_list_offsets,
pt_trace_rays_list, pt_within_radius_list and the _host variants, ptamd.list_offsets, Scene.trace_rays_all, Scene.within_radius;
DESIGN.md section 37).

On the CPU: the C-ABI surface and where its section sits, the argument checks with a fake scene and fake device addresses, the
wrappers' own checks, and the yardstick (tests/lists_ref.py: the brute forces of tests/ray_hits_ref.py and tests/nearest_k_ref.py cut at
the count) pinned to the K lists wherever a list has at most 32 members; the tall sheet stack's set and its chains.

On the GPU: bits only, no tolerance, and no query left out of a comparison.  Every offset, record and detail record of the four scenes of
tests/test_ray_hits.py and the 600-layer stack, both flag values, and of tests/nearest_k_ref.PointSets on the scenes of
tests/test_nearest.py; agreement with trace_rays / closest_points, trace_rays_k / nearest_k (k = 32) and the counts; the scan alone at
its sizes and past 2^31; segments that do not fit, between sentinels, inside a larger allocation; partial waves; the binary walk forced
by its knob; the same bits after the rebuilds; an update and the three calls on one stream without a host wait; renders left alone; odd
rays in a batch.

Conditions on the inputs, asserted on the reference before any comparison: the ray sets together hold lists of length 0, 1, 32 and 33,
one longer than 64 and one longer than the sort's LDS tile, and ties in t inside lists of every path (LDS list, per-thread sort,
workgroup sort); every member of the tall stack's sets is reached by both trees' chains (slack_ref: none of the rays of DESIGN.md
section 33); the point sets hold lists of the whole scene, ties at f = 0 and empty lists."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dynamic_ref as R
import lists_ref as L
import nearest_k_ref as K
import ptamd
import query_ref as Q
import ray_hits_ref as H
import slack_ref as S
import test_nearest as T
import test_nearest_k as TK
import test_ray_hits as TH
import test_slack as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pathtrace-on-cuda_amd")
F = np.float32
bits = H.bits


def ibits(a):
    return bits(a).view(np.int32)      # the records as the int32 words the buffers hold


RAY_SCENES = TH.SCENES + ("tall",)
POINT_SCENES = T.SCENES
POINT_M = 100      # PointSets' m: 5 m = 500 points per scene
SENT = 0x5A5A5A5A
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class Tall:
    """tests/test_ray_hits.py's Case for the 600-layer stack of lists_ref (no spheres)."""
    name = "tall"

    def __init__(self):
        self.prims, self.spheres, self.pos = L.tall_stack(), None, None
        self.nodes, self.tris, _ = ptamd.build_bvh(self.prims)
        self.nodes0, self.tris0 = self.nodes, self.tris
        self.rays = L.tall_rays(75, 300)
        self.tris9 = H.tri_v0e1e2(self.tris)
        self.leaf_of, self.leaf_boxes = H.leaf_of_tri(self.nodes)
        self.tri_boxes = self.leaf_boxes[self.leaf_of]
        self.n_tris = self.n_prims = len(self.tris)
        assert len(self.rays) <= 4096
        self._h = {}

    hits = TH.Case.hits
    scene = TH.Case.scene


def ray_case(name):
    return _cached(("case", name), Tall) if name == "tall" else TH.case(name)


def ray_want(name, both):
    return _cached(("rays", name, both), lambda: L.ray_lists(ray_case(name).hits(both)))


def point_case(name):
    """(points, (offsets, dist2, prim, detail), PointSets) of the scene: PointSets(m = 100).points(8), which holds radius inf, the
    median-8th radius, vertices and edge midpoints at inf and at 0, and near-surface points at 7e-4."""
    def make():
        ps = K.PointSets(T._positions(name), T._spheres(name), m=POINT_M)
        pts = ps.points(8)
        off, d2, prim = L.point_lists(pts, ps.positions, ps.spheres, ps.f)
        return pts, (off, d2, prim, L.point_detail(pts, off, prim, ps.positions, ps.spheres)), ps
    return _cached(("points", name), make)


def _ties_inside(t, off, lo, hi):
    """Queries with lo < length <= hi whose list holds two adjacent members with equal keys (compared as floats)."""
    n = 0
    for i in np.nonzero((np.diff(off) > lo) & (np.diff(off) <= hi))[0]:
        seg = t[off[i]:off[i + 1]]
        n += int((seg[1:] == seg[:-1]).any())
    return n


def ray_figures():
    def make():
        lengths, ties = set(), {"lds": 0, "thread": 0, "workgroup": 0}
        for name in RAY_SCENES:
            for both in (False, True):
                off, t, _, _ = ray_want(name, both)
                lengths |= set(np.diff(off).tolist())
                ties["lds"] += _ties_inside(t, off, 1, 8)
                ties["thread"] += _ties_inside(t, off, 8, 32)
                ties["workgroup"] += _ties_inside(t, off, 32, 1 << 30)
        return lengths, ties
    return _cached("ray_figures", make)


def assert_ray_conditions():
    lengths, ties = ray_figures()
    print(f"ray list lengths: {len(lengths)} distinct, longest {max(lengths)}; lists with a tie inside: {ties}")
    assert {0, 1, 32, 33} <= lengths
    assert max(lengths) > 64 and max(lengths) > L.SORT_TILE
    assert all(v > 0 for v in ties.values()), ties


def assert_point_conditions(name):
    pts, (off, d2, prim, _), ps = point_case(name)
    cnt = np.diff(off)
    n_prims = T._n_prims(name)
    whole = int((cnt == n_prims).sum())
    zero_ties = int(sum(((d2[off[i]:off[i + 1]] == 0).sum() >= 2) for i in np.nonzero(pts[:, 3] == 0)[0]))
    print(f"{name}: {len(pts)} points, {whole} lists of the whole scene ({n_prims}), {zero_ties} with a tie at f = 0, {int((cnt == 0).sum())} empty")
    assert whole >= 2 * POINT_M - 20 and (cnt == 0).sum() > 0 and zero_ties > 0
    if n_prims > L.SORT_TILE:
        assert cnt.max() > L.SORT_TILE


def assert_tall_chains(c, trees, what):
    TH.assert_chains_reach_every_member(c, trees, what)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
NEW = ("pt_list_offsets_scratch_bytes", "pt_list_offsets", "pt_trace_rays_list", "pt_within_radius_list", "pt_trace_rays_list_host",
       "pt_within_radius_list_host")


def test_new_symbols_are_exported_declared_and_bound():
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    assert callable(ptamd.list_offsets) and callable(ptamd.Scene.trace_rays_all) and callable(ptamd.Scene.within_radius)
    at = hdr.index("Variable-length query results")
    assert hdr.index("First K hits along a ray and hit counts") < at < hdr.index("Radiance along the caller's own rays")
    assert hdr.index(" pt_count_hits_host(") < at < hdr.index(" pt_list_offsets_scratch_bytes(")      # directly after that section
    assert "variable-length lists" not in hdr
    l.pt_list_offsets_scratch_bytes.restype = C.c_int64
    l.pt_list_offsets_scratch_bytes.argtypes = [C.c_int64]
    assert l.pt_list_offsets_scratch_bytes(-1) == -1 and l.pt_list_offsets_scratch_bytes(0) == 0
    assert all(0 < l.pt_list_offsets_scratch_bytes(n) <= 4096 for n in (1, 65, 1 << 20, 1 << 40))


def test_yardstick_boundaries_are_the_kernels_constants():
    """lists_ref's SCAN_CHUNK, SCAN_GRID and SORT_TILE are the kernels' kScanChunk, kScanGrid and kSortTile (csrc/pt_lists.hip, pt_lists.h):
    the threshold cases sit on the real boundaries."""
    import re
    src = open(os.path.join(PKG, "csrc", "pt_lists.hip")).read() + open(os.path.join(PKG, "csrc", "pt_lists.h")).read()

    def const(name):
        return int(re.search(rf"constexpr \w+ {name} = (\d+);", src).group(1))
    assert re.search(r"kScanChunk = kScanThreads \* kScanPer;", src) and re.search(r"kSortTile = 2 \* kSegThreads;", src)
    assert L.SCAN_CHUNK == const("kScanThreads") * const("kScanPer")
    assert L.SCAN_GRID == const("kScanGrid")
    assert L.SORT_TILE == 2 * const("kSegThreads")


def test_bad_arguments_are_rejected_before_any_device_call():
    """A fake scene and fake device addresses: never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    base = 1 << 40
    scene, q, offs, out, det, cnt, scr = (C.c_void_p(base + (i << 20)) for i in range(7))
    at = lambda p, k: C.c_void_p(p.value + k)      # noqa: E731
    scan = [
        ("NULL count", (None, 64, offs, scr)),
        ("NULL offsets", (cnt, 64, None, scr)),
        ("NULL scratch", (cnt, 64, offs, None)),
        ("n < 0", (cnt, -1, offs, scr)),
        ("count + 2", (at(cnt, 2), 64, offs, scr)),
        ("offsets + 4", (cnt, 64, at(offs, 4), scr)),
        ("scratch + 4", (cnt, 64, offs, at(scr, 4))),
        ("n = 0 does not excuse a NULL count", (None, 0, offs, None)),
        ("n = 0 does not excuse NULL offsets", (cnt, 0, None, None)),
    ]
    for what, a in scan:
        assert l.pt_list_offsets(*a, None) == -1, what
        assert b"pt_list_offsets:" in l.pt_last_error(), (what, l.pt_last_error())
    rays = [
        ("NULL scene", (None, q, 64, 0, offs, 100, out, None)),
        ("NULL rays", (scene, None, 64, 0, offs, 100, out, None)),
        ("NULL offsets", (scene, q, 64, 0, None, 100, out, None)),
        ("NULL hits", (scene, q, 64, 0, offs, 100, None, det)),
        ("n < 0", (scene, q, -1, 0, offs, 100, out, None)),
        ("cap < 0", (scene, q, 64, 1, offs, -1, out, None)),
        ("flags 2", (scene, q, 64, 2, offs, 100, out, None)),
        ("flags -1", (scene, q, 64, -1, offs, 100, out, None)),
        ("flags 1 << 8", (scene, q, 64, 256, offs, 100, out, None)),
        ("rays + 8", (scene, at(q, 8), 64, 0, offs, 100, out, None)),
        ("offsets + 4", (scene, q, 64, 0, at(offs, 4), 100, out, None)),
        ("hits + 4", (scene, q, 64, 0, offs, 100, at(out, 4), None)),
        ("detail + 2", (scene, q, 64, 0, offs, 100, out, at(det, 2))),
        ("n = 0 does not excuse a NULL", (scene, q, 0, 0, None, 100, out, None)),
        ("n = 0 does not excuse unknown flags", (scene, q, 0, 4, offs, 100, out, None)),
        ("n = 0 does not excuse cap < 0", (scene, q, 0, 0, offs, -5, out, None)),
    ]
    for what, a in rays:
        assert l.pt_trace_rays_list(*a, None) == -1, what
        assert b"pt_trace_rays_list:" in l.pt_last_error(), (what, l.pt_last_error())
    points = [
        ("NULL scene", (None, q, 64, offs, 100, out, None)),
        ("NULL points", (scene, None, 64, offs, 100, out, None)),
        ("NULL offsets", (scene, q, 64, None, 100, out, None)),
        ("NULL out", (scene, q, 64, offs, 100, None, det)),
        ("n < 0", (scene, q, -1, offs, 100, out, None)),
        ("cap < 0", (scene, q, 64, offs, -1, out, None)),
        ("points + 8", (scene, at(q, 8), 64, offs, 100, out, None)),
        ("offsets + 4", (scene, q, 64, at(offs, 4), 100, out, None)),
        ("out + 4", (scene, q, 64, offs, 100, at(out, 4), None)),
        ("detail + 2", (scene, q, 64, offs, 100, out, at(det, 2))),
        ("n = 0 does not excuse a NULL", (scene, None, 0, offs, 100, out, None)),
    ]
    for what, a in points:
        assert l.pt_within_radius_list(*a, None) == -1, what
        assert b"pt_within_radius_list:" in l.pt_last_error(), (what, l.pt_last_error())
    P = ptamd._ptr
    h_rays, h_pts, h_off = np.zeros((64, 8), F), np.zeros((64, 4), F), np.zeros(65, np.int64)
    h_hits, h_near = np.zeros(100, ptamd.HIT_DTYPE), np.zeros(100, ptamd.NEAREST_DTYPE)
    host_rays = [
        ("NULL scene", (None, P(h_rays), 64, 0, P(h_off), 100, P(h_hits), None)),
        ("NULL rays", (scene, None, 64, 0, P(h_off), 100, P(h_hits), None)),
        ("NULL offsets", (scene, P(h_rays), 64, 0, None, 100, None, None)),
        ("n < 0", (scene, P(h_rays), -3, 0, P(h_off), 100, P(h_hits), None)),
        ("cap < 0", (scene, P(h_rays), 64, 0, P(h_off), -1, None, None)),
        ("flags 2", (scene, P(h_rays), 64, 2, P(h_off), 100, P(h_hits), None)),
    ]
    for what, a in host_rays:
        assert l.pt_trace_rays_list_host(*a) == -1, what
        assert b"pt_trace_rays_list_host:" in l.pt_last_error(), (what, l.pt_last_error())
    host_points = [
        ("NULL scene", (None, P(h_pts), 64, P(h_off), 100, P(h_near), None)),
        ("NULL points", (scene, None, 64, P(h_off), 100, P(h_near), None)),
        ("NULL offsets", (scene, P(h_pts), 64, None, 100, None, None)),
        ("n < 0", (scene, P(h_pts), -3, P(h_off), 100, P(h_near), None)),
        ("cap < 0", (scene, P(h_pts), 64, P(h_off), -1, None, None)),
    ]
    for what, a in host_points:
        assert l.pt_within_radius_list_host(*a) == -1, what
        assert b"pt_within_radius_list_host:" in l.pt_last_error(), (what, l.pt_last_error())
    # nothing to do: PT_OK, still without touching the scene or the device; the host variants write their one offset
    assert l.pt_trace_rays_list(scene, q, 0, 1, offs, 0, out, det, None) == 0
    assert l.pt_within_radius_list(scene, q, 0, offs, 7, out, None, None) == 0
    h_off[:] = 99
    assert l.pt_trace_rays_list_host(scene, P(h_rays), 0, 0, P(h_off), 0, None, None) == 0 and h_off[0] == 0 and (h_off[1:] == 99).all()
    h_off[:] = 99
    assert l.pt_within_radius_list_host(scene, P(h_pts), 0, P(h_off), 0, P(h_near), None) == 0 and h_off[0] == 0 and (h_off[1:] == 99).all()


def test_wrapper_checks_shape_dtype_and_device_on_the_host():
    import torch
    fake = TH._FakeScene()
    tra, wr = ptamd.Scene.trace_rays_all, ptamd.Scene.within_radius
    for rays in (np.zeros((4, 7), F), np.zeros(32, F), np.zeros((2, 4, 8), F)):
        with pytest.raises(ptamd.PtError):
            tra(fake, rays)
    for pts in (np.zeros((4, 3), F), np.zeros(16, F)):
        with pytest.raises(ptamd.PtError):
            wr(fake, pts)
    for rays in (torch.zeros((5, 8)), torch.zeros((5, 8), dtype=torch.float64), torch.zeros((5, 7)), torch.zeros((8, 5)).t(), [[0.0] * 8]):
        with pytest.raises(ptamd.PtError):      # a CPU tensor, a wrong dtype, a wrong shape, not contiguous, not an array
            tra(fake, rays, both_sides=True)
    for pts in (torch.zeros((5, 4)), torch.zeros((5, 4), dtype=torch.float64), torch.zeros((5, 3)), [[0.0] * 4]):
        with pytest.raises(ptamd.PtError):
            wr(fake, pts)
    for count in (np.zeros(4, np.int64), np.zeros(4, F), np.zeros((2, 2), np.int32), torch.zeros(4, dtype=torch.int32),
                  torch.zeros(4, dtype=torch.int64), torch.zeros((2, 2), dtype=torch.int32), [1, 2]):
        with pytest.raises(ptamd.PtError):      # wrong dtype or shape, a CPU tensor, not an array
            ptamd.list_offsets(count)
    off, t, prim, det = tra(fake, np.zeros((0, 8), F), both_sides=True, detail=True)      # n = 0: PT_OK without a device
    assert off.tolist() == [0] and off.dtype == np.int64 and t.shape == prim.shape == (0,) and det.shape == (0, 4)
    assert t.dtype == F and prim.dtype == np.int32
    off, d2, prim, det = wr(fake, np.zeros((0, 4), F), detail=True)
    assert off.tolist() == [0] and d2.shape == prim.shape == (0,) and det.shape == (0, 8) and d2.dtype == F


@pytest.mark.parametrize("name", RAY_SCENES)
def test_yardstick_ray_lists_are_the_k_lists_where_they_fit(name):
    """The concatenation of the brute force's rows cut at the count agrees with ray_hits_ref.lists(h, 32) wherever count <= 32."""
    for both in (False, True):
        h = ray_case(name).hits(both)
        off, t, prim, det = ray_want(name, both)
        assert np.array_equal(off, L.csr(h.count)) and len(t) == off[-1]
        kt, kp, kd = H.lists(h, 32)
        fit = np.nonzero(h.count <= 32)[0]
        assert len(fit) > 0
        for i in fit:
            c = h.count[i]
            seg = slice(off[i], off[i + 1])
            assert np.array_equal(prim[seg], kp[i, :c]) and np.array_equal(bits(t[seg]), bits(kt[i, :c])), (name, both, i)
            assert np.array_equal(bits(det[seg]), bits(kd[i, :c])) and (kp[i, c:] == -1).all(), (name, both, i)


@pytest.mark.parametrize("name", POINT_SCENES)
def test_yardstick_point_lists_are_the_k_lists_where_they_fit(name):
    """The rows of brute_k(k = number of primitives) cut at the count agree with brute_k(k = 32) wherever count <= 32."""
    pts, (off, d2, prim, _), ps = point_case(name)
    kd2, kp = K.brute_k(pts, ps.positions, ps.spheres, 32, ps.f)
    cnt = np.diff(off)
    assert np.array_equal(cnt, K.count(pts, ps.positions, ps.spheres, ps.f))
    fit = np.nonzero(cnt <= 32)[0]
    assert len(fit) > 0
    for i in fit:
        c = cnt[i]
        seg = slice(off[i], off[i + 1])
        assert np.array_equal(prim[seg], kp[i, :c]) and np.array_equal(bits(d2[seg]), bits(kd2[i, :c])) and (kp[i, c:] == -1).all(), (name, i)


def test_ray_and_point_sets_hold_what_they_should():
    assert_ray_conditions()
    for name in POINT_SCENES:
        assert_point_conditions(name)


def test_tall_stack_chains_reach_every_member():
    c = ray_case("tall")
    assert_tall_chains(c, SL.host_trees(c.prims, "lists_tall"), "tall stack, host trees")


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


def ray_scene(name):
    return _cached(("scene", name), lambda: ray_case(name).scene())


def point_scene(name):
    return _cached(("pscene", name), lambda: T._scene(name))


def assert_ray_inputs(name, sc):
    if name != "tall":
        TH.assert_inputs(name, sc)
        return
    c = ray_case(name)
    tri = sc.dbg_array("tri").reshape(-1, 12)
    lb = sc.dbg_array("leafbox").reshape(-1, 8)
    prim, leaf = tri[:, 3].view(np.int32), tri[:, 7].view(np.int32)
    assert np.array_equal(np.sort(prim), np.arange(c.n_tris))
    assert np.array_equal(bits(lb[leaf, 0:6]), bits(c.tri_boxes[prim])), "tall: the reference leaf boxes differ from the uploaded ones"
    rec = np.concatenate([tri[:, 0:3], tri[:, 4:7], tri[:, 8:11]], 1)
    assert np.array_equal(bits(rec), bits(c.tris9[prim])), "tall: V0 E1 E2 differ from the uploaded records"
    assert_tall_chains(c, S.Trees(sc.dbg_array("nodes"), sc.dbg_array("quad"), sc.dbg_array("tri"), sc.dbg_array("leafbox")), "tall, device trees")


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def assert_csr(got, want, what):
    """got, want: (offsets, key, prim[, detail]); every array bit for bit."""
    off, key, prim = (_np(x) for x in got[:3])
    assert off.dtype == np.int64 and np.array_equal(off, want[0]), f"{what}: offsets differ at {np.nonzero(off != want[0])[0][:5] if off.shape == want[0].shape else off.shape}"
    assert key.dtype == F and prim.dtype == np.int32 and prim.shape == want[2].shape, what
    bad = prim != want[2]
    assert not bad.any(), f"{what}: {bad.sum()} prims differ, first at record {np.nonzero(bad)[0][:5]}"
    bad = bits(key) != bits(want[1])
    assert not bad.any(), f"{what}: {bad.sum()} keys differ, first at record {np.nonzero(bad)[0][:5]}"
    if len(got) > 3 and len(want) > 3:
        det = _np(got[3])
        assert det.shape == want[3].shape, what
        bad = (bits(det) != bits(want[3])).any(1)
        assert not bad.any(), f"{what}: {bad.sum()} detail records differ, first at record {np.nonzero(bad)[0][:5]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", RAY_SCENES)
def test_ray_lists_are_brute_forces(_gpu, name):
    import torch
    assert_ray_conditions()
    c, sc = ray_case(name), ray_scene(name)
    assert_ray_inputs(name, sc)
    d_rays = torch.from_numpy(c.rays).cuda()
    for both in (False, True):
        want = ray_want(name, both)
        what = f"{name}, both = {both}"
        assert_csr(sc.trace_rays_all(d_rays, both_sides=both, detail=True), want, what + ", device path")
        assert_csr(sc.trace_rays_all(c.rays, both_sides=both), want[:3], what + ", host path")
        assert_csr(sc.trace_rays_all(c.rays, both_sides=both, detail=True), want, what + ", host path with detail")


@pytest.mark.gpu
@pytest.mark.parametrize("name", POINT_SCENES)
def test_point_lists_are_brute_forces(_gpu, name):
    import torch
    assert_point_conditions(name)
    pts, want, _ = point_case(name)
    sc = point_scene(name)
    TK._assert_walk(sc, name)
    assert_csr(sc.within_radius(torch.from_numpy(pts).cuda(), detail=True), want, f"{name}, device path")
    assert_csr(sc.within_radius(pts), want[:3], f"{name}, host path")
    assert_csr(sc.within_radius(pts, detail=True), want, f"{name}, host path with detail")


def _prefix_k(off, key, prim, k):
    """(key, prim) padded to (n, k) from the lists of at most k members, and the mask of those queries."""
    cnt = np.diff(off)
    fit = cnt <= k
    j = np.arange(k)[None, :]
    live = (j < cnt[:, None]) & fit[:, None]
    idx = np.where(live, off[:-1, None] + j, 0)
    return np.where(live, key[idx], F(0)), np.where(live, prim[idx], -1), fit


@pytest.mark.gpu
@pytest.mark.parametrize("name", RAY_SCENES)
def test_ray_lists_agree_with_the_calls_that_exist(_gpu, name):
    """Slot 0 against trace_rays, every list of at most 32 members against trace_rays_k(k = 32), the segment lengths against count_hits."""
    c, sc = ray_case(name), ray_scene(name)
    for both in (False, True):
        off, t, prim, det = sc.trace_rays_all(c.rays, both_sides=both, detail=True)
        cnt = sc.count_hits(c.rays, both_sides=both)
        assert np.array_equal(np.diff(off), cnt), name
        kt, kp, kd = sc.trace_rays_k(c.rays, 32, both_sides=both, detail=True)
        pt, pp, fit = _prefix_k(off, t, prim, 32)
        assert fit.sum() > 0
        assert np.array_equal(pp[fit], kp[fit]) and np.array_equal(bits(pt[fit]), bits(kt[fit])), f"{name}, both = {both}: not trace_rays_k's"
        for i in np.nonzero(fit)[0]:
            assert np.array_equal(bits(det[off[i]:off[i + 1]]), bits(kd[i, :cnt[i]])), (name, both, i)
        if not both:
            t0, p0 = sc.trace_rays(c.rays)
            hit = cnt > 0
            assert np.array_equal(p0[hit], prim[off[:-1][hit]]) and np.array_equal(bits(t0[hit]), bits(t[off[:-1][hit]])), name
            assert (p0[~hit] == -1).all(), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", POINT_SCENES)
def test_point_lists_agree_with_the_calls_that_exist(_gpu, name):
    """Slot 0 against closest_points, every list of at most 32 members against nearest_k(k = 32), the lengths against count_within."""
    pts, _, _ = point_case(name)
    sc = point_scene(name)
    off, d2, prim, det = sc.within_radius(pts, detail=True)
    cnt = sc.count_within(pts)
    assert np.array_equal(np.diff(off), cnt), name
    kd2, kp, kdet = sc.nearest_k(pts, 32, detail=True)
    pd, pp, fit = _prefix_k(off, d2, prim, 32)
    assert fit.sum() > 0
    assert np.array_equal(pp[fit], kp[fit]) and np.array_equal(bits(pd[fit]), bits(kd2[fit])), f"{name}: not nearest_k's"
    for i in np.nonzero(fit)[0]:
        assert np.array_equal(bits(det[off[i]:off[i + 1]]), bits(kdet[i, :cnt[i]])), (name, i)
    c2, cp = sc.closest_points(pts)
    hit = cnt > 0
    assert np.array_equal(cp[hit], prim[off[:-1][hit]]) and np.array_equal(bits(c2[hit]), bits(d2[off[:-1][hit]])), name
    assert (cp[~hit] == -1).all(), name


def _scan(count, pad=16):
    """pt_list_offsets on the device, the offsets inside a sentinel-filled buffer: (the n + 1 offsets, whether the tail kept its sentinels)."""
    import torch
    l = ptamd.lib()
    n = len(count)
    d_cnt = torch.from_numpy(np.ascontiguousarray(count, np.int32)).cuda() if n else torch.zeros(1, dtype=torch.int32, device="cuda")
    buf = torch.full((n + 1 + pad,), SENT, dtype=torch.int64, device="cuda")
    scr = torch.empty(max(l.pt_list_offsets_scratch_bytes(n), 8), dtype=torch.uint8, device="cuda")
    assert l.pt_list_offsets(C.c_void_p(d_cnt.data_ptr()), n, C.c_void_p(buf.data_ptr()), C.c_void_p(scr.data_ptr()), None) == 0, l.pt_last_error()
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    return b[:n + 1], bool((b[n + 1:] == SENT).all())


@pytest.mark.gpu
def test_offsets_alone(_gpu):
    rs = np.random.RandomState(91)
    chunk, grid = L.SCAN_CHUNK, L.SCAN_GRID
    sizes = (0, 1, 63, 64, 65, chunk - 1, chunk, chunk + 1, grid * chunk - 1, grid * chunk, grid * chunk + 1, 3 * grid * chunk + 777)
    for n in sizes:
        count = rs.randint(-6, 40, n).astype(np.int32)
        count[rs.rand(n) < 0.2] = 0      # zeros and negatives
        got, tail = _scan(count)
        assert tail, f"n = {n}: written past d_offsets[n]"
        assert np.array_equal(got, L.csr(count)), f"n = {n}: offsets differ at {np.nonzero(got != L.csr(count))[0][:5]}"
        again, _ = _scan(count)
        assert np.array_equal(again, got), f"n = {n}: not the same bits twice"
    got, tail = _scan(np.full(3, 1 << 30, np.int32))
    assert tail and got.tolist() == [0, 1 << 30, 1 << 31, 3 << 30]
    got, tail = _scan(np.array([2 ** 31 - 1] * 5 + [-(2 ** 31)] * 2 + [7], np.int32))
    assert tail and got.tolist() == [0] + [(2 ** 31 - 1) * k for k in range(1, 6)] + [(2 ** 31 - 1) * 5] * 2 + [(2 ** 31 - 1) * 5 + 7]
    import torch
    off = ptamd.list_offsets(torch.from_numpy(np.array([3, -1, 0, 5], np.int32)).cuda())
    assert off.dtype == torch.int64 and off.cpu().tolist() == [0, 3, 3, 3, 8]
    assert ptamd.list_offsets(np.array([], np.int32)).tolist() == [0]


def _fill(kind, sc, q, off, cap, flags=0, pad=4096, detail=True):
    """One fill with caller-made offsets: the records (and detail records) inside sentinel-filled allocations, d_hits pointing `pad`
    records into them, so that any offset within pad of [0, cap] lands inside the allocation.  Returns (records (cap + 2 pad, 2) int32,
    detail (cap + 2 pad, D) int32 or None)."""
    import torch
    l = ptamd.lib()
    D = 4 if kind == "rays" else 8
    d_q = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    d_off = torch.from_numpy(np.ascontiguousarray(off, np.int64)).cuda()
    rec = torch.full(((cap + 2 * pad) * 2,), SENT, dtype=torch.int32, device="cuda")
    det = torch.full(((cap + 2 * pad) * D,), SENT, dtype=torch.int32, device="cuda") if detail else None
    p_rec = C.c_void_p(rec.data_ptr() + 8 * pad)
    p_det = C.c_void_p(det.data_ptr() + 4 * D * pad) if detail else None
    n = len(q)
    if kind == "rays":
        rc = l.pt_trace_rays_list(sc._h, C.c_void_p(d_q.data_ptr()), n, flags, C.c_void_p(d_off.data_ptr()), cap, p_rec, p_det, None)
    else:
        rc = l.pt_within_radius_list(sc._h, C.c_void_p(d_q.data_ptr()), n, C.c_void_p(d_off.data_ptr()), cap, p_rec, p_det, None)
    assert rc == 0, l.pt_last_error()
    torch.cuda.synchronize()
    return rec.cpu().numpy().reshape(-1, 2), (det.cpu().numpy().reshape(-1, D) if detail else None)


def _combo(keybits, prim):
    """One int64 per record: the key's bits and the prim, so that records compare as numbers."""
    return (np.asarray(keybits, np.int64) << 32) | (np.asarray(prim, np.int64) & 0xFFFFFFFF)


def _assert_undersized(rec, det, want, b, e, pad, float_key, what):
    """Every slot of every segment a member of that query's list, none twice, sorted; its detail record the member's."""
    off, key, prim, wdet = want
    wall = _combo(bits(key), prim)
    wdet = ibits(wdet)
    for i in range(len(b)):
        seg = rec[pad + b[i]:pad + e[i]]
        if not len(seg):
            continue
        w = wall[off[i]:off[i + 1]]
        g = _combo(seg[:, 0], seg[:, 1])
        order = np.argsort(w)
        at = np.minimum(np.searchsorted(w[order], g), len(w) - 1)
        pos = order[at]
        assert (w[pos] == g).all() and len(np.unique(g)) == len(g), f"{what}, query {i}: not distinct members of its list"
        k = seg[:, 0].view(F) if float_key else seg[:, 0]
        ok = (k[:-1] < k[1:]) | ((k[:-1] == k[1:]) & (seg[:-1, 1] > seg[1:, 1]))
        assert ok.all(), f"{what}, query {i}: not sorted"
        assert np.array_equal(det[pad + b[i]:pad + e[i]], wdet[off[i]:off[i + 1]][pos]), f"{what}, query {i}: detail records"


def _assert_only_segments(rec, det, b, e, pad, what):
    written = np.zeros(len(rec), bool)
    for lo, hi in zip(b, e):
        written[pad + lo:pad + hi] = True
    for name, buf in (("records", rec), ("detail", det)):
        assert (buf[~written] == SENT).all(), f"{what}: {name} written outside the segments at {np.nonzero((buf != SENT).any(1) & ~written)[0][:5] - pad}"


def _segment_cases(kind, sc, q, want, flags, float_key, n_prims, what):
    off0 = want[0]
    cnt = np.diff(off0)
    n, pad = len(q), 4096
    # counts + 3: the padding is miss records, their detail zeros
    off = L.csr(cnt + 3)
    rec, det = _fill(kind, sc, q, off, int(off[-1]), flags, pad)
    b, e = L.segments(off, off[-1])
    _assert_only_segments(rec, det, b, e, pad, what + ", counts + 3")
    for i in range(n):
        seg, d = rec[pad + b[i]:pad + e[i]], det[pad + b[i]:pad + e[i]]
        c = cnt[i]
        s = slice(off0[i], off0[i + 1])
        assert np.array_equal(seg[:c, 1], want[2][s]) and np.array_equal(seg[:c, 0], ibits(want[1][s])), f"{what}, counts + 3, query {i}"
        assert (seg[c:] == [0, -1]).all() and (d[c:] == 0).all() and np.array_equal(d[:c], ibits(want[3][s])), f"{what}, counts + 3, query {i}: padding"
    # undersized: max(count - 1, 0) and count // 2, the two halves of the batch in two calls with a gap of sentinels between them
    for shrink, label in ((np.maximum(cnt - 1, 0), "count - 1"), (cnt // 2, "count // 2")):
        h = n // 2
        o1, o2 = L.csr(shrink[:h]), L.csr(shrink[h:])
        gap = 37
        o2 = o2 + o1[-1] + gap
        cap = int(o2[-1]) + 5
        import torch
        l = ptamd.lib()
        D = 4 if kind == "rays" else 8
        recs = torch.full(((cap + 2 * pad) * 2,), SENT, dtype=torch.int32, device="cuda")
        dets = torch.full(((cap + 2 * pad) * D,), SENT, dtype=torch.int32, device="cuda")
        for lo, hi, o in ((0, h, o1), (h, n, o2)):
            d_q = torch.from_numpy(np.ascontiguousarray(q[lo:hi])).cuda()
            d_off = torch.from_numpy(o).cuda()
            args = (C.c_void_p(d_q.data_ptr()), hi - lo)
            outs = (C.c_void_p(recs.data_ptr() + 8 * pad), C.c_void_p(dets.data_ptr() + 4 * D * pad), None)
            if kind == "rays":
                rc = l.pt_trace_rays_list(sc._h, *args, flags, C.c_void_p(d_off.data_ptr()), cap, *outs)
            else:
                rc = l.pt_within_radius_list(sc._h, *args, C.c_void_p(d_off.data_ptr()), cap, *outs)
            assert rc == 0, l.pt_last_error()
            torch.cuda.synchronize()
        rec, det = recs.cpu().numpy().reshape(-1, 2), dets.cpu().numpy().reshape(-1, D)
        b = np.concatenate([o1[:-1], o2[:-1]])
        e = np.concatenate([o1[1:], o2[1:]])
        _assert_only_segments(rec, det, b, e, pad, f"{what}, {label}")
        assert (rec[pad + o1[-1]:pad + o1[-1] + gap] == SENT).all()
        assert ((shrink < cnt) & (shrink > 32)).any() or n_prims <= 64, f"{what}, {label}: no undersized long segment"
        _assert_undersized(rec, det, want, b, e, pad, float_key, f"{what}, {label}")
    # bad offsets: negative, decreasing, beyond cap; nothing outside the clamped segments changes, every prim in range
    rs = np.random.RandomState(5)
    cap = 3000
    off = rs.randint(-1000, cap + 1000, n + 1).astype(np.int64)
    off[::7] = np.sort(off[::7])
    rec, det = _fill(kind, sc, q, off, cap, flags, pad)
    b, e = L.segments(off, cap)
    assert (b < 0).sum() == 0 and (e <= cap).all() and ((off[1:] < off[:-1]).sum() > 10) and (off < 0).any() and (off > cap).any()
    _assert_only_segments(rec, det, b, e, pad, what + ", bad offsets")
    inside = rec[pad:pad + cap]
    touched = (inside != SENT).any(1)
    assert ((inside[touched, 1] >= -1) & (inside[touched, 1] < n_prims)).all(), what + ", bad offsets: a prim out of range"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tall", "sheet"])
def test_ray_segments_that_do_not_fit(_gpu, name):
    c, sc = ray_case(name), ray_scene(name)
    both = name == "tall"
    _segment_cases("rays", sc, c.rays, ray_want(name, both), int(both), True, c.n_prims, f"{name}, both = {both}")


@pytest.mark.gpu
def test_point_segments_that_do_not_fit(_gpu):
    name = "standin24_spheres"
    pts, want, _ = point_case(name)
    _segment_cases("points", point_scene(name), pts, want, 0, False, T._n_prims(name), name)


@pytest.mark.gpu
def test_partial_waves_between_sentinels(_gpu):
    """n = 1, 63, 64, 65 and 130 (tests/test_nearest_k.py's slices), offsets from the slice's own counts: the records are the
    reference's and nothing around them is written."""
    cases = [("rays", ray_scene("tall"), ray_case("tall").rays, ray_want("tall", True), 1, True),
             ("rays", ray_scene("sheet"), ray_case("sheet").rays, ray_want("sheet", False), 0, False)]
    pts, pwant, _ = point_case("attribute")
    cases.append(("points", point_scene("attribute"), pts, pwant, 0, False))
    pad = 256
    for kind, sc, q, want, flags, _ in cases:
        for lo, m in TK.SLICES:
            off = want[0][lo:lo + m + 1] - want[0][lo]
            rec, det = _fill(kind, sc, q[lo:lo + m], off, int(off[-1]), flags, pad)
            what = f"{kind}, n = {m} from {lo}"
            s = slice(want[0][lo], want[0][lo + m])
            assert (rec[:pad] == SENT).all() and (rec[-pad:] == SENT).all() and (det[:pad] == SENT).all() and (det[-pad:] == SENT).all(), what
            assert np.array_equal(rec[pad:-pad, 1], want[2][s]) and np.array_equal(rec[pad:-pad, 0], ibits(want[1][s])), what
            assert np.array_equal(det[pad:-pad], ibits(want[3][s])), what


CHILD = r"""
import sys
import numpy as np
import ptamd
out = sys.argv[2]
res = {}
with np.load(sys.argv[1], allow_pickle=False) as g:
    sph = g["spheres"] if "spheres" in g.files else None
    sc = ptamd.Scene(g["nodes"].view(ptamd.NODE_DTYPE).reshape(-1), g["tris"], sph)
    assert not (3 * sc.tree_info()["quad_depth"] + 2 > 40)      # the 4-wide walk would fit: the knob alone forces the binary one
    for both in (0, 1):
        for key, x in zip("otpd", sc.trace_rays_all(g["rays"], both_sides=bool(both), detail=True)):
            res[f"r{key}_{both}"] = x
    for key, x in zip("odpe", sc.within_radius(g["points"], detail=True)):
        res[f"p{key}"] = x
np.savez(out, **res)
"""


@pytest.mark.gpu
def test_binary_walk_forced_by_its_knob_gives_the_same_bits(_gpu, tmp_path):
    """PTAMD_QUERY_QUAD=0 in a fresh process (the knob is read when a scene is created), as tests/test_query.py sets it."""
    name = "standin24_spheres"
    c = ray_case(name)
    pts, pwant, _ = point_case(name)
    scene_file, out = str(tmp_path / "scene.npz"), str(tmp_path / "child.npz")
    np.savez(scene_file, nodes=np.frombuffer(c.nodes.tobytes(), np.uint8), tris=c.tris, spheres=c.spheres, rays=c.rays, points=pts)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]), PTAMD_QUERY_QUAD="0")
    subprocess.run([sys.executable, "-c", CHILD, scene_file, out], check=True, env=env, timeout=600)
    g = np.load(out)
    for both in (0, 1):
        assert_csr(tuple(g[f"r{k}_{both}"] for k in "otpd"), ray_want(name, bool(both)), f"PTAMD_QUERY_QUAD=0, rays, both = {both}")
    assert_csr(tuple(g[f"p{k}"] for k in "odpe"), pwant, "PTAMD_QUERY_QUAD=0, points")


@pytest.mark.gpu
def test_the_result_does_not_depend_on_the_tree(_gpu):
    """A fresh upload, then rebuild_tree, rebuild_tree with a depth budget (rebuild_tree_ex) and rebuild_tree_optimized: the same bits."""
    name = "standin24_spheres"
    c = ray_case(name)
    pts, pwant, _ = point_case(name)
    sc = ptamd.Scene(c.nodes, c.tris, c.spheres)

    def check(what):
        for both in (False, True):
            assert_csr(sc.trace_rays_all(c.rays, both_sides=both, detail=True), ray_want(name, both), f"{what}, rays, both = {both}")
        assert_csr(sc.within_radius(pts, detail=True), pwant, f"{what}, points")
    check("upload")
    sc.rebuild_tree()
    check("after rebuild_tree")
    sc.rebuild_tree(depth_budget=26, large_fraction=1 / 16)
    check("after rebuild_tree(26, 1/16)")
    sc.rebuild_tree_optimized()
    check("after rebuild_tree_optimized")
    assert sc.tree_info()["rebuilds"] == 3


@pytest.mark.gpu
def test_update_and_the_three_calls_on_one_stream_without_a_host_wait(_gpu):
    """Behind a vertex update on a non-default stream: count, offsets and fill on that stream, records allocated for the reference's total
    beforehand, no host wait in between; the lists are brute force's at the moved pose."""
    import torch
    name = "standin24_spheres"
    c = ray_case(name)
    pos2, _, _, hs = TH._moved(name)
    sc = ptamd.Scene(c.nodes, c.tris, c.spheres)
    sc.update_vertices(R.positions(c.tris).reshape(-1, 9))      # the first update allocates the scene's maps: not what is measured below
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    bytes0 = sc.device_bytes
    l = ptamd.lib()
    wants = {both: L.ray_lists(hs[both]) for both in (False, True)}
    with torch.cuda.stream(st):
        d_pos = torch.from_numpy(pos2).to(dev)
        d_rays = torch.from_numpy(c.rays).to(dev)
        sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
        got = {}
        for both in (False, True):
            cnt = sc.count_hits(d_rays, both_sides=both, stream_ptr=st.cuda_stream)
            off = ptamd.list_offsets(cnt, stream_ptr=st.cuda_stream)
            total = int(wants[both][0][-1])
            hits = torch.empty((total, 2), dtype=torch.int32, device=dev)
            det = torch.empty((total, 4), dtype=torch.float32, device=dev)
            assert l.pt_trace_rays_list(sc._h, C.c_void_p(d_rays.data_ptr()), len(c.rays), int(both), C.c_void_p(off.data_ptr()), total,
                                        C.c_void_p(hits.data_ptr()), C.c_void_p(det.data_ptr()), C.c_void_p(st.cuda_stream)) == 0
            got[both] = (cnt, off, hits, det)
        assert sc.device_bytes == bytes0      # a query allocates nothing
    st.synchronize()
    for both, (cnt, off, hits, det) in got.items():
        h = hits.cpu().numpy()
        assert_csr((off, np.ascontiguousarray(h[:, 0]).view(F), np.ascontiguousarray(h[:, 1]), det), wants[both], f"behind an update, both = {both}")
        assert np.array_equal(cnt.cpu().numpy(), hs[both].count)


@pytest.mark.gpu
def test_queries_leave_renders_alone(_gpu):
    import torch
    name = "standin24_spheres"
    c = ray_case(name)
    pts, _, _ = point_case(name)
    cam, prm = ptamd.make_camera(100, 52), ptamd.default_params(passes=3, spp_per_pass=4)
    sc = ptamd.Scene(c.nodes, c.tris, c.spheres)
    sc.trace_rays_all(c.rays)      # before the first render, too
    sc.enable_counters(True)
    img = sc.render(cam, prm)
    state = (sc.last_iterations(), sc.device_bytes)
    counters = sc.counters()
    sc.trace_rays_all(c.rays, both_sides=True, detail=True)
    sc.within_radius(pts, detail=True)
    sc.trace_rays_all(torch.from_numpy(c.rays).cuda(), detail=True)
    sc.within_radius(torch.from_numpy(pts).cuda())
    torch.cuda.synchronize()
    assert (sc.last_iterations(), sc.device_bytes) == state
    assert np.array_equal(counters, sc.counters())
    img2 = sc.render(cam, prm)
    assert np.array_equal(bits(img), bits(img2)) and np.array_equal(bits(img), bits(ptamd.Scene(c.nodes, c.tris, c.spheres).render(cam, prm)))
    assert (sc.last_iterations(), sc.device_bytes) == state


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["standin24_spheres", "comb32"])
def test_odd_rays_end_and_leave_their_neighbours_alone(_gpu, name):
    """query_ref.odd_rays spread over a batch of 200, offsets from the device's own counts: the calls return, every prim is in range,
    and every other ray's list is brute force's."""
    import torch
    c, sc = ray_case(name), ray_scene(name)
    odd = Q.odd_rays()
    rays = c.rays[:200].copy()
    at = 3 + 16 * np.arange(len(odd))
    rays[at] = odd
    keep = np.ones(len(rays), bool)
    keep[at] = False
    for both in (False, True):
        off, t, prim, det = (_np(x) for x in sc.trace_rays_all(torch.from_numpy(rays).cuda(), both_sides=both, detail=True))
        assert ((prim >= -1) & (prim < c.n_prims)).all()
        wo, wt, wp, wd = ray_want(name, both)
        for i in np.nonzero(keep)[0]:
            s, w = slice(off[i], off[i + 1]), slice(wo[i], wo[i + 1])
            assert np.array_equal(prim[s], wp[w]) and np.array_equal(bits(t[s]), bits(wt[w])), (name, both, i)
            assert np.array_equal(bits(det[s]), bits(wd[w])), (name, both, i)
