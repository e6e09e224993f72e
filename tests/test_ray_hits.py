"""The first K hits along a ray and the hit count (pt_trace_rays_k, pt_count_hits and their _host variants, Scene.trace_rays_k,
Scene.count_hits).

On the CPU: the C-ABI surface, the argument checks with a fake scene and fake device addresses, the wrapper's own checks, the yardstick
(tests/ray_hits_ref.py: a numpy float32 evaluation of the header's definition over every (ray, primitive) pair) pinned to the oracle's
Triangle::hit and Sphere::hit, to slack_ref.box_test and to the oracle's RayCast, and the yardstick's properties.

On the GPU: bits only, no tolerance, and no ray left out of a comparison.  Every slot of every list for K in (1, 2, 5, 8, 9, 32) and both
flag values against brute force, the detail records against numpy, the counts against len(H), column 0 against Scene.trace_rays,
partial waves between sentinels, the binary walk forced by its knob and taken by itself, the same bits whatever tree the scene holds,
stream order behind an update, no side effects on renders, and a batch with odd rays.

Conditions on the inputs, asserted on the reference before any comparison: every member of every H is reached by both trees' chains of
boxes with the cull at tmax (slack_ref.quad_chain_accepts, binary_chain_accepts: this rules out the rays of the known defect of
DESIGN.md section 33; on the CPU on the trees as the host builds them, on the GPU on the downloaded ones), and the sets hold what they
claim (CLAIMS below)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import deep_tree_ref as Dp
import dynamic_ref as R
import ptamd
import query_ref as Q
import ray_hits_ref as H
import slack_ref as S
import test_nearest as T
import test_nearest_k as TK
import test_query as TQ
import test_slack as SL
from scenes_util import attribute_scene, make_prims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pathtrace-on-cuda_amd")
F = np.float32
bits = H.bits
SLICES = TK.SLICES
KS = H.KS
SCENES = ("attribute", "standin24_spheres", "sheet", "comb32")
SEEDS = {"attribute": 71, "standin24_spheres": 72, "sheet": 73, "comb32": 74}
M_RAYS = {"attribute": 400, "standin24_spheres": 240, "sheet": 250, "comb32": 600}      # the `m` of the scene's ray recipe
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


class Case:
    """A scene on the host (prims for the host build, nodes / tris at the pose the device scene will hold, spheres), what brute force
    runs over (V0 E1 E2 and the reference leaf box of every triangle) and its ray set."""

    def __init__(self, name):
        self.name = name
        self.pos = None      # the pose a deep scene is moved to after its upload
        if name == "comb32":
            pos = np.ascontiguousarray(Dp.comb_positions(32), F).reshape(-1, 3, 3)
            n = len(pos)
            rs = np.random.RandomState(23)      # test_nearest._deep_scene's carrier: any host-built scene of as many triangles, two of them lights
            a = rs.uniform(-8, 8, (n, 3)).astype(F) + F([0, 20, 0])
            b, c = a + rs.uniform(-3, 3, a.shape).astype(F), a + rs.uniform(-3, 3, a.shape).astype(F)
            self.prims = np.concatenate([make_prims(a[:n - 2], b[:n - 2], c[:n - 2]), make_prims(a[n - 2:], b[n - 2:], c[n - 2:], albedo=(0, 0, 0), emit=(6, 6, 6))])
            self.nodes0, self.tris0, _ = ptamd.build_bvh(self.prims)
            self.pos = pos
            self.tris = R.restate_tris(self.tris0, pos.reshape(-1, 9))
            self.nodes = R.refit_nodes(self.nodes0, self.tris)
            self.spheres = None
            self.rays = Dp.comb_query_rays(SEEDS[name], M_RAYS[name])
        else:
            if name == "sheet":
                self.prims, self.spheres = H.sheet_stack(), H.sheet_spheres()
            elif name == "attribute":
                self.prims, self.spheres = attribute_scene(T.ATTR_SEED, 12)[0], None
            else:
                self.prims, self.spheres = ptamd.gen_scene(1, 24), TQ.make_test_spheres()
            self.nodes, self.tris, _ = ptamd.build_bvh(self.prims)
            self.nodes0, self.tris0 = self.nodes, self.tris
            if name == "sheet":
                self.rays = H.sheet_rays(SEEDS[name], M_RAYS[name])
            else:
                self.rays = H.scene_rays(SEEDS[name], M_RAYS[name], R.positions(self.tris), self.spheres)
        self.tris9 = H.tri_v0e1e2(self.tris)
        self.leaf_of, self.leaf_boxes = H.leaf_of_tri(self.nodes)
        self.tri_boxes = self.leaf_boxes[self.leaf_of]
        self.n_tris = len(self.tris)
        self.n_prims = self.n_tris + (0 if self.spheres is None else len(self.spheres))
        assert len(self.rays) <= 4096
        self._h = {}

    def hits(self, both):
        if both not in self._h:
            self._h[both] = H.brute(self.rays, self.tris9, self.tri_boxes, self.spheres, both)
        return self._h[both]

    def scene(self):
        sc = ptamd.Scene(self.nodes0, self.tris0, self.spheres)
        if self.pos is not None:
            sc.update_vertices(self.pos.reshape(-1, 9))
            sc.rebuild_tree()
        return sc


def case(name):
    return _cached(("case", name), lambda: Case(name))


def members(c, both):
    """(ray index, prim) of every triangle member of every H of the case's set."""
    h = c.hits(both)
    i, j = np.nonzero((h.prim >= 0) & (h.prim < c.n_tris))
    return i, h.prim[i, j].astype(np.int64)


def assert_chains_reach_every_member(c, trees, what):
    """Both trees' chains of boxes let every member's ray through with the cull at tmax: none of the sets' rays is one of the known defect's."""
    i, prim = members(c, True)
    assert len(i) > 0
    rays = c.rays[i]
    okq = S.quad_chain_accepts(trees, rays, prim, rays[:, 7])
    okb = S.binary_chain_accepts(trees, rays, prim, rays[:, 7])
    assert okq.all() and okb.all(), f"{what}: {(~okq).sum()} / {(~okb).sum()} of {len(i)} members are refused by the 4-wide / binary chain, rays {np.unique(i[~(okq & okb)])[:8]}"


# What each scene's set must hold, asserted by assert_sets_hold_what_they_claim (counts of rays).  "more32": |H| > 32; "fewer": 1 <= |H| < k
# at k = 8; "none": |H| = 0; "cut_ties": an exact tie in t between slot k - 1 and the first member left out, at the k named; "inside_ties":
# a tie inside the list at k = 8; "both_roots" / "inside_sphere": rays with both roots of a sphere / with its far root only; "mixed": a
# sphere and a triangle on one ray; "degenerate": a zero direction component; "segments": un-normalised, tmax = 1, and hit; "back_only":
# rays whose both-sides H has members the front H lacks.
CLAIMS = {
    "attribute": {"fewer": 50, "none": 50, "cut_ties": {1: 5}, "inside_ties": 10, "degenerate": 100, "segments": 20, "back_only": 200},
    "standin24_spheres": {"fewer": 50, "none": 20, "both_roots": 30, "inside_sphere": 30, "mixed": 30, "degenerate": 50, "segments": 10, "back_only": 100},
    "sheet": {"more32": 100, "fewer": 50, "none": 20, "cut_ties": {1: 20, 2: 1, 5: 1, 8: 20, 9: 1, 32: 20}, "inside_ties": 100, "both_roots": 50, "inside_sphere": 50,
              "mixed": 100, "degenerate": 300, "segments": 50, "back_only": 300},
    "comb32": {"fewer": 50, "none": 20, "degenerate": 20, "back_only": 100},
}


def set_figures(c):
    hf, hb = c.hits(False), c.hits(True)
    fig = {"more32": int((hf.count > 32).sum()), "degenerate": int((c.rays[:, 3:6] == 0).any(1).sum()),
           "segments": int(((c.rays[:, 7] == 1) & (hf.count > 0)).sum()), "back_only": int((hb.count > hf.count).sum())}
    f8 = H.figures(hf, 8)
    fig.update(fewer=f8["fewer"], none=f8["none"], inside_ties=f8["inside_ties"])
    fig["cut_ties"] = {k: max(H.figures(hf, k)["cut_ties"], H.figures(hb, k)["cut_ties"]) for k in KS}
    sph = hb.prim >= c.n_tris
    twice, leaving_only = np.zeros(len(c.rays), bool), np.zeros(len(c.rays), bool)
    for j in range(c.n_prims - c.n_tris):
        mine = hb.prim == c.n_tris + j
        twice |= mine.sum(1) == 2
        leaving_only |= (mine.sum(1) == 1) & (mine & (hb.facing < 0)).any(1)
    fig["both_roots"], fig["inside_sphere"] = int(twice.sum()), int(leaving_only.sum())
    fig["mixed"] = int((sph.any(1) & ((hb.prim >= 0) & ~sph).any(1)).sum())
    return fig


def assert_sets_hold_what_they_claim(name):
    c = case(name)
    fig = _cached(("fig", name), lambda: set_figures(c))
    print(f"{name}: {len(c.rays)} rays, {fig}")
    for key, want in CLAIMS[name].items():
        if key == "cut_ties":
            for k, m in want.items():
                assert fig[key][k] >= m, (name, key, k, fig[key])
        else:
            assert fig[key] >= want, (name, key, fig[key], want)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
NEW = ("pt_trace_rays_k", "pt_trace_rays_k_host", "pt_count_hits", "pt_count_hits_host")


def test_new_symbols_are_exported_declared_and_bound(tmp_path):
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    assert callable(ptamd.Scene.trace_rays_k) and callable(ptamd.Scene.count_hits)
    assert ptamd.RAY_HITS_KMAX == 32 and (ptamd.HITS_FRONT, ptamd.HITS_BOTH_SIDES) == (0, 1)
    src = tmp_path / "kmax.c"
    src.write_text('#include "pt_api.h"\n_Static_assert(PT_RAY_HITS_KMAX == 32, "PT_RAY_HITS_KMAX");\n'
                   '_Static_assert(PT_HITS_FRONT == 0 && PT_HITS_BOTH_SIDES == 1, "flags");\n')
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    at = hdr.index("First K hits along a ray and hit counts")
    assert hdr.index("K nearest and counts within a radius") < at < hdr.index("Radiance along the caller's own rays")
    assert hdr.index(" pt_count_within_host(") < at      # directly after that section: its last declaration comes before, the next section after


def test_bad_arguments_are_rejected_before_any_device_call():
    """A fake scene and fake device addresses: never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    base = 1 << 40
    scene, rays, out, det, cnt = (C.c_void_p(base + (i << 20)) for i in range(5))
    off = lambda p, k: C.c_void_p(p.value + k)      # noqa: E731
    dev = [
        ("NULL scene", (None, rays, 64, 8, 0, out, None)),
        ("NULL rays", (scene, None, 64, 8, 0, out, None)),
        ("NULL hits", (scene, rays, 64, 8, 0, None, None)),
        ("n < 0", (scene, rays, -1, 8, 0, out, None)),
        ("k = 0", (scene, rays, 64, 0, 0, out, None)),
        ("k = 33", (scene, rays, 64, 33, 1, out, None)),
        ("k = -1", (scene, rays, 64, -1, 0, out, None)),
        ("flags 2", (scene, rays, 64, 8, 2, out, None)),
        ("flags 3", (scene, rays, 64, 8, 3, out, None)),
        ("flags -1", (scene, rays, 64, 8, -1, out, None)),
        ("flags 1 << 8", (scene, rays, 64, 8, 256, out, None)),
        ("rays + 4", (scene, off(rays, 4), 64, 8, 0, out, None)),
        ("rays + 8", (scene, off(rays, 8), 64, 8, 1, out, None)),
        ("hits + 4", (scene, rays, 64, 8, 0, off(out, 4), None)),
        ("detail + 2", (scene, rays, 64, 8, 0, out, off(det, 2))),
        ("n = 0 does not excuse a NULL", (scene, None, 0, 8, 0, out, None)),
        ("n = 0 does not excuse k = 0", (scene, rays, 0, 0, 0, out, None)),
        ("n = 0 does not excuse unknown flags", (scene, rays, 0, 8, 4, out, None)),
    ]
    for what, a in dev:
        assert l.pt_trace_rays_k(*a, None) == -1, what
        assert b"pt_trace_rays_k:" in l.pt_last_error(), (what, l.pt_last_error())
    dev_count = [
        ("NULL scene", (None, rays, 64, 0, cnt)),
        ("NULL rays", (scene, None, 64, 0, cnt)),
        ("NULL count", (scene, rays, 64, 1, None)),
        ("n < 0", (scene, rays, -1, 0, cnt)),
        ("flags 2", (scene, rays, 64, 2, cnt)),
        ("rays + 8", (scene, off(rays, 8), 64, 0, cnt)),
        ("count + 2", (scene, rays, 64, 0, off(cnt, 2))),
        ("n = 0 does not excuse a NULL", (scene, rays, 0, 0, None)),
        ("n = 0 does not excuse unknown flags", (scene, rays, 0, 7, cnt)),
    ]
    for what, a in dev_count:
        assert l.pt_count_hits(*a, None) == -1, what
        assert b"pt_count_hits:" in l.pt_last_error(), (what, l.pt_last_error())
    h_rays, h_out, h_det, h_cnt = np.zeros((64, 8), F), np.zeros((64, 8), ptamd.HIT_DTYPE), np.zeros((64, 8, 4), F), np.zeros(64, np.int32)
    P = ptamd._ptr
    host = [
        ("NULL scene", (None, P(h_rays), 64, 8, 0, P(h_out), None)),
        ("NULL rays", (scene, None, 64, 8, 0, P(h_out), None)),
        ("NULL hits", (scene, P(h_rays), 64, 8, 0, None, P(h_det))),
        ("n < 0", (scene, P(h_rays), -5, 8, 0, P(h_out), None)),
        ("k = 0", (scene, P(h_rays), 64, 0, 0, P(h_out), None)),
        ("k = 33", (scene, P(h_rays), 64, 33, 0, P(h_out), None)),
        ("flags 2", (scene, P(h_rays), 64, 8, 2, P(h_out), None)),
    ]
    for what, a in host:
        assert l.pt_trace_rays_k_host(*a) == -1, what
        assert b"pt_trace_rays_k_host:" in l.pt_last_error(), (what, l.pt_last_error())
    host_count = [
        ("NULL scene", (None, P(h_rays), 64, 0, P(h_cnt))),
        ("NULL rays", (scene, None, 64, 0, P(h_cnt))),
        ("NULL count", (scene, P(h_rays), 64, 0, None)),
        ("n < 0", (scene, P(h_rays), -5, 1, P(h_cnt))),
        ("flags -2", (scene, P(h_rays), 64, -2, P(h_cnt))),
    ]
    for what, a in host_count:
        assert l.pt_count_hits_host(*a) == -1, what
        assert b"pt_count_hits_host:" in l.pt_last_error(), (what, l.pt_last_error())
    # nothing to do: PT_OK, still without touching the scene or the device
    assert l.pt_trace_rays_k(scene, rays, 0, 1, 0, out, None, None) == 0
    assert l.pt_trace_rays_k(scene, rays, 0, 32, 1, out, det, None) == 0
    assert l.pt_trace_rays_k_host(scene, P(h_rays), 0, 8, 0, P(h_out), None) == 0
    assert l.pt_count_hits(scene, rays, 0, 1, cnt, None) == 0
    assert l.pt_count_hits_host(scene, P(h_rays), 0, 0, P(h_cnt)) == 0


class _FakeScene:
    n_tris, device, _h = 5, 0, C.c_void_p(1 << 40)


def test_wrapper_checks_shape_dtype_device_and_k_on_the_host():
    import torch
    fake = _FakeScene()
    tk, ch = ptamd.Scene.trace_rays_k, ptamd.Scene.count_hits
    for rays in (np.zeros((4, 7), F), np.zeros(32, F), np.zeros((2, 4, 8), F)):
        with pytest.raises(ptamd.PtError):
            tk(fake, rays, 4)
        with pytest.raises(ptamd.PtError):
            ch(fake, rays)
    for rays in (torch.zeros((5, 8)), torch.zeros((5, 8), dtype=torch.float64), torch.zeros((5, 7)), torch.zeros((8, 5)).t(), [[0.0] * 8]):
        with pytest.raises(ptamd.PtError):      # a CPU tensor, a wrong dtype, a wrong shape, not contiguous, not an array
            tk(fake, rays, 4)
        with pytest.raises(ptamd.PtError):
            ch(fake, rays, both_sides=True)
    for k in (0, 33, -1):
        with pytest.raises(ptamd.PtError):
            tk(fake, np.zeros((4, 8), F), k)
    t, prim, det = tk(fake, np.zeros((0, 8), F), 7, both_sides=True, detail=True)      # n = 0: PT_OK without a device
    assert t.shape == (0, 7) and prim.shape == (0, 7) and det.shape == (0, 7, 4) and t.dtype == F and prim.dtype == np.int32
    cnt = ch(fake, np.zeros((0, 8), F))
    assert cnt.shape == (0,) and cnt.dtype == np.int32


PINNED = ("attribute", "standin24_spheres", "sheet")      # the host-built scenes


def _tris48(tris):
    return np.concatenate([tris[:, 0:9], tris[:, R.T_N:R.T_N + 9], tris[:, R.T_T:R.T_T + 9], tris[:, R.T_B:R.T_B + 9], tris[:, R.T_MAT0:R.T_MAT0 + 12]], 1)


@pytest.mark.parametrize("name", PINNED)
def test_yardstick_triangle_acceptance_and_t_are_the_oracles(name):
    """Front acceptance (the range tests; the leaf box is pinned below) and t of EVERY (ray, triangle) pair against the oracle's
    Triangle::hit with t_min 0 and t_max = tmax, bit for bit."""
    import oracle_lib as O
    c = case(name)
    _, t, _, _, front, _ = H.tri_eval(c.rays, c.tris9)
    tris48 = _tris48(c.tris)
    n = len(c.rays)
    hit = np.zeros_like(front)
    for k in range(c.n_tris):
        r10 = np.concatenate([np.full((n, 1), k, F), c.rays[:, 0:6], np.zeros((n, 1), F), c.rays[:, 7:8], np.zeros((n, 1), F)], 1)
        out = O.tri_hit(tris48, r10)
        hit[:, k] = out[:, 0] > 0
        same = bits(out[:, 1]) == bits(t[:, k])
        assert same[hit[:, k]].all(), (name, k)
    assert np.array_equal(hit, front), f"{name}: {(hit != front).sum()} pairs are accepted differently"
    assert front.sum() > 1000


@pytest.mark.parametrize("name", ["standin24_spheres", "sheet"])
def test_yardstick_sphere_roots_are_the_oracles(name):
    import oracle_lib as O
    c = case(name)
    r1, r2, v1, v2 = H.sphere_eval(c.rays, c.spheres)
    n, entering, leaving = len(c.rays), 0, 0
    for j in range(len(c.spheres)):
        r10 = np.concatenate([np.full((n, 1), j, F), c.rays[:, 0:6], np.zeros((n, 1), F), c.rays[:, 7:8], np.zeros((n, 1), F)], 1)
        out = O.sphere_hit(c.spheres, r10)
        hit = out[:, 0] > 0
        assert np.array_equal(hit, v1[:, j] | v2[:, j]), (name, j)
        root = np.where(v1[:, j], r1[:, j], r2[:, j])
        assert np.array_equal(bits(out[hit, 1]), bits(root[hit])), (name, j)
        entering, leaving = entering + int((hit & v1[:, j]).sum()), leaving + int((hit & ~v1[:, j]).sum())
    assert entering > 50 and leaving > 20      # the near root and, from inside, the far one


@pytest.mark.parametrize("name", PINNED)
def test_yardstick_leaf_box_test_is_slack_refs(name):
    c = case(name)
    invD, deg = H.inv_dir(c.rays)
    inv_s, _, deg_s = S.ray_setup(c.rays[:, 3:6])
    assert np.array_equal(deg, deg_s) and np.array_equal(bits(invD[~deg]), bits(inv_s[~deg]))
    got = H.box_pass(c.rays, c.leaf_boxes)
    inf = np.full(len(c.rays), np.inf, F)
    for b in range(len(c.leaf_boxes)):
        want, _ = S.box_test(np.tile(c.leaf_boxes[b, 0:6], (len(c.rays), 1)), c.rays[:, 0:3], invD, inf)
        assert np.array_equal(got[~deg, b], want[~deg]), (name, b)
    assert got[~deg].any() and not got[~deg].all()


@pytest.mark.parametrize("name", PINNED)
def test_yardstick_first_member_is_the_oracles_raycast(name):
    """On the rays with |1 / dir| >= 1 (tests/test_query.py: LONG_DIRECTIONS) the first member of the front H is RayCast's answer."""
    import oracle_lib as O
    O.set_libm(1)
    c = case(name)
    with np.errstate(all="ignore"):
        inv = F(1) / c.rays[:, 3:6]
        ok = ~(((inv * inv).sum(1)) < 1)
    assert ok.sum() > 0.6 * len(c.rays)
    hits_o, prim_o, _ = O.Scene(c.nodes.tobytes(), c.tris, c.spheres).raycast(c.rays)
    t, prim, _ = H.lists(c.hits(False), 1)
    assert np.array_equal(prim[ok, 0], prim_o[ok]), f"{name}: {(prim[ok, 0] != prim_o[ok]).sum()} first members are not the oracle's"
    assert np.array_equal(bits(t[ok, 0]), bits(hits_o[ok, 1]))
    assert (prim_o[ok] >= 0).sum() > 100 and (prim_o[ok] < 0).sum() > 10


@pytest.mark.parametrize("name", PINNED)
def test_sets_hold_what_they_claim_and_the_chains_reach_every_member(name):
    assert_sets_hold_what_they_claim(name)
    c = case(name)
    assert_chains_reach_every_member(c, SL.host_trees(c.prims, "ray_hits_" + name), name)


def test_comb_set_holds_what_it_claims():
    assert_sets_hold_what_they_claim("comb32")


@pytest.mark.parametrize("name", PINNED)
def test_yardstick_properties(name):
    """k = 1 is the closest hit, a shorter list is a prefix of a longer one, the front set is a subset of the both-sides set, the count is
    the list's length, and the order is the definition's."""
    c = case(name)
    for both in (False, True):
        h = c.hits(both)
        ls = {k: H.lists(h, k) for k in KS}
        for k in KS:
            t, prim, det = ls[k]
            assert np.array_equal((prim >= 0).sum(1), np.minimum(h.count, k))
            assert ((prim >= 0)[:, :-1] >= (prim >= 0)[:, 1:]).all(), "a miss slot before a hit"
            assert (bits(t)[prim < 0] == 0).all() and (bits(det)[prim < 0] == 0).all()
            assert ((t >= 0) & (t <= c.rays[:, 7:8]))[prim >= 0].all()
            later = prim[:, 1:] >= 0
            same_sphere = (prim[:, 1:] == prim[:, :-1]) & (prim[:, 1:] >= c.n_tris)
            assert ((t[:, 1:] > t[:, :-1]) | ((t[:, 1:] == t[:, :-1]) & (prim[:, 1:] < prim[:, :-1])) | ~later).all(), "the order of the definition"
            assert not (same_sphere & ~both).any() and (t[:, 1:] > t[:, :-1])[same_sphere & later].all()
            for k2 in KS:
                if k < k2:
                    assert all(np.array_equal(bits(x), bits(y[:, :k])) for x, y in zip(ls[k], ls[k2])), (k, k2)
        if not both:
            # the closest hit by its own rule: the smallest t, among equal t the largest prim
            t1, p1, _ = ls[1]
            hit = h.count > 0
            assert (h.t[hit, 0] == np.where(h.prim >= 0, h.t, np.inf).min(1)[hit]).all()
            tied = (h.t == h.t[:, 0:1]) & (h.prim >= 0)
            assert (p1[hit, 0] == np.where(tied, h.prim, -1).max(1)[hit]).all()
    hf, hb = c.hits(False), c.hits(True)
    assert (hb.count >= hf.count).all()
    for i in range(0, len(c.rays), 7):      # every front record is a both-sides record, with its facing
        fr = set(zip(bits(hf.t[i, :hf.count[i]]).tolist(), hf.prim[i, :hf.count[i]].tolist()))
        bo = set(zip(bits(hb.t[i, :hb.count[i]]).tolist(), hb.prim[i, :hb.count[i]].tolist()))
        assert fr <= bo, i
    tri_f = (hf.prim >= 0) & (hf.prim < c.n_tris)
    assert (hf.facing[tri_f] == 1).all() and (hb.facing[(hb.prim >= 0)] != 0).all() and (hb.facing < 0).any()


def _coincident_pairs(c):
    """{the larger index: the smaller} of the triangles of `tris` that share all nine position floats with another."""
    seen, out = {}, {}
    for k, key in enumerate(r.tobytes() for r in np.ascontiguousarray(c.tris[:, 0:9])):
        if key in seen:
            out[k] = seen[key]
        seen.setdefault(key, k)
    return out


def test_yardstick_puts_a_duplicated_triangle_before_the_one_it_copies():
    """attribute_scene's 40 duplicated triangles and the sheet stack's three duplicated layers: the two of a pair are accepted together,
    tie in t, and the one with the larger index comes first — everything between them shares the t."""
    for name, n_pairs, floor in (("attribute", 40, 5), ("sheet", 6, 500)):
        pairs_of = _coincident_pairs(case(name))
        assert len(pairs_of) == n_pairs, (name, len(pairs_of))
        cc = case(name)
        pairs = 0
        for both in (False, True):
            h = cc.hits(both)
            for i in range(len(cc.rays)):
                row = h.prim[i, :h.count[i]]
                for j, p in enumerate(row.tolist()):
                    if p not in pairs_of:
                        continue
                    at = np.nonzero(row == pairs_of[p])[0]
                    assert len(at) == 1 and at[0] > j, (name, i, p)      # the same floats: accepted together
                    assert (bits(h.t[i, j:at[0] + 1]) == bits(h.t[i, j])).all(), (name, i, p)
                    pairs += 1
        print(f"{name}: {pairs} duplicate pairs in lists")
        assert pairs >= floor


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


def _device_scene(name):
    return _cached(("scene", name), lambda: case(name).scene())


def assert_lists(got, want, what):
    """got: (t, prim[, detail]) of shape (n, k[, 4]); want: the same from the yardstick."""
    t, prim = np.asarray(got[0]), np.asarray(got[1])
    assert t.shape == want[0].shape and prim.shape == want[1].shape and t.dtype == F and prim.dtype == np.int32, what
    bad = (prim != want[1]).any(1)
    assert not bad.any(), f"{what}: the prims of {bad.sum()} rays differ, first at {np.nonzero(bad)[0][:5]}: {prim[bad][:2]} want {want[1][bad][:2]}"
    bad = (bits(t) != bits(want[0])).any(1)
    assert not bad.any(), f"{what}: t differs at {np.nonzero(bad)[0][:5]}"
    if len(got) > 2:
        det = np.asarray(got[2])
        assert det.shape == want[2].shape, what
        bad = (bits(det) != bits(want[2])).any((1, 2))
        assert not bad.any(), f"{what}: the detail records of {bad.sum()} rays differ, first at {np.nonzero(bad)[0][:5]}"


def assert_inputs(name, sc):
    """The conditions on the inputs, on the device's own arrays: the yardstick's leaf boxes are the uploaded ones, the walk is the one the
    scene should take, the sets hold what they claim, and both downloaded trees' chains reach every member."""
    c = case(name)
    assert (3 * sc.tree_info()["quad_depth"] + 2 > 40) == (name == "comb32")      # the comb takes the binary walk by itself
    tri = sc.dbg_array("tri").reshape(-1, 12)
    lb = sc.dbg_array("leafbox").reshape(-1, 8)
    prim, leaf = tri[:, 3].view(np.int32), tri[:, 7].view(np.int32)
    assert np.array_equal(np.sort(prim), np.arange(c.n_tris))
    assert np.array_equal(bits(lb[leaf, 0:6]), bits(c.tri_boxes[prim])), f"{name}: the reference leaf boxes differ from the uploaded ones"
    rec = np.concatenate([tri[:, 0:3], tri[:, 4:7], tri[:, 8:11]], 1)
    assert np.array_equal(bits(rec), bits(c.tris9[prim])), f"{name}: V0 E1 E2 differ from the uploaded records"
    assert_sets_hold_what_they_claim(name)
    assert_chains_reach_every_member(c, S.Trees(sc.dbg_array("nodes"), sc.dbg_array("quad"), sc.dbg_array("tri"), sc.dbg_array("leafbox")), name + ", device trees")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_lists_details_and_counts_are_brute_forces(_gpu, name):
    c, sc = case(name), _device_scene(name)
    assert_inputs(name, sc)
    for both in (False, True):
        h = c.hits(both)
        for k in KS:
            want = H.lists(h, k)
            assert_lists(sc.trace_rays_k(c.rays, k, both_sides=both, detail=True), want, f"{name}, K = {k}, both = {both}")
            assert_lists(sc.trace_rays_k(c.rays, k, both_sides=both), want[:2], f"{name}, K = {k}, both = {both}, without detail")
        got = sc.count_hits(c.rays, both_sides=both)
        assert got.dtype == np.int32 and np.array_equal(got, h.count), f"{name}, both = {both}: {(got != h.count).sum()} counts differ, first at {np.nonzero(got != h.count)[0][:5]}"
    t, prim = sc.trace_rays(c.rays)
    for k in (1, 5, 32):
        tk, pk = sc.trace_rays_k(c.rays, k)
        assert np.array_equal(bits(tk[:, 0]), bits(t)) and np.array_equal(pk[:, 0], prim), f"{name}, K = {k}: column 0 is not trace_rays'"


@pytest.mark.gpu
def test_column_0_is_trace_rays_on_its_own_ray_sets(_gpu):
    """The 20,000-ray set of tests/test_query.py, set C's long segments and the sphere rays: slot 0 under HITS_FRONT is the closest-hit
    query's record, bit for bit, and a count of 0 is a miss."""
    name = "standin24_spheres"
    rays = np.concatenate([TQ._rays(name), Q.set_c(4000, np.random.RandomState(112)), Q.sphere_only_rays()])
    sc = TQ._scene(name)
    t, prim = sc.trace_rays(rays)
    assert (prim >= 0).mean() > 0.5 and (prim < 0).sum() > 1000
    for k in (1, 4, 9):
        tk, pk = sc.trace_rays_k(rays, k)
        assert np.array_equal(bits(tk[:, 0]), bits(t)) and np.array_equal(pk[:, 0], prim), f"K = {k}"
    cnt = sc.count_hits(rays)
    assert np.array_equal(cnt > 0, prim >= 0)
    assert (sc.count_hits(rays, both_sides=True) >= cnt).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sheet", "comb32"])
def test_partial_waves_write_their_own_records_only(_gpu, name):
    """n = 1, 63, 64, 65 and 130 on the device path, the outputs inside larger sentinel-filled buffers: the records of the rays are brute
    force's and nothing before or past them is written."""
    import torch
    c, sc = case(name), _device_scene(name)
    dev = torch.device("cuda:0")
    l = ptamd.lib()
    pad, sent = 256, 0x5A5A5A5A
    for both in (False, True):
        h = c.hits(both)
        for k in (1, 5, 8, 32):
            want = H.lists(h, k)
            for lo, m in SLICES:
                d_rays = torch.from_numpy(np.ascontiguousarray(c.rays[lo:lo + m])).to(dev)
                hits = torch.full((m * k * 2 + 2 * pad,), sent, dtype=torch.int32, device=dev)
                det = torch.full((m * k * 4 + 2 * pad,), sent, dtype=torch.int32, device=dev)
                cnt = torch.full((m + 2 * pad,), sent, dtype=torch.int32, device=dev)
                rc = l.pt_trace_rays_k(sc._h, C.c_void_p(d_rays.data_ptr()), m, k, int(both), C.c_void_p(hits.data_ptr() + 4 * pad),
                                       C.c_void_p(det.data_ptr() + 4 * pad), None)
                assert rc == 0, l.pt_last_error()
                assert l.pt_count_hits(sc._h, C.c_void_p(d_rays.data_ptr()), m, int(both), C.c_void_p(cnt.data_ptr() + 4 * pad), None) == 0
                torch.cuda.synchronize()
                what = f"{name}, K = {k}, both = {both}, n = {m}"
                for buf in (hits, det, cnt):
                    b = buf.cpu().numpy()
                    assert (b[:pad] == sent).all() and (b[-pad:] == sent).all(), what + ": written outside the records"
                rec = hits.cpu().numpy()[pad:-pad].reshape(m, k, 2)
                got = (np.ascontiguousarray(rec[:, :, 0]).view(F), np.ascontiguousarray(rec[:, :, 1]), det.cpu().numpy()[pad:-pad].view(F).reshape(m, k, 4))
                assert_lists(got, tuple(x[lo:lo + m] for x in want), what)
                assert np.array_equal(cnt.cpu().numpy()[pad:-pad], h.count[lo:lo + m]), what


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
    rays = g["rays"]
    for both in (0, 1):
        for k in (1, 2, 5, 8, 9, 32):
            t, prim, det = sc.trace_rays_k(rays, k, both_sides=bool(both), detail=True)
            res.update({f"t_{both}_{k}": t, f"prim_{both}_{k}": prim, f"det_{both}_{k}": det})
        res[f"cnt_{both}"] = sc.count_hits(rays, both_sides=bool(both))
    res["t"], res["prim"] = sc.trace_rays(rays)
np.savez(out, **res)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sheet", "standin24_spheres"])
def test_binary_walk_forced_by_its_knob_gives_the_same_bits(_gpu, tmp_path, name):
    """PTAMD_QUERY_QUAD=0 in a fresh process (the knob is read when a scene is created), as tests/test_query.py sets it."""
    c = case(name)
    scene_file, out = str(tmp_path / "scene.npz"), str(tmp_path / "child.npz")
    np.savez(scene_file, nodes=np.frombuffer(c.nodes.tobytes(), np.uint8), tris=c.tris, spheres=c.spheres, rays=c.rays)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]), PTAMD_QUERY_QUAD="0")
    subprocess.run([sys.executable, "-c", CHILD, scene_file, out], check=True, env=env, timeout=600)
    g = np.load(out)
    assert_sets_hold_what_they_claim(name)
    for both in (0, 1):
        h = c.hits(bool(both))
        for k in KS:
            assert_lists((g[f"t_{both}_{k}"], g[f"prim_{both}_{k}"], g[f"det_{both}_{k}"]), H.lists(h, k), f"PTAMD_QUERY_QUAD=0, {name}, K = {k}, both = {both}")
        assert np.array_equal(g[f"cnt_{both}"], h.count), f"PTAMD_QUERY_QUAD=0, {name}, both = {both}: counts"
    assert np.array_equal(bits(g["t_0_1"][:, 0]), bits(g["t"])) and np.array_equal(g["prim_0_1"][:, 0], g["prim"])


def _moved(name):
    """The case's scene at the turned pose of tests/test_nearest.py: (pos2, tris2, nodes2, {both: Hits})."""
    def make():
        c = case(name)
        pos2 = T._turned(c.tris)
        tris2 = R.restate_tris(c.tris, pos2)
        nodes2 = R.refit_nodes(c.nodes, tris2)
        leaf_of, boxes = H.leaf_of_tri(nodes2)
        tris9 = H.tri_v0e1e2(tris2)
        return pos2, tris2, nodes2, {both: H.brute(c.rays, tris9, boxes[leaf_of], c.spheres, both) for both in (False, True)}
    return _cached(("moved", name), make)


def _assert_pose(sc, rays, hs, what, ks=KS):
    for both in (False, True):
        for k in ks:
            assert_lists(sc.trace_rays_k(rays, k, both_sides=both, detail=True), H.lists(hs[both], k), f"{what}, K = {k}, both = {both}")
        assert np.array_equal(sc.count_hits(rays, both_sides=both), hs[both].count), f"{what}, both = {both}: counts"


@pytest.mark.gpu
def test_the_result_does_not_depend_on_the_tree(_gpu):
    """The tree from the upload, a refit with unchanged positions, a refit at another pose, a fresh upload at that pose and the three
    rebuilds hold different boxes and different topologies: the same bits from all of them at a pose, and they are brute force's."""
    name = "standin24_spheres"
    c = case(name)
    same = {both: c.hits(both) for both in (False, True)}
    sc = ptamd.Scene(c.nodes, c.tris, c.spheres)
    sc.update_vertices(R.positions(c.tris).reshape(-1, 9))
    _assert_pose(sc, c.rays, same, "after update_vertices with unchanged positions")
    pos2, tris2, nodes2, hs = _moved(name)
    moved = (H.lists(hs[True], 8)[1] != H.lists(same[True], 8)[1]).any(1)
    print(f"the move changed {moved.mean():.3f} of the lists")
    assert moved.mean() > 0.2
    sc.update_vertices(pos2)
    _assert_pose(sc, c.rays, hs, "after update_vertices")
    _assert_pose(ptamd.Scene(nodes2, tris2, c.spheres), c.rays, hs, "fresh scene at the pose", (1, 8, 32))
    sc.rebuild_tree()
    _assert_pose(sc, c.rays, hs, "after rebuild_tree")
    sc.rebuild_tree(depth_budget=26, large_fraction=1 / 16)
    _assert_pose(sc, c.rays, hs, "after rebuild_tree(26, 1/16)")
    sc.rebuild_tree_optimized()
    _assert_pose(sc, c.rays, hs, "after rebuild_tree_optimized")
    assert sc.tree_info()["rebuilds"] == 3


@pytest.mark.gpu
def test_queries_after_an_update_on_the_same_stream_see_the_moved_geometry(_gpu):
    """The device path on a non-default stream: behind a vertex update on that stream, with no host wait in between, the lists are brute
    force's on the moved positions — and so are the host path's afterwards."""
    import torch
    name = "standin24_spheres"
    c = case(name)
    pos2, _, _, hs = _moved(name)
    sc = ptamd.Scene(c.nodes, c.tris, c.spheres)
    sc.update_vertices(R.positions(c.tris).reshape(-1, 9))      # the first update allocates the scene's maps: not what is measured below
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    bytes0 = sc.device_bytes
    host = {}
    with torch.cuda.stream(st):
        d_pos = torch.from_numpy(pos2).to(dev)
        d_rays = torch.from_numpy(c.rays).to(dev)
        sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
        got = {(k, both): sc.trace_rays_k(d_rays, k, both_sides=both, detail=True, stream_ptr=st.cuda_stream)
               + (sc.count_hits(d_rays, both_sides=both, stream_ptr=st.cuda_stream),) for k in (5, 32) for both in (False, True)}      # no host wait in between
        assert sc.device_bytes == bytes0      # a query allocates nothing
        g = got[(5, False)]
        assert g[0].dtype == torch.float32 and g[1].dtype == torch.int32 and g[0].shape == g[1].shape == (len(c.rays), 5)
        assert g[2].shape == (len(c.rays), 5, 4) and g[3].dtype == torch.int32 and g[0].device == dev
        for key in got:
            host[key] = [x.cpu().numpy() for x in got[key]]
    st.synchronize()
    for (k, both), h in host.items():
        assert_lists((np.ascontiguousarray(h[0]), np.ascontiguousarray(h[1]), h[2]), H.lists(hs[both], k), f"device path behind an update, K = {k}, both = {both}")
        assert np.array_equal(h[3], hs[both].count), f"device path behind an update, K = {k}, both = {both}: counts"
        assert_lists(sc.trace_rays_k(c.rays, k, both_sides=both, detail=True), tuple(np.ascontiguousarray(x) for x in h[:3]), "the host path against the device path")


@pytest.mark.gpu
def test_queries_leave_renders_alone(_gpu):
    import torch
    name = "standin24_spheres"
    c = case(name)
    cam, prm = ptamd.make_camera(100, 52), ptamd.default_params(passes=3, spp_per_pass=4)
    sc = ptamd.Scene(c.nodes, c.tris, c.spheres)
    sc.trace_rays_k(c.rays, 8)      # before the first render, too
    sc.count_hits(c.rays)
    sc.enable_counters(True)
    img = sc.render(cam, prm)
    cast = sc.raycast(c.rays)
    state = (sc.last_iterations(), sc.device_bytes)
    counters = sc.counters()
    d_rays = torch.from_numpy(c.rays).cuda()
    sc.trace_rays_k(c.rays, 32, both_sides=True, detail=True)
    sc.count_hits(c.rays, both_sides=True)
    sc.trace_rays_k(d_rays, 3, detail=True)
    sc.count_hits(d_rays)
    torch.cuda.synchronize()
    assert (sc.last_iterations(), sc.device_bytes) == state
    assert np.array_equal(counters, sc.counters())
    cast2 = sc.raycast(c.rays)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(cast, cast2))
    img2 = sc.render(cam, prm)
    assert np.array_equal(bits(img), bits(img2)) and np.array_equal(bits(img), bits(ptamd.Scene(c.nodes, c.tris, c.spheres).render(cam, prm)))
    assert (sc.last_iterations(), sc.device_bytes) == state


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["standin24_spheres", "comb32"])
def test_odd_rays_end_and_leave_their_neighbours_alone(_gpu, name):
    """query_ref.odd_rays (zero directions, NaN and inf components, a NaN, infinite and negative tmax) spread over a batch of 200: the
    calls return, those rows keep every prim and count in range, and every other row is brute force's."""
    c, sc = case(name), _device_scene(name)
    odd = Q.odd_rays()
    rays = c.rays[:200].copy()
    at = 3 + 16 * np.arange(len(odd))      # in every wave
    rays[at] = odd
    keep = np.ones(len(rays), bool)
    keep[at] = False
    n_sph = 0 if c.spheres is None else len(c.spheres)
    for both in (False, True):
        h = c.hits(both)
        for k in (1, 8, 32):
            want = tuple(x[:200][keep] for x in H.lists(h, k))
            got = sc.trace_rays_k(rays, k, both_sides=both, detail=True)
            assert ((got[1] >= -1) & (got[1] < c.n_prims)).all()
            assert_lists(tuple(x[keep] for x in got), want, f"{name}, K = {k}, both = {both}, the rows beside the odd ones")
        cnt = sc.count_hits(rays, both_sides=both)
        assert ((cnt >= 0) & (cnt <= c.n_tris + 2 * n_sph)).all()
        assert np.array_equal(cnt[keep], h.count[:200][keep]), f"{name}, both = {both}: counts beside the odd ones"
