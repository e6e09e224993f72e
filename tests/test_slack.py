"""Worst cases of the traversal's slack: the 2^-20 widening of quad_order (csrc/pt_trace.h) against rays searched on
the CPU for the largest slack they need, and the same rays on the binary walk's box_test.

On the CPU: the numpy models of tests/slack_ref.py against the kernels' own functions compiled for the host (bit for bit), the restated
acceptance against the oracle, and a census per ray family on the trees as they are uploaded (tools/dump_accel.cpp --prims).  The census
FINDS rays the reference accepts whose chain of boxes refuses them at the shipped constants (the MISS sets: float Moeller-Trumbore accepts
rays that pass the triangle's own padded box by far more than 2^-20 of the slab terms; the reference's leaf box, up to four triangles, is
larger).  Their numbers are pinned here, and on the GPU every such ray must return exactly what the chains leave: the closest hit among
the accepted triangles whose chain lets the ray through.  Every other searched ray (the 256 per family that need the most slack, and 256
at random) must give the oracle's bits on every query: fresh, after a refit, after each kind of rebuild wherever the chains of the rebuilt
trees accept it (the rays they refuse are pinned as well), and through pt_render_rays on wf_trace and on wf_drain.  The shadow margin is
held against veils in front of a light on four placements."""
import atexit
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import dynamic_ref as R
import oracle_lib as O
import placement_ref as P
import ptamd
import scenes_util as U
import slack_ref as S
import test_query as Tq

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pathtrace-on-cuda_amd")
N_CAND, CHUNK, KEEP, FLOOR = 1_000_000, 250_000, 256, 16
ATTR_SEED = 7
# family: (scene, generator, seed, nearest and farthest origin)
FAMILIES = {
    "a_attribute": ("attribute", "sliver", 3301, 4.0, 64.0),
    "a_needle": ("needle", "sliver", 3302, 4.0, 64.0),
    "b_attribute": ("attribute", "sliver", 3303, 2.0 ** 8, 2.0 ** 19.5),
    "b_needle": ("needle", "sliver", 3304, 2.0 ** 8, 2.0 ** 19.5),
    "c_home": ("home", "corner", 3305, 2.0 ** 10, 2.0 ** 19.5),
    "c_attribute": ("attribute", "corner", 3306, 2.0 ** 10, 2.0 ** 19.5),
    "d_mixed": ("mixed", "cluster", 3307, 2.0 ** 15, 2.0 ** 19.5),
}
# The MISS sets of the census, (4-wide walk, binary walk, and of each those refused by the slabs alone, with no cull): rays of the N_CAND
# candidates whose oracle hit has a chain that refuses the ray at the shipped constants with the cull at the oracle's t.  The documented
# limit of DESIGN.md section 33, pinned: a change of a pad, of the slack or of a builder moves these numbers and has to say so.
MISS_SIZES = {"a_attribute": (39, 57, 25, 50), "a_needle": (257, 222, 60, 73), "b_attribute": (9646, 9253, 7675, 9252),
              "b_needle": (11581, 5613, 3812, 4105), "c_home": (34, 49, 9, 49), "c_attribute": (58, 108, 36, 108), "d_mixed": (2, 40, 0, 40)}
# Families whose kept rays do not reach the floor of FLOOR rays that need any slack, and how many do: with the origin in the room
# (a) the pads alone carry every ray that the chain lets through at all, and on mixed (d) every box is widened by a whole unit
# (maxabs * 2^-20).  A library with no slack is NOT shown to fail on these families.
BELOW_FLOOR = {"a_attribute": 0, "a_needle": 0, "d_mixed": 0}

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# host tools, compiled once per process into a directory of their own: nothing is written into the source tree
# ---------------------------------------------------------------------------------------------------------------------------------
def _tools():
    def make():
        d = tempfile.mkdtemp(prefix="pt_slack_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        objs = []
        for name in ("accel_build", "bvh_build", "scenes", "pt_host", "obj_loader"):      # the Makefile's own g++ flags, as tests/test_dynamic.py
            objs.append(os.path.join(d, f"{name}.o"))
            subprocess.run(["g++", "-std=c++17", "-O2", "-fPIC", "-fvisibility=hidden", "-Wall", "-ffp-contract=off", "-fno-fast-math", "-pthread",
                            "-c", os.path.join(PKG, "host", f"{name}.cpp"), "-o", objs[-1]], check=True)
        subprocess.run(["g++", "-std=c++17", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "dump_accel.cpp")] + objs +
                       ["-pthread", "-o", os.path.join(d, "dump_accel")], check=True)
        return d
    return _cached("tools", make)


def host_trees(prims, tag):
    """slack_ref.Trees of the arrays pt_build_accel makes for `prims`, without a GPU."""
    d = _tools()
    src, pre = os.path.join(d, tag + ".prims"), os.path.join(d, tag)
    np.ascontiguousarray(prims, F).tofile(src)
    env = {k: v for k, v in os.environ.items() if k not in ("PTAMD_TREE", "PTAMD_LEAF", "PTAMD_BFS")}
    subprocess.run([os.path.join(d, "dump_accel"), "--prims", src, pre], check=True, env=env)
    a = {k: np.fromfile(f"{pre}.{k}.bin", np.uint32) for k in ("wide", "quad", "tri", "leafbox")}
    return S.Trees(a["wide"].view(F), a["quad"], a["tri"].view(F), a["leafbox"].view(F))


def _function_text(src, head):
    """The text of the function that starts with `head`, to its closing brace."""
    at = src.index(head)
    depth, k = 0, src.index("{", at)
    while True:
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        k += 1
        if depth == 0:
            return src[at:k]


def slack_host(ksl):
    """tools/slack_host.cpp around box_test and quad_order as csrc/pt_trace.h has them, quad_order's slack constant set to `ksl`."""
    def make():
        d = os.path.join(_tools(), f"host_{ksl}")
        os.makedirs(d)
        src = open(os.path.join(PKG, "csrc", "pt_trace.h")).read()
        text = _function_text(src, "PT_DEV bool box_test(") + "\n" + _function_text(src, "PT_DEV void quad_order(")
        assert text.count("9.5367431640625e-7f") == 1, "quad_order's slack constant is not where the test looks for it"
        open(os.path.join(d, "slack_kernel_fns.inc"), "w").write(text.replace("9.5367431640625e-7f", "PT_TEST_KSL"))
        exe = os.path.join(d, "slack_host")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas", "-I", d, f"-DPT_TEST_KSL={ksl}",
                        os.path.join(ROOT, "tools", "slack_host.cpp"), "-o", exe], check=True)
        return exe
    return _cached(("slack_host", ksl), make)


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes and searched sets, each made once
# ---------------------------------------------------------------------------------------------------------------------------------
class World:
    def __init__(self, name):
        self.name = name
        if name == "attribute":
            self.prims, groups = U.attribute_scene(ATTR_SEED, 12)
        elif name == "needle":
            self.prims = U.needle_scene(U.NEEDLE_SEED, 512)[0]
        else:
            self.prims = P.placed_prims(P.home_scene(mixed=(name == "mixed")), *P.placement(name))[0]
        self.nodes, self.tris, _ = ptamd.build_bvh(self.prims)
        self.pos = R.positions(self.tris).astype(np.float64)
        self.kappa = S.condition_number(self.pos)
        if name == "attribute":
            t2i = U.attr_tri_to_input(self.prims, self.tris)
            self.thin = np.nonzero(np.isin(t2i, groups["slivers"]))[0]
            assert len(self.thin) == 30 and (self.kappa[self.thin] > 1000).all()
        elif name == "needle":
            self.thin = np.nonzero(self.kappa > 100)[0]
            assert len(self.thin) == 512
        self.sel = {}
        if name == "attribute":
            self.sel = {"slivers": np.isin(t2i, groups["slivers"]), "mesh": np.isin(t2i, groups["mesh"])}
        elif name == "home":
            scene = P.home_scene()
            placed = P.placed_prims(scene, *P.placement(name))[1]
            self.sel = {"mesh": scene["group"][P.tri_to_input(self.tris, placed)] == P.GROUPS.index("mesh")}
        self.trees = host_trees(self.prims, name)
        assert self.trees.n == len(self.tris)
        O.set_libm(1)
        self.oracle = O.Scene(self.nodes.tobytes(), self.tris)

    def candidates(self, kind, rs, n, lo, hi):
        if kind == "sliver":
            return S.sliver_rays(rs, n, self.pos, self.thin, lo, hi)[0]
        boxes = self.trees.leaf_child_boxes()
        if kind == "corner":
            return S.corner_rays(rs, n, boxes, lo, hi)
        diag = np.sqrt(((self.pos.max(1) - self.pos.min(1)) ** 2).sum(1))
        small = np.nonzero(diag < 0.1)[0]
        assert len(small) == 64
        centre = 0.5 * (boxes[:, 0:3] + boxes[:, 3:6])
        near = (np.abs(centre - np.array(P.CLUSTER_CENTRE)) < 1.5).all(1)      # the boxes are at least 2 wide: maxabs * 2^-20 = 1 on each side
        assert near.sum() >= 16
        return S.cluster_rays(rs, n, self.pos, small, boxes[near], lo, hi)


def world(name):
    return _cached(("world", name), lambda: World(name))


class Family:
    """The census of one family and the sets it keeps."""

    def __init__(self, name):
        scene, kind, seed, lo, hi = FAMILIES[name]
        self.name, self.w = name, world(scene)
        w, T = self.w, self.w.trees
        rs = np.random.RandomState(seed)
        n_hit, prims_hit, self.hist = 0, set(), {}
        keep, control = [], None
        for _ in range(N_CAND // CHUNK):
            rays = w.candidates(kind, rs, CHUNK, lo, hi)
            hits, prim, _ = w.oracle.raycast(rays)
            sel = (prim >= 0) & ~S.ray_setup(rays[:, 3:6])[2]
            r, p, t = rays[sel], prim[sel].astype(np.int64), hits[sel, 1]
            n_hit += len(r)
            prims_hit.update(np.unique(p).tolist())
            need = S.needed_slack(T, r, p, t)
            binary = S.binary_chain_accepts(T, r, p, t)
            if control is None:
                ok = np.nonzero((need <= F(S.K_SL)) & binary)[0]
                pick = ok[np.random.RandomState(seed + 1).permutation(len(ok))[:KEEP]]
                control = (r[pick], p[pick], t[pick], need[pick])
            m = (need > 0) | ~binary
            keep.append((r[m], p[m], t[m], need[m], binary[m]))
        r, p, t, need, binary = (np.concatenate(x) for x in zip(*keep))
        self.n_hit, self.prims_hit = n_hit, len(prims_hit)
        miss_q, miss_b = need > F(S.K_SL), ~binary
        self.miss = {"quad": (r[miss_q], p[miss_q], t[miss_q]), "binary": (r[miss_b], p[miss_b], t[miss_b])}
        far = np.full(len(r), 999999.0, F)      # no cull: refused by the slabs alone, whatever the order of the walk
        self.definite = {"quad": ~S.quad_chain_accepts(T, r[miss_q], p[miss_q], far[miss_q]), "binary": ~S.binary_chain_accepts(T, r[miss_b], p[miss_b], far[miss_b])}
        self.need_all = need
        good = np.nonzero(~miss_q & ~miss_b)[0]
        self.needy = (r[good], p[good], t[good], need[good])      # every ray that needs some slack and no more than is shipped
        # the same rays with no cull at all: what the slabs alone need, whatever the order of the walk and the device's cull scale
        self.need_slab = S.needed_slack(T, r[good], p[good], far[good])
        top = good[np.argsort(-need[good], kind="stable")[:KEEP]]
        self.kept = (r[top], p[top], t[top], need[top])
        self.control = control
        if len(top) < KEEP:      # fewer than 256 rays need any slack: filled up with rays that need none, from the control's pool
            fill = KEEP - len(top)
            self.kept = tuple(np.concatenate([a, b[:fill]]) for a, b in zip(self.kept, control))

    def rays(self):
        return {"kept": self.kept[0], "control": self.control[0]}

    def report(self):
        need = self.need_all
        fin = need[np.isfinite(need) & (need > 0)]
        e, c = np.unique(np.floor(np.log2(fin.astype(np.float64))).astype(int), return_counts=True) if len(fin) else ((), ())
        mx = float(need.max()) if len(need) else 0.0
        kmx = float(self.kept[3].max())
        return (f"{self.name}: {N_CAND} candidates, oracle hits {self.n_hit / N_CAND:.3f}, primitives hit {self.prims_hit}, rays that need slack {len(fin)}, "
                f"log2 needed slack {dict(zip((int(x) for x in e), (int(x) for x in c)))}, maximum {mx:.3e} (headroom 2^-20 / max {S.K_SL / mx if mx else np.inf:.3g}); "
                f"of the rays within the shipped slack, by the slabs alone (no cull): {int((self.need_slab > 0).sum())} need slack, maximum {float(self.need_slab.max()) if len(self.need_slab) else 0.0:.3e} "
                f"(headroom {S.K_SL / float(self.need_slab.max()) if len(self.need_slab) and self.need_slab.max() > 0 else np.inf:.3g}); "
                f"kept: {int((self.kept[3] > 0).sum())} of {KEEP} need slack, maximum {kmx:.3e} (headroom {S.K_SL / kmx if kmx else np.inf:.3g}); "
                f"MISS 4-wide {len(self.miss['quad'][0])} ({int(self.definite['quad'].sum())} by the slabs alone), binary {len(self.miss['binary'][0])} ({int(self.definite['binary'].sum())}); "
                f"kappa of the MISS primitives {_kappa_range(self.w, self.miss['quad'][1])}")


def _kappa_range(w, prim):
    if not len(prim):
        return "-"
    k = w.kappa[np.unique(prim)]
    return f"{k.min():.3g} .. {k.max():.3g} ({len(k)} primitives)"


def family(name):
    return _cached(("family", name), lambda: Family(name))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
def test_dump_accel_reads_primitive_records():
    """--prims gives the arrays of the procedural scene's own records, and refuses a file that is no whole number of records."""
    d = _tools()
    prims = ptamd.gen_scene(1, 16)
    host_trees(prims, "gen")
    subprocess.run([os.path.join(d, "dump_accel"), "1", "16", os.path.join(d, "kind")], check=True,
                   env={k: v for k, v in os.environ.items() if k not in ("PTAMD_TREE", "PTAMD_LEAF", "PTAMD_BFS")})
    for k in ("wide", "quad", "tri", "tripair", "leafbox"):
        assert open(os.path.join(d, f"gen.{k}.bin"), "rb").read() == open(os.path.join(d, f"kind.{k}.bin"), "rb").read(), k
    bad = os.path.join(d, "bad.prims")
    open(bad, "wb").write(b"\0" * 337)
    assert subprocess.run([os.path.join(d, "dump_accel"), "--prims", bad, os.path.join(d, "bad")], stderr=subprocess.DEVNULL).returncode == 1


@pytest.mark.parametrize("ksl", ["9.5367431640625e-7f", "4.76837158203125e-7f", "0.f"])
def test_the_models_restate_the_kernels_code(ksl, tmp_path):
    """quad_child_accepts and binary_child_accepts against quad_order and box_test compiled for the host, on 10^5 (node, ray) pairs: rays
    of the far families against the nodes of their own chains (grazing: the near and far sides meet within the slack) and against
    random nodes.  Every key of quad_order (the entry distance's bits or kQuadMiss) with its child ref, both verdicts and entry
    distances of box_test."""
    slack = float(ksl.rstrip("f"))
    n = 100_000
    rs = np.random.RandomState(11)
    parts = []
    for name, share in (("attribute", 0.4), ("needle", 0.3), ("mixed", 0.3)):
        w = world(name)
        T = w.trees
        m = int(n * share)
        kind = {"attribute": "sliver", "needle": "corner", "mixed": "cluster"}[name]
        rays = w.candidates(kind, rs, m, 4.0 if name == "attribute" else 2.0 ** 12, 2.0 ** 19.5)
        hits, prim, _ = w.oracle.raycast(rays)
        inv, cscale, deg = S.ray_setup(rays[:, 3:6])
        p = np.where(prim >= 0, prim, rs.randint(0, T.n, m)).astype(np.int64)
        qn, qs, ql = T.quad_chain
        bn, _, bl = T.bin_chain
        lvl = rs.randint(0, 64, m)
        own = rs.uniform(0, 1, m) < 0.7
        node_q = np.where(own, qn[p, lvl % ql[p]], rs.randint(0, len(T.quad), m))
        node_b = np.where(own, bn[p, lvl % bl[p]], rs.randint(0, len(T.nodes), m))
        t = np.where(prim >= 0, hits[:, 1], F(999999.0)).astype(F)
        cull = np.where(rs.uniform(0, 1, m) < 0.5, t * cscale, F(np.inf)).astype(F)
        ok = ~deg
        parts.append((T, node_q[ok], node_b[ok], rays[ok, 0:3], inv[ok], cull[ok]))
    total = 0
    for k, (T, node_q, node_b, org, inv, cull) in enumerate(parts):
        m = len(org)
        total += m
        query = np.zeros((m, 9), np.uint32)
        query[:, 0], query[:, 1] = node_q, node_b
        query[:, 2:5], query[:, 5:8], query[:, 8] = bits(org), bits(inv), bits(cull)
        src, dst = str(tmp_path / f"in{k}.bin"), str(tmp_path / f"out{k}.bin")
        with open(src, "wb") as f:
            f.write(np.array([len(T.quad), len(T.nodes), m], np.int32).tobytes() + T.quad.tobytes() + T.nodes.tobytes() + query.tobytes())
        subprocess.run([slack_host(ksl), src, dst], check=True)
        out = np.fromfile(dst, np.uint32).reshape(m, 12)
        key = np.zeros((m, 4), np.int64)
        for c in range(4):
            acc, tn = S.quad_child_accepts(T.quad, node_q, c, org, inv, cull, slack)
            key[:, c] = np.where(acc, bits(tn).astype(np.int64), 0x7fffffff)
        ref = T.quad[node_q, 4:8].view(np.int32).astype(np.int64)
        want = np.sort(key * (1 << 32) + (ref & 0xffffffff), 1)
        got = np.sort(out[:, 0:4].astype(np.int64) * (1 << 32) + out[:, 4:8].astype(np.int64), 1)
        bad = (want != got).any(1)
        assert not bad.any(), f"quad_order, slack {slack}: {bad.sum()} of {m} (node, ray) pairs differ, first at {np.nonzero(bad)[0][:5]}"
        assert (np.diff(out[:, 0:4].astype(np.int64), axis=1) >= 0).all()
        print(f"part {k}: {m} pairs, children accepted {np.mean(key != 0x7fffffff):.3f}, nodes with an accepted and a refused child {np.mean((key != 0x7fffffff).any(1) & (key == 0x7fffffff).any(1)):.3f}")
        for side in (0, 1):
            acc, tn = S.binary_child_accepts(T.nodes, node_b, side, org, inv, cull)
            same = (out[:, 8 + 2 * side] == acc) & ((out[:, 9 + 2 * side] == bits(tn)) | np.isnan(tn))
            assert same.all(), f"box_test, side {side}: {(~same).sum()} of {m} differ, first at {np.nonzero(~same)[0][:5]}"
    assert total >= 0.99 * n


def test_fma32_rounds_once():
    """fma32 against exact rational arithmetic, on sums built to fall on and beside float32 ties."""
    from fractions import Fraction
    rs = np.random.RandomState(5)
    n = 3000
    a = rs.randint(0, 256, n).astype(F)
    b = (rs.standard_normal(n) * 2.0 ** rs.randint(-20, 20, n)).astype(F)
    c = (rs.standard_normal(n) * 2.0 ** rs.randint(-20, 20, n)).astype(F)
    # a third: c chosen so that a * b + c is within a few float64 steps of a float32 tie
    r = (a.astype(np.float64) * b + c).astype(F)
    tie = 0.5 * (r.astype(np.float64) + np.nextafter(r, F(np.inf)).astype(np.float64))
    c[::3] = (tie - a.astype(np.float64) * b)[::3].astype(F)
    got = S.fma32(a, b, c)
    for i in range(n):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = F(float(exact))                                  # float() of a Fraction rounds once to float64; search from there
        cand = [np.nextafter(lo, F(-np.inf)), lo, np.nextafter(lo, F(np.inf))]
        err = [abs(Fraction(float(x)) - exact) for x in cand]
        best = min(err)
        winners = [x for x, e in zip(cand, err) if e == best]
        want = winners[0] if len(winners) == 1 else [x for x in winners if (int(np.array(x, F).view(np.uint32)) & 1) == 0][0]
        assert bits(got[i:i + 1])[0] == bits(np.array([want], F))[0], (i, a[i], b[i], c[i], got[i], want)


def test_the_oracles_ray_render_is_its_camera_render():
    """oracle_lib.Scene.render_rays, the yardstick of test_kept_rays_render_is_the_oracles: along the rays of a camera's pixels (direction of
    o_pixel_dir, seed py * W + px, stride W * H) it is the oracle's own frame, bit for bit, pass by pass."""
    nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, 12))
    O.set_libm(1)
    so = O.Scene(nodes.tobytes(), tris)
    W, H = 16, 12
    cam = O.make_camera(W, H)
    py, px = np.divmod(np.arange(W * H, dtype=np.int32), np.int32(W))
    for ps in (0, 2):
        rays = np.zeros((W * H, 8), F)
        rays[:, 0:3], rays[:, 7] = np.float32((0.0, 20.0, 60.0)), 999999.0
        rays[:, 3:6] = O.pixel_dir(cam, np.stack([px, py, np.full(W * H, ps, np.int32)], 1))[:, 2:5]
        ref, _ = so.render(cam, O.make_params(W, H, 1, 4, first_pass=ps), 4)
        got = so.render_rays(rays, O.make_params(W, H, 1, 4, first_pass=ps), (py * W + px).astype(np.int32), W * H)
        assert (ref > 0).mean() > 0.5 and np.array_equal(bits(got).reshape(H, W, 3), bits(ref)), ps


@pytest.mark.parametrize("name", list(FAMILIES))
def test_restated_acceptance_is_the_oracles(name):
    """Triangle::hit and the leaf-box test as slack_ref restates them, over ALL triangles with no tree: the oracle's closest hit, bit
    for bit, on the kept, control and MISS rays.  (What walk_result restricts to the accepted chains is this.)"""
    f = family(name)
    T = f.w.trees
    rays = np.concatenate([f.kept[0], f.control[0], f.miss["quad"][0][:512], f.miss["binary"][0][:512]])
    hits, prim, _ = f.w.oracle.raycast(rays)
    ok, t = S.tri_accepts(T, rays)
    gt, gp = S.closest_among(T, ok, t)
    hit = prim >= 0
    assert np.array_equal(gp, prim), f"{name}: {(gp != prim).sum()} prims differ"
    assert np.array_equal(bits(gt[hit]), bits(hits[hit, 1]))


@pytest.mark.parametrize("name", list(FAMILIES))
def test_census(name):
    f = family(name)
    print(f.report())
    r, p, t, need = f.kept
    # holds by construction (the kept rays are chosen among those the chains accept): a check of the selection, not of the kernel.  What the
    # kernel's soundness rests on are the MISS sets below, and they are not empty.
    assert (need <= F(S.K_SL)).all() and S.quad_chain_accepts(f.w.trees, r, p, t).all() and S.binary_chain_accepts(f.w.trees, r, p, t).all()
    assert (f.control[3] <= F(S.K_SL)).all()
    assert len(r) == KEEP and len(f.control[0]) == KEEP
    # the family is adversarial: a library with no slack at all refuses at least FLOOR of its kept rays
    if name in BELOW_FLOOR:
        assert (need > 0).sum() == BELOW_FLOOR[name] < FLOOR, f"{name}: {(need > 0).sum()} kept rays need slack"
    else:
        assert (need > 0).sum() >= FLOOR, f"{name}: only {(need > 0).sum()} kept rays need any slack"
    # the documented limit, pinned
    for walk, (mr, mp, mt) in f.miss.items():
        hits, prim, _ = f.w.oracle.raycast(mr)
        assert np.array_equal(prim, mp) and np.array_equal(bits(hits[:, 1]), bits(mt))
    refused = ~S.quad_chain_accepts(f.w.trees, *f.miss["quad"])
    assert refused.all()
    got = (len(f.miss["quad"][0]), len(f.miss["binary"][0]), int(f.definite["quad"].sum()), int(f.definite["binary"].sum()))
    assert got == MISS_SIZES[name], f"{name}: MISS sets {got}"


# ---------------------------------------------------------------------------------------------------------------------------------
# the shadow ray's early stop: veils in front of the light
# ---------------------------------------------------------------------------------------------------------------------------------
VEIL_PLACEMENTS = {"home": ((1.0, 1.0, 1.0), (0.0, 0.0, 0.0)), "far12": P.PLACEMENTS["far12"], "far17": P.PLACEMENTS["far17"],
                   "x100": ((100.0, 100.0, 100.0), (0.0, 0.0, 0.0))}
VEIL_SEED, VEIL_W, VEIL_H, VEIL_PASSES, VEIL_SPP = 4401, 32, 24, 2, 4
# lit rows that need more than half of EPS, where a placement does not reach 32 of them (asserted as found): from far12 on a float32
# step of the light's height (2^-11 and more) is above every veil distance, the veils fall onto the light's plane or a whole step below
# it, and a lit row's closest hit is at the light point itself
VEIL_BELOW_FLOOR = {}


class Veil:
    def __init__(self, name):
        self.name = name
        self.D, self.t = (np.array(x, np.float64) for x in VEIL_PLACEMENTS[name])
        self.prims, self.centres = S.veil_scene(self.D, self.t, U.make_prims, U._cornell_walls())
        self.nodes, self.tris, _ = ptamd.build_bvh(self.prims)
        O.set_libm(1)
        self.oracle = O.Scene(self.nodes.tobytes(), self.tris)
        self.rows = S.veil_rows(np.random.RandomState(VEIL_SEED), self.centres, self.D, self.t)
        self.nee = self.oracle.nee(self.rows)
        self.lit = (self.nee[:, 8:11] != 0).any(1)
        self.ray = S.shadow_ray(self.rows[:, 0:3], self.nee[:, 1:4])
        self.hits, self.prim, _ = self.oracle.raycast(self.ray)
        self.need = S.shadow_needed_margin(self.rows[:, 0:3], self.nee[:, 1:4], self.nee[:, 6], self.hits[:, 1], self.lit)
        self.margin = S.shadow_stop_margin(self.rows[:, 0:3], self.nee[:, 6])

    def camera_pos(self):
        return P.map_camera_pos(self.D, self.t)

    def frame(self):
        def make():
            ref, _ = self.oracle.render(O.make_camera(VEIL_W, VEIL_H, pos=self.camera_pos()), O.make_params(VEIL_W, VEIL_H, VEIL_PASSES, VEIL_SPP), 8)
            return ref
        return _cached(("veil frame", self.name), make)


def veil(name):
    return _cached(("veil", name), lambda: Veil(name))


@pytest.mark.parametrize("name", list(VEIL_PLACEMENTS))
def test_shadow_margin_covers_every_lit_row(name):
    v = veil(name)
    n = len(v.rows)
    # the restated shadow ray is GetLightColor's: its t_max, its closest primitive and its verdict are o_nee's
    assert np.array_equal(bits(v.ray[:, 7]), bits(v.nee[:, 6])) and np.array_equal(v.prim, v.nee[:, 7].view(np.int32))
    with np.errstate(invalid="ignore"):
        hp = v.hits[:, 5:8] - v.nee[:, 1:4]
        near = (v.prim >= 0) & (np.sqrt((hp[:, 0] * hp[:, 0] + hp[:, 1] * hp[:, 1]) + hp[:, 2] * hp[:, 2]) < S.EPS)
    emissive = np.zeros(n, bool)
    emissive[v.prim >= 0] = R.emissive(v.tris)[v.prim[v.prim >= 0]]
    assert np.array_equal(v.lit, near & emissive), f"{name}: {(v.lit != (near & emissive)).sum()} verdicts are not the restated ray's"
    veil_tri = (R.emissive(v.tris)) & (np.abs(v.tris[:, 54:57] - 15.0) > 0.5).any(1)      # mat0's emittance is not the light's
    lit_by_veil = v.lit & veil_tri[np.maximum(v.prim, 0)]
    need, margin = v.need[v.lit], v.margin[v.lit]
    big = int((need > 0.5 * float(S.EPS)).sum())
    print(f"{name}: {n} rows, lit {v.lit.mean():.3f}, lit through a veil {lit_by_veil.mean():.3f}; needed margin of the lit rows: maximum {need.max():.3e}, "
          f"above EPS / 2 on {big}; shipped margin {margin.min():.3e} .. {margin.max():.3e}, headroom (least margin / need) {(margin / np.maximum(need, 1e-30)).min():.3g}")
    assert v.lit.sum() >= 500
    assert (need < margin).all(), f"{name}: {(need >= margin).sum()} lit rows need more than the shipped margin"
    if name in VEIL_BELOW_FLOOR:
        assert big == VEIL_BELOW_FLOOR[name] < 32
    else:
        assert big >= 32, f"{name}: only {big} lit rows need more than EPS / 2"


def test_veils_from_1_1_eps_on_are_dark_at_normal_incidence():
    """home: a point straight under a light point that lies under a veil at 1.1 EPS or more sees the veil 1.1 EPS in front of the
    light point: dark; under the veils at 0.25, 0.5 and 0.9 EPS it is lit with the veil's own emittance."""
    v = veil("home")
    P_ = v.nee[:, 1:4]
    p = P_.copy()
    p[:, 1] = P_[:, 1] - F(10.0)
    rows = np.ascontiguousarray(np.concatenate([p, v.rows[:, 3:5]], 1), F)
    out = v.oracle.nee(rows)
    assert np.array_equal(bits(out[:, 1:4]), bits(P_))      # the same seeds draw the same light points
    strip = np.clip(np.floor((P_[:, 0].astype(np.float64) + S.VEIL_HALF) * 7.0 / (2 * S.VEIL_HALF)).astype(int), 0, 6)
    on_light = P_[:, 1] == F(S.VEIL_LIGHT_Y)
    inner = on_light & (np.abs((P_[:, 0].astype(np.float64) + S.VEIL_HALF) * 7.0 / (2 * S.VEIL_HALF) - strip - 0.5) < 0.49)
    lit = (out[:, 8:11] != 0).any(1)
    assert inner.sum() >= 1000
    for k in range(7):
        m = inner & (strip == k)
        assert m.sum() >= 50
        if S.VEIL_DISTANCES[k] >= 1.1e-4:
            assert not lit[m].any(), f"veil {k}: {lit[m].sum()} rows lit"
        else:
            assert lit[m].all() and (out[m, 8:11] == np.array(S.veil_emittance(k), F)).all(), f"veil {k}"


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    O.set_libm(1)
    yield


def _scene(w, walk):
    import test_placement as Tp
    return Tp._scene(w.nodes, w.tris, walk)


def _device_trees(sc):
    return S.Trees(sc.dbg_array("nodes"), sc.dbg_array("quad"), sc.dbg_array("tri"), sc.dbg_array("leafbox"))


class _Set:
    """What test_placement.check_rays asks of a world: the ray sets and the oracle's answers."""

    def __init__(self, f):
        self.f, self.tris, self.oracle_sees = f, f.w.tris, True

    def rays(self):
        return self.f.rays()

    def want_rays(self):
        return _cached(("want", self.f.name), lambda: {k: self.f.w.oracle.raycast(r)[:2] for k, r in self.f.rays().items()})


@pytest.mark.gpu
def test_ray_setup_is_the_models(_gpu):
    """pt_dbg_ray_setup: the device's Normalize(inv(dir)) has the model's bits, and its cull scale is never below the model's worst case."""
    d = np.concatenate([family(n).kept[0][:, 3:6] for n in FAMILIES] + [family(n).control[0][:, 3:6] for n in FAMILIES])
    got = ptamd.dbg_ray_setup(d)
    inv, cscale, deg = S.ray_setup(d)
    assert not deg.any() and (got[:, 4] == 0).all()
    assert np.array_equal(bits(got[:, 0:3]), bits(inv))
    assert (got[:, 3] >= cscale).all(), f"{(got[:, 3] < cscale).sum()} cull scales below the model's worst case"
    near = S.ray_setup(d, worst_rcp=False)[1]
    print(f"cull scale: device / model's worst case {np.max(got[:, 3] / cscale):.9f} at most, equal to 1 / L rounded to nearest on {np.mean(got[:, 3] == near):.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("walk", ["quad", "binary"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_kept_rays_are_the_oracles(_gpu, name, walk):
    """The 256 rays of a family that need the most slack, and its 256 control rays: the chains of the DOWNLOADED trees accept them at
    2^-20, then pt_dbg_raycast, pt_trace_rays (closest hit with surface records, any hit) and pt_aov_rays (wf_trace) give the oracle's bits."""
    import test_placement as Tp
    f = family(name)
    sc = _scene(f.w, walk)
    T = _device_trees(sc)
    for which, (r, p, t, _) in (("kept", f.kept), ("control", f.control)):
        need = S.needed_slack(T, r, p, t)
        assert (need <= F(S.K_SL)).all() and S.binary_chain_accepts(T, r, p, t).all(), f"{name}, {which}: the uploaded trees are not the host's"
    Tp.check_rays(sc, _Set(f), f"{name}, {walk} walk")
    for which, rays in f.rays().items():
        hits_o, prim_o = _Set(f).want_rays()[which]
        aov, prim = sc.aov_rays(rays)
        assert np.array_equal(prim, prim_o), f"{name}, {which}: pt_aov_rays differs from the oracle on {(prim != prim_o).sum()} rays"
        assert np.array_equal(bits(aov[:, 6]), bits(np.where(prim_o >= 0, hits_o[:, 1], F(0)))), f"{name}, {which}: pt_aov_rays' t"


def _assert_bracketed(sc, T, r, walk, what):
    """pt_trace_rays' closest hit of rays r on scene sc, whose downloaded trees are T, against slack_ref.walk_result: the answer is an
    accepted triangle whose chain passes with no cull, with that triangle's own t; no farther than the closest hit the walk is bound to
    test, no closer than the closest it can reach (equal t: the tie rule); where both agree, exactly that hit.  Returns (t, prim, model)."""
    m = S.walk_result(T, r, walk)
    (t_lo, p_lo), (t_hi, p_hi) = m["lo"], m["hi"]
    sure = (p_lo == p_hi) & (bits(t_lo) == bits(t_hi))
    gt, gp = sc.trace_rays(r)
    col = np.argsort(T.prim_of)[np.maximum(gp, 0)]
    row = np.arange(len(r))
    hit = gp >= 0
    member = m["a_hi"][row, col] & (bits(m["t"][row, col]) == bits(gt))
    assert member[hit].all(), f"{what}: {(~member[hit]).sum()} answers are no triangle the chains can reach, first at {np.nonzero(hit & ~member)[0][:5]}"
    assert (gt[~hit] == 0).all() and not m["a_lo"][~hit].any(), f"{what}: a ray returns nothing although the chains are bound to find a hit"
    lo_hit = p_lo >= 0
    assert ((gt < t_lo) | ((gt == t_lo) & (gp >= p_lo)))[lo_hit & hit].all() and hit[lo_hit].all(), f"{what}: farther than a hit the walk is bound to find"
    assert ((gt > t_hi) | ((gt == t_hi) & (gp <= p_hi)))[hit].all(), f"{what}: closer than anything the chains can reach"
    bad = sure & ((gp != p_lo) | (bits(gt) != bits(t_lo)))
    assert not bad.any(), f"{what}: {bad.sum()} of the {sure.sum()} rays the chains decide do not return what they leave, first at {np.nonzero(bad)[0][:5]}"
    return gt, gp, m


def _check_on_trees(sc, rays, hits_o, prim_o, walk, what):
    """Every query on scene sc against the oracle's answers (hits_o, prim_o) for `rays`, judged by the chains of the trees as DOWNLOADED
    from sc now.  A ray whose oracle hit has a chain that accepts it at the shipped constants (needed_slack <= 2^-20 on the 4-wide tree,
    box_test on the binary one; a ray the oracle misses has nothing to refuse) must give the oracle's bits: pt_trace_rays closest hit with
    surface records and any hit on the scene's own walk, pt_dbg_raycast (it walks the binary tree) where the binary chain accepts,
    pt_aov_rays where both do.  The others are this tree's MISS rays: _assert_bracketed.  Returns how many the 4-wide and the binary
    chains refuse, which the callers pin."""
    T = _device_trees(sc)
    hit = prim_o >= 0
    p, t = np.maximum(prim_o, 0).astype(np.int64), hits_o[:, 1]
    acc_q = ~hit | (S.needed_slack(T, rays, p, t) <= F(S.K_SL))
    acc_b = ~hit | S.binary_chain_accepts(T, rays, p, t)
    own = acc_q if walk == "quad" else acc_b
    gt, gp, surf = sc.trace_rays(rays, surface=True)
    Tq._assert_closest((gt[own], gp[own], surf[own]), hits_o[own], prim_o[own], f"{what}, closest hit")
    at, ap = sc.trace_rays(rays, any_hit=True)
    Tq._assert_any(at[own], ap[own], gt[own], gp[own], rays[own], len(T.tri), f"{what}, any hit")
    hits, prim = sc.raycast(rays)
    bad = acc_b & ((prim != prim_o) | ~Tq.same_bits_or_nan(hits, hits_o).all(1))
    assert not bad.any(), f"{what}: pt_dbg_raycast differs from the oracle on {bad.sum()} rays its chain accepts, first at {np.nonzero(bad)[0][:5]}"
    both = acc_q & acc_b
    aov, aprim = sc.aov_rays(rays)
    assert np.array_equal(aprim[both], prim_o[both]) and np.array_equal(bits(aov[both, 6]), bits(np.where(hit, t, F(0))[both])), f"{what}: pt_aov_rays"
    if (~own).any():
        _assert_bracketed(sc, T, rays[~own], walk, f"{what}, the rays this tree refuses")
    return int((~acc_q).sum()), int((~acc_b).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FAMILIES))
def test_kept_rays_render_is_the_oracles(_gpu, name):
    """pt_render_rays with one bounce along the kept and control rays, their directions made unit vectors: wf_trace with the pipeline to
    the end, and wf_drain from the first poll, against the oracle's render of the same rays (oracle_lib.Scene.render_rays: ray i in the
    place of a pixel), bit for bit.  A normalised direction is another ray: the chains are asked again, and a ray they refuse is left out."""
    f = family(name)
    rays = _kept_and_control(f).copy()
    d = rays[:, 3:6]
    rays[:, 3:6] = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    hits_o, prim_o, _ = f.w.oracle.raycast(rays)
    sc = _scene(f.w, "quad")
    T = _device_trees(sc)
    hit = prim_o >= 0
    p, t = np.maximum(prim_o, 0).astype(np.int64), hits_o[:, 1]
    ok = ~hit | ((S.needed_slack(T, rays, p, t) <= F(S.K_SL)) & S.binary_chain_accepts(T, rays, p, t))
    assert ok.sum() >= 0.9 * len(rays), f"{name}: only {ok.sum()} of the normalised rays pass their chains"
    rays = np.ascontiguousarray(rays[ok])
    want = f.w.oracle.render_rays(rays, O.make_params(len(rays), 1, passes=1, spp=4, max_bounce=1))
    assert np.isfinite(want).all() and (want > 0).any(1).mean() >= 0.05, f"{name}: the oracle's render is dark"
    prm = ptamd.default_params(passes=1, spp_per_pass=4, max_bounce=1)
    try:
        for drain, which in ((0, "the pipeline to the end"), (1 << 30, "wf_drain from the first poll")):
            sc.set_drain_threshold(drain)
            got = sc.render_rays(rays, prm)
            same = (bits(got) == bits(want)).all(1)
            assert same.all(), f"{name}, {which}: {(~same).sum()} of {len(rays)} rays differ from the oracle's render, first at {np.nonzero(~same)[0][:5]}"
    finally:
        sc.set_drain_threshold(80000)
    print(f"{name}: {len(rays)} rays rendered, {(want > 0).any(1).mean():.3f} of them not black")


REBUILDS = {"rebuild_tree": lambda sc: sc.rebuild_tree(), "rebuild_tree_26_16": lambda sc: sc.rebuild_tree(depth_budget=26, large_fraction=1.0 / 16.0),
            "rebuild_tree_optimized_1": lambda sc: sc.rebuild_tree_optimized(1)}
# Of the 512 kept and control rays of a family (all accepted by the uploaded trees): how many the 4-wide and the binary chains of the
# REBUILT trees refuse, after each of REBUILDS in turn.  A rebuilt tree has other boxes and so other MISS rays; pinned.
REBUILD_MISS = {"a_attribute": ((0, 0),) * 3, "a_needle": ((4, 0),) * 3, "b_attribute": ((77, 115), (83, 115), (101, 115)),
                "b_needle": ((56, 14), (56, 14), (59, 14)), "c_home": ((0, 0),) * 3, "c_attribute": ((0, 0),) * 3, "d_mixed": ((0, 0),) * 3}
# The same after a refit: (family, what moved) -> the kept and control rays that the refit trees' chains refuse for the oracle's hit on
# the MOVED scene.
REFIT_MISS = {}      # filled below: no refit tree refuses a kept or control ray


def _kept_and_control(f):
    return np.concatenate([f.kept[0], f.control[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("walk", ["quad", "binary"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_kept_rays_after_each_rebuild(_gpu, name, walk):
    """The kept and control rays after pt_scene_rebuild_tree, its budgeted form (26, 1/16) and one treelet pass, on both walks: every
    query gives the oracle's bits wherever the chains of the rebuilt trees accept the ray at 2^-20, and the rays they refuse - a rebuilt
    tree has its own MISS rays - are counted, pinned and held to what those chains leave."""
    f = family(name)
    rays = _kept_and_control(f)
    hits_o, prim_o, _ = f.w.oracle.raycast(rays)
    sc = _scene(f.w, walk)
    got = []
    for which, rebuild in REBUILDS.items():
        rebuild(sc)
        got.append(_check_on_trees(sc, rays, hits_o, prim_o, walk, f"{name}, {walk} walk after {which}"))
    print(f"REBUILD_MISS {name!r}: {tuple(got)}")
    assert tuple(got) == REBUILD_MISS[name], f"{name}: the rebuilt trees refuse {got}"


REFITS = [("a_attribute", "slivers"), ("a_attribute", "mesh"), ("b_attribute", "slivers"), ("b_attribute", "mesh"), ("c_attribute", "slivers"),
          ("c_attribute", "mesh"), ("c_home", "mesh")]


REFIT_MISS.update({case: (0, 0) for case in REFITS})


def moved(wname, what):
    """(positions (n, 9) float32 after dynamic_ref.move_rigid_wobble of the selected triangles, the oracle of the moved scene)."""
    def make():
        w = world(wname)
        pos = R.move_rigid_wobble(R.positions(w.tris), w.sel[what], np)
        pos = np.ascontiguousarray(pos, F).reshape(-1, 9)
        tris2 = R.restate_tris(w.tris, pos)
        O.set_libm(1)
        return pos, O.Scene(R.refit_nodes(w.nodes, tris2).tobytes(), tris2)
    return _cached(("moved", wname, what), make)


@pytest.mark.gpu
@pytest.mark.parametrize("walk", ["quad", "binary"])
@pytest.mark.parametrize("name,what", REFITS)
def test_kept_rays_after_a_refit(_gpu, name, what, walk):
    """pt_scene_update_vertices with dynamic_ref.move_rigid_wobble of the slivers, and of the mesh: the refit in csrc/pt_dynamic.hip makes the
    leaf bounds anew.  The kept and control rays against the oracle ON THE MOVED SCENE, judged by the chains of the refit trees as
    downloaded, on both walks, as test_kept_rays_after_each_rebuild judges them."""
    f = family(name)
    pos, oracle = moved(FAMILIES[name][0], what)
    rays = _kept_and_control(f)
    hits_o, prim_o, _ = oracle.raycast(rays)
    sc = _scene(f.w, walk)
    sc.update_vertices(pos)
    got = _check_on_trees(sc, rays, hits_o, prim_o, walk, f"{name}, {what} moved, {walk} walk")
    print(f"REFIT_MISS {(name, what)!r}: {got}, the oracle hits {(prim_o >= 0).sum()} of {len(rays)}")
    assert got == REFIT_MISS[(name, what)], f"{name}, {what} moved: the refit trees refuse {got}"


@pytest.mark.gpu
@pytest.mark.parametrize("walk", ["quad", "binary"])
@pytest.mark.parametrize("name", list(FAMILIES))
def test_miss_rays_return_what_the_chains_leave(_gpu, name, walk):
    """The documented limit: a MISS ray's oracle hit lies behind a box that refuses the ray, so the walk cannot
    return it.  What it must return is exactly the closest hit among the accepted triangles whose chain the model accepts: the
    restated Triangle::hit and leaf-box test, restricted to those (slack_ref.walk_result)."""
    f = family(name)
    r, p, t = (x[:1024] for x in f.miss[walk])
    assert len(r) > 0      # MISS_SIZES pins every set non-empty
    sc = _scene(f.w, walk)
    T = _device_trees(sc)
    gt, gp, m = _assert_bracketed(sc, T, r, walk, f"{name}, {walk} walk")
    p_hi = m["hi"][1]
    definite = p_hi != p                       # refused by the slabs alone: no order of the walk reaches the oracle's triangle
    assert np.array_equal(definite, f.definite[walk][:1024]), f"{name}, {walk} walk: the uploaded trees are not the host's"
    print(f"{name}, {walk} walk: {len(r)} MISS rays, {definite.sum()} refused by the slabs alone; the device returns the "
          f"oracle's primitive on {(gp == p).sum()}, another on {((gp != p) & (gp >= 0)).sum()}, nothing on {(gp < 0).sum()}")
    assert (gp[definite] != p[definite]).all()
    # pt_dbg_raycast walks the binary tree whatever the scene's query walk is: on these rays the two walks need not agree
    hits, prim = sc.raycast(r)
    same = (prim == gp) & (bits(np.where(prim >= 0, hits[:, 1], F(0))) == bits(gt))
    print(f"{name}, {walk} walk: pt_dbg_raycast differs from pt_trace_rays on {(~same).sum()} of {len(r)} MISS rays")
    if walk == "binary":
        assert same.all(), "pt_dbg_raycast is not pt_trace_rays on the binary walk"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VEIL_PLACEMENTS))
def test_veil_rows_and_frames_are_the_oracles(_gpu, name):
    """pt_dbg_nee on the veil rows, and the frame in mode 0 and on the five pipeline schedules of tests/test_params.py (wf_trace's early
    stop `bestT < stopBelow` and wf_drain's): the oracle's bits.  A shadow_stop_t margin below EPS turns the rows lit through a veil dark."""
    import test_params as Tpar
    v = veil(name)
    assert v.lit.mean() >= 0.1 and (v.frame() > 0).any(-1).mean() >= 0.9      # on the oracle alone, first
    sc = ptamd.Scene(v.nodes, v.tris)
    got = sc.nee(v.rows)
    bad = (bits(got) != bits(v.nee)).any(1)
    assert not bad.any(), f"{name}: pt_dbg_nee differs from the oracle on {bad.sum()} of {len(bad)} rows"
    cam = ptamd.make_camera(VEIL_W, VEIL_H, pos=v.camera_pos())
    prm = ptamd.default_params(passes=VEIL_PASSES, spp_per_pass=VEIL_SPP)
    streams = ((VEIL_W + 7) // 8) * ((VEIL_H + 7) // 8) * 64 * VEIL_PASSES
    for sched, (mode, rounds, early, drain) in Tpar.SCHEDULES.items():
        sc.set_mode(mode)
        sc.set_shade_rounds(rounds)
        sc.set_early_shade(streams if early else 0)
        sc.set_drain_threshold(drain)
        img = sc.render(cam, prm)
        same = (bits(img) == bits(v.frame())).all(-1)
        assert same.all(), f"{name}, schedule {sched}: {(~same).sum()} pixels differ from the oracle"
