"""Convex-region queries (include/pt_api.h: pt_convex_count, pt_convex_any, pt_convex_list, pt_camera_frustum; csrc/pt_convex.hip; DESIGN.md
section 42): which primitives lie inside or touch the caller's frusta, oriented boxes, slabs — intersections of up to 8 half-spaces.

The yardstick is tests/convex_ref.py: the class key h(Q, k) of the header in numpy float32, operation by operation, and brute force over
every primitive with the lists' order.  On the CPU the kernels' own three functions are compiled for the host and held to it bit for
bit, the node test is shown never to reject a box that holds a member (the floor), the float32 vertex test is held against float64 with
a derived bound, and the yardstick's own properties and pt_camera_frustum are asserted.  On the GPU every result is compared bit for
bit, no tolerance and no region left out, on the scenes of tests/test_nearest.py and on both walks."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import box_ref as B
import convex_ref as V
import dynamic_ref as R
import filters_ref as X
import nearest_ref as N
import ptamd
import test_nearest as T
from scenes_util import attribute_scene
from scenes_util import test_spheres as make_test_spheres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pathtrace-on-cuda_amd")
F = np.float32
INF = F(np.inf)
NEW = ("pt_convex_count", "pt_convex_any", "pt_convex_list", "pt_convex_count_host", "pt_convex_any_host", "pt_convex_list_host", "pt_camera_frustum")
SLICES = ((0, 1), (7, 63), (100, 64), (33, 65), (211, 130))      # partial waves, one wave, a wave and a lane, two waves and two lanes
PAIRS = 2_000_000                                                # per family
PLANE_COUNTS = (1, 2, 4, 6, 8)
FAMILY_SEED = {"ordinary": T.ATTR_SEED, "needles": T.NEEDLE_SEED, "far": T.ATTR_SEED}
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the surface of the library
# ---------------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_declared_and_bound(tmp_path):
    l = C.CDLL(ptamd.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "pt_api.h")).read()
    bound = {n for n, _, _ in ptamd.API}
    for name in NEW:
        assert hasattr(l, name), name
        assert f" {name}(" in hdr and name in bound, name
    for m in ("convex_count", "convex_any", "in_convex", "select_window"):
        assert callable(getattr(ptamd.Scene, m)), m
    assert callable(ptamd.frustum_planes) and callable(ptamd.obb_planes) and callable(ptamd.aabb_planes)
    assert (ptamd.CONVEX_TOUCHING, ptamd.CONVEX_INSIDE, ptamd.CONVEX_MAX_PLANES) == (0, 1, 8)
    src = tmp_path / "convex.c"
    src.write_text('#include "pt_api.h"\n_Static_assert(PT_CONVEX_TOUCHING == 0 && PT_CONVEX_INSIDE == 1, "flags");\n'
                   '_Static_assert(PT_CONVEX_MAX_PLANES == 8, "planes");\n_Static_assert(sizeof(PtBoxMember) == 8, "records are PtBoxMember");\n')
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    at = hdr.index("Convex-region queries (new")
    assert hdr.index("Box queries (new") < at < hdr.index("Radiance along the caller's own rays")
    assert hdr.index(" pt_box_list_host(") < at      # directly after the box section's last declaration
    assert all(at < hdr.index(f" {name}(") < hdr.index("Radiance along the caller's own rays") for name in NEW)


def test_bad_arguments_are_rejected_before_any_device_call():
    """A fake scene and fake device addresses: never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    base = 1 << 40
    scene, planes, out, cnt, offs, arr = (C.c_void_p(base + (i << 20)) for i in range(6))
    off = lambda p, k: C.c_void_p(p.value + k)      # noqa: E731
    flt = lambda **kw: C.byref(ptamd.PtQueryFilter(kw.get("prim"), kw.get("query"), kw.get("skip"), 0xFFFFFFFF, kw.get("flags", 0)))      # noqa: E731
    # (what, scene, planes, n, n_planes, flags, filter): the arguments the three device calls share
    shared = [
        ("NULL scene", None, planes, 64, 6, 0, None),
        ("NULL planes", scene, None, 64, 6, 0, None),
        ("n < 0", scene, planes, -1, 6, 0, None),
        ("n_planes 0", scene, planes, 64, 0, 0, None),
        ("n_planes 9", scene, planes, 64, 9, 0, None),
        ("n_planes -1", scene, planes, 64, -1, 1, None),
        ("flags 2", scene, planes, 64, 6, 2, None),
        ("flags -1", scene, planes, 64, 8, -1, None),
        ("planes + 8", scene, off(planes, 8), 64, 1, 0, None),
        ("PT_FILTER_TMIN", scene, planes, 64, 6, 0, flt(flags=ptamd.FILTER_TMIN)),
        ("unknown filter flags", scene, planes, 64, 6, 1, flt(flags=2)),
        ("filter d_prim_bits + 2", scene, planes, 64, 6, 0, flt(prim=arr.value + 2)),
        ("filter d_query_bits + 2", scene, planes, 64, 6, 0, flt(query=arr.value + 2)),
        ("filter d_skip_prim + 2", scene, planes, 64, 6, 1, flt(skip=arr.value + 2)),
        ("n = 0 does not excuse a NULL", scene, None, 0, 6, 0, None),
        ("n = 0 does not excuse n_planes 9", scene, planes, 0, 9, 0, None),
    ]
    for what, s, p, n, m, flags, f in shared:
        assert l.pt_convex_count(s, p, n, m, flags, f, cnt, None) == -1 and b"pt_convex_count:" in l.pt_last_error(), (what, l.pt_last_error())
        assert l.pt_convex_any(s, p, n, m, flags, f, out, None) == -1 and b"pt_convex_any:" in l.pt_last_error(), (what, l.pt_last_error())
        assert l.pt_convex_list(s, p, n, m, flags, offs, 100, f, out, None) == -1 and b"pt_convex_list:" in l.pt_last_error(), (what, l.pt_last_error())
    assert l.pt_convex_count(scene, planes, 64, 9, 0, None, cnt, None) == -1 and b"n_planes" in l.pt_last_error()
    assert l.pt_convex_count(scene, planes, 64, 9, 7, None, off(cnt, 2), None) == -1 and b"n_planes" in l.pt_last_error()      # the parameter before the alignment
    own = [
        ("count NULL", l.pt_convex_count, (scene, planes, 64, 6, 0, None, None, None)),
        ("count + 2", l.pt_convex_count, (scene, planes, 64, 6, 0, None, off(cnt, 2), None)),
        ("n = 0 does not excuse a NULL count", l.pt_convex_count, (scene, planes, 0, 6, 0, None, None, None)),
        ("any out NULL", l.pt_convex_any, (scene, planes, 64, 6, 1, None, None, None)),
        ("any out + 4", l.pt_convex_any, (scene, planes, 64, 6, 0, None, off(out, 4), None)),
        ("list offsets NULL", l.pt_convex_list, (scene, planes, 64, 6, 0, None, 100, None, out, None)),
        ("list offsets + 4", l.pt_convex_list, (scene, planes, 64, 6, 0, off(offs, 4), 100, None, out, None)),
        ("list out NULL", l.pt_convex_list, (scene, planes, 64, 6, 0, offs, 100, None, None, None)),
        ("list out + 4", l.pt_convex_list, (scene, planes, 64, 6, 0, offs, 100, None, off(out, 4), None)),
        ("list cap < 0", l.pt_convex_list, (scene, planes, 64, 6, 0, offs, -1, None, out, None)),
    ]
    for what, fn, a in own:
        assert fn(*a) == -1, what
        assert fn.__name__.encode() + b":" in l.pt_last_error(), (what, l.pt_last_error())
    h_planes, h_cnt, h_out, h_off = np.zeros((64, 6, 4), F), np.zeros(64, np.int32), np.zeros(64, ptamd.BOX_DTYPE), np.zeros(65, np.int64)
    P = ptamd._ptr
    host = [
        ("NULL scene", l.pt_convex_count_host, (None, P(h_planes), 64, 6, 0, P(h_cnt))),
        ("NULL planes", l.pt_convex_count_host, (scene, None, 64, 6, 0, P(h_cnt))),
        ("NULL count", l.pt_convex_count_host, (scene, P(h_planes), 64, 6, 0, None)),
        ("n < 0", l.pt_convex_count_host, (scene, P(h_planes), -3, 6, 0, P(h_cnt))),
        ("flags 5", l.pt_convex_count_host, (scene, P(h_planes), 64, 6, 5, P(h_cnt))),
        ("n_planes 0", l.pt_convex_count_host, (scene, P(h_planes), 64, 0, 0, P(h_cnt))),
        ("NULL scene", l.pt_convex_any_host, (None, P(h_planes), 64, 6, 0, P(h_out))),
        ("NULL out", l.pt_convex_any_host, (scene, P(h_planes), 64, 6, 0, None)),
        ("flags 2", l.pt_convex_any_host, (scene, P(h_planes), 64, 6, 2, P(h_out))),
        ("n_planes 9", l.pt_convex_any_host, (scene, P(h_planes), 64, 9, 0, P(h_out))),
        ("NULL scene", l.pt_convex_list_host, (None, P(h_planes), 64, 6, 0, P(h_off), 10, P(h_out))),
        ("NULL planes", l.pt_convex_list_host, (scene, None, 64, 6, 0, P(h_off), 10, P(h_out))),
        ("NULL offsets", l.pt_convex_list_host, (scene, P(h_planes), 64, 6, 0, None, 10, P(h_out))),
        ("cap < 0", l.pt_convex_list_host, (scene, P(h_planes), 64, 6, 0, P(h_off), -1, P(h_out))),
        ("flags 3", l.pt_convex_list_host, (scene, P(h_planes), 64, 6, 3, P(h_off), 10, None)),
        ("n_planes -1", l.pt_convex_list_host, (scene, P(h_planes), 64, -1, 0, P(h_off), 10, None)),
    ]
    for what, fn, a in host:
        assert fn(*a) == -1, what
        assert fn.__name__.encode() + b":" in l.pt_last_error(), (what, l.pt_last_error())
    # nothing to do: PT_OK, still without touching the scene or the device
    assert l.pt_convex_count(scene, planes, 0, 6, 0, None, cnt, None) == 0
    assert l.pt_convex_any(scene, planes, 0, 1, 1, flt(prim=arr.value), out, None) == 0
    assert l.pt_convex_list(scene, planes, 0, 8, 0, offs, 0, None, out, None) == 0
    assert l.pt_convex_count_host(scene, P(h_planes), 0, 6, 1, P(h_cnt)) == 0
    h_off[0] = 77
    assert l.pt_convex_list_host(scene, P(h_planes), 0, 6, 0, P(h_off), 0, None) == 0 and h_off[0] == 0


class _FakeScene:
    n_tris, n_spheres, device, _h = 5, 0, 0, C.c_void_p(1 << 40)


def test_wrappers_check_shape_dtype_and_device_on_the_host():
    import torch
    fake = _FakeScene()
    for fn in (ptamd.Scene.convex_count, ptamd.Scene.convex_any, ptamd.Scene.in_convex):
        for p in (np.zeros((4, 6), F), np.zeros(24, F), np.zeros((2, 6, 3), F), np.zeros((2, 9, 4), F), np.zeros((2, 0, 4), F), np.zeros((2, 3, 6, 4), F)):
            with pytest.raises(ptamd.PtError):
                fn(fake, p)
        for p in (torch.zeros((5, 6, 4)), torch.zeros((5, 6, 4), dtype=torch.float64), torch.zeros((5, 24)), torch.zeros((4, 6, 5)).transpose(0, 2),
                  [[[0.0] * 4] * 6]):
            with pytest.raises(ptamd.PtError):      # a CPU tensor, a wrong dtype, a wrong shape, not contiguous, not an array
                fn(fake, p)
    cnt = ptamd.Scene.convex_count(fake, np.zeros((0, 6, 4), F))      # n = 0: PT_OK without a device
    assert cnt.shape == (0,) and cnt.dtype == np.int32
    cls, prim = ptamd.Scene.convex_any(fake, np.zeros((0, 1, 4), F), inside=True)
    assert cls.shape == (0,) and prim.shape == (0,) and cls.dtype == F and prim.dtype == np.int32
    off, cls, prim = ptamd.Scene.in_convex(fake, np.zeros((0, 8, 4), F))
    assert off.tolist() == [0] and cls.shape == (0,) and prim.shape == (0,)
    with pytest.raises(ptamd.PtError):
        ptamd.QueryFilter(tmin=True).struct(fake, 3)      # tmin on a region query
    for bad in ((np.zeros(2), np.eye(3), np.ones(3)), (np.zeros(3), np.eye(4), np.ones(3)), (np.zeros(3), np.eye(3), np.ones(2))):
        with pytest.raises(ptamd.PtError):
            ptamd.obb_planes(*bad)
    with pytest.raises(ptamd.PtError):
        ptamd.aabb_planes((0, 0), (1, 1, 1))
    with pytest.raises(ptamd.PtError):
        ptamd.frustum_planes(ptamd.make_camera(8, 8), (0, 0, 4))


def test_plane_helpers_make_the_planes_they_document():
    rs = np.random.RandomState(5)
    rot, c, h = V.rotations(rs, 7), rs.uniform(-20, 20, (7, 3)), rs.uniform(0.1, 3, (7, 3))
    many = V.obb_many(c, rot, h)
    for i in range(7):
        one = ptamd.obb_planes(c[i], rot[i], h[i])
        assert one.shape == (6, 4) and one.dtype == F and np.array_equal(bits(one), bits(many[i]))
        assert np.array_equal(bits(one[0::2, 0:3]), bits(rot[i].astype(F))) and np.array_equal(bits(one[1::2, 0:3]), bits((-rot[i]).astype(F)))
        n64 = np.stack([rot[i, 0], -rot[i, 0], rot[i, 1], -rot[i, 1], rot[i, 2], -rot[i, 2]])
        assert np.array_equal(bits(one[:, 3]), bits((n64 @ c[i] + np.repeat(h[i], 2)).astype(F)))      # float64, rounded once
    lo, hi = F([-1.5, 2, 3]), F([0.25, 2, np.inf])
    a = ptamd.aabb_planes(lo, hi)
    assert a.shape == (6, 4) and np.array_equal(a[:, 0:3], np.stack([np.eye(3), -np.eye(3)], 1).reshape(6, 3))
    assert np.array_equal(a[0::2, 3], hi) and np.array_equal(a[1::2, 3], -lo) and np.array_equal(bits(V.aabb_many(lo, hi)[0]), bits(a))
    assert np.array_equal(V.natural_planes(V.pad(a[None, :2])), [2]) and np.array_equal(V.natural_planes(np.zeros((1, 8, 4), F)), [1])


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the kernels' own functions, compiled for the host
# ---------------------------------------------------------------------------------------------------------------------------------
def convex_host():
    """tools/convex_host.cpp around convex_tri_key, convex_sphere_key and convex_overlaps as csrc/pt_convex.h has them, built with the
    library's numerics flags."""
    def make():
        d = tempfile.mkdtemp(prefix="pt_convex_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src = open(os.path.join(PKG, "csrc", "pt_convex.h")).read()
        text = "\n".join(_function_text(src, head) for head in ("PT_DEV float convex_tri_key(", "PT_DEV float convex_sphere_key(", "PT_DEV bool convex_overlaps("))
        open(os.path.join(d, "convex_kernel_fns.inc"), "w").write(text)
        exe = os.path.join(d, "convex_host")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas", "-I", d,
                        os.path.join(ROOT, "tools", "convex_host.cpp"), "-o", exe], check=True)
        return d, exe
    return _cached("convex_host", make)


def _function_text(src, head):
    """The text of the function that starts with `head`, to its closing brace."""
    at = src.index(head)
    depth, k = 0, src.index("{", at)
    while True:
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        k += 1
        if depth == 0:
            return src[at:k]


def host_eval(m, tri_pairs=None, sph_pairs=None, box_pairs=None):
    """What the kernels' functions give: tri_pairs (n, 4 m + 9) planes a ab ac, sph_pairs (n, 4 m + 4) planes centre rad, box_pairs
    (n, 4 m + 6) planes lo hi -> (triangle keys, sphere keys, overlaps as bool)."""
    d, exe = convex_host()
    src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    parts = [np.ascontiguousarray(np.zeros((0, 4 * m + w), F) if p is None else p, F).reshape(-1, 4 * m + w) for p, w in ((tri_pairs, 9), (sph_pairs, 4), (box_pairs, 6))]
    with open(src, "wb") as f:
        f.write(np.array([m] + [len(p) for p in parts], np.int32).tobytes())
        for p in parts:
            f.write(p.tobytes())
    subprocess.run([exe, src, dst], check=True)
    out = np.fromfile(dst, F)
    os.remove(src)
    os.remove(dst)
    nt, ns = len(parts[0]), len(parts[1])
    return out[:nt], out[nt:nt + ns], out[nt + ns:] != 0


def _family(name):
    """(planes (n, 6, 4), positions, float32 keys) of a family, made once."""
    def make():
        pl, pos = V.family(name, FAMILY_SEED[name], PAIRS)
        return pl, pos, V.tri_key(pl, *N.edges(pos))
    return _cached(("family", name), make)


def _attribute():
    return _cached("attribute", lambda: R.positions(ptamd.build_bvh(attribute_scene(T.ATTR_SEED, 12)[0])[1]))


def _ysets():
    def make():
        pos, sph = _attribute(), np.ascontiguousarray(make_test_spheres(), F)
        sets = V.ConvexSets(pos, sph, 3)
        return pos, sph, sets, V.key_matrix(sets.planes, pos, sph)
    return _cached("yardstick sets", make)


def _edge_set():
    """Every region of the attribute scene's sets against every triangle of it and against the test spheres: (triangle pairs, sphere
    pairs) as host_eval takes them, m = 8."""
    def make():
        pos, sph, sets, _ = _ysets()
        pl = sets.planes.reshape(len(sets.planes), 32)
        a, ab, ac = N.edges(pos)
        nr, nt, ns = len(pl), len(a), len(sph)
        tri = np.concatenate([np.repeat(pl, nt, 0), np.tile(a, (nr, 1)), np.tile(ab, (nr, 1)), np.tile(ac, (nr, 1))], 1)
        sp = np.concatenate([np.repeat(pl, ns, 0), np.tile(sph[:, 0:4], (nr, 1))], 1)
        return tri, sp
    return _cached("edge set", make)


@pytest.mark.parametrize("name", sorted(B.FAMILIES) + ["edge set"])
def test_the_kernels_functions_compiled_for_the_host_are_the_yardsticks_bit_for_bit(name):
    if name == "edge set":
        tri, sp = _edge_set()
        _, _, _, K = _ysets()
        nt = len(_attribute())
        want_t, want_s, m = K[:, :nt].reshape(-1), K[:, nt:].reshape(-1), 8
    else:
        pl, pos, want_t = _family(name)
        tri, sp, want_s, m = np.concatenate([pl.reshape(len(pl), 24)] + list(N.edges(pos)), 1), None, np.zeros(0, F), 6
    got_t, got_s, _ = host_eval(m, tri, sp)
    hist = [int((want_t == v).sum()) for v in (0, 1, INF)]
    print(f"{name}: {len(tri)} triangle pairs (inside, touching, none) = {hist}, {len(want_s)} sphere pairs {[int((want_s == v).sum()) for v in (0, 1, INF)]}")
    assert sum(hist) == len(tri) and all(h > 0 for h in hist)      # all three classes occur
    assert np.array_equal(bits(got_t), bits(want_t)), f"{name}: {(bits(got_t) != bits(want_t)).sum()} triangle keys differ, first at {np.nonzero(bits(got_t) != bits(want_t))[0][:5]}"
    assert np.array_equal(bits(got_s), bits(want_s)), f"{name}: {(bits(got_s) != bits(want_s)).sum()} sphere keys differ"
    if name == "edge set":
        assert all((want_s == v).any() for v in (0, 1, INF))


@pytest.mark.parametrize("name", ["ordinary", "edge set"])
def test_the_node_test_never_rejects_a_box_that_holds_a_member(name):
    """The floor (include/pt_api.h; csrc/pt_convex.h): if convex_overlaps — the kernels' own, compiled for the host — rejects the
    triangle's own record box, or that box widened as the binary tree's walk widens it, the key is +inf.  The theorem has no exception."""
    if name == "edge set":
        tri, _ = _edge_set()
        _, _, _, K = _ysets()
        key, m = K[:, :len(_attribute())].reshape(-1), 8
    else:
        pl, pos, key = _family(name)
        tri, m = np.concatenate([pl.reshape(len(pl), 24)] + list(N.edges(pos)), 1), 6
    w = 4 * m
    tlo, thi = N.tri_box(tri[:, w:w + 3], tri[:, w + 3:w + 6], tri[:, w + 6:w + 9])
    for what, (lo, hi) in (("record box", (tlo, thi)), ("widened box", V.widened(tlo, thi))):
        _, _, ok = host_eval(m, box_pairs=np.concatenate([tri[:, :w], lo, hi], 1))
        assert np.array_equal(ok, V.overlaps(tri[:, :w].reshape(-1, m, 4), lo, hi)), f"{name}, {what}: the node test differs from its restatement"
        rejected = ~ok
        print(f"{name}, {what}: {rejected.sum()} of {len(ok)} boxes rejected, {(rejected & (key != INF)).sum()} of them hold a member")
        assert rejected.any() and (~rejected).any()
        assert (key[rejected] == INF).all(), f"{name}, {what}: a rejected box holds a member"
    # and the test is not vacuous the other way: a non-member's box is not always rejected (the walk looks, the key decides)
    assert ((key == INF) & ok).any()


@pytest.mark.parametrize("name", sorted(B.FAMILIES))
def test_the_float32_vertex_test_agrees_with_float64_beyond_2_to_the_minus_20(name):
    """With M the largest absolute coordinate of the family and delta = 2^-20 * M * |n| (|n| in float64): for every one of the 2 * 10^6
    (plane, vertex) pairs with float64 signed distance e = n.v - d, e > delta implies float32 says outside and e < -delta inside.  The
    bound is derived: three products and two sums err by at most 3 * 2^-24 * sum |n_i x_i| <= 5.2 * 2^-24 * M |n| < 2^-21 * M |n|.
    Measured with these seeds: 0 exceptions at 2^-20 and at 2^-22 in every family; at 2^-24 ordinary 554, needles 168, far 17,492
    (below the rounding of s itself, where float32 cannot follow)."""
    acc, M = V.vertex_accuracy(name, FAMILY_SEED[name], PAIRS, shifts=(20, 22, 24))
    for s in sorted(acc):
        print(f"{name}: M = {M:.6g}, delta = 2^-{s} * M * |n|: {acc[s]} exceptions in {PAIRS} pairs")
    assert acc[20] == 0, f"{name}: {acc[20]} exceptions at 2^-20 * M * |n|"


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the yardstick's own properties
# ---------------------------------------------------------------------------------------------------------------------------------
def test_yardstick_inside_members_are_a_subset_of_the_touching_ones_and_come_first():
    pos, sph, sets, K = _ysets()
    ct, (ot, kt, pt) = V.brute(sets.planes, pos, sph, V.TOUCHING, K=K)
    ci, (oi, ki, pi) = V.brute(sets.planes, pos, sph, V.INSIDE, K=K)
    assert (ci <= ct).all() and (ci > 0).any() and (ci < ct).any() and set(np.unique(kt).tolist()) == {0.0, 1.0} and (ki == 0).all()
    for q in range(len(sets.planes)):
        row_t, row_i = pt[ot[q]:ot[q + 1]], pi[oi[q]:oi[q + 1]]
        assert np.array_equal(row_t[:len(row_i)], row_i) and (kt[ot[q]:ot[q + 1]][len(row_i):] == 1).all()      # inside first, in the same order
        k = kt[ot[q]:ot[q + 1]]
        assert ((np.diff(k) > 0) | ((np.diff(k) == 0) & (np.diff(row_t) < 0))).all()      # cls ascending, then the larger prim first
    # the three sorting classes of the lists and the longest list
    assert ((ct > 0) & (ct <= 8)).any() and ((ct > 8) & (ct <= 32)).any() and (ct > 32).any() and ct.max() == K.shape[1]


def test_yardstick_invalid_and_empty_regions_have_no_member_and_the_scene_region_has_every_primitive_inside():
    pos, sph, sets, K = _ysets()
    inv = sets.parts["invalid"]
    assert np.isnan(inv[..., 0:3]).any() and np.isposinf(inv[..., 0:3]).any() and np.isneginf(inv[..., 0:3]).any() and np.isnan(inv[..., 3]).any()
    assert (~np.isfinite(inv).all((1, 2))).all()
    assert (K[sets.rows("invalid")] == INF).all() and (K[sets.rows("empty")] == INF).all() and (K[sets.rows("far")] == INF).all()
    e = sets.parts["empty"]
    assert ((e[..., 0:3] == 0).all(-1) & (e[..., 3] == -1)).any(1).sum() == 2 and np.isneginf(e[..., 3]).any(1).sum() == 2
    assert (K[sets.rows("scene")] == 0).all() and K.shape[1] == len(pos) + len(sph)
    assert (K[sets.rows("obb")[:6]] <= 1).any(1).all()      # the regions the empty ones were made from do hold something
    # planes of a region beyond those it needs are neutral: cutting them off changes no key, for every plane count the GPU tests use
    assert set(PLANE_COUNTS) <= set(sets.natural.tolist()) | {8} and all((sets.natural <= m).sum() >= 20 for m in PLANE_COUNTS)
    for m in PLANE_COUNTS:
        rows, pl = sets.with_planes(m)
        assert pl.shape[1:] == (m, 4) and np.array_equal(bits(V.key_matrix(pl, pos, sph)), bits(K[rows])), m


def test_yardstick_half_spaces_and_slabs_are_the_box_definitions_keys_and_exact():
    """m = 1 and m = 2 axis-aligned planes give box_ref.tri_key of the half-space / slab box with infinite coordinates bit for bit: both
    are decided by the record's extent on one axis ((0*x + 1*y) + 0*z is y exactly).  And any half-space or slab is answered exactly:
    class 1 means the record's vertices lie on both sides."""
    pos = _attribute()
    a, ab, ac = N.edges(pos)
    v = pos.reshape(-1, 3)
    rs = np.random.RandomState(11)
    seen = set()
    for ax in range(3):
        for t in np.concatenate([rs.choice(v[:, ax], 6), rs.uniform(v[:, ax].min(), v[:, ax].max(), 3).astype(F)]):
            e = np.eye(3, dtype=F)[ax]
            lo, hi = np.full(3, -np.inf, F), np.full(3, np.inf, F)
            hi[ax] = t
            below = V.tri_key(np.concatenate([e, [t]]).astype(F)[None, None], a, ab, ac)
            assert np.array_equal(bits(below), bits(B.tri_key(lo, hi, a, ab, ac))), (ax, t)
            lo2, hi2 = lo.copy(), hi.copy()
            lo2[ax] = t - F(3)
            slab = V.tri_key(np.stack([np.concatenate([e, [t]]), np.concatenate([-e, [-(t - F(3))]])]).astype(F)[None], a, ab, ac)
            assert np.array_equal(bits(slab), bits(B.tri_key(lo2, hi2, a, ab, ac))), (ax, t)
            seen |= set(below.tolist()) | set(slab.tolist())
    assert seen == {0.0, 1.0, float("inf")}
    _, sph, sets, K = _ysets()
    nt = len(pos)
    own = np.stack([a, a + ab, a + ac], 1).astype(np.float64)
    for part in ("halfspace", "slab", "thin"):
        for row, pl in zip(sets.rows(part), sets.parts[part]):
            pl = pl[:V.natural_planes(pl[None])[0]].astype(np.float64)
            e = (own @ pl[:, 0:3].T) - pl[:, 3]      # (triangles, vertices, planes) signed distances in float64
            span = np.abs(own).max() * np.abs(pl[:, 0:3]).sum(1).max() * 2.0 ** -20
            clear = (np.abs(e) > span).all((1, 2))     # no vertex within rounding of a plane
            if len(pl) == 1:
                exact = np.where((e <= 0).all((1, 2)), 0.0, np.where((e > 0).all((1, 2)), np.inf, 1.0))
            else:      # parallel planes: the vertices' interval along the normal against [lo, hi]
                s = own @ pl[0, 0:3]
                lo_, hi_ = -pl[1, 3], pl[0, 3]
                exact = np.where((s.min(1) > hi_) | (s.max(1) < lo_), np.inf, np.where((s.min(1) >= lo_) & (s.max(1) <= hi_), 0.0, 1.0))
            assert np.array_equal(K[row, :nt][clear], exact[clear].astype(F)), part
    thin = K[sets.rows("thin"), :nt]
    assert (thin <= 1).any(1).all() and (thin != 0).all()      # a slab of no thickness through a vertex: that vertex's triangles touch, nothing is inside


def test_yardstick_aabb_planes_agree_with_the_box_query_on_class_0_and_hold_its_touching_members():
    pos, sph, sets, K = _ysets()
    boxes = B.BoxSets(pos, sph, 3).boxes[:len(sets.parts["aabb"])]
    lo, hi = B.split(boxes)
    assert np.array_equal(bits(V.pad(V.aabb_many(lo, hi))), bits(sets.parts["aabb"]))
    KB, KV = B.key_matrix(boxes, pos, sph), K[sets.rows("aabb")]
    finite = np.isfinite(lo).all(1) & np.isfinite(hi).all(1)
    nt = len(pos)
    assert finite.sum() > 40 and np.array_equal(KB[finite][:, :nt] == 0, KV[finite][:, :nt] == 0)      # class 0: equal sets
    assert ((KB[finite] <= 1) <= (KV[finite] <= 1)).all()                                               # touching: a superset
    more = int(((KV[finite][:, :nt] == 1) & (KB[finite][:, :nt] == INF)).sum())
    print(f"aabb_planes: {more} of {int((KV[finite][:, :nt] == 1).sum())} class-1 triangle pairs are over-reports the box query's separating axes reject")
    inv = ~finite & ~np.isinf(lo).any(1) & ~np.isinf(hi).any(1)      # a NaN coordinate: no member either way
    assert (KV[inv] == INF).all() and (KB[inv] == INF).all()


def test_yardstick_puts_a_duplicated_triangle_before_the_one_it_copies():
    pos = _attribute()
    dup = np.concatenate([pos, pos[5:6]])      # triangle 5 again, as the last one
    region = V.pad(ptamd.aabb_planes(pos[5].min(0) - F(0.5), pos[5].max(0) + F(0.5))[None])
    _, (off, cls, prim) = V.brute(region, dup)
    at5, at_dup = int(np.nonzero(prim == 5)[0][0]), int(np.nonzero(prim == len(pos))[0][0])
    assert bits(cls[at5]) == bits(cls[at_dup]) and at_dup < at5      # among equal keys the larger index first
    assert (np.diff(prim[cls == cls[at5]]) < 0).all()


def test_yardstick_regions_inside_around_and_across_a_sphere():
    pos, sph, sets, K = _ysets()
    rows, kind = sets.rows("spheres"), sets.sphere_kind
    own = K[rows][:, len(pos):][np.arange(len(rows)), sets.sphere_index]
    assert all((kind == v).sum() > 3 for v in (0, 1, 2))
    # wholly inside the ball: touching, the conservative case the header names; around the ball: inside; across its surface: touching
    assert (own[kind == 0] == 1).all() and (own[kind == 1] == 0).all() and (own[kind == 2] == 1).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: pt_camera_frustum
# ---------------------------------------------------------------------------------------------------------------------------------
def _pixel_dirs(cam, fx, fy):
    """pixel_direction of csrc/pt_shade.h at screen positions (fx, fy), in float64 from the camera's fields, unnormalised"""
    fwd, up, right = (np.array(v[:], np.float64) for v in (cam.forward, cam.up, cam.right))
    fovy = F(cam.fovy_deg) * F(0.01745329251994329576923690768489)
    ty = F(np.tan(np.float64(fovy * F(0.5))))
    fovx = F(2) * F(np.arctan2(np.float64(F(np.tan(np.float64(fovy * F(0.5)))) * F(cam.aspect)), 1.0))
    tx = F(np.tan(np.float64(fovx * F(0.5))))
    a = 2.0 * (np.asarray(fx, np.float64) / (cam.W - 1) - 0.5) * float(tx)
    b = -2.0 * (np.asarray(fy, np.float64) / (cam.H - 1) - 0.5) * float(ty)
    return fwd + a[..., None] * right + b[..., None] * up


def test_camera_frustum_planes_contain_the_eye_hold_the_centre_and_share_their_sides():
    rs = np.random.RandomState(21)
    for i in range(40):
        W, H = int(rs.randint(2, 200)), int(rs.randint(2, 120))
        cam = ptamd.make_camera(W, H, pos=tuple(rs.uniform(-30, 30, 3).tolist()), rot_deg=tuple(rs.uniform(0, 360, 3).tolist()), fovy_deg=float(rs.uniform(10, 100)))
        x0, y0 = rs.uniform(0, W - 1), rs.uniform(0, H - 1)
        x1, y1 = rs.uniform(x0 + 0.5, W), rs.uniform(y0 + 0.5, H)
        if i % 4 == 0:
            x0, y0, x1, y1 = 0, 0, W, H
        near, far = (-1.0, np.inf) if i % 2 else (0.5, 90.0)
        pl = ptamd.frustum_planes(cam, (x0, y0, x1, y1), near, far)
        assert pl.shape == (6, 4) and pl.dtype == F
        pos = np.array(cam.pos[:], np.float64)
        n64 = pl[:, 0:3].astype(np.float64)
        # the side planes contain pos to within the rounding of d (one float32 rounding of n . pos, and of n)
        err = np.abs(n64[:4] @ pos - pl[:4, 3])
        assert (err <= 2.0 ** -22 * (np.abs(n64[:4]) @ np.abs(pos)) + 1e-30).all(), (i, err)
        x0, y0, x1, y1 = (float(F(t)) for t in (x0, y0, x1, y1))
        mid = _pixel_dirs(cam, 0.5 * (x0 + x1), 0.5 * (y0 + y1))
        assert (n64[:4] @ mid < 0).all()                             # the centre direction is strictly inside the four sides
        if near < 0:
            assert np.array_equal(pl[4:], F([[0, 0, 0, np.inf]] * 2))
            assert (n64[:4] @ (pos + 7.0 * mid) - pl[:4, 3] < 0).all()
        else:
            fwd = np.array(cam.forward[:], np.float64)
            p = pos + mid * (0.5 * (near + far) / (mid @ fwd))      # on the centre direction, halfway between near and far
            assert (n64 @ p - pl[:, 3] < 0).all()                    # strictly inside all six
            assert abs(-(fwd @ pos + near) - pl[4, 3]) <= 1e-5 * (1 + abs(pl[4, 3])) and abs((fwd @ pos + far) - pl[5, 3]) <= 1e-5 * (1 + abs(pl[5, 3]))
        # corners of the window lie on their two planes, up to rounding
        for (fx, fy), (p0, p1) in (((x0, y0), (0, 2)), ((x1, y0), (1, 2)), ((x0, y1), (0, 3)), ((x1, y1), (1, 3))):
            d = _pixel_dirs(cam, fx, fy)
            assert (np.abs(n64[[p0, p1]] @ d) <= 1e-6 * np.abs(n64[[p0, p1]]).sum(1) * np.abs(d).sum()).all()
        # neighbours share their common side up to sign, bit for bit
        xm, ym = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
        lft, rgt = ptamd.frustum_planes(cam, [(x0, y0, xm, y1), (xm, y0, x1, y1)], near, far)
        assert np.array_equal(bits(np.abs(lft[1])), bits(np.abs(rgt[0]))) and np.array_equal(np.signbit(lft[1])[lft[1] != 0], ~np.signbit(rgt[0])[rgt[0] != 0])
        top, bot = ptamd.frustum_planes(cam, [(x0, y0, x1, ym), (x0, ym, x1, y1)], near, far)
        assert np.array_equal(bits(np.abs(top[3])), bits(np.abs(bot[2]))) and np.array_equal(np.signbit(top[3])[top[3] != 0], ~np.signbit(bot[2])[bot[2] != 0])
        assert np.array_equal(bits(lft[0]), bits(pl[0])) and np.array_equal(bits(rgt[1]), bits(pl[1]))
    whole = ptamd.frustum_planes(cam)
    assert np.array_equal(bits(whole), bits(ptamd.frustum_planes(cam, (0, 0, cam.W, cam.H))))


def test_camera_frustum_rejects_bad_windows_and_cameras():
    l = ptamd.lib()
    cam = ptamd.make_camera(64, 48)
    out = np.zeros(24, F)
    P = ptamd._ptr
    assert l.pt_camera_frustum(C.byref(cam), 0, 0, 64, 48, -1.0, np.inf, P(out)) == 0
    bad = [(-1, 0, 8, 8), (0, -0.5, 8, 8), (8, 0, 8, 8), (9, 0, 8, 8), (0, 8, 8, 8), (0, 0, 64.5, 8), (0, 0, 8, 48.25), (np.nan, 0, 8, 8), (0, 0, 8, np.nan),
           (0, 0, np.inf, 8)]
    for w in bad:
        assert l.pt_camera_frustum(C.byref(cam), *w, -1.0, np.inf, P(out)) == -1 and b"pt_camera_frustum:" in l.pt_last_error(), w
        with pytest.raises(ptamd.PtError):
            ptamd.frustum_planes(cam, w)
    assert l.pt_camera_frustum(None, 0, 0, 8, 8, -1.0, np.inf, P(out)) == -1 and l.pt_camera_frustum(C.byref(cam), 0, 0, 8, 8, -1.0, np.inf, None) == -1
    for near, far in ((np.nan, 10.0), (1.0, np.nan), (5.0, 2.0)):
        assert l.pt_camera_frustum(C.byref(cam), 0, 0, 8, 8, near, far, P(out)) == -1, (near, far)
    for field, value in (("W", 1), ("H", 0), ("fovy_deg", np.nan), ("fovy_deg", 0.0), ("aspect", np.inf)):
        c = ptamd.make_camera(64, 48)
        setattr(c, field, value)
        assert l.pt_camera_frustum(C.byref(c), 0, 0, 1, 1, -1.0, np.inf, P(out)) == -1, field
    for vec in ("pos", "forward", "up", "right"):
        c = ptamd.make_camera(64, 48)
        getattr(c, vec)[1] = np.nan
        assert l.pt_camera_frustum(C.byref(c), 0, 0, 8, 8, -1.0, np.inf, P(out)) == -1, vec
    c = ptamd.make_camera(64, 48)
    c.forward[:] = [0, 0, 0]
    assert l.pt_camera_frustum(C.byref(c), 0, 0, 8, 8, -1.0, np.inf, P(out)) == -1


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


def _sets(name):
    return _cached(("sets", name), lambda: V.ConvexSets(T._positions(name), T._spheres(name), 80 + T.SCENES.index(name)))


def _keys(name):
    return _cached(("keys", name), lambda: V.key_matrix(_sets(name).planes, T._positions(name), T._spheres(name)))


def _want(name, flags):
    """(counts, (offsets, cls, prim)) by brute force, computed once per scene and flag."""
    return _cached(("want", name, flags), lambda: V.brute(None, None, None, flags, K=_keys(name)))


def assert_sets_hold_what_they_should(name):
    sets, K = _sets(name), _keys(name)
    cnt = (K <= 1).sum(1)
    assert K.shape == (len(sets.planes), T._n_prims(name)) and len(sets.planes) >= 211 + 130 + 1
    assert (cnt[sets.rows("obb")] > 0).mean() > 0.9 and (cnt[sets.rows("frusta")] > 0).mean() > 0.4
    assert (K[sets.rows("scene")] == 0).all()
    assert (cnt[sets.rows("invalid")] == 0).all() and (cnt[sets.rows("empty")] == 0).all() and (cnt[sets.rows("far")] == 0).all()
    assert (cnt[sets.rows("thin")] > 0).all() and (cnt[sets.rows("halfspace")] > 0).all()      # each passes through a vertex of the scene, by equality
    if T._spheres(name) is not None:
        own = K[sets.rows("spheres")][:, len(T._positions(name)):][np.arange(len(sets.sphere_index)), sets.sphere_index]
        assert (own[sets.sphere_kind == 1] == 0).all() and (own[sets.sphere_kind != 1] == 1).all()
    return cnt


def assert_csr(got, want, what):
    got = tuple(np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in got)
    assert np.array_equal(got[0], want[0]), f"{what}: offsets differ at {np.nonzero(got[0] != want[0])[0][:5]}"
    assert np.array_equal(got[2], want[2]), f"{what}: {(got[2] != want[2]).sum()} prims differ, first at {np.nonzero(got[2] != want[2])[0][:5]}"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{what}: cls differs at {np.nonzero(bits(got[1]) != bits(want[1]))[0][:5]}"


def assert_any(got, counts, K, bound, what, allowed=None):
    """pt_convex_any's contract against the counts: prim >= 0 exactly where the count is above 0, then a member with its own key."""
    cls, prim = (np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in got)
    hit = counts > 0
    assert np.array_equal(prim >= 0, hit), f"{what}: {((prim >= 0) != hit).sum()} regions decide differently from the count"
    assert (prim[~hit] == -1).all() and (bits(cls[~hit]) == 0).all() and (prim < K.shape[1]).all(), what
    key = K[np.nonzero(hit)[0], prim[hit]]
    assert np.array_equal(bits(cls[hit]), bits(key)) and (key <= bound).all(), f"{what}: the record is not a member with its own key"
    if allowed is not None:
        assert allowed[np.nonzero(hit)[0], prim[hit]].all(), f"{what}: a filtered-out primitive was returned"


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sub(H, rows):
    """The CSR lists of the queries `rows` of H, in that order"""
    off, cls, prim = H
    idx = np.concatenate([np.arange(off[r], off[r + 1]) for r in rows]) if len(rows) else np.zeros(0, np.int64)
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(off[rows + 1] - off[rows])]), cls[idx.astype(np.int64)], prim[idx.astype(np.int64)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.SCENES)
def test_counts_any_and_lists_are_brute_forces(_gpu, name):
    sets, K = _sets(name), _keys(name)
    cnt = assert_sets_hold_what_they_should(name)
    print(f"{name}: {len(sets.planes)} regions, {K.shape[1]} primitives; members per region: max {cnt.max()}, at most 8: {(cnt <= 8).sum()}, "
          f"9-32: {((cnt > 8) & (cnt <= 32)).sum()}, above 32: {(cnt > 32).sum()}; inside {(K == 0).sum()}, touching {(K == 1).sum()}")
    if name == "attribute":
        assert ((cnt > 0) & (cnt <= 8)).any() and ((cnt > 8) & (cnt <= 32)).any() and (cnt > 32).any() and cnt.max() == K.shape[1]      # the three sorting classes
    sc = T._scene(name)
    assert (3 * sc.tree_info()["quad_depth"] + 2 > 40) == (name in T.DEEP)      # the deep trees take the binary walk
    d_planes = _dev(sets.planes)
    for flags in (V.TOUCHING, V.INSIDE):
        inside, what = flags == V.INSIDE, f"{name}, flags {flags}"
        counts, H = _want(name, flags)
        assert np.array_equal(sc.convex_count(d_planes, inside=inside).cpu().numpy(), counts), what
        assert_any(sc.convex_any(d_planes, inside=inside), counts, K, 1 - flags, what + " any")
        assert_csr(sc.in_convex(d_planes, inside=inside), H, what + " list")
        # the host variants against the device route
        assert np.array_equal(sc.convex_count(sets.planes, inside=inside), counts), what + " count_host"
        assert_any(sc.convex_any(sets.planes, inside=inside), counts, K, 1 - flags, what + " any_host")
        assert_csr(sc.in_convex(sets.planes, inside=inside), H, what + " list_host")
        for lo, m in SLICES:
            sub = d_planes[lo:lo + m].contiguous()
            assert np.array_equal(sc.convex_count(sub, inside=inside).cpu().numpy(), counts[lo:lo + m]), f"{what}, n = {m}"
            assert_any(sc.convex_any(sub, inside=inside), counts[lo:lo + m], K[lo:lo + m], 1 - flags, f"{what} any, n = {m}")
            assert_csr(sc.in_convex(sub, inside=inside), X.rows(H, lo, m), f"{what} list, n = {m}")
        # every plane count: the regions that need no more planes, cut to that many, are the same regions
        for m in PLANE_COUNTS[:-1]:
            rows, pl = sets.with_planes(m)
            assert len(rows) >= 20
            d, whatm = _dev(pl), f"{what}, n_planes {m}"
            assert np.array_equal(sc.convex_count(d, inside=inside).cpu().numpy(), counts[rows]), whatm
            assert_any(sc.convex_any(d, inside=inside), counts[rows], K[rows], 1 - flags, whatm + " any")
            assert_csr(sc.in_convex(d, inside=inside), _sub(H, rows), whatm + " list")
            assert_csr(sc.in_convex(pl, inside=inside), _sub(H, rows), whatm + " list_host")
            assert np.array_equal(sc.convex_count(pl, inside=inside), counts[rows]), whatm + " count_host"


def _raw_list(sc, d_planes, flags, off, cap, guard=256, filt=None):
    """pt_convex_list into a buffer with a guard band on either side of [0, cap): (records (cap, 2) int32, both bands untouched?)."""
    import torch
    buf = torch.full((cap + 2 * guard, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_off = _dev(np.ascontiguousarray(off, np.int64))
    rc = ptamd.lib().pt_convex_list(sc._h, C.c_void_p(d_planes.data_ptr()), d_planes.shape[0], d_planes.shape[1], flags, C.c_void_p(d_off.data_ptr()), cap, filt,
                                    C.c_void_p(buf.data_ptr() + guard * 8), None)
    assert rc == 0, ptamd.lib().pt_last_error()
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    return h[guard:guard + cap], bool((h[:guard] == 0x5A5A5A5A).all() and (h[guard + cap:] == 0x5A5A5A5A).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["attribute", "standin24_spheres", "comb32"])
def test_undersized_segments_hold_distinct_members_sorted_and_nothing_is_written_outside(_gpu, name):
    sets, K = _sets(name), _keys(name)
    sc = T._scene(name)
    d_planes = _dev(sets.planes)
    counts, H = _want(name, V.TOUCHING)
    n = len(counts)
    # segments one short, half as long, a single slot, and full with three to spare, by turns
    m = np.where(np.arange(n) % 4 == 0, counts - 1, np.where(np.arange(n) % 4 == 1, counts // 2, np.where(np.arange(n) % 4 == 2, 1, counts + 3))).clip(0)
    off = np.concatenate([np.zeros(1, np.int64), np.cumsum(m, dtype=np.int64)])
    rec, clean = _raw_list(sc, d_planes, V.TOUCHING, off, int(off[-1]))
    assert clean
    short = 0
    for q in range(n):
        seg = rec[off[q]:off[q + 1]]
        live = min(int(m[q]), int(counts[q]))
        prim, cls = seg[:live, 1], seg[:live, 0].view(F)
        assert (seg[live:, 1] == -1).all() and (seg[live:, 0] == 0).all(), f"{name}, region {q}: no miss records after the members"
        assert len(set(prim.tolist())) == live and (prim >= 0).all() and (prim < K.shape[1]).all(), f"{name}, region {q}: members repeat"
        assert np.array_equal(bits(cls), bits(K[q, prim])) and (cls <= 1).all(), f"{name}, region {q}: not members with their keys"
        assert ((np.diff(cls) > 0) | ((np.diff(cls) == 0) & (np.diff(prim) < 0))).all(), f"{name}, region {q}: not sorted"
        if m[q] >= counts[q]:
            assert np.array_equal(prim, H[2][H[0][q]:H[0][q + 1]]), f"{name}, region {q}: a segment that holds the list is not the list"
        else:
            short += 1
    assert short > n // 4
    # garbage offsets: negative, beyond cap, decreasing — every write stays inside [0, cap), every record written is a record
    rs = np.random.RandomState(9)
    cap = 700
    junk = rs.randint(-300, 1200, n + 1).astype(np.int64)
    junk[::7] = np.int64(1) << 40
    junk[3::11] = -(np.int64(1) << 40)
    rec, clean = _raw_list(sc, d_planes, V.TOUCHING, junk, cap)
    assert clean, f"{name}: garbage offsets wrote outside [0, cap)"
    written = rec[:, 0] != 0x5A5A5A5A
    assert written.any() and (rec[written, 1] >= -1).all() and (rec[written, 1] < K.shape[1]).all() and np.isin(rec[written, 0], [0, 0x3F800000]).all()


def _filter(sc, prim_bits, m, skip):
    scalar = np.ndim(m) == 0
    return ptamd.QueryFilter(prim_bits=prim_bits, bits=int(m) if scalar else 0xFFFFFFFF, query_bits=None if scalar else np.ascontiguousarray(m, np.uint32),
                             skip=None if skip is None else np.ascontiguousarray(skip, np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["standin24_spheres", "attribute", "chain28"])
def test_a_filtered_result_is_the_host_side_selection_from_the_unfiltered_list(_gpu, name):
    import torch
    sets, K = _sets(name), _keys(name)
    pos = T._positions(name)
    sc = T._scene(name)
    d_planes = _dev(sets.planes)
    n_prims = K.shape[1]
    recipe = X.Recipe(_want(name, V.TOUCHING)[1], n_prims, len(pos), 77, False)
    dropped = 0
    for flags in (V.TOUCHING, V.INSIDE):
        inside = flags == V.INSIDE
        counts, H = _want(name, flags)
        # the neutral filter runs the unfiltered kernels: the same bits
        neutral = ptamd.QueryFilter()
        assert np.array_equal(sc.convex_count(d_planes, inside=inside, filter=neutral).cpu().numpy(), counts)
        assert_csr(sc.in_convex(d_planes, inside=inside, filter=neutral), H, f"{name}, flags {flags}, neutral filter")
        a, b = sc.convex_any(d_planes, inside=inside, filter=neutral), sc.convex_any(d_planes, inside=inside)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
        for what, prim_bits, m, skip, _ in recipe.filters():
            what = f"{name}, flags {flags}, {what}"
            want = X.select(H, prim_bits, m, skip, None)
            wc, wH = V.brute(None, None, None, flags, (prim_bits, m, skip), K=K)
            assert X.same(want, wH) and np.array_equal(np.diff(want[0]), wc), what + ": the two yardsticks disagree"
            dropped += int(H[0][-1] - want[0][-1])
            f = _filter(sc, prim_bits, m, skip)
            assert np.array_equal(sc.convex_count(d_planes, inside=inside, filter=f).cpu().numpy(), wc), what
            assert_csr(sc.in_convex(d_planes, inside=inside, filter=f), want, what + " list")
            words = np.full(n_prims, 0xFFFFFFFF, np.uint32) if prim_bits is None else prim_bits
            allowed = (words[None, :] & np.broadcast_to(np.asarray(m, np.uint32), (len(wc),))[:, None]) != 0
            if skip is not None:
                allowed &= np.arange(n_prims)[None, :] != np.asarray(skip, np.int64)[:, None]
            assert_any(sc.convex_any(d_planes, inside=inside, filter=f), wc, K, 1 - flags, what + " any", allowed)
            lo, mm = SLICES[3]
            fs = _filter(sc, prim_bits, m if np.ndim(m) == 0 else m[lo:lo + mm], None if skip is None else skip[lo:lo + mm])
            assert np.array_equal(sc.convex_count(sets.planes[lo:lo + mm], inside=inside, filter=fs), wc[lo:lo + mm]), what + ", numpy, n = 65"
    assert dropped > 100


CHILD = r"""
import sys
import numpy as np
import ptamd
from scenes_util import test_spheres
planes, out = np.load(sys.argv[1]), sys.argv[2]
nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, 24))
sc = ptamd.Scene(nodes, tris, test_spheres())
res = {}
for flags in (0, 1):
    res[f"count{flags}"] = sc.convex_count(planes, inside=bool(flags))
    res[f"acls{flags}"], res[f"aprim{flags}"] = sc.convex_any(planes, inside=bool(flags))
    res[f"off{flags}"], res[f"cls{flags}"], res[f"prim{flags}"] = sc.in_convex(planes, inside=bool(flags))
np.savez(out, **res)
"""


@pytest.mark.gpu
def test_binary_walk_forced_by_its_knob_gives_the_same_bits(_gpu, tmp_path):
    """PTAMD_QUERY_QUAD=0 in a fresh process (the knob is read when a scene is created), as tests/test_box_queries.py sets it."""
    name = "standin24_spheres"
    plane_file, out = str(tmp_path / "planes.npy"), str(tmp_path / "child.npz")
    np.save(plane_file, _sets(name).planes)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]), PTAMD_QUERY_QUAD="0")
    subprocess.run([sys.executable, "-c", CHILD, plane_file, out], check=True, env=env, timeout=600)
    g = np.load(out)
    for flags in (V.TOUCHING, V.INSIDE):
        counts, H = _want(name, flags)
        assert np.array_equal(g[f"count{flags}"], counts)
        assert_any((g[f"acls{flags}"], g[f"aprim{flags}"]), counts, _keys(name), 1 - flags, f"PTAMD_QUERY_QUAD=0 any, flags {flags}")
        assert_csr((g[f"off{flags}"], g[f"cls{flags}"], g[f"prim{flags}"]), H, f"PTAMD_QUERY_QUAD=0, flags {flags}")


def _assert_pose(sc, d_planes, K, wants, what):
    for flags in (V.TOUCHING, V.INSIDE):
        counts, H = wants[flags]
        assert np.array_equal(sc.convex_count(d_planes, inside=bool(flags)).cpu().numpy(), counts), f"{what}, flags {flags}"
        assert_csr(sc.in_convex(d_planes, inside=bool(flags)), H, f"{what}, flags {flags}")
        assert_any(sc.convex_any(d_planes, inside=bool(flags)), counts, K, 1 - flags, f"{what} any, flags {flags}")


@pytest.mark.gpu
def test_the_result_does_not_depend_on_the_tree(_gpu):
    """A refit tree, a fresh upload at the same pose and the three rebuilds hold different boxes and different topologies over the same
    positions: the same bits from all of them, and they are brute force's at the moved positions."""
    name = "standin24_spheres"
    nodes, tris, sph = T._host_scene(name)
    planes = _sets(name).planes
    pos2 = T._turned(tris)
    K = V.key_matrix(planes, pos2.reshape(-1, 3, 3), sph)
    wants = {flags: V.brute(None, None, None, flags, K=K) for flags in (V.TOUCHING, V.INSIDE)}
    moved = (wants[0][0] != _want(name, 0)[0]).mean()
    print(f"the move changed the counts of {moved:.3f} of the regions")
    assert moved > 0.1
    d_planes = _dev(planes)
    sc = ptamd.Scene(nodes, tris, sph)
    sc.update_vertices(pos2)
    _assert_pose(sc, d_planes, K, wants, "after update_vertices")
    tris2 = R.restate_tris(tris, pos2)
    _assert_pose(ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph), d_planes, K, wants, "fresh scene at the pose")
    sc.rebuild_tree()
    _assert_pose(sc, d_planes, K, wants, "after rebuild_tree")
    sc.rebuild_tree(depth_budget=26, large_fraction=1 / 16)
    _assert_pose(sc, d_planes, K, wants, "after rebuild_tree(26, 1/16)")
    sc.rebuild_tree_optimized()
    _assert_pose(sc, d_planes, K, wants, "after rebuild_tree_optimized")
    assert sc.tree_info()["rebuilds"] == 3


@pytest.mark.gpu
def test_queries_on_a_stream_behind_an_update_allocate_nothing_and_leave_renders_alone(_gpu):
    import torch
    name = "standin24_spheres"
    nodes, tris, sph = T._host_scene(name)
    planes = _sets(name).planes
    pos2 = T._turned(tris)
    K = V.key_matrix(planes, pos2.reshape(-1, 3, 3), sph)
    counts, H = V.brute(None, None, None, V.TOUCHING, K=K)
    sc = ptamd.Scene(nodes, tris, sph)
    sc.update_vertices(R.positions(tris).reshape(-1, 9))      # the first update allocates the scene's maps: not what is measured below
    cam, prm = ptamd.make_camera(100, 52), ptamd.default_params(passes=2, spp_per_pass=4)
    img = sc.render(cam, prm)
    state = (sc.last_iterations(), sc.device_bytes)
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    with torch.cuda.stream(st):
        d_pos = torch.from_numpy(pos2).to(dev)
        d_planes = torch.from_numpy(planes).to(dev)
        sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
        got_c = sc.convex_count(d_planes, stream_ptr=st.cuda_stream)      # no host wait in between
        got_a = sc.convex_any(d_planes, stream_ptr=st.cuda_stream)
        got_l = sc.in_convex(d_planes, stream_ptr=st.cuda_stream)
        assert (sc.last_iterations(), sc.device_bytes) == state      # a query allocates nothing and leaves the render state alone
        assert got_c.dtype == torch.int32 and got_a[0].dtype == torch.float32 and got_l[0].dtype == torch.int64 and got_c.device == dev
        host = [x.cpu().numpy() for x in (got_c,) + got_a + got_l]
    st.synchronize()
    assert np.array_equal(host[0], counts)
    assert_any(tuple(host[1:3]), counts, K, 1, "device path behind an update, any")
    assert_csr(tuple(host[3:6]), H, "device path behind an update")
    sc.update_vertices(R.positions(tris).reshape(-1, 9))
    assert np.array_equal(bits(sc.render(cam, prm)), bits(img))


def _centre_rays(cam):
    """The rays through the pixel centres (u1 = u2 = 0.5) of `cam`, built in numpy as pixel_direction builds them: (H * W, 8) RAY8."""
    px, py = np.meshgrid(np.arange(cam.W), np.arange(cam.H))
    d = _pixel_dirs(cam, px.reshape(-1) + 0.5, py.reshape(-1) + 0.5)
    d /= np.sqrt((d * d).sum(1, keepdims=True))
    rays = np.zeros((cam.W * cam.H, 8), F)
    rays[:, 0:3], rays[:, 3:6], rays[:, 7] = np.array(cam.pos[:], F), d.astype(F), 999999.0
    return rays, px.reshape(-1), py.reshape(-1)


@pytest.mark.gpu
def test_a_windows_frustum_holds_what_its_pixels_rays_hit_and_nothing_inside_it_is_hit_from_elsewhere(_gpu):
    """End to end with the camera: the 8 x 8-pixel windows of a 64 x 48 frame against rays through the pixel centres.  The centres are
    half a pixel inside their window and the outside rays half a pixel beyond the window grown by one: the margin against rounding."""
    name = "standin24_spheres"
    sc = T._scene(name)
    cam = ptamd.make_camera(64, 48)
    rays, px, py = _centre_rays(cam)
    _, prim = sc.trace_rays(rays)
    assert (prim >= 0).mean() > 0.5      # the room is open towards the camera: most rays hit something
    wins = [(x, y, x + 8, y + 8) for y in range(0, 48, 8) for x in range(0, 64, 8)]
    planes = ptamd.frustum_planes(cam, wins)
    assert planes.shape == (48, 6, 4)
    off, cls, member = sc.in_convex(planes)
    n_prims = T._n_prims(name)
    held = hit_outside = 0
    for w, (x0, y0, x1, y1) in enumerate(wins):
        mem, c = member[off[w]:off[w + 1]], cls[off[w]:off[w + 1]]
        inside_w = (px >= x0) & (px < x1) & (py >= y0) & (py < y1) & (prim >= 0)
        hit = np.unique(prim[inside_w])
        assert np.isin(hit, mem).all(), f"window {w}: primitives {hit[~np.isin(hit, mem)][:5]} are hit through it but are no members"
        held += len(hit)
        beyond = ((px < x0 - 1) | (px >= x1 + 1) | (py < y0 - 1) | (py >= y1 + 1)) & (prim >= 0)
        cls0 = np.zeros(n_prims, bool)
        cls0[mem[c == 0]] = True
        assert not cls0[prim[beyond]].any(), f"window {w}: a primitive wholly inside it is hit by a ray that passes it by"
        hit_outside += int(cls0.sum())
    assert held > 48 and hit_outside > 0      # both properties had something to say
    sel = sc.select_window(cam, (0, 0, 64, 48))
    assert sel.dtype == np.int32 and (np.diff(sel) > 0).all() and np.isin(np.unique(prim[prim >= 0]), sel).all()
    assert np.array_equal(sel, np.sort(np.asarray(sc.in_convex(_dev(ptamd.frustum_planes(cam)[None]))[2].cpu())))
    ins = sc.select_window(cam, (8, 8, 56, 40), inside=True)
    assert np.isin(ins, sc.select_window(cam, (8, 8, 56, 40))).all() and len(ins) > 0
