"""Box queries (include/pt_api.h: pt_box_count, pt_box_any, pt_box_list; csrc/pt_box.hip): which primitives lie
inside or touch the caller's axis-aligned boxes.

The yardstick is tests/box_ref.py: the class key g(Q, k) of the header in numpy float32, operation by operation, and brute force over
every primitive with the lists' order.  On the CPU the kernels' own two functions are compiled for the host and held to it bit for bit,
the definition is held against a float64 evaluation on boxes grown and shrunk by 2^-14 of the largest coordinate, and the yardstick's
own properties are asserted.  On the GPU every result is compared bit for bit, no tolerance and no query left out, on the scenes of
tests/test_nearest.py and on both walks."""
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
NEW = ("pt_box_count", "pt_box_any", "pt_box_list", "pt_box_count_host", "pt_box_any_host", "pt_box_list_host")
SLICES = ((0, 1), (7, 63), (100, 64), (33, 65), (211, 130))      # partial waves, one wave, a wave and a lane, two waves and two lanes
PAIRS = 2_000_000                                                # per family of the accuracy test
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
    for m in ("box_count", "box_any", "in_boxes", "voxelize"):
        assert callable(getattr(ptamd.Scene, m)), m
    assert callable(ptamd.grid_boxes)
    assert (ptamd.BOX_TOUCHING, ptamd.BOX_INSIDE) == (0, 1)
    assert C.sizeof(ptamd.PtBoxMember) == 8 and ptamd.BOX_DTYPE.itemsize == 8 and ptamd.BOX_DTYPE.names == ("cls", "prim")
    assert ptamd.PtBoxMember.cls.offset == 0 and ptamd.PtBoxMember.prim.offset == 4
    assert ptamd.BOX_DTYPE.fields["cls"][1] == 0 and ptamd.BOX_DTYPE.fields["prim"][1] == 4
    src = tmp_path / "box.c"
    src.write_text('#include <stddef.h>\n#include "pt_api.h"\n_Static_assert(sizeof(PtBoxMember) == 8, "PtBoxMember");\n'
                   '_Static_assert(offsetof(PtBoxMember, cls) == 0 && offsetof(PtBoxMember, prim) == 4, "fields");\n'
                   '_Static_assert(PT_BOX_TOUCHING == 0 && PT_BOX_INSIDE == 1, "flags");\n')
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    at = hdr.index("Box queries (new")
    assert hdr.index("Query filters (new") < at < hdr.index("Radiance along the caller's own rays")
    assert hdr.index(" pt_within_radius_list_f(") < at      # directly after the filters' last declaration
    assert all(at < hdr.index(f" {name}(") < hdr.index("Radiance along the caller's own rays") for name in NEW)


def test_bad_arguments_are_rejected_before_any_device_call():
    """A fake scene and fake device addresses: never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    base = 1 << 40
    scene, boxes, out, cnt, offs, arr = (C.c_void_p(base + (i << 20)) for i in range(6))
    off = lambda p, k: C.c_void_p(p.value + k)      # noqa: E731
    flt = lambda **kw: C.byref(ptamd.PtQueryFilter(kw.get("prim"), kw.get("query"), kw.get("skip"), 0xFFFFFFFF, kw.get("flags", 0)))      # noqa: E731
    # (what, scene, boxes, n, flags, filter): the arguments the three device calls share
    shared = [
        ("NULL scene", None, boxes, 64, 0, None),
        ("NULL boxes", scene, None, 64, 0, None),
        ("n < 0", scene, boxes, -1, 0, None),
        ("flags 2", scene, boxes, 64, 2, None),
        ("flags -1", scene, boxes, 64, -1, None),
        ("boxes + 8", scene, off(boxes, 8), 64, 0, None),
        ("PT_FILTER_TMIN", scene, boxes, 64, 0, flt(flags=ptamd.FILTER_TMIN)),
        ("unknown filter flags", scene, boxes, 64, 1, flt(flags=2)),
        ("filter d_prim_bits + 2", scene, boxes, 64, 0, flt(prim=arr.value + 2)),
        ("filter d_query_bits + 2", scene, boxes, 64, 0, flt(query=arr.value + 2)),
        ("filter d_skip_prim + 2", scene, boxes, 64, 1, flt(skip=arr.value + 2)),
        ("n = 0 does not excuse a NULL", scene, None, 0, 0, None),
    ]
    for what, s, b, n, flags, f in shared:
        assert l.pt_box_count(s, b, n, flags, f, cnt, None) == -1 and b"pt_box_count:" in l.pt_last_error(), (what, l.pt_last_error())
        assert l.pt_box_any(s, b, n, flags, f, out, None) == -1 and b"pt_box_any:" in l.pt_last_error(), (what, l.pt_last_error())
        assert l.pt_box_list(s, b, n, flags, offs, 100, f, out, None) == -1 and b"pt_box_list:" in l.pt_last_error(), (what, l.pt_last_error())
    own = [
        ("count NULL", l.pt_box_count, (scene, boxes, 64, 0, None, None, None)),
        ("count + 2", l.pt_box_count, (scene, boxes, 64, 0, None, off(cnt, 2), None)),
        ("n = 0 does not excuse a NULL count", l.pt_box_count, (scene, boxes, 0, 0, None, None, None)),
        ("any out NULL", l.pt_box_any, (scene, boxes, 64, 1, None, None, None)),
        ("any out + 4", l.pt_box_any, (scene, boxes, 64, 0, None, off(out, 4), None)),
        ("list offsets NULL", l.pt_box_list, (scene, boxes, 64, 0, None, 100, None, out, None)),
        ("list offsets + 4", l.pt_box_list, (scene, boxes, 64, 0, off(offs, 4), 100, None, out, None)),
        ("list out NULL", l.pt_box_list, (scene, boxes, 64, 0, offs, 100, None, None, None)),
        ("list out + 4", l.pt_box_list, (scene, boxes, 64, 0, offs, 100, None, off(out, 4), None)),
        ("list cap < 0", l.pt_box_list, (scene, boxes, 64, 0, offs, -1, None, out, None)),
    ]
    for what, fn, a in own:
        assert fn(*a) == -1, what
        assert fn.__name__.encode() + b":" in l.pt_last_error(), (what, l.pt_last_error())
    h_boxes, h_cnt, h_out, h_off = np.zeros((64, 8), F), np.zeros(64, np.int32), np.zeros(64, ptamd.BOX_DTYPE), np.zeros(65, np.int64)
    P = ptamd._ptr
    host = [
        ("NULL scene", l.pt_box_count_host, (None, P(h_boxes), 64, 0, P(h_cnt))),
        ("NULL boxes", l.pt_box_count_host, (scene, None, 64, 0, P(h_cnt))),
        ("NULL count", l.pt_box_count_host, (scene, P(h_boxes), 64, 0, None)),
        ("n < 0", l.pt_box_count_host, (scene, P(h_boxes), -3, 0, P(h_cnt))),
        ("flags 5", l.pt_box_count_host, (scene, P(h_boxes), 64, 5, P(h_cnt))),
        ("NULL scene", l.pt_box_any_host, (None, P(h_boxes), 64, 0, P(h_out))),
        ("NULL out", l.pt_box_any_host, (scene, P(h_boxes), 64, 0, None)),
        ("flags 2", l.pt_box_any_host, (scene, P(h_boxes), 64, 2, P(h_out))),
        ("NULL scene", l.pt_box_list_host, (None, P(h_boxes), 64, 0, P(h_off), 10, P(h_out))),
        ("NULL boxes", l.pt_box_list_host, (scene, None, 64, 0, P(h_off), 10, P(h_out))),
        ("NULL offsets", l.pt_box_list_host, (scene, P(h_boxes), 64, 0, None, 10, P(h_out))),
        ("cap < 0", l.pt_box_list_host, (scene, P(h_boxes), 64, 0, P(h_off), -1, P(h_out))),
        ("flags 3", l.pt_box_list_host, (scene, P(h_boxes), 64, 3, P(h_off), 10, None)),
    ]
    for what, fn, a in host:
        assert fn(*a) == -1, what
        assert fn.__name__.encode() + b":" in l.pt_last_error(), (what, l.pt_last_error())
    # nothing to do: PT_OK, still without touching the scene or the device
    assert l.pt_box_count(scene, boxes, 0, 0, None, cnt, None) == 0
    assert l.pt_box_any(scene, boxes, 0, 1, flt(prim=arr.value), out, None) == 0
    assert l.pt_box_list(scene, boxes, 0, 0, offs, 0, None, out, None) == 0
    assert l.pt_box_count_host(scene, P(h_boxes), 0, 1, P(h_cnt)) == 0
    h_off[0] = 77
    assert l.pt_box_list_host(scene, P(h_boxes), 0, 0, P(h_off), 0, None) == 0 and h_off[0] == 0


class _FakeScene:
    n_tris, n_spheres, device, _h = 5, 0, 0, C.c_void_p(1 << 40)


def test_wrappers_check_shape_dtype_and_device_on_the_host():
    import torch
    fake = _FakeScene()
    for fn in (ptamd.Scene.box_count, ptamd.Scene.box_any, ptamd.Scene.in_boxes):
        for b in (np.zeros((4, 6), F), np.zeros(16, F), np.zeros((2, 4, 8), F)):
            with pytest.raises(ptamd.PtError):
                fn(fake, b)
        for b in (torch.zeros((5, 8)), torch.zeros((5, 8), dtype=torch.float64), torch.zeros((5, 6)), torch.zeros((8, 5)).t(), [[0.0] * 8]):
            with pytest.raises(ptamd.PtError):      # a CPU tensor, a wrong dtype, a wrong shape, not contiguous, not an array
                fn(fake, b)
    cnt = ptamd.Scene.box_count(fake, np.zeros((0, 8), F))      # n = 0: PT_OK without a device
    assert cnt.shape == (0,) and cnt.dtype == np.int32
    cls, prim = ptamd.Scene.box_any(fake, np.zeros((0, 8), F), inside=True)
    assert cls.shape == (0,) and prim.shape == (0,) and cls.dtype == F and prim.dtype == np.int32
    fs = ptamd.QueryFilter(bits=3).struct(fake, 5)      # the struct a caller of the C-ABI passes: no array, nothing uploaded
    assert isinstance(fs, ptamd.PtQueryFilter) and (fs.d_prim_bits, fs.d_query_bits, fs.d_skip_prim, fs.bits, fs.flags) == (None, None, None, 3, 0)
    with pytest.raises(ptamd.PtError):
        ptamd.QueryFilter(prim_bits=np.zeros(4, np.uint32)).struct(fake, 5)      # 4 words for 5 primitives
    with pytest.raises(ptamd.PtError):
        ptamd.QueryFilter(tmin=True).struct(fake, 5)                             # tmin on a box or point query


def test_voxelize_checks_its_arguments_before_any_device_call():
    fake = _FakeScene()
    bad = [((0, 0, 0), (1, 1, 1), (2, 2)), ((0, 0, 0), (1, 1, 1), (2, 0, 2)), ((0, 0, 0), (1, 1, 1), (2, -1, 2)), ((0, 0), (1, 1, 1), (2, 2, 2)),
           ((0, 0, 0), (1, np.nan, 1), (2, 2, 2)), ((0, 0, 0), (1, np.inf, 1), (2, 2, 2)), ((0, 2, 0), (1, 1, 1), (2, 2, 2)),
           ((0, 0, 0), (1, 1, 1), (2048, 2048, 2048)), ((0, 0, 0), (1, 1, 1), "abc"), ((0, 0, 0), (1, 1, 1), 4)]
    for lo, hi, shape in bad:
        with pytest.raises(ptamd.PtError):
            ptamd.Scene.voxelize(fake, lo, hi, shape)
        with pytest.raises(ptamd.PtError):
            ptamd.grid_boxes(lo, hi, shape, device=None)


def test_grid_boxes_share_their_faces_bit_for_bit_and_end_on_hi():
    lo, hi, shape = (-19.7, 0.1, -20.3), (20.9, 39.3, 31.1), (7, 3, 5)
    g = ptamd.grid_boxes(lo, hi, shape, device=None)
    nx, ny, nz = shape
    assert g.shape == (nx * ny * nz, 8) and g.dtype == F and (g[:, 3] == 0).all() and (g[:, 7] == 0).all()
    v = g.reshape(nz, ny, nx, 8)
    for ax, (a, b) in enumerate(((v[:, :, :-1], v[:, :, 1:]), (v[:, :-1], v[:, 1:]), (v[:-1], v[1:]))):
        assert np.array_equal(bits(a[..., 4 + ax]), bits(b[..., ax])), f"axis {ax}: a voxel's hi is not its neighbour's lo"
    assert np.array_equal(bits(v[0, 0, 0, 0:3]), bits(F(lo))) and np.array_equal(bits(v[-1, -1, -1, 4:7]), bits(F(hi)))
    assert np.array_equal(bits(v[:, :, -1, 4]), bits(np.full((nz, ny), hi[0], F))) and np.array_equal(bits(v[-1, :, :, 6]), bits(np.full((ny, nx), hi[2], F)))
    assert (g[:, 0:3] < g[:, 4:7]).all()
    # x fastest: row (iz * ny + iy) * nx + ix; every edge is lo + (hi - lo) * (i / n) in float32
    ex = (F(lo[0]) + (F(hi[0]) - F(lo[0])) * (np.arange(nx + 1, dtype=F) / F(nx))).astype(F)
    assert np.array_equal(bits(g[(2 * ny + 1) * nx + 3, 0:1]), bits(ex[3:4])) and np.array_equal(bits(v[2, 1, 3]), bits(g[(2 * ny + 1) * nx + 3]))
    one = ptamd.grid_boxes((1, 2, 3), (1, 2, 3), (1, 1, 1), device=None)      # a point is a grid, too
    assert np.array_equal(one, F([[1, 2, 3, 0, 1, 2, 3, 0]]))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the kernels' own functions, compiled for the host
# ---------------------------------------------------------------------------------------------------------------------------------
def box_host():
    """tools/box_host.cpp around box_tri_key and box_sphere_key as csrc/pt_box.h has them, built with the library's numerics flags."""
    def make():
        d = tempfile.mkdtemp(prefix="pt_box_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src = open(os.path.join(PKG, "csrc", "pt_box.h")).read()
        text = "\n".join(_function_text(src, head) for head in ("PT_DEV float box_tri_key(", "PT_DEV float box_sphere_key("))
        open(os.path.join(d, "box_kernel_fns.inc"), "w").write(text)
        exe = os.path.join(d, "box_host")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas", "-I", d,
                        os.path.join(ROOT, "tools", "box_host.cpp"), "-o", exe], check=True)
        return d, exe
    return _cached("box_host", make)


def _function_text(src, head):
    """The text of the function that starts with `head`, to its closing brace."""
    at = src.index(head)
    depth, k = 0, src.index("{", at)
    while True:
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        k += 1
        if depth == 0:
            return src[at:k]


def host_keys(tri_pairs, sph_pairs):
    """The keys the kernels' functions give: tri_pairs (n, 15) lo hi a ab ac, sph_pairs (m, 10) lo hi centre rad."""
    d, exe = box_host()
    src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    tri_pairs, sph_pairs = np.ascontiguousarray(tri_pairs, F).reshape(-1, 15), np.ascontiguousarray(sph_pairs, F).reshape(-1, 10)
    with open(src, "wb") as f:
        f.write(np.array([len(tri_pairs), len(sph_pairs)], np.int32).tobytes())
        f.write(tri_pairs.tobytes())
        f.write(sph_pairs.tobytes())
    subprocess.run([exe, src, dst], check=True)
    out = np.fromfile(dst, F)
    os.remove(src)
    os.remove(dst)
    return out[:len(tri_pairs)], out[len(tri_pairs):]


def _family(name):
    """(lo, hi, positions, accuracy figures, float32 keys) of a family, made once."""
    def make():
        lo, hi, pos = B.FAMILIES[name](FAMILY_SEED[name], PAIRS)
        acc, key = B.accuracy(lo, hi, pos)
        return lo, hi, pos, acc, key
    return _cached(("family", name), make)


def _attribute():
    return _cached("attribute", lambda: R.positions(ptamd.build_bvh(attribute_scene(T.ATTR_SEED, 12)[0])[1]))


def _edge_set():
    """Every box of the attribute scene's box sets against every triangle of it (ties, slivers, zero-area triangles; point boxes,
    slices, faces through vertex coordinates, infinite, inverted and NaN boxes), and the sphere boxes against the test spheres."""
    def make():
        pos, sph = _attribute(), np.ascontiguousarray(make_test_spheres(), F)
        sets = B.BoxSets(pos, sph, 3)
        lo, hi = B.split(sets.boxes)
        a, ab, ac = N.edges(pos)
        nb, nt, ns = len(lo), len(a), len(sph)
        rep = lambda x, n: np.repeat(x, n, 0)      # noqa: E731
        tri = np.concatenate([rep(lo, nt), rep(hi, nt), np.tile(a, (nb, 1)), np.tile(ab, (nb, 1)), np.tile(ac, (nb, 1))], 1)
        sp = np.concatenate([rep(lo, ns), rep(hi, ns), np.tile(sph[:, 0:4], (nb, 1))], 1)
        return tri, sp
    return _cached("edge set", make)


@pytest.mark.parametrize("name", sorted(B.FAMILIES) + ["edge set"])
def test_the_kernels_functions_compiled_for_the_host_are_the_yardsticks_bit_for_bit(name):
    if name == "edge set":
        tri, sp = _edge_set()
        want_t = B.tri_key(tri[:, 0:3], tri[:, 3:6], tri[:, 6:9], tri[:, 9:12], tri[:, 12:15])
        want_s = B.sphere_key(sp[:, 0:3], sp[:, 3:6], sp[:, 6:9], sp[:, 9])
    else:
        lo, hi, pos, _, want_t = _family(name)
        tri, sp, want_s = np.concatenate([lo, hi] + list(N.edges(pos)), 1), np.zeros((0, 10), F), np.zeros(0, F)
    got_t, got_s = host_keys(tri, sp)
    hist = [int((want_t == v).sum()) for v in (0, 1, INF)]
    print(f"{name}: {len(tri)} triangle pairs (inside, touching, none) = {hist}, {len(sp)} sphere pairs {[int((want_s == v).sum()) for v in (0, 1, INF)]}")
    assert sum(hist) == len(tri) and hist[1] > 0 and hist[2] > 0 and (name == "needles" or hist[0] > 0)
    assert np.array_equal(bits(got_t), bits(want_t)), f"{name}: {(bits(got_t) != bits(want_t)).sum()} triangle keys differ, first at {np.nonzero(bits(got_t) != bits(want_t))[0][:5]}"
    assert np.array_equal(bits(got_s), bits(want_s)), f"{name}: {(bits(got_s) != bits(want_s)).sum()} sphere keys differ"
    if name == "edge set":
        assert all((want_s == v).any() for v in (0, 1, INF))


@pytest.mark.parametrize("name", sorted(B.FAMILIES))
def test_the_float32_key_agrees_with_float64_on_boxes_grown_and_shrunk_by_2_to_the_minus_14(name):
    """With M the largest absolute coordinate of the family and delta = 2^-14 * M, for every one of the 2 * 10^6 pairs: a pair the
    float64 test calls disjoint on the box grown by delta is no member, a pair it calls overlapping on the box shrunk by delta is a
    member, a pair it calls inside the shrunk box has key 0.  Measured with these seeds (grown-disjoint members, shrunk-overlapping
    non-members, inside misses): ordinary and far 0 exceptions down to 2^-20; needles 0 at 2^-14, 11 at 2^-16, 34 at 2^-18, 43 at
    2^-20, all of the second kind (a box thinner than ~0.015 sitting on a needle, which the float32 plane test loses: the normal of a
    1:10,000 needle is tilted by ~6e-4).  The margin on the needles is thin: another seed gave 1 exception in 2 * 10^6 at 2^-14."""
    lo, hi, pos, acc, key = _family(name)
    for s in sorted(acc):
        print(f"{name}: delta = 2^-{s} * M: {acc[s][0]} members the grown box calls disjoint, {acc[s][1]} non-members the shrunk box calls overlapping, "
              f"{acc[s][2]} inside the shrunk box without key 0")
    assert set(acc) >= {14, 16, 18, 20}
    assert acc[14] == (0, 0, 0), f"{name}: {acc[14]} exceptions at 2^-14 * M"


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the yardstick's own properties
# ---------------------------------------------------------------------------------------------------------------------------------
def _ysets():
    def make():
        pos, sph = _attribute(), np.ascontiguousarray(make_test_spheres(), F)
        sets = B.BoxSets(pos, sph, 3)
        return pos, sph, sets, B.key_matrix(sets.boxes, pos, sph)
    return _cached("yardstick sets", make)


def test_yardstick_inside_members_are_a_subset_of_the_touching_ones_and_come_first():
    pos, sph, sets, K = _ysets()
    ct, (ot, kt, pt) = B.brute(sets.boxes, pos, sph, B.TOUCHING, K=K)
    ci, (oi, ki, pi) = B.brute(sets.boxes, pos, sph, B.INSIDE, K=K)
    assert (ci <= ct).all() and (ci > 0).any() and (ci < ct).any() and set(np.unique(kt).tolist()) == {0.0, 1.0} and (ki == 0).all()
    for q in range(len(sets.boxes)):
        row_t, row_i = pt[ot[q]:ot[q + 1]], pi[oi[q]:oi[q + 1]]
        assert np.array_equal(row_t[:len(row_i)], row_i) and (kt[ot[q]:ot[q + 1]][len(row_i):] == 1).all()      # inside first, in the same order
        k = kt[ot[q]:ot[q + 1]]
        assert ((np.diff(k) > 0) | ((np.diff(k) == 0) & (np.diff(row_t) < 0))).all()      # cls ascending, then the larger prim first
    assert np.array_equal(bits(F(0)), np.uint32([0])) and bits(F(0))[0] < bits(F(1))[0] < 0x7f800000      # the keys' bits order as ints


def test_yardstick_invalid_boxes_have_no_member_and_the_whole_scene_box_has_every_primitive_inside():
    pos, sph, sets, K = _ysets()
    n_prims = len(pos) + len(sph)
    assert np.isnan(B.split(sets.parts["invalid"])[0]).any() and np.isnan(B.split(sets.parts["invalid"])[1]).any()
    lo, hi = B.split(sets.parts["invalid"])
    assert ((lo > hi).any(1) | np.isnan(lo).any(1) | np.isnan(hi).any(1)).all() and (lo > hi).any()
    assert (K[sets.rows("invalid")] == INF).all()
    assert (K[sets.rows("scene")] == 0).all() and K.shape[1] == n_prims
    half, slab, column = K[sets.rows("halfspace")]      # below a plane, between two, a column through the scene
    assert all((half == v).any() for v in (0, 1, INF)) and (slab <= 1).any() and (slab == INF).any() and (column == INF).any()
    plane = B.split(sets.parts["halfspace"])[1][0, 1]      # a half-space is answered exactly: by the record's own y extent
    tlo, thi = N.tri_box(*N.edges(pos))
    assert np.array_equal(half[:len(pos)] == 0, thi[:, 1] <= plane) and np.array_equal(half[:len(pos)] <= 1, tlo[:, 1] <= plane)
    assert (K[sets.rows("far")] == INF).all()


def test_yardstick_a_point_box_on_a_vertex_touches_that_vertexs_triangles():
    pos = _attribute()
    a, ab, ac = N.edges(pos)
    own = B.tri_key(a, a, a, ab, ac)      # the box lo == hi == V0 of every triangle against that triangle
    point_like = (ab == 0).all(1) & (ac == 0).all(1)
    assert (own[~point_like] == 1).all() and (own[point_like] == 0).all() and (~point_like).sum() > 200
    K = B.key_matrix(B.make_boxes(a, a), pos)
    shared = (pos[None, :, :, :] == a[:, None, None, :]).all(-1)[:, :, 0]      # triangles whose V0 is this very point
    assert (K[shared] <= 1).all() and shared.sum() >= len(a)


def test_yardstick_puts_a_duplicated_triangle_before_the_one_it_copies():
    pos = _attribute()
    dup = np.concatenate([pos, pos[5:6]])      # triangle 5 again, as the last one
    box = B.make_boxes(pos[5].min(0) - F(0.5), pos[5].max(0) + F(0.5))
    _, (off, cls, prim) = B.brute(box, dup)
    at5, at_dup = int(np.nonzero(prim == 5)[0][0]), int(np.nonzero(prim == len(pos))[0][0])
    assert bits(cls[at5]) == bits(cls[at_dup]) and at_dup < at5      # among equal keys the larger index first
    assert (np.diff(prim[cls == cls[at5]]) < 0).all()


def test_yardstick_a_box_inside_a_sphere_has_no_sphere_member_and_one_around_it_has_it_inside():
    pos, sph, sets, K = _ysets()
    rows, kind = sets.rows("spheres"), sets.sphere_kind
    S = K[rows][:, len(pos):]
    lo, hi = B.split(sets.parts["spheres"])
    for j, s in enumerate(sph):
        corner = np.sqrt((np.maximum(np.abs(lo.astype(np.float64) - s[0:3]), np.abs(hi.astype(np.float64) - s[0:3])) ** 2).sum(1))
        strictly_inside = corner < s[3] * (1 - 1e-6)
        assert (S[strictly_inside, j] == INF).all()
    own = S[np.arange(len(rows)), sets.sphere_index]
    assert all((kind == v).sum() > 3 for v in (0, 1, 2))
    assert (own[kind == 0] == INF).all() and (own[kind == 1] == 0).all() and (own[kind == 2] == 1).all()      # inside the ball, around it, across its surface


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


def _sets(name):
    return _cached(("sets", name), lambda: B.BoxSets(T._positions(name), T._spheres(name), 60 + T.SCENES.index(name)))


def _keys(name):
    return _cached(("keys", name), lambda: B.key_matrix(_sets(name).boxes, T._positions(name), T._spheres(name)))


def _want(name, flags):
    """(counts, (offsets, cls, prim)) by brute force, computed once per scene and flag."""
    return _cached(("want", name, flags), lambda: B.brute(_sets(name).boxes, T._positions(name), T._spheres(name), flags, K=_keys(name)))


def assert_sets_hold_what_they_should(name):
    sets, K = _sets(name), _keys(name)
    pos, sph = T._positions(name), T._spheres(name)
    n_prims = T._n_prims(name)
    cnt = (K <= 1).sum(1)
    assert K.shape == (len(sets.boxes), n_prims) and len(sets.boxes) >= 212 + 130
    assert (cnt[sets.rows("around")] > 0).mean() > 0.9      # a box with a vertex or a centroid in its interior
    # a point box ON vertex V0 of a triangle touches that triangle, exactly (key 1; 0 where the whole triangle is that point): the record's
    # b = a + ab may miss V1 by an ulp and a needle's plane test loses a box of no thickness, so the other point boxes and the slices
    # are asserted to be what they are, not to hold something
    lo, hi = B.split(sets.parts["points"])
    assert np.array_equal(bits(lo), bits(hi))
    on_v0 = np.nonzero(sets.point_vertex == 0)[0]
    tri = sets.point_tri[on_v0]
    a, ab, ac = N.edges(pos)
    own = B.tri_key(a, a, a, ab, ac)
    assert len(on_v0) >= len(lo) // 4 and np.array_equal(bits(lo[on_v0]), bits(a[tri]))
    assert np.array_equal(bits(K[sets.rows("points")[on_v0], tri]), bits(own[tri])) and (own[tri] <= 1).all()
    assert (own[tri][~((ab[tri] == 0).all(1) & (ac[tri] == 0).all(1))] == 1).all()
    lo, hi = B.split(sets.parts["slices"])
    assert ((lo == hi).sum(1) == 1).all()
    lo, hi = B.split(sets.parts["faces"])
    v = np.unique(pos.reshape(-1, 3)[:, 0]), np.unique(pos.reshape(-1, 3)[:, 1]), np.unique(pos.reshape(-1, 3)[:, 2])
    tb = np.concatenate(N.tri_box(*N.edges(pos)))
    on_a_coordinate = sum(np.isin(lo[:, ax], tb[:, ax]) | np.isin(hi[:, ax], tb[:, ax]) | np.isin(hi[:, ax], v[ax]) for ax in range(3))
    assert (on_a_coordinate > 0).all()                                               # a face passes through a coordinate of the scene
    assert (K[sets.rows("faces")][0::3] == 0).any(1).all()                           # a triangle's own box holds it, by equality
    assert (K[sets.rows("scene")] == 0).all() and np.isinf(sets.parts["halfspace"][:, [0, 1, 2, 4, 5, 6]]).sum(1).tolist() == [5, 4, 2]
    assert 0 < cnt[sets.rows("halfspace")[0]] <= n_prims     # the half-space below the scene's middle (a comb reaches into it with every tooth)
    assert (cnt[sets.rows("invalid")] == 0).all() and (cnt[sets.rows("far")] == 0).all()
    if sph is not None:
        S = K[sets.rows("spheres")][:, len(pos):]
        own = S[np.arange(len(S)), sets.sphere_index]
        assert (own[sets.sphere_kind == 0] == INF).all() and (own[sets.sphere_kind == 1] == 0).all() and (own[sets.sphere_kind == 2] == 1).all()
    return cnt


def assert_csr(got, want, what):
    got = tuple(np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in got)
    assert np.array_equal(got[0], want[0]), f"{what}: offsets differ at {np.nonzero(got[0] != want[0])[0][:5]}"
    assert np.array_equal(got[2], want[2]), f"{what}: {(got[2] != want[2]).sum()} prims differ, first at {np.nonzero(got[2] != want[2])[0][:5]}"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{what}: cls differs at {np.nonzero(bits(got[1]) != bits(want[1]))[0][:5]}"


def assert_any(got, counts, K, bound, what, allowed=None):
    """pt_box_any's contract against the counts: prim >= 0 exactly where the count is above 0, then a member with its own key."""
    cls, prim = (np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in got)
    hit = counts > 0
    assert np.array_equal(prim >= 0, hit), f"{what}: {((prim >= 0) != hit).sum()} boxes decide differently from the count"
    assert (prim[~hit] == -1).all() and (bits(cls[~hit]) == 0).all() and (prim < K.shape[1]).all(), what
    key = K[np.nonzero(hit)[0], prim[hit]]
    assert np.array_equal(bits(cls[hit]), bits(key)) and (key <= bound).all(), f"{what}: the record is not a member with its own key"
    if allowed is not None:
        assert allowed[np.nonzero(hit)[0], prim[hit]].all(), f"{what}: a filtered-out primitive was returned"


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.SCENES)
def test_counts_any_and_lists_are_brute_forces(_gpu, name):
    sets, K = _sets(name), _keys(name)
    cnt = assert_sets_hold_what_they_should(name)
    print(f"{name}: {len(sets.boxes)} boxes, {K.shape[1]} primitives; members per box: max {cnt.max()}, at most 8: {(cnt <= 8).sum()}, "
          f"9-32: {((cnt > 8) & (cnt <= 32)).sum()}, above 32: {(cnt > 32).sum()}; inside {(K == 0).sum()}, touching {(K == 1).sum()}")
    if name == "attribute":
        assert ((cnt > 0) & (cnt <= 8)).any() and ((cnt > 8) & (cnt <= 32)).any() and (cnt > 32).any() and cnt.max() == K.shape[1]      # the three sorting classes
    sc = T._scene(name)
    assert (3 * sc.tree_info()["quad_depth"] + 2 > 40) == (name in T.DEEP)      # the deep trees take the binary walk
    d_boxes = _dev(sets.boxes)
    for flags in (B.TOUCHING, B.INSIDE):
        inside, what = flags == B.INSIDE, f"{name}, flags {flags}"
        counts, H = _want(name, flags)
        assert np.array_equal(sc.box_count(d_boxes, inside=inside).cpu().numpy(), counts), what
        assert_any(sc.box_any(d_boxes, inside=inside), counts, K, 1 - flags, what + " any")
        assert_csr(sc.in_boxes(d_boxes, inside=inside), H, what + " list")
        # the host variants against the device route
        assert np.array_equal(sc.box_count(sets.boxes, inside=inside), counts), what + " count_host"
        assert_any(sc.box_any(sets.boxes, inside=inside), counts, K, 1 - flags, what + " any_host")
        assert_csr(sc.in_boxes(sets.boxes, inside=inside), H, what + " list_host")
        for lo, m in SLICES:
            sub = d_boxes[lo:lo + m].contiguous()
            assert np.array_equal(sc.box_count(sub, inside=inside).cpu().numpy(), counts[lo:lo + m]), f"{what}, n = {m}"
            assert_any(sc.box_any(sub, inside=inside), counts[lo:lo + m], K[lo:lo + m], 1 - flags, f"{what} any, n = {m}")
            assert_csr(sc.in_boxes(sub, inside=inside), X.rows(H, lo, m), f"{what} list, n = {m}")


def _raw_list(sc, d_boxes, flags, off, cap, guard=256, filt=None):
    """pt_box_list into a buffer with a guard band on either side of [0, cap): (records (cap, 2) int32, both bands untouched?)."""
    import torch
    buf = torch.full((cap + 2 * guard, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_off = _dev(np.ascontiguousarray(off, np.int64))
    rc = ptamd.lib().pt_box_list(sc._h, C.c_void_p(d_boxes.data_ptr()), d_boxes.shape[0], flags, C.c_void_p(d_off.data_ptr()), cap, filt,
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
    d_boxes = _dev(sets.boxes)
    counts, H = _want(name, B.TOUCHING)
    n = len(counts)
    # segments one short, half as long, a single slot, and full with three to spare, by turns
    m = np.where(np.arange(n) % 4 == 0, counts - 1, np.where(np.arange(n) % 4 == 1, counts // 2, np.where(np.arange(n) % 4 == 2, 1, counts + 3))).clip(0)
    off = np.concatenate([np.zeros(1, np.int64), np.cumsum(m, dtype=np.int64)])
    rec, clean = _raw_list(sc, d_boxes, B.TOUCHING, off, int(off[-1]))
    assert clean
    short = 0
    for q in range(n):
        seg = rec[off[q]:off[q + 1]]
        live = min(int(m[q]), int(counts[q]))
        prim, cls = seg[:live, 1], seg[:live, 0].view(F)
        assert (seg[live:, 1] == -1).all() and (seg[live:, 0] == 0).all(), f"{name}, box {q}: no miss records after the members"
        assert len(set(prim.tolist())) == live and (prim >= 0).all() and (prim < K.shape[1]).all(), f"{name}, box {q}: members repeat"
        assert np.array_equal(bits(cls), bits(K[q, prim])) and (cls <= 1).all(), f"{name}, box {q}: not members with their keys"
        assert ((np.diff(cls) > 0) | ((np.diff(cls) == 0) & (np.diff(prim) < 0))).all(), f"{name}, box {q}: not sorted"
        if m[q] >= counts[q]:
            assert np.array_equal(prim, H[2][H[0][q]:H[0][q + 1]]), f"{name}, box {q}: a segment that holds the list is not the list"
        else:
            short += 1
    assert short > n // 4
    # garbage offsets: negative, beyond cap, decreasing — every write stays inside [0, cap), every record written is a record
    rs = np.random.RandomState(9)
    cap = 700
    junk = rs.randint(-300, 1200, n + 1).astype(np.int64)
    junk[::7] = np.int64(1) << 40
    junk[3::11] = -(np.int64(1) << 40)
    rec, clean = _raw_list(sc, d_boxes, B.TOUCHING, junk, cap)
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
    pos, sph = T._positions(name), T._spheres(name)
    sc = T._scene(name)
    d_boxes = _dev(sets.boxes)
    n_prims = K.shape[1]
    recipe = X.Recipe(_want(name, B.TOUCHING)[1], n_prims, len(pos), 77, False)
    dropped = 0
    for flags in (B.TOUCHING, B.INSIDE):
        inside = flags == B.INSIDE
        counts, H = _want(name, flags)
        # the neutral filter runs the unfiltered kernels: the same bits
        neutral = ptamd.QueryFilter()
        assert np.array_equal(sc.box_count(d_boxes, inside=inside, filter=neutral).cpu().numpy(), counts)
        assert_csr(sc.in_boxes(d_boxes, inside=inside, filter=neutral), H, f"{name}, flags {flags}, neutral filter")
        a, b = sc.box_any(d_boxes, inside=inside, filter=neutral), sc.box_any(d_boxes, inside=inside)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
        for what, prim_bits, m, skip, _ in recipe.filters():
            what = f"{name}, flags {flags}, {what}"
            want = X.select(H, prim_bits, m, skip, None)
            wc, wH = B.brute(sets.boxes, pos, sph, flags, (prim_bits, m, skip), K=K)
            assert X.same(want, wH) and np.array_equal(np.diff(want[0]), wc), what + ": the two yardsticks disagree"
            dropped += int(H[0][-1] - want[0][-1])
            f = _filter(sc, prim_bits, m, skip)
            assert np.array_equal(sc.box_count(d_boxes, inside=inside, filter=f).cpu().numpy(), wc), what
            assert_csr(sc.in_boxes(d_boxes, inside=inside, filter=f), want, what + " list")
            words = np.full(n_prims, 0xFFFFFFFF, np.uint32) if prim_bits is None else prim_bits
            allowed = (words[None, :] & np.broadcast_to(np.asarray(m, np.uint32), (len(wc),))[:, None]) != 0
            if skip is not None:
                allowed &= np.arange(n_prims)[None, :] != np.asarray(skip, np.int64)[:, None]
            assert_any(sc.box_any(d_boxes, inside=inside, filter=f), wc, K, 1 - flags, what + " any", allowed)
            lo, mm = SLICES[3]
            fs = _filter(sc, prim_bits, m if np.ndim(m) == 0 else m[lo:lo + mm], None if skip is None else skip[lo:lo + mm])
            assert np.array_equal(sc.box_count(sets.boxes[lo:lo + mm], inside=inside, filter=fs), wc[lo:lo + mm]), what + ", numpy, n = 65"
    assert dropped > 100


CHILD = r"""
import sys
import numpy as np
import ptamd
from scenes_util import test_spheres
boxes, out = np.load(sys.argv[1]), sys.argv[2]
nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, 24))
sc = ptamd.Scene(nodes, tris, test_spheres())
res = {}
for flags in (0, 1):
    res[f"count{flags}"] = sc.box_count(boxes, inside=bool(flags))
    res[f"acls{flags}"], res[f"aprim{flags}"] = sc.box_any(boxes, inside=bool(flags))
    res[f"off{flags}"], res[f"cls{flags}"], res[f"prim{flags}"] = sc.in_boxes(boxes, inside=bool(flags))
np.savez(out, **res)
"""


@pytest.mark.gpu
def test_binary_walk_forced_by_its_knob_gives_the_same_bits(_gpu, tmp_path):
    """PTAMD_QUERY_QUAD=0 in a fresh process (the knob is read when a scene is created), as tests/test_nearest.py sets it."""
    name = "standin24_spheres"
    box_file, out = str(tmp_path / "boxes.npy"), str(tmp_path / "child.npz")
    np.save(box_file, _sets(name).boxes)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]), PTAMD_QUERY_QUAD="0")
    subprocess.run([sys.executable, "-c", CHILD, box_file, out], check=True, env=env, timeout=600)
    g = np.load(out)
    for flags in (B.TOUCHING, B.INSIDE):
        counts, H = _want(name, flags)
        assert np.array_equal(g[f"count{flags}"], counts)
        assert_any((g[f"acls{flags}"], g[f"aprim{flags}"]), counts, _keys(name), 1 - flags, f"PTAMD_QUERY_QUAD=0 any, flags {flags}")
        assert_csr((g[f"off{flags}"], g[f"cls{flags}"], g[f"prim{flags}"]), H, f"PTAMD_QUERY_QUAD=0, flags {flags}")


def _assert_pose(sc, d_boxes, K, wants, what):
    for flags in (B.TOUCHING, B.INSIDE):
        counts, H = wants[flags]
        assert np.array_equal(sc.box_count(d_boxes, inside=bool(flags)).cpu().numpy(), counts), f"{what}, flags {flags}"
        assert_csr(sc.in_boxes(d_boxes, inside=bool(flags)), H, f"{what}, flags {flags}")
        assert_any(sc.box_any(d_boxes, inside=bool(flags)), counts, K, 1 - flags, f"{what} any, flags {flags}")


@pytest.mark.gpu
def test_the_result_does_not_depend_on_the_tree(_gpu):
    """A refit tree, a fresh upload at the same pose and the three rebuilds hold different boxes and different topologies over the same
    positions: the same bits from all of them, and they are brute force's."""
    name = "standin24_spheres"
    nodes, tris, sph = T._host_scene(name)
    boxes = _sets(name).boxes
    pos2 = T._turned(tris)
    K = B.key_matrix(boxes, pos2.reshape(-1, 3, 3), sph)
    wants = {flags: B.brute(boxes, pos2.reshape(-1, 3, 3), sph, flags, K=K) for flags in (B.TOUCHING, B.INSIDE)}
    moved = (wants[0][0] != _want(name, 0)[0]).mean()
    print(f"the move changed the counts of {moved:.3f} of the boxes")
    assert moved > 0.1
    d_boxes = _dev(boxes)
    sc = ptamd.Scene(nodes, tris, sph)
    sc.update_vertices(pos2)
    _assert_pose(sc, d_boxes, K, wants, "after update_vertices")
    tris2 = R.restate_tris(tris, pos2)
    _assert_pose(ptamd.Scene(R.refit_nodes(nodes, tris2), tris2, sph), d_boxes, K, wants, "fresh scene at the pose")
    sc.rebuild_tree()
    _assert_pose(sc, d_boxes, K, wants, "after rebuild_tree")
    sc.rebuild_tree(depth_budget=26, large_fraction=1 / 16)
    _assert_pose(sc, d_boxes, K, wants, "after rebuild_tree(26, 1/16)")
    sc.rebuild_tree_optimized()
    _assert_pose(sc, d_boxes, K, wants, "after rebuild_tree_optimized")
    assert sc.tree_info()["rebuilds"] == 3


@pytest.mark.gpu
def test_queries_after_an_update_on_the_same_stream_see_the_moved_geometry(_gpu):
    import torch
    name = "standin24_spheres"
    nodes, tris, sph = T._host_scene(name)
    boxes = _sets(name).boxes
    pos2 = T._turned(tris)
    K = B.key_matrix(boxes, pos2.reshape(-1, 3, 3), sph)
    counts, H = B.brute(boxes, pos2.reshape(-1, 3, 3), sph, B.TOUCHING, K=K)
    sc = ptamd.Scene(nodes, tris, sph)
    sc.update_vertices(R.positions(tris).reshape(-1, 9))      # the first update allocates the scene's maps: not what is measured below
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    bytes0 = sc.device_bytes
    with torch.cuda.stream(st):
        d_pos = torch.from_numpy(pos2).to(dev)
        d_boxes = torch.from_numpy(boxes).to(dev)
        sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
        got_c = sc.box_count(d_boxes, stream_ptr=st.cuda_stream)      # no host wait in between
        got_a = sc.box_any(d_boxes, stream_ptr=st.cuda_stream)
        got_l = sc.in_boxes(d_boxes, stream_ptr=st.cuda_stream)
        assert sc.device_bytes == bytes0      # a query allocates nothing
        assert got_c.dtype == torch.int32 and got_a[0].dtype == torch.float32 and got_l[0].dtype == torch.int64 and got_c.device == dev
        host = [x.cpu().numpy() for x in (got_c,) + got_a + got_l]
    st.synchronize()
    assert np.array_equal(host[0], counts)
    assert_any(tuple(host[1:3]), counts, K, 1, "device path behind an update, any")
    assert_csr(tuple(host[3:6]), H, "device path behind an update")


@pytest.mark.gpu
def test_queries_leave_renders_alone(_gpu):
    import torch
    name = "standin24_spheres"
    boxes = _sets(name).boxes
    cam, prm = ptamd.make_camera(100, 52), ptamd.default_params(passes=3, spp_per_pass=4)
    sc = T._scene(name)
    sc.box_count(boxes)      # before the first render, too
    img = sc.render(cam, prm)
    state = (sc.last_iterations(), sc.device_bytes)
    d_boxes = _dev(boxes)
    for b in (boxes, d_boxes):
        sc.box_count(b)
        sc.box_any(b, inside=True)
        sc.in_boxes(b)
    sc.box_count(d_boxes, filter=ptamd.QueryFilter(bits=1, prim_bits=np.ones(T._n_prims(name), np.uint32)))
    torch.cuda.synchronize()
    assert (sc.last_iterations(), sc.device_bytes) == state
    img2 = sc.render(cam, prm)
    assert np.array_equal(bits(img), bits(img2)) and np.array_equal(bits(img), bits(T._scene(name).render(cam, prm)))
    assert (sc.last_iterations(), sc.device_bytes) == state


@pytest.mark.gpu
def test_voxelize_is_brute_force_on_the_grids_boxes(_gpu):
    name = "attribute"
    pos = T._positions(name)
    v = pos.reshape(-1, 3)
    lo, hi, shape = v.min(0), v.max(0), (4, 3, 5)
    g = ptamd.grid_boxes(lo, hi, shape, device=None)
    sc = T._scene(name)
    assert np.array_equal(ptamd.grid_boxes(lo, hi, shape).cpu().numpy(), g)
    for flags in (B.TOUCHING, B.INSIDE):
        counts, _ = B.brute(g, pos, None, flags)
        got = sc.voxelize(lo, hi, shape, inside=bool(flags))
        assert tuple(got.shape) == (5, 3, 4) and np.array_equal(got.cpu().numpy().reshape(-1), counts), f"flags {flags}"
        if flags == B.TOUCHING:
            assert counts.sum() > len(pos)      # a primitive that touches a shared face counts in both voxels
    mask = (np.arange(len(pos)) % 2).astype(np.uint32)
    counts, _ = B.brute(g, pos, None, B.TOUCHING, (mask, np.uint32(1), None))
    assert np.array_equal(sc.voxelize(lo, hi, shape, filter=ptamd.QueryFilter(prim_bits=mask, bits=1)).cpu().numpy().reshape(-1), counts)
