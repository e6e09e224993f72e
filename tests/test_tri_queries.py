"""Triangle queries (include/pt_api.h: pt_tri_count, pt_tri_any, pt_tri_list; csrc/pt_tri.hip): which primitives
the caller's own triangles cut, and along which segments.

The yardstick is tests/tri_ref.py: the membership and the section segment of the header in numpy float32, operation by operation, and
brute force over every primitive with the lists' order.  On the CPU the kernels' own functions are compiled for the host and held to it
bit for bit, the node test is held to the cull theorem on every member pair, the definition is held against float64 from both sides,
and the yardstick's own properties are asserted.  On the GPU every result is compared bit for bit, no tolerance and no query left out,
on the scenes of tests/test_nearest.py and on both walks."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import dynamic_ref as R
import filters_ref as X
import nearest_ref as N
import ptamd
import test_nearest as T
import tri_ref as Q
from scenes_util import make_prims

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pathtrace-on-cuda_amd")
F = np.float32
NEW = ("pt_tri_count", "pt_tri_any", "pt_tri_list", "pt_tri_count_host", "pt_tri_any_host", "pt_tri_list_host")
SLICES = ((0, 1), (7, 63), (100, 64), (33, 65), (211, 130))      # the box tests': partial waves, one wave, a wave and a lane, two waves and two lanes
PAIRS = 400_000                                                  # per family
SEED = 11
N_QUERIES = 352                                                  # per scene: the slices reach 211 + 130
# The smallest power of two k at which the family's 400,000 pairs (seed 11) show no violation of either implication or of the segment
# bound, delta = k 2^-24 scale (DESIGN.md section 44 has the table); the tests assert 4 x it: the sample's worst case is not the
# population's.  The needles' scale carries the scene triangle's kappa (10,000), hence their small k; "needles, no kappa" is the same
# family with the plain scale, which this definition also holds (it never forms the scene triangle's normal).
K_MEASURED = {"ordinary": 4, "needles": 2.0 ** -11, "needles, no kappa": 4, "far": 2, "zero-area scene": 2, "near-coplanar": 256, "on the plane": 2}
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
    for m in ("tri_count", "tri_any", "cut_by_triangles", "slice"):
        assert callable(getattr(ptamd.Scene, m)), m
    assert callable(ptamd.tri_records) and callable(ptamd.quad_triangles) and callable(ptamd.slice_triangles)
    src = tmp_path / "tri.c"
    src.write_text('#include <stddef.h>\n#include "pt_api.h"\n_Static_assert(sizeof(PtBoxMember) == 8, "PtBoxMember");\n'
                   'int (*count)(PtScene*, const float*, int64_t, const PtQueryFilter*, int32_t*, void*) = pt_tri_count;\n'
                   'int (*list)(PtScene*, const float*, int64_t, const int64_t*, int64_t, const PtQueryFilter*, PtBoxMember*, float*, void*) = pt_tri_list;\n'
                   'int (*hlist)(PtScene*, const float*, int64_t, int64_t*, int64_t, PtBoxMember*, float*) = pt_tri_list_host;\n')
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], check=True)
    at = hdr.index("Triangle queries (new")
    assert hdr.index("Sphere casts (new") < at < hdr.index("Radiance along the caller's own rays")
    assert hdr.index(" pt_sweep_spheres_host(") < at      # directly after the sphere casts' last declaration
    assert all(at < hdr.index(f" {name}(") < hdr.index("Radiance along the caller's own rays") for name in NEW)


def test_bad_arguments_are_rejected_before_any_device_call():
    """A fake scene and fake device addresses: never dereferenced, and no HIP call is made, when an argument is bad."""
    l = ptamd.lib()
    base = 1 << 40
    scene, tris, out, cnt, offs, arr, det = (C.c_void_p(base + (i << 20)) for i in range(7))
    off = lambda p, k: C.c_void_p(p.value + k)      # noqa: E731
    flt = lambda **kw: C.byref(ptamd.PtQueryFilter(kw.get("prim"), kw.get("query"), kw.get("skip"), 0xFFFFFFFF, kw.get("flags", 0)))      # noqa: E731
    # (what, scene, tris, n, filter): the arguments the three device calls share
    shared = [
        ("NULL scene", None, tris, 64, None),
        ("NULL tris", scene, None, 64, None),
        ("n < 0", scene, tris, -1, None),
        ("TRI12 + 8", scene, off(tris, 8), 64, None),
        ("PT_FILTER_TMIN", scene, tris, 64, flt(flags=ptamd.FILTER_TMIN)),
        ("unknown filter flags", scene, tris, 64, flt(flags=2)),
        ("filter d_prim_bits + 2", scene, tris, 64, flt(prim=arr.value + 2)),
        ("filter d_query_bits + 2", scene, tris, 64, flt(query=arr.value + 2)),
        ("filter d_skip_prim + 2", scene, tris, 64, flt(skip=arr.value + 2)),
        ("n = 0 does not excuse a NULL", scene, None, 0, None),
    ]
    for what, s, t, n, f in shared:
        assert l.pt_tri_count(s, t, n, f, cnt, None) == -1 and b"pt_tri_count:" in l.pt_last_error(), (what, l.pt_last_error())
        assert l.pt_tri_any(s, t, n, f, out, None) == -1 and b"pt_tri_any:" in l.pt_last_error(), (what, l.pt_last_error())
        assert l.pt_tri_list(s, t, n, offs, 100, f, out, det, None) == -1 and b"pt_tri_list:" in l.pt_last_error(), (what, l.pt_last_error())
    own = [
        ("count NULL", l.pt_tri_count, (scene, tris, 64, None, None, None)),
        ("count + 2", l.pt_tri_count, (scene, tris, 64, None, off(cnt, 2), None)),
        ("n = 0 does not excuse a NULL count", l.pt_tri_count, (scene, tris, 0, None, None, None)),
        ("any out NULL", l.pt_tri_any, (scene, tris, 64, None, None, None)),
        ("any out + 4", l.pt_tri_any, (scene, tris, 64, None, off(out, 4), None)),
        ("list offsets NULL", l.pt_tri_list, (scene, tris, 64, None, 100, None, out, None, None)),
        ("list offsets + 4", l.pt_tri_list, (scene, tris, 64, off(offs, 4), 100, None, out, None, None)),
        ("list out NULL", l.pt_tri_list, (scene, tris, 64, offs, 100, None, None, det, None)),
        ("list out + 4", l.pt_tri_list, (scene, tris, 64, offs, 100, None, off(out, 4), None, None)),
        ("list cap < 0", l.pt_tri_list, (scene, tris, 64, offs, -1, None, out, None, None)),
        ("list detail + 2", l.pt_tri_list, (scene, tris, 64, offs, 100, None, out, off(det, 2), None)),
    ]
    for what, fn, a in own:
        assert fn(*a) == -1, what
        assert fn.__name__.encode() + b":" in l.pt_last_error(), (what, l.pt_last_error())
    h_tris, h_cnt, h_out, h_off = np.zeros((64, 12), F), np.zeros(64, np.int32), np.zeros(64, ptamd.BOX_DTYPE), np.zeros(65, np.int64)
    h_det = np.zeros((64, 8), F)
    P = ptamd._ptr
    host = [
        ("NULL scene", l.pt_tri_count_host, (None, P(h_tris), 64, P(h_cnt))),
        ("NULL tris", l.pt_tri_count_host, (scene, None, 64, P(h_cnt))),
        ("NULL count", l.pt_tri_count_host, (scene, P(h_tris), 64, None)),
        ("n < 0", l.pt_tri_count_host, (scene, P(h_tris), -3, P(h_cnt))),
        ("NULL scene", l.pt_tri_any_host, (None, P(h_tris), 64, P(h_out))),
        ("NULL out", l.pt_tri_any_host, (scene, P(h_tris), 64, None)),
        ("NULL scene", l.pt_tri_list_host, (None, P(h_tris), 64, P(h_off), 10, P(h_out), P(h_det))),
        ("NULL tris", l.pt_tri_list_host, (scene, None, 64, P(h_off), 10, P(h_out), None)),
        ("NULL offsets", l.pt_tri_list_host, (scene, P(h_tris), 64, None, 10, P(h_out), None)),
        ("cap < 0", l.pt_tri_list_host, (scene, P(h_tris), 64, P(h_off), -1, P(h_out), None)),
    ]
    for what, fn, a in host:
        assert fn(*a) == -1, what
        assert fn.__name__.encode() + b":" in l.pt_last_error(), (what, l.pt_last_error())
    # nothing to do: PT_OK, still without touching the scene or the device
    assert l.pt_tri_count(scene, tris, 0, None, cnt, None) == 0
    assert l.pt_tri_any(scene, tris, 0, flt(prim=arr.value), out, None) == 0
    assert l.pt_tri_list(scene, tris, 0, offs, 0, None, out, det, None) == 0
    assert l.pt_tri_count_host(scene, P(h_tris), 0, P(h_cnt)) == 0
    h_off[0] = 77
    assert l.pt_tri_list_host(scene, P(h_tris), 0, P(h_off), 0, None, None) == 0 and h_off[0] == 0


class _FakeScene:
    n_tris, n_spheres, device, _h = 5, 0, 0, C.c_void_p(1 << 40)


def test_wrappers_check_their_arguments_on_the_host():
    import torch
    fake = _FakeScene()
    for fn in (ptamd.Scene.tri_count, ptamd.Scene.tri_any, ptamd.Scene.cut_by_triangles):
        for b in (np.zeros((4, 9), F), np.zeros(24, F), np.zeros((2, 4, 12), F)):
            with pytest.raises(ptamd.PtError):
                fn(fake, b)
        for b in (torch.zeros((5, 12)), torch.zeros((5, 12), dtype=torch.float64), torch.zeros((5, 9)), torch.zeros((12, 5)).t(), [[0.0] * 12]):
            with pytest.raises(ptamd.PtError):      # a CPU tensor, a wrong dtype, a wrong shape, not contiguous, not an array
                fn(fake, b)
    for fn in (ptamd.Scene.tri_count, ptamd.Scene.tri_any):      # a detail buffer is allowed only on the list call
        with pytest.raises(ptamd.PtError, match="only on the list call"):
            fn(fake, np.zeros((0, 12), F), detail=True)
    cnt = ptamd.Scene.tri_count(fake, np.zeros((0, 12), F))      # n = 0: PT_OK without a device
    assert cnt.shape == (0,) and cnt.dtype == np.int32
    cls, prim = ptamd.Scene.tri_any(fake, np.zeros((0, 12), F))
    assert cls.shape == (0,) and prim.shape == (0,) and cls.dtype == F and prim.dtype == np.int32
    for bad in ((0, 0, 0), (np.nan, 1, 0), (1, 0)):
        with pytest.raises(ptamd.PtError):
            ptamd.Scene.slice(fake, (0, 0, 0), bad, 1.0)
    with pytest.raises(ptamd.PtError):
        ptamd.Scene.slice(fake, (0, 0, 0), (0, 1, 0), 0.0)


def test_tri_records_and_quad_triangles():
    a, b, c = np.arange(6, dtype=F).reshape(2, 3), np.arange(6, 12, dtype=F).reshape(2, 3), F([7, 8, 9])
    r = ptamd.tri_records(a, b, c)
    assert r.shape == (2, 12) and r.dtype == F and (r[:, [3, 7, 11]] == 0).all()
    assert np.array_equal(r[:, 0:3], a) and np.array_equal(r[:, 4:7], b) and np.array_equal(r[1, 8:11], c)
    assert ptamd.tri_records((0, 0, 0), (1, 0, 0), (0, 1, 0)).shape == (1, 12)
    with pytest.raises(ptamd.PtError):
        ptamd.tri_records(np.zeros((2, 3)), np.zeros((3, 3)), np.zeros((2, 3)))
    with pytest.raises(ptamd.PtError):
        ptamd.tri_records(np.zeros((2, 2)), np.zeros((2, 2)), np.zeros((2, 2)))
    q = ptamd.quad_triangles((1, 2, 3), (2, 0, 0), (0, 0, 3))
    assert q.shape == (2, 12) and q.dtype == F
    assert np.array_equal(q[0, 0:3], q[1, 0:3]) and np.array_equal(q[0, 8:11], q[1, 4:7])      # the two share the diagonal p00 .. p11
    assert np.array_equal(q[0], F([-1, 2, 0, 0, 3, 2, 0, 0, 3, 2, 6, 0])) and np.array_equal(q[1, 8:11], F([-1, 2, 6]))
    qa, qb, qc = Q.split(q)
    n = N.cross(qb - qa, qc - qa)
    assert (N.dot(n[0:1], n[1:2]) > 0).all()      # wound alike
    with pytest.raises(ptamd.PtError):
        ptamd.quad_triangles((0, 0), (1, 0, 0), (0, 1, 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the kernels' own functions, compiled for the host
# ---------------------------------------------------------------------------------------------------------------------------------
def tri_host():
    """tools/tri_host.cpp around the self-contained part of csrc/pt_tri.h, built with the library's numerics flags."""
    def make():
        d = tempfile.mkdtemp(prefix="pt_tri_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        src = open(os.path.join(PKG, "csrc", "pt_tri.h")).read()
        text = src[src.index("// ---- self-contained: begin"):src.index("// ---- self-contained: end")]
        assert "tri_tri_key" in text and "tri_sphere_key" in text and "tri_node_test" in text and "#include" not in text
        open(os.path.join(d, "tri_kernel_fns.inc"), "w").write(text)
        exe = os.path.join(d, "tri_host")
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I", d, os.path.join(ROOT, "tools", "tri_host.cpp"), "-o", exe],
                       check=True)
        return d, exe
    return _cached("tri_host", make)


def host_keys(tri=None, sph=None, box=None):
    """What the kernels' functions give: tri (n, 18) qa qb qc a ab ac -> (n, 7) key p q; sph (m, 13) qa qb qc centre rad -> (m, 4) key c;
    box (k, 15) qa qb qc lo hi -> (k,) 1 where the node test enters."""
    d, exe = tri_host()
    src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
    tri = np.ascontiguousarray(np.zeros((0, 18), F) if tri is None else tri, F).reshape(-1, 18)
    sph = np.ascontiguousarray(np.zeros((0, 13), F) if sph is None else sph, F).reshape(-1, 13)
    box = np.ascontiguousarray(np.zeros((0, 15), F) if box is None else box, F).reshape(-1, 15)
    with open(src, "wb") as f:
        f.write(np.array([len(tri), len(sph), len(box)], np.int32).tobytes())
        f.write(tri.tobytes())
        f.write(sph.tobytes())
        f.write(box.tobytes())
    subprocess.run([exe, src, dst], check=True)
    out = np.fromfile(dst, F)
    os.remove(src)
    os.remove(dst)
    nt, ns = len(tri) * 7, len(sph) * 4
    return out[:nt].reshape(-1, 7), out[nt:nt + ns].reshape(-1, 4), out[nt + ns:]


def _family(name):
    """(T, S, member, p, q) of a family by the yardstick, made once."""
    def make():
        Tq, S = Q.family(name, SEED, PAIRS)
        ok, p, q = Q.tri_key(Q.lane(Tq[:, 0], Tq[:, 1], Tq[:, 2]), *N.edges(S))
        return Tq, S, ok, p, q
    return _cached(("family", name), make)


def _decides(name, ok):
    """The issue's condition on a family: at least 20 % members and 20 % non-members; the families that have no member by definition are
    exempt from the first half."""
    share = float(ok.mean())
    assert share <= 0.8, f"{name}: {share:.3f} of the pairs are members"
    if name in Q.NO_MEMBERS:
        assert share == 0.0, f"{name}: a member where the definition allows none"
    else:
        assert share >= 0.2, f"{name}: only {share:.3f} of the pairs are members"


@pytest.mark.parametrize("name", Q.TRI_FAMILIES)
def test_the_kernels_key_compiled_for_the_host_is_the_yardsticks_bit_for_bit(name):
    Tq, S, ok, p, q = _family(name)
    a, ab, ac = N.edges(S)
    got, _, _ = host_keys(np.concatenate([Tq.reshape(-1, 9), a, ab, ac], 1))
    print(f"{name}: {len(ok)} pairs, {ok.mean():.4f} members, {(ok & (bits(p) == bits(q)).all(1)).sum()} of them with p == q")
    _decides(name, ok)
    assert set(np.unique(got[:, 0]).tolist()) <= {1.0, np.inf}
    assert np.array_equal(got[:, 0] == 1, ok), f"{name}: membership differs on {((got[:, 0] == 1) != ok).sum()} pairs"
    assert np.array_equal(bits(got[:, 1:4]), bits(p)) and np.array_equal(bits(got[:, 4:7]), bits(q)), f"{name}: segments differ"
    if name == "zero-area scene":
        assert (bits(p[ok]) == bits(q[ok])).all(1).mean() > 0.5      # a zero-area triangle that pierces the query: p == q
    if name == "on the plane":
        on = (Q.plane(Q.lane(Tq[:, 0], Tq[:, 1], Tq[:, 2]), S.transpose(1, 0, 2)) == 0).any(0)
        assert on.mean() > 0.5 and ok[on].any() and (~ok[on]).any()      # vertices exactly on the plane, deciding either way


def test_the_sphere_key_compiled_for_the_host_is_the_yardsticks_bit_for_bit():
    Tq, sp = Q.sphere_family(SEED, PAIRS)
    ok, c = Q.sphere_key(Tq[:, 0], Tq[:, 1], Tq[:, 2], sp[:, 0:3], sp[:, 3])
    _, got, _ = host_keys(sph=np.concatenate([Tq.reshape(-1, 9), sp], 1))
    kind = np.arange(PAIRS) % 4
    print("spheres: members from outside, across, within, a vertex on the surface:", [round(float(ok[kind == j].mean()), 3) for j in range(4)])
    _decides("spheres", ok)
    assert ok[kind == 0].any() and (~ok[kind == 0]).any() and (~ok[kind == 2]).mean() > 0.9 and ok[kind == 3].mean() > 0.8
    assert np.array_equal(got[:, 0] == 1, ok) and np.array_equal(bits(got[:, 1:4]), bits(c))
    # NaN and zero-area queries against a sphere: one answer, the same in both
    Tn = Tq[:4000].copy()
    Tn[::2, 1, 0] = np.nan
    Tn[1::2, 2] = Tn[1::2, 1]
    ok, c = Q.sphere_key(Tn[:, 0], Tn[:, 1], Tn[:, 2], sp[:4000, 0:3], sp[:4000, 3])
    _, got, _ = host_keys(sph=np.concatenate([Tn.reshape(-1, 9), sp[:4000]], 1))
    assert np.array_equal(got[:, 0] == 1, ok) and np.array_equal(bits(got[:, 1:4]), bits(c)) and ok[1::2].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the cull theorem
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in Q.TRI_FAMILIES if n not in Q.NO_MEMBERS])
def test_no_box_of_a_member_is_rejected_by_the_node_test(name):
    """For every member pair: the node test passes on the record's own box, on random boxes that contain it, and on those boxes as either
    tree's walk decodes and widens them — in numpy and in the kernels' own node test compiled for the host."""
    Tq, S, ok, _, _ = _family(name)
    Tq, S = Tq[ok], S[ok]
    L = Q.lane(Tq[:, 0], Tq[:, 1], Tq[:, 2])
    a, ab, ac = N.edges(S)
    b, c = a + ab, a + ac
    tlo, thi = Q.smin(Q.smin(a, b), c), Q.smax(Q.smax(a, b), c)
    rs = np.random.RandomState(5)
    boxes = [("the record's own box", tlo, thi)]
    for r in range(3):
        grow = F(10.0) ** rs.uniform(-7, 1, (len(a), 3)).astype(F) * np.maximum(np.abs(tlo), np.abs(thi)).max(1, keepdims=True)
        lo, hi = tlo - grow * (rs.uniform(0, 1, tlo.shape) < 0.7), thi + grow * (rs.uniform(0, 1, tlo.shape) < 0.7)
        lo, hi = np.minimum(lo.astype(F), tlo), np.maximum(hi.astype(F), thi)
        boxes.append((f"containing boxes {r}", lo, hi))
        boxes.append((f"containing boxes {r}, binary walk", *Q.widen_binary(lo, hi)))
        plo, phi = lo - grow * F(rs.uniform(0, 30)), hi + grow * F(rs.uniform(0, 30))
        qlo, qhi = Q.quad_box(lo, hi, plo.astype(F), phi.astype(F))
        boxes.append((f"containing boxes {r}, 4-wide walk", np.minimum(qlo, lo), np.maximum(qhi, hi)))
    for what, lo, hi in boxes:
        assert (lo <= tlo).all() and (hi >= thi).all(), what
        enter = Q.node_test(L, lo, hi)
        assert enter.all(), f"{name}, {what}: the box of {(~enter).sum()} members of {len(enter)} is rejected"
    _, _, got = host_keys(box=np.concatenate([Tq.reshape(-1, 9), boxes[-1][1], boxes[-1][2]], 1))
    assert (got == 1).all()
    # and the node test decides something: boxes beside the plane, and boxes beside the query's box, are rejected in both restatements
    far = np.abs(tlo).max() * 4 + 100
    lo, hi = np.concatenate([tlo, tlo + F(far)]), np.concatenate([thi, thi + F(far)])
    Tw = np.concatenate([Tq, Tq])
    L2 = Q.lane(Tw[:, 0], Tw[:, 1], Tw[:, 2])
    want = Q.node_test(L2, lo, hi)
    _, _, got = host_keys(box=np.concatenate([Tw.reshape(-1, 9), lo, hi], 1))
    assert np.array_equal(got == 1, want) and want[:len(tlo)].all() and not want[len(tlo):].any()


def test_the_node_test_compiled_for_the_host_is_the_yardsticks_on_boxes_that_hold_nothing():
    """Random boxes about non-members, too: the two restatements agree bit for bit whether the box is entered or not."""
    Tq, S, ok, _, _ = _family("ordinary")
    rs = np.random.RandomState(6)
    ctr = S.mean(1) + rs.uniform(-1.5, 1.5, (len(S), 3)).astype(F)
    half = rs.uniform(0, 1.0, (len(S), 3)).astype(F)
    lo, hi = ctr - half, ctr + half
    want = Q.node_test(Q.lane(Tq[:, 0], Tq[:, 1], Tq[:, 2]), lo, hi)
    _, _, got = host_keys(box=np.concatenate([Tq.reshape(-1, 9), lo, hi], 1))
    print(f"node test: {want.mean():.3f} of {len(want)} boxes entered")
    assert 0.1 < want.mean() < 0.9 and np.array_equal(got == 1, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: geometric truth, with no pair left out
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K_MEASURED))
def test_the_float32_definition_is_held_by_float64_from_both_sides(name):
    """delta = k 2^-24 scale, scale the largest coordinate magnitude of the pair (times the scene triangle's kappa for the needles).  Lower
    side: a pair that is a float64 member for T and for T moved by +-delta along its normal and two in-plane directions is a float32
    member.  Upper side: a float32 member's triangles are at most delta apart in float64 (nine edge pairs, six vertex-face pairs, 0
    where they cross).  Segments: p and q lie within delta of both triangles.  Asserted at 4 x the smallest power of two that leaves no
    violation on these 400,000 pairs (K_MEASURED; DESIGN.md section 44 has the table).
    Measured (violations lower / upper / segment at k = K_MEASURED / 2, then the share of pairs neither implication constrains at 4 k):
    see the printed lines; DESIGN.md records them."""
    Tq, S, ok, p, q = _family(name.split(",")[0])
    k = K_MEASURED[name]
    by_kappa = name == "needles"
    lower, upper, seg, free = Q.truth(Tq, S, k, ok, p, q, by_kappa)
    print(f"{name}: k = {k}: lower {lower.sum()}, upper {upper.sum()}, segment {seg.sum()} violations; unconstrained {free.mean():.4f}")
    lower, upper, seg, free = Q.truth(Tq, S, 4 * k, ok, p, q, by_kappa)
    print(f"{name}: k = {4 * k} (asserted): lower {lower.sum()}, upper {upper.sum()}, segment {seg.sum()} violations; unconstrained {free.mean():.4f}")
    assert lower.sum() == 0, f"{name}: {lower.sum()} pairs are float64 members with all six translates, yet no float32 member"
    assert upper.sum() == 0, f"{name}: {upper.sum()} float32 members are farther apart than delta in float64"
    assert seg.sum() == 0, f"{name}: {seg.sum()} segments leave a triangle by more than delta"
    assert free.mean() < 0.75, f"{name}: the implications constrain too little"


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU: the yardstick's own properties
# ---------------------------------------------------------------------------------------------------------------------------------
def test_yardstick_in_float64_is_symmetric_in_the_two_triangles():
    asym = {}
    for name in ("ordinary", "needles", "near-coplanar"):
        Tq, S, _, _, _ = _family(name)
        a, b = Q.member64(Tq, S), Q.member64(S, Tq)
        asym[name] = int((a != b).sum())
        assert 0.1 < a.mean() < 0.9
    print("float64 members that depend on which triangle is the query:", asym)
    assert asym == {"ordinary": 0, "needles": 0, "near-coplanar": 0}


def _closed():
    return _cached("closed", Q.closed_mesh)


def _slicing(pos, nrm, offset=0.0137):
    v = pos.reshape(-1, 3).astype(np.float64)
    mid, ext = (v.min(0) + v.max(0)) / 2, float((v.max(0) - v.min(0)).max())
    nrm = np.asarray(nrm, np.float64) / np.linalg.norm(nrm)
    return mid + offset * nrm, nrm, ext


def _pairs_up(seg, tol):
    """Does every end point of the (m, 2, 3) segments have a partner — an end point of ANOTHER segment — within tol?  (m, 2) bool."""
    e = seg.reshape(-1, 3).astype(np.float64)
    d = np.sqrt(((e[:, None, :] - e[None, :, :]) ** 2).sum(-1))
    own = np.arange(len(e)) // 2
    d[own[:, None] == own[None, :]] = np.inf
    return (d.min(1) <= tol).reshape(-1, 2)


def test_yardstick_a_closed_mesh_cut_by_a_quad_larger_than_it_gives_closed_curves():
    pos = _closed()
    edges = {}
    for t in pos:
        for i in range(3):
            key = tuple(sorted((t[i].tobytes(), t[(i + 1) % 3].tobytes())))
            edges[key] = edges.get(key, 0) + 1
    assert set(edges.values()) == {2}, "the mesh is not closed"
    total = 0
    for nrm in ([0, 1, 0], [0.3, 0.8, -0.52], [1, 0.02, 0.01]):
        at, nrm, ext = _slicing(pos, nrm)
        quad = ptamd.slice_triangles(at, nrm, ext)
        counts, (off, cls, prim, det) = Q.brute(quad, pos)
        assert (det[:, 6] == 1).all() and (cls == 1).all() and counts.sum() >= 2 * 14 and (counts > 0).all()
        # each end point is within delta of the true crossing of a mesh edge with the plane, or of the segment with the diagonal: its partner's
        # end point, from the neighbour across that edge or from the other half of the quad, is within delta of the same point
        delta = 4 * K_MEASURED["ordinary"] * 2.0 ** -24 * float(np.abs(Q.split(quad)[0]).max() + ext)
        ok = _pairs_up(det[:, 0:6].reshape(-1, 2, 3), 2 * delta)
        assert ok.all(), f"{(~ok).sum()} end points of {ok.size} have no partner within {2 * delta:.2e}"
        total += len(det)
    print(f"closed mesh of {len(pos)} triangles: {total} segments in three sections, every end point paired")


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def _gpu():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    yield


def _queries(name, n=N_QUERIES):
    return _cached(("queries", name, n), lambda: Q.scene_queries(T._positions(name), T._spheres(name), 80 + T.SCENES.index(name), n))


def _want(name, n=N_QUERIES):
    """(counts, (offsets, cls, prim, detail)) by brute force, computed once per scene."""
    return _cached(("want", name, n), lambda: Q.brute(_queries(name, n), T._positions(name), T._spheres(name)))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(x):
    return np.asarray(x.cpu() if hasattr(x, "cpu") else x)


def assert_csr(got, want, what):
    got = tuple(_np(x) for x in got)
    assert np.array_equal(got[0], want[0]), f"{what}: offsets differ at {np.nonzero(got[0] != want[0])[0][:5]}"
    assert np.array_equal(got[2], want[2]), f"{what}: {(got[2] != want[2]).sum()} prims differ, first at {np.nonzero(got[2] != want[2])[0][:5]}"
    assert np.array_equal(bits(got[1]), bits(want[1])), f"{what}: cls differs"
    if len(got) > 3:
        assert np.array_equal(bits(got[3]), bits(want[3])), f"{what}: {(bits(got[3]) != bits(want[3])).any(1).sum()} segments differ, first at {np.nonzero((bits(got[3]) != bits(want[3])).any(1))[0][:5]}"


def assert_any(got, H, what, allowed=None):
    """pt_tri_any's contract against the list: prim >= 0 exactly where the list has a member, then a member of it, cls 1."""
    cls, prim = (_np(x) for x in got)
    off, members = H[0], H[2]
    hit = np.diff(off) > 0
    assert np.array_equal(prim >= 0, hit), f"{what}: {((prim >= 0) != hit).sum()} queries decide differently from the count"
    assert (prim[~hit] == -1).all() and (bits(cls[~hit]) == 0).all() and (bits(cls[hit]) == 0x3F800000).all(), what
    for i in np.nonzero(hit)[0]:
        assert prim[i] in members[off[i]:off[i + 1]], f"{what}: query {i} returns {prim[i]}, no member"
    if allowed is not None:
        assert allowed[np.nonzero(hit)[0], prim[hit]].all(), f"{what}: a filtered-out primitive was returned"


def assert_queries_hold_what_they_should(name):
    q, (counts, H) = _queries(name), _want(name)
    kind = np.arange(len(q)) % 16
    qa, qb, qc = Q.split(q)
    assert np.isnan(q[kind == 11][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]).any(1).all() and (qb[kind == 5] == qc[kind == 5]).all()
    det = H[3]
    own = X.owners(H[0])
    n_tris = len(T._positions(name))
    tri_rows = H[2] < n_tris
    assert (counts[(kind == 11) | (kind == 5)] == 0).all() or T._spheres(name) is not None      # no triangle member ...
    assert not (tri_rows & np.isin(own, np.nonzero((kind == 11) | (kind == 5))[0])).any()      # ... spheres aside
    assert (det[tri_rows, 6] == 1).all() and (det[~tri_rows, 6] == 2).all() and (det[:, 7] == 0).all()
    surface = ~np.isin(kind, (5, 9, 11, 13))
    assert (counts[surface] > 0).mean() > 0.3 and (counts[surface] == 0).any(), f"{name}: {(counts[surface] > 0).mean():.2f} of the surface triangles cut something"
    quads = np.nonzero(kind == 13)[0][:4]
    assert len(quads) == 4 and (counts[quads] > 0).any(), f"{name}: the slicing quads cut nothing: {counts[quads]}"
    if name not in T.DEEP:
        assert (counts[quads] > 0).all(), f"{name}: a half of a slicing quad cuts nothing: {counts[quads]}"
    if T._spheres(name) is not None:
        assert (~tri_rows).sum() > 3
    return counts


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.SCENES)
def test_counts_any_and_lists_with_segments_are_brute_forces(_gpu, name):
    q, (counts, H) = _queries(name), _want(name)
    assert_queries_hold_what_they_should(name)
    print(f"{name}: {len(q)} queries, {T._n_prims(name)} primitives; members per query: max {counts.max()}, at most 8: {(counts <= 8).sum()}, "
          f"9-32: {((counts > 8) & (counts <= 32)).sum()}, above 32: {(counts > 32).sum()}; total {H[0][-1]}")
    sc = T._scene(name)
    assert (3 * sc.tree_info()["quad_depth"] + 2 > 40) == (name in T.DEEP)      # the deep trees take the binary walk
    d_q = _dev(q)
    assert np.array_equal(sc.tri_count(d_q).cpu().numpy(), counts), name
    assert_any(sc.tri_any(d_q), H, name + " any")
    assert_csr(sc.cut_by_triangles(d_q, segments=True), H, name + " list")
    assert_csr(sc.cut_by_triangles(d_q), H[:3], name + " list without segments")
    # the host variants against the device route
    assert np.array_equal(sc.tri_count(q), counts), name + " count_host"
    assert_any(sc.tri_any(q), H, name + " any_host")
    assert_csr(sc.cut_by_triangles(q, segments=True), H, name + " list_host")
    assert_csr(sc.cut_by_triangles(q), H[:3], name + " list_host without segments")
    for lo, m in SLICES:
        sub = d_q[lo:lo + m].contiguous()
        assert np.array_equal(sc.tri_count(sub).cpu().numpy(), counts[lo:lo + m]), f"{name}, n = {m}"
        assert_any(sc.tri_any(sub), X.rows(H, lo, m), f"{name} any, n = {m}")
        assert_csr(sc.cut_by_triangles(sub, segments=True), X.rows(H, lo, m), f"{name} list, n = {m}")
    # a NaN or zero-area record leaves the others alone: the same records with those rows replaced by ordinary ones
    kind = np.arange(len(q)) % 16
    q2 = q.copy()
    q2[(kind == 11) | (kind == 5)] = q[0]
    keep = ~((kind == 11) | (kind == 5))
    assert np.array_equal(sc.tri_count(_dev(q2)).cpu().numpy()[keep], counts[keep])
    # nothing to do: n = 0 writes nothing (an empty tensor has no address, and n = 0 does not excuse a NULL: the records' address is d_q's)
    import torch
    guard = torch.full((8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    l, P = ptamd.lib(), lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    assert l.pt_tri_count(sc._h, P(d_q), 0, None, P(guard), None) == 0 and l.pt_tri_any(sc._h, P(d_q), 0, None, P(guard), None) == 0
    assert l.pt_tri_list(sc._h, P(d_q), 0, P(torch.zeros(1, dtype=torch.int64, device="cuda")), 4, None, P(guard), None, None) == 0
    torch.cuda.synchronize()
    assert (guard.cpu().numpy() == 0x5A5A5A5A).all()
    off0 = sc.cut_by_triangles(d_q[:0].contiguous(), segments=True)
    assert _np(off0[0]).tolist() == [0] and len(off0) == 4 and tuple(off0[3].shape) == (0, 8)
    assert sc.tri_count(q[:0]).shape == (0,) and sc.cut_by_triangles(q[:0], segments=True)[0].tolist() == [0]


@pytest.mark.gpu
def test_a_batch_of_a_few_thousand(_gpu):
    name, n = "standin24_spheres", 4099
    q, (counts, H) = _queries(name, n), _want(name, n)
    sc = T._scene(name)
    d_q = _dev(q)
    assert np.array_equal(sc.tri_count(d_q).cpu().numpy(), counts)
    assert_any(sc.tri_any(d_q), H, "4,099 queries, any")
    assert_csr(sc.cut_by_triangles(d_q, segments=True), H, "4,099 queries")


def _raw_list(sc, d_q, off, cap, guard=256, filt=None, detail=True):
    """pt_tri_list into buffers with a guard band on either side of [0, cap): (records (cap, 2) int32, detail (cap, 8) float32 bits, both
    bands of both untouched?)."""
    import torch
    buf = torch.full((cap + 2 * guard, 2), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    det = torch.full((cap + 2 * guard, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    d_off = _dev(np.ascontiguousarray(off, np.int64))
    rc = ptamd.lib().pt_tri_list(sc._h, C.c_void_p(d_q.data_ptr()), d_q.shape[0], C.c_void_p(d_off.data_ptr()), cap, filt,
                                 C.c_void_p(buf.data_ptr() + guard * 8), C.c_void_p(det.data_ptr() + guard * 32) if detail else None, None)
    assert rc == 0, ptamd.lib().pt_last_error()
    torch.cuda.synchronize()
    h, hd = buf.cpu().numpy(), det.cpu().numpy()
    clean = (h[:guard] == 0x5A5A5A5A).all() and (h[guard + cap:] == 0x5A5A5A5A).all() and (hd[:guard] == 0x5A5A5A5A).all() and (hd[guard + cap:] == 0x5A5A5A5A).all()
    return h[guard:guard + cap], hd[guard:guard + cap], bool(clean)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["attribute", "standin24_spheres", "comb32"])
def test_undersized_segments_hold_distinct_members_sorted_and_nothing_is_written_outside(_gpu, name):
    q, (counts, H) = _queries(name), _want(name)
    sc = T._scene(name)
    d_q = _dev(q)
    n, n_prims = len(counts), T._n_prims(name)
    # segments one short, half as long, a single slot, and full with three to spare, by turns
    m = np.where(np.arange(n) % 4 == 0, counts - 1, np.where(np.arange(n) % 4 == 1, counts // 2, np.where(np.arange(n) % 4 == 2, 1, counts + 3))).clip(0)
    off = np.concatenate([np.zeros(1, np.int64), np.cumsum(m, dtype=np.int64)])
    rec, det, clean = _raw_list(sc, d_q, off, int(off[-1]))
    assert clean
    short = 0
    for i in range(n):
        seg, dseg = rec[off[i]:off[i + 1]], det[off[i]:off[i + 1]]
        live = min(int(m[i]), int(counts[i]))
        prim = seg[:live, 1]
        mine = H[2][H[0][i]:H[0][i + 1]]
        assert (seg[live:, 1] == -1).all() and (seg[live:, 0] == 0).all() and (dseg[live:] == 0).all(), f"{name}, query {i}: no miss records after the members"
        assert len(set(prim.tolist())) == live and np.isin(prim, mine).all() and (seg[:live, 0] == 0x3F800000).all(), f"{name}, query {i}: not distinct members"
        assert (np.diff(prim) < 0).all(), f"{name}, query {i}: not sorted"
        want_det = H[3][H[0][i]:H[0][i + 1]][np.searchsorted(-mine, -prim)]      # each slot's segment is its member's
        assert np.array_equal(dseg[:live].view(np.uint32), bits(want_det)), f"{name}, query {i}: a segment is not its member's"
        if m[i] >= counts[i]:
            assert np.array_equal(prim, mine), f"{name}, query {i}: a segment that holds the list is not the list"
        else:
            short += 1
    assert short > n // 8
    # garbage offsets: negative, beyond cap, decreasing — every write stays inside [0, cap), every record written is a record
    rs = np.random.RandomState(9)
    cap = 700
    junk = rs.randint(-300, 1200, n + 1).astype(np.int64)
    junk[::7] = np.int64(1) << 40
    junk[3::11] = -(np.int64(1) << 40)
    rec, det, clean = _raw_list(sc, d_q, junk, cap)
    assert clean, f"{name}: garbage offsets wrote outside [0, cap)"
    written = rec[:, 0] != 0x5A5A5A5A
    assert written.any() and (rec[written, 1] >= -1).all() and (rec[written, 1] < n_prims).all() and np.isin(rec[written, 0], [0, 0x3F800000]).all()
    assert np.isin(det[written, 6].view(F), [0, 1, 2]).all() and (det[written, 7] == 0).all()
    # cap = 0: nothing is written at all
    rec, det, clean = _raw_list(sc, d_q, H[0], 0)
    assert clean and len(rec) == 0


def _filter(sc, prim_bits, m, skip):
    scalar = np.ndim(m) == 0
    return ptamd.QueryFilter(prim_bits=prim_bits, bits=int(m) if scalar else 0xFFFFFFFF, query_bits=None if scalar else np.ascontiguousarray(m, np.uint32),
                             skip=None if skip is None else np.ascontiguousarray(skip, np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["standin24_spheres", "attribute", "chain28"])
def test_a_filtered_result_is_the_host_side_selection_from_the_unfiltered_list(_gpu, name):
    import torch
    q, (counts, H) = _queries(name), _want(name)
    sc = T._scene(name)
    d_q = _dev(q)
    n_prims = T._n_prims(name)
    recipe = X.Recipe(H, n_prims, len(T._positions(name)), 78, False)
    neutral = ptamd.QueryFilter()      # runs the unfiltered kernels: the twin's bits
    assert np.array_equal(sc.tri_count(d_q, filter=neutral).cpu().numpy(), counts)
    assert_csr(sc.cut_by_triangles(d_q, segments=True, filter=neutral), H, f"{name}, neutral filter")
    a, b = sc.tri_any(d_q, filter=neutral), sc.tri_any(d_q)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    dropped = 0
    for what, prim_bits, m, skip, _ in recipe.filters():
        what = f"{name}, {what}"
        want = X.select(H, prim_bits, m, skip, None)
        wc = np.diff(want[0]).astype(np.int32)
        dropped += int(H[0][-1] - want[0][-1])
        f = _filter(sc, prim_bits, m, skip)
        assert np.array_equal(sc.tri_count(d_q, filter=f).cpu().numpy(), wc), what
        assert_csr(sc.cut_by_triangles(d_q, segments=True, filter=f), want, what + " list")
        words = np.full(n_prims, 0xFFFFFFFF, np.uint32) if prim_bits is None else prim_bits
        allowed = (words[None, :] & np.broadcast_to(np.asarray(m, np.uint32), (len(wc),))[:, None]) != 0
        if skip is not None:
            allowed &= np.arange(n_prims)[None, :] != np.asarray(skip, np.int64)[:, None]
        assert_any(sc.tri_any(d_q, filter=f), want, what + " any", allowed)
        lo, mm = SLICES[3]
        fs = _filter(sc, prim_bits, m if np.ndim(m) == 0 else m[lo:lo + mm], None if skip is None else skip[lo:lo + mm])
        assert np.array_equal(sc.tri_count(q[lo:lo + mm], filter=fs), wc[lo:lo + mm]), what + ", numpy, n = 65"
    assert dropped > 100


CHILD = r"""
import sys
import numpy as np
import ptamd
from scenes_util import test_spheres
q, out = np.load(sys.argv[1]), sys.argv[2]
nodes, tris, _ = ptamd.build_bvh(ptamd.gen_scene(1, 24))
sc = ptamd.Scene(nodes, tris, test_spheres())
res = {"count": sc.tri_count(q)}
res["acls"], res["aprim"] = sc.tri_any(q)
res["off"], res["cls"], res["prim"], res["det"] = sc.cut_by_triangles(q, segments=True)
np.savez(out, **res)
"""


@pytest.mark.gpu
def test_binary_walk_forced_by_its_knob_gives_the_same_bits(_gpu, tmp_path):
    """PTAMD_QUERY_QUAD=0 in a fresh process (the knob is read when a scene is created), as tests/test_nearest.py sets it."""
    name = "standin24_spheres"
    q_file, out = str(tmp_path / "tris.npy"), str(tmp_path / "child.npz")
    np.save(q_file, _queries(name))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, os.path.join(ROOT, "tests"), os.environ.get("PYTHONPATH", "")]), PTAMD_QUERY_QUAD="0")
    subprocess.run([sys.executable, "-c", CHILD, q_file, out], check=True, env=env, timeout=600)
    g = np.load(out)
    counts, H = _want(name)
    assert np.array_equal(g["count"], counts)
    assert_any((g["acls"], g["aprim"]), H, "PTAMD_QUERY_QUAD=0 any")
    assert_csr((g["off"], g["cls"], g["prim"], g["det"]), H, "PTAMD_QUERY_QUAD=0")


@pytest.mark.gpu
def test_the_same_bits_after_a_vertex_update_and_each_rebuild_on_one_stream(_gpu):
    """A refit tree and the three rebuilds hold different boxes and topologies over the same positions: brute force's bits from all of
    them, each edit and the queries behind it enqueued on one stream with no host wait in between, and nothing allocated."""
    import torch
    name = "standin24_spheres"
    nodes, tris, sph = T._host_scene(name)
    q = _queries(name)
    pos2 = T._turned(tris)
    counts, H = Q.brute(q, pos2.reshape(-1, 3, 3), sph)
    moved = (counts != _want(name)[0]).mean()
    print(f"the move changed the counts of {moved:.3f} of the queries")
    assert moved > 0.1
    sc = ptamd.Scene(nodes, tris, sph)
    sc.update_vertices(R.positions(tris).reshape(-1, 9))      # the first update allocates the scene's maps: not what is measured below
    sc.rebuild_tree()                                         # and the first rebuild its workspace
    sc.rebuild_tree_optimized()
    dev = torch.device("cuda:0")
    st = torch.cuda.Stream(dev)
    edits = [("update_vertices", None), ("rebuild_tree", lambda: sc.rebuild_tree(stream_ptr=st.cuda_stream)),
             ("rebuild_tree(26, 1/16)", lambda: sc.rebuild_tree(depth_budget=26, large_fraction=1 / 16, stream_ptr=st.cuda_stream)),
             ("rebuild_tree_optimized", lambda: sc.rebuild_tree_optimized(stream_ptr=st.cuda_stream))]
    with torch.cuda.stream(st):
        d_pos, d_q = torch.from_numpy(pos2).to(dev), torch.from_numpy(q).to(dev)
        for what, edit in edits:
            bytes0 = sc.device_bytes
            if edit is None:
                sc.update_vertices(d_pos, stream_ptr=st.cuda_stream)
            else:
                edit()
            if what != "update_vertices":
                bytes0 = sc.device_bytes      # a rebuild may grow its own workspace; the queries behind it must not
            got_c = sc.tri_count(d_q, stream_ptr=st.cuda_stream)      # no host wait in between
            got_a = sc.tri_any(d_q, stream_ptr=st.cuda_stream)
            got_l = sc.cut_by_triangles(d_q, segments=True, stream_ptr=st.cuda_stream)
            assert sc.device_bytes == bytes0, what      # a query allocates nothing
            assert np.array_equal(got_c.cpu().numpy(), counts), what
            assert_any(got_a, H, what + " any")
            assert_csr(got_l, H, what)
    st.synchronize()


@pytest.mark.gpu
def test_queries_leave_renders_and_the_scenes_memory_alone(_gpu):
    import torch
    name = "standin24_spheres"
    q = _queries(name)
    cam, prm = ptamd.make_camera(100, 52), ptamd.default_params(passes=3, spp_per_pass=4)
    sc = T._scene(name)
    sc.tri_count(q)      # before the first render, too
    img = sc.render(cam, prm)
    state = (sc.last_iterations(), sc.device_bytes)
    d_q = _dev(q)
    for t in (q, d_q):
        sc.tri_count(t)
        sc.tri_any(t)
        sc.cut_by_triangles(t, segments=True)
    sc.tri_count(d_q, filter=ptamd.QueryFilter(bits=1, prim_bits=np.ones(T._n_prims(name), np.uint32)))
    torch.cuda.synchronize()
    assert (sc.last_iterations(), sc.device_bytes) == state
    img2 = sc.render(cam, prm)
    assert np.array_equal(bits(img), bits(img2)) and np.array_equal(bits(img), bits(T._scene(name).render(cam, prm)))
    assert (sc.last_iterations(), sc.device_bytes) == state


@pytest.mark.gpu
def test_slice_of_a_closed_mesh_is_the_yardsticks_and_closes(_gpu):
    mesh = _closed()
    prims = np.concatenate([make_prims(mesh[:-2, 0], mesh[:-2, 1], mesh[:-2, 2]),
                            make_prims(mesh[-2:, 0], mesh[-2:, 1], mesh[-2:, 2], albedo=(0, 0, 0), emit=(6, 6, 6))])
    nodes, tris, _ = ptamd.build_bvh(prims)
    pos = R.positions(tris)
    assert len(pos) == len(mesh)
    sc = ptamd.Scene(nodes, tris)
    for nrm in ([0, 1, 0], [0.3, 0.8, -0.52]):
        at, nrm, ext = _slicing(pos, nrm)
        seg, prim = sc.slice(at, nrm, ext)
        quad = ptamd.slice_triangles(at, nrm, ext)
        _, (off, cls, wprim, det) = Q.brute(quad, pos)
        assert seg.shape == (len(wprim), 2, 3) and seg.dtype == F and len(wprim) >= 2 * 14
        assert np.array_equal(prim, wprim) and np.array_equal(bits(seg.reshape(-1, 6)), bits(det[:, 0:6]))
        delta = 4 * K_MEASURED["ordinary"] * 2.0 ** -24 * float(np.abs(Q.split(quad)[0]).max() + ext)
        assert _pairs_up(seg, 2 * delta).all()
